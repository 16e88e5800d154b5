"""The numpy reference segment caster of the ray-cast tests (tests/ray_ref.py) on scenes with a known answer, against the
renderer's reference (tests/render_ref.py), and the share of marginal rays of the committed ray sets - on the reference alone,
before a GPU sees them (no GPU here)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_ref as ry  # noqa: E402
import render_ref as rr  # noqa: E402

from trex_gym import _capi  # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_rollout.npz"))
I3, Z3 = np.eye(3)[None], np.zeros((1, 3))


def _sphere_scene(r=0.5, floor_z=-100.0):
    return rr.Scene(np.array([[0, 0, 1.0]]), np.array([r]), [0, 1], [0, 1], floor_z=floor_z)


def _cube_scene(h=0.5, floor_z=-100.0):
    cube = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (1 - h, 1 + h)])
    return rr.Scene(cube, np.zeros(8), [0, 8], [0, 8], floor_z=floor_z)


def test_sphere_analytic():
    frm = np.array([[3.0, 0, 1.0], [3.0, 0.3, 1.0], [3.0, 0.6, 1.0], [0.0, 0, 1.0], [3.0, 0, 1.0]])
    to = np.array([[-3.0, 0, 1.0], [-3.0, 0.3, 1.0], [-3.0, 0.6, 1.0], [3.0, 0, 1.0], [1.0, 0, 1.0]])
    f, lab, pos, nrm, mg, _ = ry.cast(_sphere_scene(), I3, Z3, frm, to)
    np.testing.assert_allclose(f[0], 2.5 / 6, rtol=1e-12)
    np.testing.assert_allclose(pos[0], [0.5, 0, 1.0], atol=1e-12)
    np.testing.assert_allclose(nrm[0], [1.0, 0, 0], atol=1e-12)
    np.testing.assert_allclose(f[1], (3 - 0.4) / 6, rtol=1e-12)
    np.testing.assert_allclose(nrm[1], [0.8, 0.6, 0], atol=1e-12)
    assert list(lab) == [0, 0, ry.MISS, ry.MISS, ry.MISS]      # passes it, starts inside it, ends before it
    assert f[2] == f[3] == f[4] == 1.0 and (nrm[2:] == 0).all()
    np.testing.assert_allclose(pos[2:], to[2:])
    np.testing.assert_allclose(mg[2], 0.1, rtol=1e-9)          # the line passes 0.1 m from the sphere
    np.testing.assert_allclose(mg[3], 0.5, rtol=1e-9)          # the origin is 0.5 m behind the entry
    np.testing.assert_allclose(mg[4], 0.5, rtol=1e-9)          # the segment ends 0.5 m before the entry


def test_box_hull_analytic():
    frm = np.array([[0.2, 0.1, 3.0], [2.0, 0.1, 1.2], [0.0, 0.0, 1.0], [0.49, 0.0, 3.0]])
    to = np.array([[0.2, 0.1, 0.0], [-2.0, 0.1, 1.2], [0.0, 0.0, 3.0], [0.49, 0.0, 0.0]])
    f, lab, pos, nrm, mg, nm = ry.cast(_cube_scene(), I3, Z3, frm, to)
    np.testing.assert_allclose(f[:2], [1.5 / 3, 1.5 / 4], rtol=1e-12)
    np.testing.assert_allclose(nrm[:2], [[0, 0, 1.0], [1.0, 0, 0]], atol=1e-12)
    np.testing.assert_allclose(pos[:2], [[0.2, 0.1, 1.5], [0.5, 0.1, 1.2]], atol=1e-12)
    assert list(lab) == [0, 0, ry.MISS, 0]                     # the third starts at the cube's centre and looks out of it
    np.testing.assert_allclose(mg[2], 0.5, rtol=1e-9)
    np.testing.assert_allclose(mg[0], 1.0, rtol=1e-9)          # 1 m through the cube; 1.5 m to either end of the segment
    assert nm[3] == np.inf or nm[3] > 0.5                      # a vertical ray has one entering plane only


def test_floor_and_degenerate_rays():
    sc = _sphere_scene(floor_z=0.25)
    frm = np.array([[5.0, 5, 2.25], [5.0, 5, 2.25], [5.0, 5, 0.0], [5.0, 5, 2.25], [1.0, 1, 1.0], [np.nan, 0, 1.0], [0.0, 0, 9.0]])
    to = np.array([[5.0, 5, -1.75], [8.0, 5, 0.25], [5.0, 5, -1.0], [5.0, 5, 1.25], [1.0, 1, 1.0], [0.0, 0, 0.0], [np.inf, 0, 0.0]])
    f, lab, pos, nrm, mg, _ = ry.cast(sc, I3, Z3, frm, to)
    np.testing.assert_allclose(f[:2], [0.5, 1.0], rtol=1e-12)
    assert list(lab) == [ry.FLOOR, ry.FLOOR, ry.MISS, ry.MISS, ry.MISS, ry.MISS, ry.MISS]   # below the floor; too short; bad rays
    assert (nrm[:2] == [0, 0, 1.0]).all() and (f[2:] == 1.0).all() and (nrm[2:] == 0).all()
    np.testing.assert_allclose(mg[3], 1.0, rtol=1e-9)
    assert mg[1] == 0.0                                        # the hit IS the segment's end: marginal
    f2, lab2 = ry.cast(sc, I3, Z3, frm, to, hit_floor=False)[:2]
    assert (lab2 == ry.MISS).all() and (f2 == 1.0).all()
    f3, lab3 = ry.cast(sc, I3, Z3, [[0, 0, 3.0]], [[0, 0, 0.0]], body_mask=0)[:2]
    assert lab3[0] == ry.FLOOR and abs(f3[0] - 2.75 / 3) < 1e-12


@pytest.mark.parametrize("scene", [_sphere_scene(floor_z=0.0), _cube_scene(floor_z=0.0)])
def test_against_render_reference(scene):
    W, H, near, far = 64, 48, 0.1, 30.0
    eye, dirs, fwd = rr.camera_rays(6.0, 30.0, -20.0, 50.0, W, H, (0, 0, 1.0))
    seg, depth, _, sm, _ = rr.render(scene, I3, Z3, eye, dirs, near, far)
    D = dirs.reshape(-1, 3)
    f, lab, pos, nrm, mg, _ = ry.cast(scene, I3, Z3, np.tile(eye, (len(D), 1)), eye + far * D)
    ok = (sm.reshape(-1) > 1e-9) & (mg > 1e-9)
    assert ok.mean() > 0.95 and (depth > near).all()           # (nothing nearer than `near`: the two rules coincide)
    assert (lab[ok] == seg.reshape(-1)[ok]).all()
    np.testing.assert_allclose((f * far)[ok], depth.reshape(-1)[ok], rtol=1e-9)


def _poses(oracle64, state):
    s = oracle64.new_state()
    oracle64.reset(s)
    if state is not None:
        oracle64.set_state(s, state)
    pos, rot = oracle64.body_poses(s)
    return rot, pos, oracle64.get_state(s)[:3]


@pytest.mark.parametrize("collision", ["hulls", "primitives"])
def test_committed_ray_sets_stay_under_the_marginal_cap(oracle64, collision):
    model = _capi.Model()
    if collision == "primitives":
        model.use_primitive_collision(0.2)
    scene = ry.Scene.from_model(model)
    names = [n for n, _ in model.links()]
    lb, ltf = model.array("link_body").astype(int), model.array("link_tf").reshape(-1, 12)
    states = [None, GOLD["random_state"][20], GOLD["random_state"][40], GOLD["crouch_state"][60], GOLD["zero_state"][40]]
    for k, st in enumerate(states):
        R, p, base = _poses(oracle64, st)

        def frame(name):
            l = names.index(name)
            Rl = R[lb[l]] @ ltf[l, :9].reshape(3, 3)
            return Rl, p[lb[l]] + R[lb[l]] @ ltf[l, 9:]
        cases = {"random": ry.random_segments(1, 300, base[None], seed=k)[0].astype(np.float64),
                 "fan": np.concatenate(ry.to_world(ry.head_fan(), *frame(ry.HEAD_LINK)), 1),
                 "single": np.concatenate(ry.to_world(ry.single_ray(), *frame(ry.BASE_LINK)), 1)}
        for foot in ry.FOOT_LINKS:
            cases[foot] = np.concatenate(ry.to_world(ry.foot_rays(), *frame(foot)), 1)
        for name, rays in cases.items():
            f, lab, _, _, mg, _ = ry.cast(scene, R, p, rays[:, :3], rays[:, 3:])
            share = (mg < ry.MARGIN).mean()
            assert share <= ry.MARGINAL_CAP, (collision, k, name, share)
            if name == "random":
                assert (lab >= 0).sum() >= 5 and (lab == ry.FLOOR).sum() == 0 and (lab == ry.MISS).sum() > 100
            if name == "fan" or name in ry.FOOT_LINKS:
                assert (lab != ry.MISS).any(), (collision, k, name)
