"""The renderer (trex_batch_render: csrc/render.hip, render.cpp, the argument path of capi_queries.cpp) at the edges of its tiling, culling
and clipping, and the pose pass it shares with the ray casts (csrc/render_pose.h) on generated models with bent joints. The cases
are tests/render_cases.py, qualified on the reference alone by tests/test_render_cases_host.py. What each test reaches:

  test_parity_over_the_cases        ragged, sub-tile and one-pixel-wide frames, 4096 x 1 and 1 x 4096 (x1 = min(..., width), `valid`,
                                    best = -1 of an invalid lane, the cull frustum of a partial tile, tan_x / tan_y = 4096 and its
                                    inverse); the near plane through hulls and spheres (pl < 0, te = near_z, cz > near_z - r); the
                                    eye inside a hull / a sphere; the eye below the floor (tf = near_z); a far plane that crops
                                    (best = far_z, cz < far_z + r); fov 150 and 5, pitch -90, grazing floor rays; a base 64 m from
                                    the origin - against the f64 reference caster, and how many pixels the comparison keeps
  test_exact_answers_bitwise        below_floor, all_sky, inside: the one answer every pixel must have
  test_output_subsets               the three nullable outputs, one, two and three at a time
  test_no_write_outside_the_image   ragged frames write no byte before or behind [V, H, W]
  test_views_grow_and_reuse         render_ids through grow, reuse and NULL (capi_queries.cpp: sync, free, reallocate)
  test_generated_models_bent        render_pose.h at tree depth 6, oblique non-unit axes, rpy on joint origins, 4 children; hulls
                                    with a dense faceted underside
  test_ray_cast_on_bent_models      the same pose pass and primitive table under trex_batch_ray_test

Tolerances: those of render_compare and ray_compare (tests/gpu_render_support.py), unchanged. On top of them, the
share of pixels the rgb comparison uses is bounded from below (render_cases.RGB_USED_MIN), and the rgb margin of a floor pixel is
reduced by the f32 resolution of its hit point (render_cases.condition): both only take pixels OUT of what may pass unseen.
The reference sees the poses the kernel's own state gives, read back through link_transforms (as everywhere in the renderer's
tests). Figures measured on an MI355X: profiles/r06_render.txt.

What the cases found (fixed in render.hip): with poses and eye in world coordinates, the close view of the state 64 m from the
origin missed the depth tolerance on sphere collision (1.43e-4 relative; 6.4e-5 on the hulls) - the kernel now works relative
to the env's base position (8.6e-5 and 1.9e-5, the rest being the f32 rounding of the poses the reference is given)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_ref as ry  # noqa: E402
import render_cases as rc  # noqa: E402
import render_ref as rr  # noqa: E402
import synthetic_models as sm  # noqa: E402
from gpu_render_support import (ray_cast, ray_compare, ray_flat, ray_poses, ray_reference, ray_world, render_all,  # noqa: E402
                                render_compare, render_reference)
from gpu_support import DEV  # noqa: E402

from trex_gym.vec_env import TrexVecEnv  # noqa: E402

pytestmark = pytest.mark.gpu


def _body_poses(env):
    """per env (R [nb, 3, 3], p [nb, 3]) from link_transforms, as render_reference does"""
    lt = env.link_transforms().cpu().numpy()
    lb, ltf = env.model.array("link_body"), env.model.array("link_tf")
    return [rr.body_poses(lt[e], lb, ltf, env.model.num_bodies) for e in range(env.num_envs)]


@pytest.fixture(scope="module")
def trex(oracle64):
    """collision -> (env of the five states, scene, body poses): made on first use, shared, never changed (render only reads)"""
    states = torch.tensor(rc.trex_states(oracle64))
    made = {}

    def get(collision):
        if collision not in made:
            env = TrexVecEnv(len(states), device=DEV, collision=collision)
            env.reset_tensor()
            env.set_state(states)
            torch.cuda.synchronize()
            made[collision] = (env, rr.Scene.from_model(env.model), _body_poses(env))
        return made[collision]
    yield get
    for env, _, _ in made.values():
        env.close()


def _calls(cam, poses):
    """[(env ids, Camera)] that render every env with the case's camera: one call, or one per env if the target is anchored"""
    if rc.anchored(cam):
        return [([k], rc.resolve(cam, *poses[k])) for k in range(len(poses))]
    return [(list(range(len(poses))), rc.resolve(cam))]


def _conditioned(env, refs, c, W, H, ids):
    """the references of render_reference with the rgb margin of floor pixels reduced by the f32 resolution of the hit point
    (render_cases.condition): far out on the floor f32 cannot tell which checker square a point lies in"""
    base = env.get_state()[:, :3].cpu().numpy()
    return [rc.condition(r, *rc.view_rays(c, W, H, base[e])) for r, e in zip(refs, ids)]


def _figures(gpu, ref):
    """what render_compare looks at, as numbers: (pixels, share left out by seg margin, share left out by rgb margin, label agreement,
    worst relative depth error, worst rgb difference, share of pixels the rgb comparison uses)"""
    rgb, dep, seg = gpu
    rseg, rdep, rrgb, smg, rmg = ref
    agree = seg == rseg
    ok = agree & (smg >= 1e-4)
    okc = ok & (rmg >= 1e-4)
    rel = (np.abs(dep[ok] - rdep[ok]) / np.maximum(rdep[ok], 1e-6)).max() if ok.any() else 0.0
    diff = np.abs(rgb[okc].astype(int) - rrgb[okc].astype(int)).max() if okc.any() else 0
    return seg.size, (smg < 1e-4).mean(), (rmg < 1e-4).mean(), agree.mean(), rel, diff, okc.mean()


def _check_view(gpu, ref, what, rgb_used=True):
    f = _figures(gpu, ref)
    print("render %s: pixels %d out by seg margin %.4f by rgb margin %.4f agree %.4f depth rel %.2e rgb diff %d rgb used %.4f"
          % ((what,) + f))
    render_compare(gpu, ref, what)
    if rgb_used and f[0] >= rc.RGB_PIXELS:
        # the rgb comparison of render_compare skips what it cannot judge; it must not skip its way to a pass
        assert f[6] >= rc.RGB_USED_MIN, (what, f[6])


# a ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collision,name", [("hulls", n) for n in rc.CAMERAS] + [("primitives", n) for n in rc.PRIMITIVE_CAMERAS])
def test_parity_over_the_cases(collision, name, trex):
    env, scene, poses = trex(collision)
    for (W, H) in rc.frames(name):
        cam = rc.case_camera(name, collision, (W, H))
        for ids, c in _calls(cam, poses):
            rgb, dep, seg = render_all(env, c, W, H, ids)
            assert rgb.shape == (len(ids), H, W, 3) and dep.shape == seg.shape == (len(ids), H, W)
            refs = _conditioned(env, render_reference(env, scene, c, W, H, ids), c, W, H, ids)
            for j, k in enumerate(ids):
                what = (collision, name, W, H, rc.STATE_NAMES[k])
                _check_view((rgb[j], dep[j], seg[j]), refs[j], what)
                rc.paths_reached(name, cam, W, H, seg[j], dep[j], k)       # on the GPU's own picture


# b ------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["below_floor", "all_sky", "inside"])
def test_exact_answers_bitwise(name, trex):
    env, scene, poses = trex("hulls")
    cam = rc.case_camera(name)
    near, far = np.float32(cam[4]), np.float32(cam[5])
    for (W, H) in rc.EXACT_FRAMES:
        rgb, dep, seg = render_all(env, rc.resolve(cam), W, H)
        if name == "below_floor":
            assert (seg == -1).all() and (_bits(dep) == _bits(near)).all()
        elif name == "all_sky":
            assert (seg == -2).all() and (_bits(dep) == _bits(far)).all()
            assert (rgb == np.array(rc.SKY_RGB, np.uint8)).all()
        else:
            for e in range(env.num_envs):
                assert seg[e].min() == seg[e].max() >= 0, (W, H, e)
            assert (seg == seg[0, 0, 0]).all()                              # the same body - the pelvis - in every state
            assert (_bits(dep) == _bits(near)).all()


# c ------------------------------------------------------------------------------------------------------------------------
def test_output_subsets(trex):
    env, _, _ = trex("hulls")
    W, H = 33, 41
    cam = rc.resolve(rc.case_camera("near_cuts", "hulls", (W, H)))
    V = env.num_envs
    make = dict(rgb=lambda: torch.full((V, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV),
                depth=lambda: torch.full((V, H, W), float("nan"), device=DEV),
                seg=lambda: torch.full((V, H, W), 0x7FFFFFFF, dtype=torch.int32, device=DEV))
    full = {k: f() for k, f in make.items()}
    env.batch.render(cam, W, H, None, **full)
    want = {k: t.cpu().numpy().tobytes() for k, t in full.items()}
    assert (full["seg"] >= 0).any() and torch.isfinite(full["depth"]).all()
    for subset in (("rgb",), ("depth",), ("seg",), ("rgb", "depth"), ("rgb", "seg"), ("depth", "seg")):
        out = {k: make[k]() for k in subset}
        env.batch.render(cam, W, H, None, **out)
        for k, t in out.items():
            assert t.cpu().numpy().tobytes() == want[k], (subset, k)


# d ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(17, 15), (1, 40), (15, 1)])
def test_no_write_outside_the_image(W, H, trex):
    """Every output is the middle of a larger tensor of ONE allocation, sentinel bytes before and behind it: the padding is the
    test's own memory, so an overrun shows as a changed sentinel."""
    env, _, _ = trex("hulls")
    ids, V, PAD, SENT = [4, 0, 2], 3, 8192, 0xA5
    cam = rc.resolve(rc.case_camera("near_cuts", "hulls", (W, H)))
    ordinary = {k: t.cpu().numpy().tobytes() for k, t in zip(("rgb", "depth", "seg"), env.render_tensor(ids, W, H, cam, True, True))}
    size = dict(rgb=3, depth=4, seg=4)
    dtype = dict(rgb=torch.uint8, depth=torch.float32, seg=torch.int32)
    big = {k: torch.full((PAD + V * H * W * size[k] + PAD,), SENT, dtype=torch.uint8, device=DEV) for k in size}
    mid = {k: big[k][PAD:PAD + V * H * W * size[k]].view(dtype[k]).view((V, H, W, 3) if k == "rgb" else (V, H, W)) for k in size}
    for k in size:
        assert mid[k].data_ptr() == big[k].data_ptr() + PAD and mid[k].is_contiguous()
    env.batch.render(cam, W, H, ids, **mid)
    torch.cuda.synchronize()
    for k in size:
        b = big[k].cpu().numpy()
        assert (b[:PAD] == SENT).all() and (b[-PAD:] == SENT).all(), (k, W, H)
        assert b[PAD:-PAD].tobytes() == ordinary[k], (k, W, H)


# e ------------------------------------------------------------------------------------------------------------------------
def test_views_grow_and_reuse(oracle64):
    """ONE batch of 3 envs; env_ids of 2, then 70 (the id buffer grows: synchronise, free, reallocate), then 5 (reused, larger
    than needed), then NULL: every view is, bytes for bytes, the row of its env in the all-env render."""
    env = TrexVecEnv(3, device=DEV)
    env.reset_tensor()
    env.set_state(torch.tensor(rc.trex_states(oracle64)[:3]))
    W, H = 17, 15
    cam = rc.resolve(rc.case_camera("far_view", "hulls", (W, H)))
    lists = [[2, 0], [(k * k + k // 7) % 3 for k in range(70)], [1, 1, 2, 0, 1]]
    assert set(lists[1]) == {0, 1, 2} and any(a == b for a, b in zip(lists[1], lists[1][1:]))
    got = [render_all(env, cam, W, H, ids) for ids in lists]
    every = render_all(env, cam, W, H, None)
    assert every[0].shape == (3, H, W, 3)
    assert not (every[2][0] == every[2][1]).all()                          # the envs' pictures differ
    for ids, g in zip(lists, got):
        for x, y in zip(g, every):
            assert x.shape[0] == len(ids) and x.tobytes() == y[ids].tobytes(), len(ids)
    env.close()


# f, g ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """name -> dict(env of the model's two states (sampled, bent), scene, cameras, om): built once, shared, never changed"""
    out = {}

    def get(name):
        if name not in out:
            path, props, om = sm.compile_both(name, tmp_path_factory.mktemp(name))
            states = rc.synth_states(name, om, sm.state_set(name, om, props["params"])["states"])
            env = TrexVecEnv(2, urdf_path=path, device=DEV, params=props["params"])
            env.reset_tensor()
            env.set_state(torch.tensor(states))
            torch.cuda.synchronize()
            out[name] = dict(env=env, om=om, scene=rr.Scene.from_model(env.model), cams=rc.synth_cameras(name, om))
        return out[name]
    yield get
    for m in out.values():
        m["env"].close()


@pytest.mark.parametrize("name", rc.SYNTH_MODELS)
def test_generated_models_bent(name, synth):
    """render_compare on both states and both cameras. The rgb-share condition of test_parity_over_the_cases does not apply: the
    jittered undersides of big_body and full_masks are many nearly coplanar facets, and up to 40 % of their pixels lie within
    1e-4 m of an edge between two of them (the rgb comparison leaves those out; seg and depth are compared on all of them)."""
    m = synth(name)
    env, om = m["env"], m["om"]
    W, H = rc.SYNTH_FRAME
    poses = _body_poses(env)
    hulled = {b for b in range(om["nb"]) if om["hull_start"][b + 1] > om["hull_start"][b]}
    for cname, cam in m["cams"].items():
        for ids, c in _calls(cam, poses):
            rgb, dep, seg = render_all(env, c, W, H, ids)
            refs = _conditioned(env, render_reference(env, m["scene"], c, W, H, ids), c, W, H, ids)
            for j, e in enumerate(ids):
                what = (name, cname, ("sampled", "bent")[e])
                _check_view((rgb[j], dep[j], seg[j]), refs[j], what, rgb_used=False)
                labels = set(seg[j][seg[j] >= 0])
                assert labels <= hulled, what
                if cname == "close":
                    assert ((seg[j] >= 0) & (_bits(dep[j]) == _bits(np.float32(cam[4])))).sum() >= 20, what
                if cname == "outside" and e == 1:
                    assert len(labels) >= rc.SYNTH_LABELS.get(name, 2), (what, sorted(labels))
                    if name == "deep_chain":
                        assert labels == hulled, (what, sorted(labels))


@pytest.mark.parametrize("name", ["deep_chain", "bushy"])
def test_ray_cast_on_bent_models(name, synth):
    """trex_batch_ray_test runs the same pose pass: random segments around the base of both states against tests/ray_ref.py, by
    the comparison of tests/test_gpu_ray_test.py."""
    m = synth(name)
    env = m["env"]
    scene, poses = ry.Scene.from_model(env.model), ray_poses(env)
    base = env.get_state()[:, :3].cpu().numpy()
    rays = rc.synth_segments(base, rc.synth_extent(m["om"]))
    gpu = ray_cast(env, rays)
    ref = ray_reference(scene, poses, ray_world(env, poses, rays, None))
    ray_compare(ray_flat(gpu), ref, (name, "bent and sampled"))
    assert (gpu[1][1] >= 0).sum() >= rc.SYNTH_RAY_HITS, (gpu[1][1] >= 0).sum()        # the bent state's bodies are hit
