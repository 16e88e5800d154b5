"""Batched ray casts on the GPU (trex_batch_ray_test, include/trex_batch.h): parity with the numpy f64 segment caster of
tests/ray_ref.py and with the renderer, the analytic floor, frames, masks, the origin-inside rule, bad rays, the tiling of rays
onto workgroups, determinism, no side effects, stream capture, argument checks, scale and the pybullet facade."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_ref as ry  # noqa: E402
import render_ref as rr  # noqa: E402
from gpu_render_support import ray_cast, ray_compare, ray_flat, ray_poses, ray_reference, ray_world  # noqa: E402
from gpu_support import random_steps  # noqa: E402

from trex_gym import _capi, sensors  # noqa: E402
from trex_gym.render import Camera  # noqa: E402
from trex_gym.vec_env import TrexVecEnv  # noqa: E402

pytestmark = pytest.mark.gpu

N = 8
CAMERA = Camera(distance=6.0, yaw=30.0, pitch=-20.0, fov=50.0, target=(0.0, 0.0, 1.5))   # CAMERAS[1] of test_gpu_render.py


def _link(env, name):
    return [n for n, _ in env.model.links()].index(name)


def _case(env, scene, poses, rays, link_name, what, **kw):
    link = None if link_name is None else _link(env, link_name)
    gpu = ray_cast(env, rays, link_name, **kw)
    ref = ray_reference(scene, poses, ray_world(env, poses, rays, link))
    ray_compare(ray_flat(gpu), ref, what)
    return gpu


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collision", ["hulls", "primitives"])
def test_parity_with_reference(collision):
    env = TrexVecEnv(N, device="cuda:0", collision=collision)
    scene = ry.Scene.from_model(env.model)
    env.reset_tensor()
    hit_bodies = 0
    for phase in ("reset", "30 steps"):
        if phase != "reset":
            random_steps(env, 30)
        torch.cuda.synchronize()
        poses = ray_poses(env)
        base = env.get_state()[:, :3].cpu().numpy()
        g = _case(env, scene, poses, ry.random_segments(N, 300, base), None, (collision, phase, "a: random"))
        hit_bodies += int((g[1] >= 0).sum())
        g = _case(env, scene, poses, ry.head_fan(), ry.HEAD_LINK, (collision, phase, "b: head fan"))
        hit_bodies += int((g[1] >= 0).sum())
        for foot in ry.FOOT_LINKS:
            g = _case(env, scene, poses, ry.foot_rays(), foot, (collision, phase, "c: " + foot))
            assert (g[1] != -2).any()
        _case(env, scene, poses, ry.single_ray(), ry.BASE_LINK, (collision, phase, "d: single"))
    assert hit_bodies > 100
    env.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_against_the_renderer():
    env = TrexVecEnv(N, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 10)
    W, H, cam = 32, 24, CAMERA
    _, dep, seg = env.render_tensor(None, W, H, cam, depth=True, segmentation=True)
    dep, seg = dep.cpu().numpy().reshape(N, -1), seg.cpu().numpy().reshape(N, -1)
    eye, dirs, fwd = rr.camera_rays(cam.distance, cam.yaw, cam.pitch, cam.fov, W, H, cam.target)
    D = dirs.reshape(-1, 3)
    rays = np.concatenate([np.tile(eye, (len(D), 1)), eye + cam.far * D], 1).astype(np.float32)
    frac, body, _, _ = ray_cast(env, rays)
    scene, poses = ry.Scene.from_model(env.model), ray_poses(env)
    r64 = rays.astype(np.float64)
    mg = ray_reference(scene, poses, {e: (r64[:, :3], r64[:, 3:]) for e in range(N)})[4].reshape(N, -1)
    length = np.linalg.norm(r64[:, 3:] - r64[:, :3], axis=1)
    along = (r64[:, 3:] - r64[:, :3]) @ fwd / length          # dir . fwd of the unit direction
    depth = frac * length * along                             # eye-space depth of the ray's hit
    use = (mg >= ry.MARGIN) & (dep > cam.near * (1 + 1e-3))   # pixels nearer than `near` are the renderer's cut, not a hit
    assert use.mean() > 0.9 and (seg[use] >= 0).any() and (seg[use] == -1).any()
    assert (body[use] == seg[use]).all()
    err = np.abs(depth - dep)[use] / (1e-4 * np.maximum(dep[use], 1.0))
    print("ray_test against the renderer: pixels %d used %.4f depth err/bound %.3f" % (use.size, use.mean(), err.max()))
    assert err.max() <= 1.0
    env.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_floor_analytic():
    env = TrexVecEnv(N, device="cuda:0")
    env.reset_tensor()
    fz = np.float32(env.model.get_param("floor_z"))
    z0 = np.array([0.5, 1.0, 2.75, 10.0, 0.125, 3.0, fz + 1, 7.5], np.float32)
    z1 = np.array([-0.5, 0.0, -1.0, -30.0, 0.0, fz - 0.25, fz, -0.001], np.float32)
    dx = np.array([0.0, 0.0, 3.0, -20.0, 0.5, 0.0, 1.0, 4.0], np.float32)
    rays = np.stack([dx * 0 + 7, dx * 0 - 4, z0, 7 + dx, -4 + 0.5 * dx, z1], 1).astype(np.float32)
    frac, body, pos, nrm = ray_cast(env, rays, bodies=[])
    want = (z0.astype(np.float64) - float(fz)) / (z0.astype(np.float64) - z1.astype(np.float64))
    assert (body == -1).all()
    assert np.abs(frac / want - 1).max() <= 1e-6, np.abs(frac / want - 1).max()
    assert (nrm == np.array([0, 0, 1], np.float32)).all()
    np.testing.assert_allclose(pos[..., 2], float(fz), atol=1e-5)
    # from below the floor, and rays that end above it: misses
    below = rays.copy()
    below[:, 2], below[:, 5] = fz - 0.5, fz - 2.0
    up = rays.copy()
    up[:, 5] = fz + 0.01
    for r in (below, up):
        frac, body, pos, nrm = ray_cast(env, r, bodies=[])
        assert (body == -2).all() and (frac == 1.0).all() and (nrm == 0).all()
        np.testing.assert_array_equal(pos, np.broadcast_to(r[:, 3:], pos.shape))
    # nothing may be hit at all: the miss encoding everywhere
    frac, body, pos, nrm = ray_cast(env, rays, bodies=[], floor=False)
    assert (body == -2).all() and (frac == 1.0).all() and (nrm == 0).all()
    env.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_link_frame_equals_world_frame():
    env = TrexVecEnv(N, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 20)
    scene, poses = ry.Scene.from_model(env.model), ray_poses(env)
    for name, rays in ((ry.BASE_LINK, ry.single_ray()), (ry.HEAD_LINK, ry.head_fan()), (ry.FOOT_LINKS[0], ry.foot_rays())):
        link = _link(env, name)
        g_link = ray_cast(env, rays, name)
        world = ray_world(env, poses, rays, link)
        wr = np.stack([np.concatenate(world[e], 1) for e in range(N)]).astype(np.float32)
        g_world = ray_cast(env, wr)
        ref = ray_reference(scene, poses, world)
        ray_compare(ray_flat(g_link), ref, ("link frame", name))
        ray_compare(ray_flat(g_world), ref, ("world frame", name))
    env.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_shared_equals_per_env_bitwise():
    env = TrexVecEnv(N, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 5)
    for name, rays in ((ry.HEAD_LINK, ry.head_fan()), (None, ry.random_segments(1, 300, [[0, 0, 0]])[0])):
        a = ray_cast(env, rays, name)
        b = ray_cast(env, np.broadcast_to(rays, (N,) + rays.shape).copy(), name)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    env.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_body_mask():
    env = TrexVecEnv(N, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 5)
    rays = ry.random_segments(N, 300, env.get_state()[:, :3].cpu().numpy(), seed=3)
    full = ray_cast(env, rays)
    hit = np.bincount(full[1][full[1] >= 0], minlength=env.model.num_bodies)
    b = int(np.argmax(hit))
    assert hit[b] > 0
    part = ray_cast(env, rays, bodies=[k for k in range(env.model.num_bodies) if k != b])
    assert (part[1] != b).all()
    keep = full[1] != b
    for x, y in zip(full, part):
        assert x[keep].tobytes() == y[keep].tobytes()
    env.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collision", ["hulls", "primitives"])
def test_origin_inside(collision):
    env = TrexVecEnv(N, device="cuda:0", collision=collision)
    env.reset_tensor()
    scene, poses = ry.Scene.from_model(env.model), ray_poses(env)
    R, p = poses[0][:2]
    checked = 0
    for k, prim in enumerate(scene.prims):
        body = prim[1]
        if prim[0] == "hull":
            _, _, n, d, c, _ = prim
            if (n @ c - d).max() > -1e-3:
                continue                                        # (the bounding sphere's centre is not well inside the hull)
            length = 5.0
        else:
            c, length = prim[2], 0.9 * prim[3]                  # (the ray stays inside the sphere)
        cw = R[body] @ c + p[body]
        rays = np.concatenate([cw, cw + [0.0, 0.0, length]])[None].astype(np.float32)
        # the reference, over the body's primitives alone: inside this one, and none of the body's others is entered
        _, rl, _, _, mg, _ = ry.cast(scene, R, p, rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64),
                                     body_mask=1 << body, hit_floor=False)
        if rl[0] != -2 or mg[0] < 1e-3:
            continue
        frac, lab, _, _ = ray_cast(env, rays, bodies=[body], floor=False)
        assert lab[0, 0] == -2 and frac[0, 0] == 1.0, (k, body)
        checked += 1
        if checked == 6:
            break
    assert checked >= 3
    env.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_bad_rays():
    env = TrexVecEnv(N, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 5)
    good = ry.random_segments(N, 96, env.get_state()[:, :3].cpu().numpy(), seed=5)
    ref = ray_cast(env, good)
    mixed = np.repeat(good, 2, axis=1)                          # lane by lane: good, bad, good, bad ...
    bad = mixed[:, 1::2]
    kinds = np.arange(bad.shape[1]) % 4
    bad[:, kinds == 0, 0] = np.nan
    bad[:, kinds == 1, 4] = np.inf
    bad[:, kinds == 2, 3:] = bad[:, kinds == 2, :3]             # zero length
    bad[:, kinds == 3, :] = -np.inf
    out = ray_cast(env, mixed)
    for x, y in zip(ref, out):
        assert x.tobytes() == np.ascontiguousarray(y[:, 0::2]).tobytes()
    assert (out[0][:, 1::2] == 1.0).all() and (out[1][:, 1::2] == -2).all() and (out[3][:, 1::2] == 0).all()
    env.step_tensor(torch.zeros(N, env.J, device=env.device))
    assert torch.isfinite(env.obs).all()
    env.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 33])
def test_tiling_edges(n):
    """A workgroup of 256 lanes holds min(8, 256 // R) whole envs for R < 256 and one 256-ray chunk of one env from R = 256
    (raycast.h: trex_ray_shape). R = 1, 3: 8 envs (the cap); 31, 32, 33: 8, 8, 7 envs; 63, 64, 65: 4, 4, 3; 85, 86: 3, 2;
    128, 129: 2, 1; 255, 256, 257: one env in 1, 1, 2 workgroups; n = 1, 5, 33 leave the last workgroup partly filled."""
    env = TrexVecEnv(n, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 3)
    dev = env.device
    state = env.get_state()
    base = state[:, :3].cpu().numpy()
    G = 64
    sets, got = {}, {}
    for R in (1, 3, 31, 32, 33, 63, 64, 65, 85, 86, 128, 129, 255, 256, 257):
        rays = ry.random_segments(n, R, base, seed=R)
        rays[:, :, 5] = np.where(np.arange(R) % 3 == 0, -0.5, rays[:, :, 5])     # (some reach the floor)
        bufs = [torch.full((n * R * k + G,), float("nan"), device=dev) for k in (1, 3, 3)]
        lab = torch.full((n * R + G,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
        view = lambda t, *s: t[:n * R * (s[0] if s else 1)].view(n, R, *s)
        env.batch.ray_test(torch.as_tensor(rays).to(dev), -1, None, 0xFFFFFFFF, True, view(bufs[0]), view(lab), view(bufs[1], 3),
                           view(bufs[2], 3))
        torch.cuda.synchronize()
        for t, k in zip(bufs, (1, 3, 3)):
            assert torch.isfinite(t[:n * R * k]).all() and torch.isnan(t[n * R * k:]).all(), (n, R)
        assert (lab[n * R:] == 0x7FFFFFFF).all() and (lab[:n * R] >= -2).all() and (lab[:n * R] < env.model.num_bodies).all()
        sets[R] = rays
        got[R] = [view(bufs[0]).cpu().numpy(), view(lab).cpu().numpy(), view(bufs[1], 3).cpu().numpy(), view(bufs[2], 3).cpu().numpy()]
    assert all((np.concatenate([g[1].ravel() for g in got.values()]) == k).any() for k in (-2, -1)) and \
        any((g[1] >= 0).any() for g in got.values())
    # every shape, every env, ray by ray: bitwise the same as the env alone in a batch of one, in chunks of 64 rays
    one = TrexVecEnv(1, device="cuda:0")
    one.reset_tensor()
    for e in range(n):
        one.set_state(state[e:e + 1])
        for R, rays in sets.items():
            for r0 in range(0, R, 64):
                part = ray_cast(one, rays[e:e + 1, r0:r0 + 64])
                for x, y in zip(got[R], part):
                    assert np.ascontiguousarray(x[e, r0:r0 + 64]).tobytes() == y[0].tobytes(), (n, R, e, r0)
    one.close()
    env.close()


# 10 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,params,sensor", [(64, None, False), (33, None, True), (64, {"warmstart": 0.85}, True)])
def test_determinism_and_no_side_effects(n, params, sensor):
    envs = [TrexVecEnv(n, device="cuda:0", params=params) for _ in range(2)]
    for e in envs:
        if sensor:
            e.enable_contact_sensor(True)
        e.reset_tensor()
        random_steps(e, 5, seed=1)
    before = envs[0].get_state().clone()
    wrench = envs[0].contact_wrench().clone() if sensor else None
    rays = ry.random_segments(n, 40, before[:, :3].cpu().numpy(), seed=2)
    a = ray_cast(envs[0], rays)
    b = ray_cast(envs[0], rays)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    ray_cast(envs[0], ry.head_fan(), ry.HEAD_LINK)
    assert envs[0].get_state().cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    if sensor:
        assert envs[0].contact_wrench().cpu().numpy().tobytes() == wrench.cpu().numpy().tobytes()
    assert (envs[0].episode_steps == envs[1].episode_steps).all()
    act = torch.rand(n, envs[0].J, generator=torch.Generator().manual_seed(5))
    lo, hi = torch.tensor(envs[0].model.lower, dtype=torch.float32), torch.tensor(envs[0].model.upper, dtype=torch.float32)
    act = (lo + (hi - lo) * act).to(envs[0].device)
    rows = []
    for e in envs:       # (the warm-start record is private: the next steps of the two batches agree only if it was left alone)
        for _ in range(2):
            e.step_tensor(act)
        rows.append(e.rows.cpu().numpy())
    assert rows[0].tobytes() == rows[1].tobytes()
    if sensor:
        assert envs[0].contact_wrench().cpu().numpy().tobytes() == envs[1].contact_wrench().cpu().numpy().tobytes()
    for e in envs:
        e.close()


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_stream_capture():
    env = TrexVecEnv(N, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 5)
    dev = env.device
    rays = torch.as_tensor(ry.head_fan()).to(dev)
    link = _link(env, ry.HEAD_LINK)
    R = rays.shape[0]
    mk = lambda: (torch.empty(N, R, device=dev), torch.empty(N, R, dtype=torch.int32, device=dev), torch.empty(N, R, 3, device=dev),
                  torch.empty(N, R, 3, device=dev))
    outs = mk()
    env.batch.ray_test(rays, link, None, 0xFFFFFFFF, True, *outs)      # the first call: makes the table, learns the buffers
    eager = [o.clone() for o in outs]
    assert (eager[1] >= -1).any()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            env.batch.ray_test(rays, link, None, 0xFFFFFFFF, True, *outs)    # the second call: one launch, one linear chain
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for o, want in zip(outs, eager):
        assert o.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    del graph
    env.close()


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    env = TrexVecEnv(4, device="cuda:0")
    env.reset_tensor()
    dev = env.device
    rays = torch.zeros(4, 16, 6, device=dev)
    rays[..., 2], rays[..., 5] = 3.0, -1.0
    frac = torch.empty(4, 16, device=dev)
    nl = len(env.model.links())
    bad = [
        dict(rays=torch.zeros(4, 0, 6, device=dev)),                                            # num_rays 0
        dict(rays=torch.zeros(16385, 6, device=dev)),                                           # num_rays 16385
        dict(rays=rays, link=nl), dict(rays=rays, link=-2),
        dict(rays=rays.cpu()),                                                                  # host memory
        dict(rays=rays, fraction=torch.empty(4, 16)),
        dict(rays=rays.double()), dict(rays=rays, body=torch.empty(4, 16, device=dev)),         # dtypes
        dict(rays=rays, fraction=torch.empty(4, 15, device=dev)),                               # shapes
        dict(rays=rays, position=torch.empty(4, 16, device=dev)), dict(rays=rays, normal=torch.empty(4, 16, 2, device=dev)),
        dict(rays=torch.zeros(3, 16, 6, device=dev)), dict(rays=torch.zeros(16, 5, device=dev)),
        dict(rays=rays, body_mask=1 << 32),
    ]
    for kw in bad:
        with pytest.raises(_capi.TrexError) as ei:
            env.batch.ray_test(kw.pop("rays"), **kw)
        assert ei.value.code == _capi.E_INVALID, kw
    # the raw C-ABI refuses by itself: null pointers and the ranges ...
    L, p = _capi.lib.trex_batch_ray_test, lambda t: C.c_void_p(t.data_ptr())
    h = env.batch.h
    for args in ((None, 16, 0, -1, 0xFFFFFFFF, 1, p(frac), None, None, None),
                 (p(rays), 16, 0, -1, 0xFFFFFFFF, 1, None, None, None, None),
                 (p(rays), 0, 0, -1, 0xFFFFFFFF, 1, p(frac), None, None, None),
                 (p(rays), 16385, 0, -1, 0xFFFFFFFF, 1, p(frac), None, None, None),
                 (p(rays), 16, 0, nl, 0xFFFFFFFF, 1, p(frac), None, None, None),
                 (p(rays), 16, 0, -2, 0xFFFFFFFF, 1, p(frac), None, None, None)):
        assert L(h, *args, None) == _capi.E_INVALID, args
    # ... and buffers shorter than the call needs (the binding's own check bypassed). On 4 096 envs x 16 384 rays every buffer
    # of the call is 268 MB or more - more than the allocation a small tensor lives in, whatever the allocator pooled around it
    big = TrexVecEnv(4096, device="cuda:0")
    big.reset_tensor()
    short = torch.empty(100, device=dev)
    pattern = torch.zeros(16384, 6, device=dev)
    for args in ((p(short), 16384, 0, -1, 0xFFFFFFFF, 1, p(short), None, None, None),           # short per-env rays
                 (p(short), 16384, 1, -1, 0xFFFFFFFF, 1, p(short), None, None, None),           # short shared rays
                 (p(pattern), 16384, 1, -1, 0xFFFFFFFF, 1, p(short), None, None, None),         # short fraction
                 (p(pattern), 16384, 1, -1, 0, 0, p(short), p(short), p(short), p(short))):     # short everything
        assert L(big.batch.h, *args, None) == _capi.E_INVALID, args
    big.step_tensor(torch.zeros(4096, big.J, device=dev))
    torch.cuda.synchronize()
    assert torch.isfinite(big.obs).all()
    big.close()
    # the batch keeps casting and stepping
    env.batch.ray_test(rays, fraction=frac)
    env.step_tensor(torch.zeros(4, env.J, device=dev))
    torch.cuda.synchronize()
    assert (frac < 1).all() and torch.isfinite(env.obs).all()
    env.close()


# 13 -----------------------------------------------------------------------------------------------------------------------
def test_scale_4096_envs():
    env = TrexVecEnv(4096, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 3)
    ids = [0, 1000, 2047, 4095]
    base = env.get_state()[:, :3].cpu().numpy()
    rays = ry.random_segments(4096, 16, base, seed=7)
    rays[:, 8:, :3] = base[:, None] + np.float32([0.0, 0.0, 2.0])         # half of them start above the base
    rays[:, 8:, 3:5] = base[:, None, :2] + (rays[:, 8:, 3:5] - base[:, None, :2]) * np.float32(0.2)   # and end under the floor,
    rays[:, 8:, 5] = -0.5                                                 # through the body or beside it
    gpu = ray_cast(env, rays)
    assert gpu[0].shape == (4096, 16) and gpu[1].shape == (4096, 16) and gpu[2].shape == gpu[3].shape == (4096, 16, 3)
    poses = ray_poses(env, ids)
    ref = ray_reference(ry.Scene.from_model(env.model), poses, ray_world(env, poses, rays, None))
    frac, body, pos, nrm = ray_flat(gpu, ids)
    ray_compare((frac, body, pos, nrm), ref, "scale")
    assert (gpu[1] >= 0).any() and (gpu[1] == -1).any()
    env.close()


# 14 -----------------------------------------------------------------------------------------------------------------------
def test_facade():
    from trex_gym.trex_env import TrexBulletEnv
    env = TrexBulletEnv()
    x, y, z = env.model.get_base_position()
    # a vertical ray through a point inside a hull (the line through the base's origin passes between the hulls of this
    # robot): the reference names the body it meets first
    scene, (R, p) = ry.Scene.from_model(env._vec.model), ray_poses(env._vec)[0][:2]
    hx, hy, _ = next(R[prim[1]] @ prim[4] + p[prim[1]] for prim in scene.prims
                     if prim[0] == "hull" and (prim[2] @ prim[4] - prim[3]).max() < -1e-2)
    frm = [[hx, hy, z + 5.0], [x + 20.0, y, 2.0], [x + 20.0, y, 2.0]]
    to = [[hx, hy, z - 5.0], [x + 20.0, y, -1.0], [x + 25.0, y, 2.0]]
    f32 = [np.asarray(a, np.float32).astype(np.float64) for a in (frm, to)]
    rf, rl, _, _, mg, _ = ry.cast(scene, R, p, *f32)
    assert rl[0] >= 0 and mg[0] > 1e-3
    out = env.rayTestBatch(frm, to)
    assert len(out) == 3 and all(len(t) == 5 for t in out)
    uid, link, frac, pos, nrm = out[0]
    assert uid == env.ROBOT_ID and 0 < frac < 1 and len(pos) == 3 and len(nrm) == 3
    assert abs(frac - rf[0]) * 10.0 <= 1e-4 * max(rf[0] * 10.0, 1.0)
    obs_order = [int(b) for b in env._vec.model.array("obs_order")]
    want = env.model._revolute_joint_indices[obs_order.index(rl[0])] if rl[0] in obs_order else -1
    assert link == want and (link == -1 or link in env.model._revolute_joint_indices)
    assert abs(np.linalg.norm(nrm) - 1.0) < 1e-5 and nrm[2] > 0
    assert out[1][0] == env.FLOOR_ID and out[1][1] == -1 and out[1][4] == (0.0, 0.0, 1.0)
    assert abs(out[1][2] - (2.0 - scene.floor_z) / 3.0) < 1e-6
    assert out[2] == (-1, -1, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    assert env.rayTest(frm[1], to[1]) == [out[1]]
    assert env.rayTestBatch([], []) == []
    # parentLinkIndex: rays in the frame of the link that pybullet's joint index names - the body that joint moves - against
    # the same rays taken to the world on the host
    m = env._vec.model
    foot = dict(m.links())[ry.FOOT_LINKS[0]]
    joint = int(m.urdf_joint_indices[obs_order.index(foot)])
    local = np.concatenate([ry.foot_rays(), ry.head_fan()[::9]]).astype(np.float64)
    wf, wt = ry.to_world(local, R[foot], p[foot])
    _, rl, _, _, mg, _ = ry.cast(scene, R, p, wf.astype(np.float32), wt.astype(np.float32))
    in_link = env.rayTestBatch(local[:, :3], local[:, 3:], parentLinkIndex=joint)
    in_world = env.rayTestBatch(wf, wt)
    length = np.linalg.norm(wt - wf, axis=1)
    use = np.flatnonzero(mg > 1e-3)
    assert len(use) >= 4 and (rl[use] != -2).sum() >= 2
    for k in use:
        (ua, la, fa, pa, na), (ub, lb, fb, pb, nb) = in_link[k], in_world[k]
        bound = 1e-4 * max(fb * length[k], 1.0)
        assert (ua, la) == (ub, lb) and abs(fa - fb) * length[k] <= bound and np.abs(np.subtract(pa, pb)).max() <= bound, k
        assert ua == (-1 if rl[k] == -2 else env.FLOOR_ID if rl[k] == -1 else env.ROBOT_ID)
    with pytest.raises(ValueError):
        env.rayTestBatch(local[:, :3], local[:, 3:], parentLinkIndex=max(m.urdf_joint_indices) + 1000)
    # RaySensor: a height scanner under the base, metres
    vec = env._vec
    sensor = sensors.RaySensor(vec, None, sensors.grid_down((x - 20.5, x - 20.0), (y - 0.5, y + 0.5), 3, 2, top=2.0, length=4.0),
                               bodies=[])
    d = sensor.read()
    assert tuple(d.shape) == (1, 6) and d.device == vec.device
    np.testing.assert_allclose(d.cpu().numpy(), 2.0 - env._vec.model.get_param("floor_z"), rtol=1e-5)
    fan = sensors.fan((0, 0, 0), (-1.0, 1.0), (-0.5, 0.0), 8, 2, 3.0)
    assert tuple(fan.shape) == (16, 6) and fan.dtype == torch.float32
    np.testing.assert_allclose((fan[:, 3:] - fan[:, :3]).norm(dim=1).numpy(), 3.0, rtol=1e-6)
    dist = sensors.RaySensor(vec, ry.HEAD_LINK, fan).read()
    assert tuple(dist.shape) == (1, 16) and (dist > 0).all() and (dist <= 3.0 * (1 + 1e-6)).all()
    env.close()
