"""The batched renderer on the GPU (trex_batch_render, include/trex_batch.h): the single env's rgb_array frame, parity with
the numpy f64 ray caster of tests/render_ref.py, determinism, no side effects on the physics, argument checks, scale."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as rr  # noqa: E402
from gpu_render_support import render_all, render_compare, render_reference  # noqa: E402
from gpu_support import random_steps  # noqa: E402

from trex_gym import _capi  # noqa: E402
from trex_gym.render import Camera  # noqa: E402
from trex_gym.vec_env import TrexVecEnv  # noqa: E402

pytestmark = pytest.mark.gpu

CAMERAS = [Camera(), Camera(distance=6.0, yaw=30.0, pitch=-20.0, fov=50.0, target=(0.0, 0.0, 1.5)),
           Camera(distance=4.0, yaw=200.0, pitch=-60.0, fov=70.0, near=0.5, far=30.0, target=(0.5, -0.3, 1.0))]


def test_single_env_rgb_array_frame():
    from trex_gym.trex_env import TrexBulletEnv
    env = TrexBulletEnv()
    img = env.render('rgb_array')
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (720, 960, 3)
    assert env.render('human').size == 0
    _, _, seg = env._vec.render_tensor([0], 960, 720, Camera(), depth=True, segmentation=True)
    seg = seg[0].cpu().numpy()
    assert (seg >= 0).sum() > 1000 and (seg == -1).sum() > 1000 and (seg == -2).sum() > 1000
    # the frame IS the rgb of that view
    rgb = env._vec.render_tensor([0], 960, 720, Camera())[0].cpu().numpy()
    np.testing.assert_array_equal(img, rgb)
    env.close()


@pytest.mark.parametrize("collision", ["hulls", "primitives"])
def test_parity_with_reference(collision):
    env = TrexVecEnv(8, device="cuda:0", collision=collision)
    scene = rr.Scene.from_model(env.model)
    W, H = 128, 96
    env.reset_tensor()
    for phase in ("reset", "30 steps"):
        if phase != "reset":
            random_steps(env, 30)
        torch.cuda.synchronize()
        for ci, cam in enumerate(CAMERAS):
            rgb, dep, seg = render_all(env, cam, W, H)
            refs = render_reference(env, scene, cam, W, H, range(8))
            for e in range(8):
                render_compare((rgb[e], dep[e], seg[e]), refs[e], (collision, phase, ci, e))
            assert (seg >= 0).any()
    env.close()


def test_determinism_and_view_selection():
    env = TrexVecEnv(8, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 10)
    a = render_all(env, CAMERAS[0], 80, 60)
    b = render_all(env, CAMERAS[0], 80, 60)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    c = render_all(env, CAMERAS[0], 80, 60, env_ids=[7, 3, 3])
    for x, y in zip(a, c):
        assert x[[7, 3, 3]].tobytes() == y.tobytes()
    # pre-filled buffers come back fully written
    rgb = torch.full((8, 60, 80, 3), 0xFF, dtype=torch.uint8, device=env.device)
    dep = torch.full((8, 60, 80), float("nan"), device=env.device)
    seg = torch.full((8, 60, 80), 0x7FFFFFFF, dtype=torch.int32, device=env.device)
    env.batch.render(CAMERAS[0], 80, 60, None, rgb, dep, seg)
    assert rgb.cpu().numpy().tobytes() == a[0].tobytes()
    d = dep.cpu().numpy()
    assert np.isfinite(d).all() and d.tobytes() == a[1].tobytes()
    s = seg.cpu().numpy()
    assert s.min() >= -2 and s.max() < env.model.num_bodies
    env.close()


@pytest.mark.parametrize("n,params", [(64, None), (33, None), (64, {"warmstart": 0.85})])
def test_render_has_no_side_effects(n, params):
    envs = [TrexVecEnv(n, device="cuda:0", params=params) for _ in range(2)]
    for e in envs:
        e.reset_tensor()
        random_steps(e, 5, seed=1)
    before = envs[0].get_state().clone()
    envs[0].render_tensor(None, 64, 48, Camera(), depth=True, segmentation=True)
    envs[0].render_tensor([0, n - 1], 32, 32, CAMERAS[2])
    torch.cuda.synchronize()
    assert envs[0].get_state().cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    assert (envs[0].episode_steps == envs[1].episode_steps).all()
    a = torch.rand(n, envs[0].J, generator=torch.Generator().manual_seed(5))
    lo, hi = torch.tensor(envs[0].model.lower, dtype=torch.float32), torch.tensor(envs[0].model.upper, dtype=torch.float32)
    a = (lo + (hi - lo) * a).to(envs[0].device)
    rows = []
    for e in envs:
        e.step_tensor(a)
        rows.append(e.rows.cpu().numpy())
    assert rows[0].tobytes() == rows[1].tobytes()
    for e in envs:
        e.close()


def test_argument_checks():
    env = TrexVecEnv(4, device="cuda:0")
    env.reset_tensor()
    dev = env.device
    rgb = torch.empty(4, 16, 16, 3, dtype=torch.uint8, device=dev)
    cam = Camera()
    bad = [
        dict(width=0, height=16, rgb=rgb),
        dict(width=5000, height=16, rgb=torch.empty(4 * 16 * 5000 * 3, dtype=torch.uint8, device=dev)),
        dict(width=16, height=16, env_ids=[4], rgb=rgb),
        dict(width=16, height=16, env_ids=[-1], rgb=rgb),
        dict(width=16, height=16, rgb=torch.empty(4, 16, 16, 3, dtype=torch.uint8)),          # host tensor
        dict(width=16, height=16, rgb=torch.empty(4, 16, 15, 3, dtype=torch.uint8, device=dev)),   # too short
        dict(width=16, height=16),                                                           # all outputs None
    ]
    for kw in bad:
        with pytest.raises(_capi.TrexError) as ei:
            env.batch.render(cam, kw.pop("width"), kw.pop("height"), kw.pop("env_ids", None), **kw)
        assert ei.value.code == _capi.E_INVALID
    # the raw C-ABI refuses a too-short buffer itself (the binding's own check bypassed): 4 x 4096 x 4096 x 3 bytes are more
    # than the allocation a small tensor lives in
    short = torch.empty(100, dtype=torch.uint8, device=dev)
    c = _capi.TrexCamera(10.0, 90.0, -30.0, 60.0, 0.1, 100.0, 1, (_capi.C.c_float * 3)())
    code = _capi.lib.trex_batch_render(env.batch.h, _capi.C.byref(c), 4096, 4096, None, 0, _capi.C.c_void_p(short.data_ptr()),
                                       None, None, None)
    assert code == _capi.E_INVALID
    # the batch keeps stepping and rendering
    env.step_tensor(torch.zeros(4, env.J, device=dev))
    env.batch.render(cam, 16, 16, None, rgb)
    torch.cuda.synchronize()
    assert torch.isfinite(env.obs).all()
    env.close()


def test_scale_4096_envs():
    env = TrexVecEnv(4096, device="cuda:0")
    env.reset_tensor()
    random_steps(env, 3)
    rgb, dep, seg = env.render_tensor(None, 64, 64, Camera(), depth=True, segmentation=True)
    assert rgb.shape == (4096, 64, 64, 3) and dep.shape == (4096, 64, 64) and seg.shape == (4096, 64, 64)
    ids = [0, 1000, 2047, 4095]
    refs = render_reference(env, rr.Scene.from_model(env.model), Camera(), 64, 64, ids)
    r, d, s = rgb.cpu().numpy(), dep.cpu().numpy(), seg.cpu().numpy()
    for k, e in enumerate(ids):
        render_compare((r[e], d[e], s[e]), refs[k], e)
    env.close()


def test_play_writes_frames(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from trex_gym.ppo import PPO
    from trex_gym.trex_train import build_environment, play
    env = build_environment(2)
    agent = PPO(env, nsteps=1, nminibatches=1, noptepochs=1)
    play(agent, 5, frames_dir=str(tmp_path), frame_size=(48, 32), log=lambda *a: None)
    files = sorted(os.listdir(tmp_path))
    assert files == ["%05d-of-00005.png" % k for k in range(5)]
    for f in files:
        im = Image.open(os.path.join(tmp_path, f))
        assert im.size == (48, 32) and im.mode == "RGB"
    env.close()
