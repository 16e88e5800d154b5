"""Shared by the renderer's and the ray casts' GPU tests: what the device returned, the f64 reference on the poses the kernel's own
state gives (read back through link_transforms), and the comparison at the stated thresholds. The references themselves are
tests/render_ref.py and tests/ray_ref.py. A helper, not a conftest."""
import numpy as np
import torch

import ray_ref as ry
import render_ref as rr


# ---------------------------------------------------------------- the renderer (trex_batch_render)
def render_reference(env, scene, cam, W, H, env_ids):
    lt = env.link_transforms().cpu().numpy()
    st = env.get_state().cpu().numpy()
    lb, ltf = env.model.array("link_body"), env.model.array("link_tf")
    out = []
    for e in env_ids:
        R, p = rr.body_poses(lt[e], lb, ltf, env.model.num_bodies)
        target = st[e, :3] if cam.target is None else cam.target
        eye, dirs, _ = rr.camera_rays(cam.distance, cam.yaw, cam.pitch, cam.fov, W, H, target)
        out.append(rr.render(scene, R, p, eye, dirs, cam.near, cam.far))
    return out


def render_compare(gpu, ref, what):
    rgb, dep, seg = gpu
    rseg, rdep, rrgb, sm, rm = ref
    agree = seg == rseg
    assert agree.mean() >= 0.995, (what, agree.mean())
    assert (sm[~agree] < 1e-4).all(), (what, sm[~agree].max())
    ok = agree & (sm >= 1e-4)
    rel = np.abs(dep[ok] - rdep[ok]) / np.maximum(rdep[ok], 1e-6)
    assert rel.max() <= 1e-4, (what, rel.max())
    okc = ok & (rm >= 1e-4)
    diff = np.abs(rgb[okc].astype(int) - rrgb[okc].astype(int))
    assert diff.max() <= 2, (what, diff.max())


def render_all(env, cam, W, H, env_ids=None):
    rgb, dep, seg = env.render_tensor(env_ids, W, H, cam, depth=True, segmentation=True)
    return rgb.cpu().numpy(), dep.cpu().numpy(), seg.cpu().numpy()


# ---------------------------------------------------------------- the ray casts (trex_batch_ray_test)
def ray_poses(env, env_ids=None):
    """per env: (R, p) of the bodies and (Rl, pl) of the links, f64, from link_transforms() as render_reference does"""
    lt = env.link_transforms().cpu().numpy()
    lb, ltf = env.model.array("link_body"), env.model.array("link_tf")
    out = {}
    for e in (range(env.num_envs) if env_ids is None else env_ids):
        out[e] = rr.body_poses(lt[e], lb, ltf, env.model.num_bodies) + ry.link_frames(lt[e])
    return out


def ray_cast(env, rays, link=None, **kw):
    out = env.ray_test(torch.as_tensor(rays), link, positions=True, normals=True, **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in out]


def ray_world(env, poses, rays, link):
    """rays [n, R, 6] or [R, 6] in a link frame (None: world) -> [(from, to)] per env, f64, from the f32 values the GPU sees"""
    rays = np.asarray(rays, np.float32).astype(np.float64)
    out = {}
    for e, (_, _, Rl, pl) in poses.items():
        r = rays if rays.ndim == 2 else rays[e]
        out[e] = (r[:, :3], r[:, 3:]) if link is None else ry.to_world(r, Rl[link], pl[link])
    return out


def ray_compare(gpu, refs, what, stats=None):
    """gpu: (fraction, body, position, normal) rows of the case's rays; refs: cast()'s tuple over the same rays + their lengths.
    The renderer's thresholds (render_compare), d = fraction x length:
    labels agree on >= 99.5 %, every disagreeing ray is marginal (< 1e-4 m), at most 2 % of the rays are marginal; on agreeing
    non-marginal rays |d - d_ref| <= 1e-4 max(d_ref, 1 m), the position within the same bound, and the normal within 1e-4
    where the normal margin is >= 1e-4 m."""
    frac, body, pos, nrm = gpu
    rf, rl, rp, rn, mg, nm, L = refs
    agree = body == rl
    marginal = mg < ry.MARGIN
    d, dr = frac * L, rf * L
    ok = agree & ~marginal
    bound = 1e-4 * np.maximum(dr, 1.0)
    derr = np.abs(d - dr)[ok] / bound[ok] if ok.any() else np.zeros(1)
    perr = np.abs(pos - rp).max(axis=1)[ok] / bound[ok] if ok.any() else np.zeros(1)
    okn = ok & (nm >= ry.MARGIN)
    nerr = np.abs(nrm - rn).max(axis=1)[okn] if okn.any() else np.zeros(1)
    print("ray_test %s: rays %d agree %.4f marginal %.4f d_err/bound %.3f p_err/bound %.3f n_err %.2e" %
          (what, len(frac), agree.mean(), marginal.mean(), derr.max(), perr.max(), nerr.max()))
    if stats is not None:
        stats.append((what, agree.mean(), marginal.mean(), derr.max(), perr.max(), nerr.max()))
    assert marginal.mean() <= ry.MARGINAL_CAP, (what, marginal.mean())
    assert agree.mean() >= 0.995, (what, agree.mean())
    assert (mg[~agree] < ry.MARGIN).all(), (what, mg[~agree].max())
    assert derr.max() <= 1.0, (what, derr.max())
    assert perr.max() <= 1.0, (what, perr.max())
    assert nerr.max() <= 1e-4, (what, nerr.max())
    assert (frac >= 0).all() and (frac <= 1).all()
    miss = body == -2
    assert (frac[miss] == 1.0).all() and (nrm[miss] == 0).all()


def ray_reference(scene, poses, world, **kw):
    parts = [ry.cast(scene, poses[e][0], poses[e][1], *world[e], **kw) + (np.linalg.norm(world[e][1] - world[e][0], axis=1),)
             for e in sorted(world)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(7))


def ray_flat(gpu, env_ids=None):
    frac, body, pos, nrm = gpu
    if env_ids is not None:
        frac, body, pos, nrm = frac[env_ids], body[env_ids], pos[env_ids], nrm[env_ids]
    return frac.reshape(-1), body.reshape(-1), pos.reshape(-1, 3), nrm.reshape(-1, 3)
