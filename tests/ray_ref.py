"""Reference segment caster in numpy f64 for the ray-cast tests (trex_batch_ray_test, include/trex_batch.h).

The geometry is render_ref's - Scene (hull planes by qhull, spheres, the floor) and body_poses - and nothing of the library's.
cast() follows the header's hit rule: the nearest ENTRY point with 0 <= t <= 1 along from -> to; a primitive that contains
`from` (t_enter < 0) is not hit; ties go to the floor, then the lower primitive index. Besides the result it records, per
ray, how close the ray comes to changing the answer - the MARGIN, in metres along the ray, the smallest of
  - |t_exit - t_enter| of any primitive that could be nearest (the interval of a grazing ray shrinks to zero; for a ray that
    passes a sphere, its distance from the sphere),
  - the gap between the nearest hit and any other entry of a different label,
  - the gap of such an entry to the segment's end,
  - |t_enter| of any primitive the ray's line meets (near zero the origin-inside rule flips),
and the NORMAL margin: the gap between the two planes a hull hit could be entering through (inf for spheres and the floor).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from render_ref import Scene, body_poses, hull_planes  # noqa: E402,F401

MISS, FLOOR = -2, -1


def cast(scene, R, p, frm, to, body_mask=0xFFFFFFFF, hit_floor=True):
    """scene: render_ref.Scene; R [nb, 3, 3], p [nb, 3]: world body poses; frm, to [P, 3] world.
    -> fraction [P], label [P] int (body, -1 floor, -2 miss), position [P, 3], normal [P, 3], margin [P], normal_margin [P]"""
    frm, to = np.asarray(frm, np.float64).reshape(-1, 3), np.asarray(to, np.float64).reshape(-1, 3)
    P = len(frm)
    INF = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        D = to - frm
        dd = np.einsum("ij,ij->i", D, D)
    good = np.isfinite(frm).all(1) & np.isfinite(to).all(1) & (dd > 0) & np.isfinite(dd)
    o = np.where(good[:, None], frm, 0.0)
    D = np.where(good[:, None], D, [0.0, 0.0, 1.0])
    dd = np.where(good, dd, 1.0)
    L = np.sqrt(dd)

    best = np.full(P, INF)                # entry parameter of the nearest hit
    label = np.full(P, MISS)
    normal = np.zeros((P, 3))
    nmargin = np.full(P, INF)
    cands = []                            # (t_enter, t_exit, label) of every primitive the ray's line comes near
    which = np.full(P, -1)                # the winner's index in cands

    def take(te, tx, lab, nrm, nm):
        nonlocal best, label, normal, nmargin, which
        hit = good & (te >= 0) & (te <= 1) & (te <= tx) & (te < best)
        best = np.where(hit, te, best)
        label = np.where(hit, lab, label)
        normal[hit] = nrm[hit] if nrm.ndim == 2 else nrm
        nmargin = np.where(hit, nm, nmargin)
        which = np.where(hit, len(cands), which)
        cands.append((te, tx, lab))

    if hit_floor:   # the half-space z <= floor_z
        with np.errstate(divide="ignore", invalid="ignore"):
            tf = (scene.floor_z - o[:, 2]) / D[:, 2]
        below = o[:, 2] <= scene.floor_z
        te = np.where(D[:, 2] < 0, tf, np.where(below, -INF, INF))
        tx = np.where(D[:, 2] > 0, tf, np.where(below | (D[:, 2] < 0), INF, -INF))
        # (from exactly on the plane, going down: t_enter = 0, a hit at fraction 0)
        take(te, tx, FLOOR, np.array([0.0, 0.0, 1.0]), np.full(P, INF))

    for prim in scene.prims:
        body = prim[1]
        if not (int(body_mask) >> body) & 1:
            continue
        if prim[0] == "sphere":
            _, _, c, r = prim
            cw = R[body] @ c + p[body]
            oc = o - cw
            hb = np.einsum("ij,ij->i", D, oc)
            disc = hb * hb - dd * (np.einsum("ij,ij->i", oc, oc) - r * r)
            sq = np.sqrt(np.maximum(disc, 0))
            te, tx = (-hb - sq) / dd, (-hb + sq) / dd
            miss = disc < 0
            # a miss: the distance of the ray's line from the sphere, as a negative interval (in units of t)
            dist = np.sqrt(np.maximum(np.einsum("ij,ij->i", oc, oc) - hb * hb / dd, 0)) - r
            tc = -hb / dd
            te = np.where(miss, tc, te)
            tx = np.where(miss, tc - dist / L, tx)
            nrm = o + te[:, None] * D - cw
            nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
            take(te, tx, body, nrm, np.full(P, INF))
            continue
        _, _, n, d, c, rb = prim
        cw = R[body] @ c + p[body]
        oc = o - cw
        hb = np.einsum("ij,ij->i", D, oc)
        disc = hb * hb - dd * (np.einsum("ij,ij->i", oc, oc) - (1.01 * rb + 1e-3) ** 2)
        rows = np.flatnonzero(disc >= 0)
        if len(rows) == 0:
            continue
        ob = (o[rows] - p[body]) @ R[body]        # R^T (o - p) per row
        db = D[rows] @ R[body]
        den = db @ n.T                            # [r, K]
        num = d[None, :] - ob @ n.T
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / den
        tent = np.where(den < 0, t, -INF)
        texit = np.where(den > 0, t, INF)
        texit = np.where((den == 0) & (num < 0), -INF, texit)
        order = np.argsort(-tent, axis=1)
        ar = np.arange(len(rows))
        k1 = order[:, 0]
        t1e = tent[ar, k1]
        # the runner-up among the planes of ANOTHER face (qhull repeats the plane of a face it has cut into triangles)
        t2e = np.where(n[k1] @ n.T > 1 - 1e-9, -INF, tent).max(axis=1)
        te, tx = np.full(P, INF), np.full(P, -INF)
        te[rows], tx[rows] = t1e, texit.min(axis=1)
        nrm = np.zeros((P, 3))
        nrm[rows] = n[k1] @ R[body].T
        nm = np.full(P, INF)
        nm[rows] = (t1e - t2e) * L[rows]
        take(te, tx, body, nrm, nm)

    hit = label != MISS
    fraction = np.where(hit, best, 1.0)
    bt = np.where(hit, best, 1.0)                 # where the answer is decided along the ray
    margin = np.full(P, INF)
    slack = 1e-3 / L
    for ci, (te, tx, lab) in enumerate(cands):
        with np.errstate(invalid="ignore"):
            met = (te <= tx) & np.isfinite(te)                           # the ray's line enters the primitive
            near = np.isfinite(te) & np.isfinite(tx) & (te <= bt + slack) & (np.maximum(te, tx) >= -slack)
            gap = np.abs(tx - te) * L
            margin = np.where(near, np.minimum(margin, gap), margin)     # grazing
            margin = np.where(met, np.minimum(margin, np.abs(te) * L), margin)               # the origin-inside rule
            ahead = met & (te >= 0)
            margin = np.where(ahead & (te <= bt + slack), np.minimum(margin, np.abs(te - 1.0) * L), margin)   # the segment's end
            other = ahead & (lab != label)
            margin = np.where(other, np.minimum(margin, np.abs(te - bt) * L), margin)        # another label as near
            rival = ahead & (which != ci)                                                    # another face as near
            nmargin = np.where(rival, np.minimum(nmargin, np.abs(te - bt) * L), nmargin)
    margin = np.where(good, margin, INF)
    position = np.where(hit[:, None], o + fraction[:, None] * D, to)
    normal[~hit] = 0.0
    return fraction, label, position, normal, margin, np.where(hit, nmargin, INF)


def link_frames(link_pose):
    """[L, 7] world link poses (xyz + quaternion xyzw) -> R [L, 3, 3], p [L, 3]"""
    link_pose = np.asarray(link_pose, np.float64)
    x, y, z, w = link_pose[:, 3], link_pose[:, 4], link_pose[:, 5], link_pose[:, 6]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    return R, link_pose[:, :3].copy()


def to_world(rays, Rl, pl):
    """rays [R, 6] in a frame (Rl [3, 3], pl [3]) -> from, to [R, 3] world"""
    rays = np.asarray(rays, np.float64)
    return rays[:, :3] @ Rl.T + pl, rays[:, 3:] @ Rl.T + pl


# ---------------------------------------------------------------- the ray sets of the tests (tests/test_gpu_ray_test.py, and
# tests/test_ray_ref_host.py, which checks the marginal-ray cap for them on the reference alone)
def random_segments(n_envs, R, base_xyz, seed=0):
    """[n, R, 6] f32 world: both ends uniform in a box of +-3 m x +-3 m x [0.05, 4] m around each env's base (x, y)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-3.0, -3.0, 0.05]), np.array([3.0, 3.0, 4.0])
    ends = lo + (hi - lo) * rng.random((n_envs, R, 2, 3))
    base = np.asarray(base_xyz, np.float64).reshape(n_envs, 1, 1, 3) * np.array([1.0, 1.0, 0.0])
    return (ends + base).reshape(n_envs, R, 6).astype(np.float32)


def head_fan():
    """[65, 6] f32: 13 x 5 rays of 6 m from the head link's origin, +-100 deg of yaw, -60 .. +20 deg of pitch."""
    yaw, pitch = np.linspace(-1.745, 1.745, 13), np.linspace(-1.047, 0.349, 5)
    P, Y = np.meshgrid(pitch, yaw, indexing="ij")
    d = np.stack([np.cos(P) * np.cos(Y), np.cos(P) * np.sin(Y), np.sin(P)], -1).reshape(-1, 3)
    return np.concatenate([np.zeros_like(d), 6.0 * d], 1).astype(np.float32)


def foot_rays():
    """[3, 6] f32: three rays from a little above a foot link's origin, 2 m along the link's -z / tilted fore and aft."""
    ends = np.array([[0.0, 0.0, -2.0], [0.35, 0.0, -1.95], [-0.35, 0.1, -1.95]])
    return np.concatenate([np.tile([0.0, 0.0, 0.3], (3, 1)), ends], 1).astype(np.float32)


def single_ray():
    """[1, 6] f32: one ray straight down through the base from 4 m above it (base link frame)."""
    return np.array([[0.02, 0.01, 4.0, 0.02, 0.01, -6.0]], np.float32)


MARGIN = 1e-4          # metres: the renderer's own threshold (tests/gpu_render_support.py::render_compare)
MARGINAL_CAP = 0.02    # at most this share of a case's rays may be marginal
HEAD_LINK, BASE_LINK = "link_cranium", "link_vertebrae_sacral"
FOOT_LINKS = ("link_tarsometatarsus_right", "link_tarsometatarsus_left")
