"""Reference ray caster in numpy f64 for the renderer's tests (trex_batch_render, include/trex_batch.h).

It starts from the same inputs as the kernel - hull vertices, body poses, camera, floor height - and trusts nothing of the
library's: its convex-hull planes come from qhull (scipy.spatial.ConvexHull), its camera from the convention written in the
header. Besides seg / depth / rgb it records, per pixel, how close the ray comes to changing the answer:
  seg_margin  min over the primitives that could be nearest of |t_exit - t_enter| (hit or miss: the interval of a ray
              near a silhouette shrinks to zero), the depth gap between the two nearest hits of different labels and the
              gap of the nearest hit to the far plane - in metres of eye-space depth;
  rgb_margin  seg_margin, and also: between the two planes a hull hit could be entering through (the normal flips at an
              edge) and, on the floor, from the hit point to the nearest checker line.
"""
import math

import numpy as np

# shading constants of render.hip (the picture is deterministic; these are its definition, not a computation)
PALETTE = np.array([[0.85, 0.55, 0.30], [0.35, 0.65, 0.35], [0.30, 0.50, 0.85], [0.85, 0.35, 0.35],
                    [0.75, 0.75, 0.30], [0.60, 0.40, 0.80], [0.30, 0.75, 0.75], [0.80, 0.80, 0.80]])
LIGHT = np.array([0.3713907, 0.2785430, 0.8854167])
AMBIENT = 0.35
FLOOR_A, FLOOR_B = np.array([0.62] * 3), np.array([0.42] * 3)
SKY = np.array([0.60, 0.75, 0.92])


# ---------------------------------------------------------------- geometry
def hull_planes(points):
    """(normals [K, 3], offsets [K]) of the convex hull of `points`, n.x <= d inside, by qhull (one plane per facet
    triangle; coplanar facets repeat a plane, which changes nothing for a ray caster)."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(points, np.float64)).equations
    return eq[:, :3].copy(), -eq[:, 3].copy()


def obj_mesh(path):
    """vertices [V, 3], triangles [T, 3] (fans of the OBJ's faces, 0-based)"""
    vs, tris = [], []
    for line in open(path):
        w = line.split()
        if not w:
            continue
        if w[0] == "v":
            vs.append([float(x) for x in w[1:4]])
        elif w[0] == "f":
            idx = [int(x.split("/")[0]) - 1 for x in w[1:]]
            for k in range(1, len(idx) - 1):
                tris.append([idx[0], idx[k], idx[k + 1]])
    return np.array(vs), np.array(tris)


def mesh_volume(v, tris):
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return abs(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def plane_polytope_volume(n, d):
    """Volume of {x : n.x <= d} from the planes alone: every plane's face polygon is cut out of a large square in the
    plane by the other half-spaces, V = sum d_i area_i / 3 (unit normals)."""
    n, d = np.asarray(n, np.float64), np.asarray(d, np.float64)
    big = 10.0 * (np.abs(d).max() + 1.0)
    vol = 0.0
    for i in range(len(d)):
        ni = n[i]
        a = np.cross(ni, [1.0, 0, 0] if abs(ni[0]) < 0.9 else [0, 1.0, 0])
        a /= np.linalg.norm(a)
        b = np.cross(ni, a)
        c = ni * d[i]
        poly = np.array([c + big * (sa * a + sb * b) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
        for _ in range(4 * len(d)):
            viol = poly @ n.T - d                      # [P, K]
            viol[:, i] = 0.0
            worst = viol.max(axis=0)
            j = int(np.argmax(worst))
            if worst[j] <= 1e-12 * big:
                break
            s = viol[:, j]
            out = []
            for k in range(len(poly)):
                p, q, sp, sq = poly[k], poly[(k + 1) % len(poly)], s[k], s[(k + 1) % len(poly)]
                if sp <= 0:
                    out.append(p)
                if (sp <= 0) != (sq <= 0):
                    out.append(p + (q - p) * (sp / (sp - sq)))
            poly = np.array(out)
            if len(poly) < 3:
                break
        if len(poly) < 3:
            continue
        area = 0.5 * np.dot(np.cross(poly - poly[0], np.roll(poly, -1, axis=0) - poly[0]).sum(axis=0), ni)
        vol += d[i] * area / 3.0
    return vol


# ---------------------------------------------------------------- camera
def camera_rays(distance, yaw, pitch, fov, width, height, target):
    """eye [3], ray directions [H, W, 3] with dir . forward = 1 (so a ray parameter IS eye-space depth), forward [3]:
    eye = target + Rz(yaw) Rx(pitch) (0, -distance, 0), up = Rz(yaw) Rx(pitch) z, vertical fov, row 0 at the top."""
    y, p = math.radians(yaw), math.radians(pitch)
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    eye = np.asarray(target, np.float64) + Rz @ Rx @ np.array([0.0, -distance, 0.0])
    up0 = Rz @ Rx @ np.array([0.0, 0.0, 1.0])
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up0)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    ty = math.tan(math.radians(fov) / 2)
    tx = ty * width / height
    xs = (np.arange(width) + 0.5) * 2.0 / width - 1.0
    ys = 1.0 - (np.arange(height) + 0.5) * 2.0 / height
    X, Y = np.meshgrid(xs, ys)
    dirs = f + X[..., None] * tx * r + Y[..., None] * ty * u
    return eye, dirs, f


# ---------------------------------------------------------------- scene
class Scene:
    """The drawable primitives of a model from its arrays (trex_model_get_array): one hull per hull group (planes by qhull
    from its radius-0 points) or one sphere per point of radius > 0, each owned by the body whose vertex range holds it."""

    def __init__(self, hull_xyz, hull_radius, hull_group_start, hull_start, floor_z):
        xyz = np.asarray(hull_xyz, np.float64).reshape(-1, 3)
        rad = np.asarray(hull_radius, np.float64)
        gs = np.asarray(hull_group_start).astype(int)
        hs = np.asarray(hull_start).astype(int)
        body_of = np.searchsorted(hs, np.arange(len(xyz)), side="right") - 1
        self.prims = []   # ("hull", body, n [K,3], d [K], centre, radius) | ("sphere", body, c, r)
        for g in range(len(gs) - 1):
            idx = np.arange(gs[g], gs[g + 1])
            for v in idx[rad[idx] > 0]:
                self.prims.append(("sphere", int(body_of[v]), xyz[v], float(rad[v])))
            pts = idx[rad[idx] == 0]
            if len(pts) >= 4:
                n, d = hull_planes(xyz[pts])
                lo, hi = xyz[pts].min(0), xyz[pts].max(0)
                c = 0.5 * (lo + hi)
                self.prims.append(("hull", int(body_of[pts[0]]), n, d, c, float(np.linalg.norm(xyz[pts] - c, axis=1).max())))
        self.floor_z = float(floor_z)

    @classmethod
    def from_model(cls, model):
        return cls(model.array("hull_xyz"), model.array("hull_radius"), model.array("hull_group_start"),
                   model.array("hull_start"), model.get_param("floor_z"))


def body_poses(link_pose, link_body, link_tf, nb):
    """World (R [nb, 3, 3], p [nb, 3]) of the bodies from the world poses of their links ([L, 7] xyz + quat xyzw, as
    trex_batch_link_transforms writes them) and the body<-link transforms ("link_tf", 12 per link): for every body, the
    link of its with the smallest offset (its own frame, up to f32 rounding)."""
    link_pose = np.asarray(link_pose, np.float64)
    link_tf = np.asarray(link_tf, np.float64).reshape(-1, 12)
    link_body = np.asarray(link_body).astype(int)
    R, p = np.zeros((nb, 3, 3)), np.zeros((nb, 3))
    for b in range(nb):
        ls = np.flatnonzero(link_body == b)
        lk = ls[np.argmin([np.abs(link_tf[l, :9] - np.eye(3).reshape(-1)).sum() + np.abs(link_tf[l, 9:]).sum() for l in ls])]
        x, y, z, w = link_pose[lk, 3:7]
        Rl = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        Rt, tt = link_tf[lk, :9].reshape(3, 3), link_tf[lk, 9:]
        # link = body o tf  ->  body = link o tf^-1
        R[b] = Rl @ Rt.T
        p[b] = link_pose[lk, :3] - R[b] @ tt
    return R, p


def render(scene, R, p, eye, dirs, near, far):
    """-> seg [H, W] int, depth [H, W], rgb [H, W, 3] uint8, seg_margin [H, W], rgb_margin [H, W]"""
    H, W, _ = dirs.shape
    D = dirs.reshape(-1, 3)
    P = len(D)
    INF = np.inf
    best = np.full(P, far)
    label = np.full(P, -2)
    normal = np.zeros((P, 3))
    nmargin = np.full(P, INF)               # entering-plane gap of the current nearest hit
    # candidates for the margins: (t_enter, t_exit, label) of every primitive the ray comes near
    cands = []
    # floor: z <= floor_z
    if eye[2] < scene.floor_z:
        tf = np.full(P, near)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            tf = np.where(D[:, 2] < 0, np.maximum((scene.floor_z - eye[2]) / D[:, 2], near), INF)
    hitf = tf < best
    best[hitf], label[hitf] = tf[hitf], -1
    normal[hitf] = [0, 0, 1]
    cands.append((tf, np.full(P, far), -1))
    dd = np.einsum("ij,ij->i", D, D)
    for prim in scene.prims:
        if prim[0] == "sphere":
            _, body, c, r = prim
            cw = R[body] @ c + p[body]
            oc = eye - cw
            hb = D @ oc
            disc = hb * hb - dd * (oc @ oc - r * r)
            sq = np.sqrt(np.maximum(disc, 0))
            t0, t1 = (-hb - sq) / dd, (-hb + sq) / dd
            te, tx = np.maximum(t0, near), np.minimum(t1, far)
            miss = disc < 0
            # a miss: the distance of the ray from the sphere, as a negative interval
            dist = np.sqrt(np.maximum(oc @ oc - hb * hb / dd, 0)) - r
            te = np.where(miss, 0.0, te)
            tx = np.where(miss, -dist, tx)
            hit = ~miss & (te <= tx) & (te < best)
            nrm = eye + te[:, None] * D - cw
            best[hit], label[hit] = te[hit], body
            normal[hit] = nrm[hit] / np.linalg.norm(nrm[hit], axis=1, keepdims=True)
            nmargin[hit] = INF
            cands.append((te, tx, body))
            continue
        _, body, n, d, c, rb = prim
        cw = R[body] @ c + p[body]
        oc = eye - cw
        hb = D @ oc
        disc = hb * hb - dd * (oc @ oc - (1.01 * rb + 1e-3) ** 2)
        rows = np.flatnonzero(disc >= 0)
        if len(rows) == 0:
            continue
        ob = R[body].T @ (eye - p[body])
        db = D[rows] @ R[body]                     # R^T d per row
        den = db @ n.T                             # [r, K]
        num = d - n @ ob                           # [K]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num[None, :] / den
        ent = den < 0
        tent = np.where(ent, t, -INF)
        texit = np.where(den > 0, t, INF)
        texit = np.where((den == 0) & (num[None, :] < 0), -INF, texit)
        order = np.argsort(-tent, axis=1)
        k1 = order[:, 0]
        t1e = tent[np.arange(len(rows)), k1]
        t2e = tent[np.arange(len(rows)), order[:, 1]] if tent.shape[1] > 1 else np.full(len(rows), -INF)
        te = np.maximum(t1e, near)
        tx = np.minimum(texit.min(axis=1), far)
        hit = (te <= tx) & (te < best[rows])
        hr = rows[hit]
        best[hr], label[hr] = te[hit], body
        inside = t1e[hit] < near
        nw = (R[body] @ n[k1[hit]].T).T
        nw[inside] = -D[hr][inside] / np.linalg.norm(D[hr][inside], axis=1, keepdims=True)
        normal[hr] = nw
        nmargin[hr] = np.where(inside, near - t1e[hit], t1e[hit] - np.maximum(t2e[hit], near))
        tea, txa = np.full(P, 0.0), np.full(P, -INF)
        tea[rows], txa[rows] = te, tx
        cands.append((tea, txa, body))
    # margins
    seg_margin = np.full(P, INF)
    for te, tx, lab in cands:
        gap = np.abs(tx - te)
        gap = np.where(np.isfinite(gap), gap, INF)
        seg_margin = np.where(te <= best + 1e-3, np.minimum(seg_margin, gap), seg_margin)   # (a later one cannot win)
        other = (lab != label) & (te <= tx)
        seg_margin = np.where(other, np.minimum(seg_margin, np.abs(te - best)), seg_margin)
    hp = eye + best[:, None] * D
    checker = np.minimum(np.abs(hp[:, 0] - np.round(hp[:, 0])), np.abs(hp[:, 1] - np.round(hp[:, 1])))
    rgb_margin = np.minimum(seg_margin, np.where(label == -1, checker, nmargin))
    # shading
    col = np.tile(SKY, (P, 1))
    fl = label == -1
    par = (np.floor(hp[:, 0]).astype(np.int64) + np.floor(hp[:, 1]).astype(np.int64)) & 1
    alb = np.where(par[:, None] == 1, FLOOR_B, FLOOR_A)
    bd = label >= 0
    alb[bd] = PALETTE[label[bd] & 7]
    lam = np.maximum(normal @ LIGHT, 0.0)
    sh = AMBIENT + (1 - AMBIENT) * lam
    col[fl | bd] = alb[fl | bd] * sh[fl | bd, None]
    rgb = np.floor(np.clip(col, 0, 1) * 255 + 0.5).astype(np.uint8)
    return (label.reshape(H, W), best.reshape(H, W), rgb.reshape(H, W, 3), seg_margin.reshape(H, W),
            rgb_margin.reshape(H, W))
