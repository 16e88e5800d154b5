"""numpy f64 restatement of the proximity query (include/trex_batch.h, "proximity between bodies"): body poses by
dynamics_ref.Kin, the closest points of two segments, the per-pair minimum over the capsules of the two bodies with the gap to
the runner-up, and the header's formulas for distance, points and normal.

Written from the definition and not from the kernel: the squared distance of two segments is a convex quadratic of (s, t) on the
unit square, so its minimum is the unconstrained critical point where that lies inside, or else on one of the four edges, where it
is a point-to-segment projection. All five candidates are evaluated and the smallest taken (the kernel projects alternately
instead). tests/test_proximity_ref.py pins this against a dense parameter grid, closed forms and invariances."""
import numpy as np

import dynamics_ref as R

EPS = 1e-6          # axis distance below which the normal is (0, 0, 1)
SPHERE2 = 1e-12     # |p1 - p0|^2 below which a capsule is stored as a sphere


def _project(p, q0, d):
    """[T] parameters in [0, 1] of the points of q0 + u d closest to p (a zero d: 0)"""
    dd = (d * d).sum(-1)
    ok = dd > 0
    return np.where(ok, np.clip(((p - q0) * d).sum(-1) / np.where(ok, dd, 1.0), 0.0, 1.0), 0.0)


def segments_closest(p1, q1, p2, q2):
    """[T, 3] each -> s, t [T] in [0, 1] minimising |(p1 + s (q1 - p1)) - (p2 + t (q2 - p2))|; among equal candidates the first of:
    interior, s = 0, s = 1, t = 0, t = 1"""
    p1, q1, p2, q2 = (np.asarray(x, np.float64).reshape(-1, 3) for x in (p1, q1, p2, q2))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e = (d1 * d1).sum(-1), (d2 * d2).sum(-1)
    n = np.cross(d1, d2)          # the critical point through n: (b f - c e) / (a e - b^2) without its cancellation
    nn = (n * n).sum(-1)
    ok = (nn > 1e-14 * a * e) & (a > 0) & (e > 0)
    safe = np.where(ok, nn, 1.0)
    si, ti = (n * np.cross(d2, r)).sum(-1) / safe, (n * np.cross(d1, r)).sum(-1) / safe
    ok &= (0.0 <= si) & (si <= 1.0) & (0.0 <= ti) & (ti <= 1.0)
    zero, one = np.zeros(len(a)), np.ones(len(a))
    S = [np.where(ok, si, 0.0), zero, one, _project(p2, p1, d1), _project(q2, p1, d1)]
    T = [np.where(ok, ti, 0.0), _project(p1, p2, d2), _project(q1, p2, d2), zero, one]
    dist = np.stack([np.linalg.norm(r + s[:, None] * d1 - t[:, None] * d2, axis=-1) for s, t in zip(S, T)], 1)
    dist[:, 0] = np.where(ok, dist[:, 0], np.inf)
    best = np.argmin(dist, 1)      # (the first of equal ones)
    rows = np.arange(len(a))
    return np.stack(S, 1)[rows, best], np.stack(T, 1)[rows, best]


def segment_closest(p1, q1, p2, q2):
    """one pair of segments: (s, t) as floats"""
    s, t = segments_closest(p1, q1, p2, q2)
    return float(s[0]), float(t[0])


def capsules_closest(caps_a, caps_b):
    """[T] world capsules each, lists of (p0, p1, radius) -> a list of T dicts as capsule_closest"""
    P = lambda caps, k: np.array([c[k] for c in caps], np.float64).reshape(-1, 3)
    p0a, p1a, p0b, p1b = P(caps_a, 0), P(caps_a, 1), P(caps_b, 0), P(caps_b, 1)
    ra, rb = np.array([c[2] for c in caps_a], np.float64), np.array([c[2] for c in caps_b], np.float64)
    s, t = segments_closest(p0a, p1a, p0b, p1b)
    a, b = p0a + s[:, None] * (p1a - p0a), p0b + t[:, None] * (p1b - p0b)
    axis = np.linalg.norm(a - b, axis=1)
    n = np.where((axis < EPS)[:, None], np.array([0.0, 0.0, 1.0]), (a - b) / np.where(axis < EPS, 1.0, axis)[:, None])
    pa, pb = a - ra[:, None] * n, b + rb[:, None] * n
    return [dict(distance=float(axis[k] - ra[k] - rb[k]), point_a=pa[k], point_b=pb[k], normal=n[k], axis=float(axis[k]), a=a[k],
                 b=b[k], s=float(s[k]), t=float(t[k])) for k in range(len(s))]


def capsule_closest(cap_a, cap_b):
    """world capsules (p0, p1, radius) -> dict(distance, point_a, point_b, normal, axis: |a - b|, a, b: the axis points, s, t)"""
    return capsules_closest([cap_a], [cap_b])[0]


def round_table(capsules):
    """[C, 7] as the batch stores it: spheres collapsed (in f64, before rounding), every value rounded to f32"""
    c = np.array(capsules, np.float64).reshape(-1, 7)
    d = c[:, 3:6] - c[:, 0:3]
    sph = (d * d).sum(1) < SPHERE2
    c[sph, 3:6] = c[sph, 0:3]
    return c.astype(np.float32).astype(np.float64)


def world_capsules(model, state, bodies, capsules):
    """the table's capsules [(p0, p1, radius)] in the world at `state`"""
    k = R.Kin(model, state)
    out = []
    for b, c in zip(bodies, np.asarray(capsules, np.float64).reshape(-1, 7)):
        out.append((k.p[b] + k.R[b] @ c[0:3], k.p[b] + k.R[b] @ c[3:6], float(c[6])))
    return out


def proximity(model, state, bodies, capsules, pairs):
    """every pair of `pairs` at `state`: a list of dicts - capsule_closest of the winning capsule pair plus capsule = (index of
    A's, index of B's), gap = distance of the runner-up minus the winner's (inf for a single test), cands = [(ia, ib, distance)]
    of every test. Ties go to the earlier (capsule of A, capsule of B) in table order."""
    wc = world_capsules(model, state, bodies, capsules)
    of_body = {}
    for c, b in enumerate(bodies):
        of_body.setdefault(int(b), []).append(c)
    tests = [[(ia, ib) for ia in of_body[int(A)] for ib in of_body[int(B)]] for A, B in pairs]
    flat = [x for t in tests for x in t]
    every = iter(capsules_closest([wc[ia] for ia, _ in flat], [wc[ib] for _, ib in flat]))
    out = []
    for t in tests:
        res = [(ia, ib, next(every)) for ia, ib in t]
        order = sorted(range(len(res)), key=lambda k: (res[k][2]["distance"], k))
        win = dict(res[order[0]][2])
        win["capsule"] = (res[order[0]][0], res[order[0]][1])
        win["gap"] = res[order[1]][2]["distance"] - win["distance"] if len(res) > 1 else np.inf
        win["cands"] = [(ia, ib, r["distance"]) for ia, ib, r in res]
        out.append(win)
    return out


def start_state(model):
    """the model's start pose at rest"""
    oo = model["obs_order"]
    J = len(oo)
    return np.concatenate([model["base_start_pos"], model["base_start_quat"], np.zeros(6), model["q_start"][oo], np.zeros(J)])


def fitted_table(model, max_radius=0.2, max_divisions=3, min_points=4):
    """(bodies [C], capsules [C, 7] f32-exact): oracle/trex_model.py's capsule fit of every hull group, body by body"""
    from oracle import trex_model as tm
    gs, hs = model["hull_group_start"], model["hull_start"]
    bodies, caps = [], []
    for b in range(model["nb"]):
        for g in range(len(gs) - 1):
            if not (hs[b] <= gs[g] < hs[b + 1]) or gs[g + 1] <= gs[g]:
                continue
            for p0, p1, r in tm.fit_primitives(model["hull_xyz"][gs[g]:gs[g + 1]], max_radius, max_divisions, min_points):
                bodies.append(b)
                caps.append(np.concatenate([p0, p1, [r]]))
    return np.array(bodies, np.int32), round_table(caps)


def all_pairs(bodies):
    """every body pair A < B with geometry on both sides"""
    have = sorted(set(int(b) for b in bodies))
    return [(a, b) for i, a in enumerate(have) for b in have[i + 1:]]


def default_pairs(model, bodies, capsules):
    """all_pairs minus parent-child pairs minus the pairs with distance < 0 at the start pose"""
    par = model["parent"]
    cand = [(a, b) for a, b in all_pairs(bodies) if par[b] != a and par[a] != b]
    res = proximity(model, start_state(model), bodies, capsules, cand)
    return [p for p, r in zip(cand, res) if not r["distance"] < 0]


def num_tests(bodies, pairs):
    cnt = np.bincount(np.asarray(bodies, int), minlength=int(max(max(p) for p in pairs)) + 1)
    return int(sum(cnt[a] * cnt[b] for a, b in pairs))
