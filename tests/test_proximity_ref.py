"""tests/proximity_ref.py pinned without a GPU: the closest points of two segments against a dense parameter grid, closed forms,
invariance under a rigid motion and under A <-> B; and the figures of the default T-rex table that the issue's study quotes, so
that a change of the capsule fit shows up here."""
import numpy as np
import pytest

import dynamics_ref as R
import proximity_cases as PC
import proximity_ref as PR


def random_segments(count, seed=0):
    """segment pairs of every kind: general, a point on one or both sides, parallel, touching"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        p1, q1, p2, q2 = rng.uniform(-1, 1, (4, 3))
        kind = k % 6
        if kind == 1:
            q1 = p1.copy()
        elif kind == 2:
            q1, q2 = p1.copy(), p2.copy()
        elif kind == 3:
            q2 = p2 + (q1 - p1) * rng.uniform(0.2, 2.0)
        elif kind == 4:
            p2 = p1 + 0.3 * (q1 - p1)
        out.append((p1, q1, p2, q2))
    for c in PC.cases():
        out.append((c["a"][0], c["a"][1], c["b"][0], c["b"][1]))
    return out


def seg_distance(seg, s, t):
    p1, q1, p2, q2 = seg
    return np.linalg.norm((p1 + s * (q1 - p1)) - (p2 + t * (q2 - p2)))


def test_dense_grid():
    """201 x 201 values of (s, t) per pair: no grid point is closer than the reference's answer, and the best grid point is within
    the grid's spacing bound of it - the distance is 1-Lipschitz in either point, and the minimiser is within half a step h / 2
    of a grid value in s and in t, so the bound is (|d1| + |d2|) h / 2"""
    u = np.linspace(0.0, 1.0, 201)
    h = u[1] - u[0]
    for seg in random_segments(60):
        p1, q1, p2, q2 = (np.asarray(x, np.float64) for x in seg)
        A = p1 + u[:, None] * (q1 - p1)
        B = p2 + u[:, None] * (q2 - p2)
        grid = np.linalg.norm(A[:, None, :] - B[None, :, :], axis=2).min()
        s, t = PR.segment_closest(p1, q1, p2, q2)
        assert 0.0 <= s <= 1.0 and 0.0 <= t <= 1.0
        ref = seg_distance((p1, q1, p2, q2), s, t)
        bound = 0.5 * h * (np.linalg.norm(q1 - p1) + np.linalg.norm(q2 - p2))
        assert grid >= ref - 1e-12, (seg, grid, ref)
        assert grid - ref <= bound + 1e-12, (seg, grid, ref, bound)


def test_closed_forms():
    z = np.zeros(3)
    cap = lambda p0, p1, r: (np.array(p0, float), np.array(p1, float), r)
    # two spheres 1 apart along x
    r = PR.capsule_closest(cap((1, 0, 0), (1, 0, 0), 0.2), cap(z, z, 0.3))
    assert abs(r["distance"] - 0.5) < 1e-15 and np.allclose(r["normal"], [1, 0, 0]) and np.allclose(r["point_a"], [0.8, 0, 0])
    assert np.allclose(r["point_b"], [0.3, 0, 0])
    # crossed at right angles, 0.4 apart in z: interior of both
    r = PR.capsule_closest(cap((-1, 0, 0.4), (1, 0, 0.4), 0.1), cap((0, -1, 0), (0, 1, 0), 0.1))
    assert abs(r["distance"] - 0.2) < 1e-15 and np.allclose(r["normal"], [0, 0, 1]) and r["s"] == 0.5 and r["t"] == 0.5
    # a 3-4-5 triangle between two ends
    r = PR.capsule_closest(cap((-1, 0, 0), (0, 0, 0), 0.0), cap((3, 4, 0), (5, 4, 0), 0.0))
    assert abs(r["distance"] - 5.0) < 1e-15 and (r["s"], r["t"]) == (1.0, 0.0) and np.allclose(r["normal"], [-0.6, -0.8, 0])
    # overlapping spheres: the depth, negative
    r = PR.capsule_closest(cap(z, z, 0.3), cap((0, 0.4, 0), (0, 0.4, 0), 0.3))
    assert abs(r["distance"] + 0.2) < 1e-15
    # the two conventions at axis distance 0
    r = PR.capsule_closest(cap(z, z, 0.1), cap(z, z, 0.15))
    assert np.array_equal(r["normal"], [0, 0, 1]) and abs(r["distance"] + 0.25) < 1e-15
    assert np.allclose(r["point_a"], [0, 0, -0.1]) and np.allclose(r["point_b"], [0, 0, 0.15])
    # (point_a - point_b) . n = distance, always
    for seg in random_segments(30, seed=1):
        r = PR.capsule_closest((seg[0], seg[1], 0.07), (seg[2], seg[3], 0.11))
        assert abs((r["point_a"] - r["point_b"]) @ r["normal"] - r["distance"]) < 1e-12


def test_rigid_motion_and_symmetry():
    rng = np.random.default_rng(2)
    for seg in random_segments(40, seed=3):
        q = rng.normal(size=4)
        Rm, tr = R.quat_to_mat(q / np.linalg.norm(q)), rng.uniform(-3, 3, 3)
        a, b = (seg[0], seg[1], 0.05), (seg[2], seg[3], 0.08)
        r0 = PR.capsule_closest(a, b)
        mv = lambda x: Rm @ x + tr
        r1 = PR.capsule_closest((mv(a[0]), mv(a[1]), a[2]), (mv(b[0]), mv(b[1]), b[2]))
        assert abs(r0["distance"] - r1["distance"]) < 1e-12
        rs = PR.capsule_closest(b, a)
        assert abs(r0["distance"] - rs["distance"]) < 1e-12
        if r0["axis"] > 1e-3:
            # (1e-7: between axes 1e-5 rad apart the distance is flat to 1e-16 over a stretch that turns the normal by 1e-8)
            assert np.abs(Rm @ r0["normal"] - r1["normal"]).max() < 1e-7
            assert np.abs(rs["normal"] + r0["normal"]).max() < 1e-7
            # the points themselves where they are well determined: axes at least 0.05 rad apart, or a point on one side
            d1, d2 = seg[1] - seg[0], seg[3] - seg[2]
            if not (d1.any() and d2.any()) or np.linalg.norm(np.cross(d1, d2)) > 0.05 * np.linalg.norm(d1) * np.linalg.norm(d2):
                assert np.abs(mv(r0["point_a"]) - r1["point_a"]).max() < 1e-9
                assert np.abs(rs["point_b"] - r0["point_a"]).max() < 1e-9 and np.abs(rs["point_a"] - r0["point_b"]).max() < 1e-9


def test_per_pair_minimum_and_ties(model):
    """the winner is the smallest test, ties go to the earlier one, the gap is the runner-up's margin"""
    s = PR.start_state(model)
    caps = np.array([[0, 0, 0, 0, 0, 0, 0.1], [0, 0, 0, 0, 0, 0, 0.1], [0.0, 0, 0, 0.2, 0, 0, 0.05]])
    bodies = [3, 3, 5]
    r = PR.proximity(model, s, bodies, caps, [(3, 5), (5, 3)])
    assert r[0]["capsule"] == (0, 2) and r[1]["capsule"] == (2, 0)
    assert len(r[0]["cands"]) == 2 and r[0]["gap"] == 0.0            # capsules 0 and 1 are the same sphere
    assert abs(r[0]["distance"] - r[1]["distance"]) < 1e-15 and np.abs(r[0]["normal"] + r[1]["normal"]).max() < 1e-12
    assert min(d for _, _, d in r[0]["cands"]) == r[0]["distance"]


def test_default_table_figures(model):
    """max_radius 0.2, 3 divisions, min_points 4 on trex_collide.urdf"""
    bodies, caps = PR.fitted_table(model)
    assert len(bodies) == 74
    count = np.bincount(bodies, minlength=model["nb"])
    assert count[0] == 45 and count[13] == 8 and sorted(np.flatnonzero(count == 0)) == [1, 12, 17] and (count > 0).sum() == 23
    every = PR.all_pairs(bodies)
    assert len(every) == 253 and PR.num_tests(bodies, every) == 1683
    par = model["parent"]
    apart = [(a, b) for a, b in every if par[b] != a and par[a] != b]
    start = PR.proximity(model, PR.start_state(model), bodies, caps, apart)
    deep = {p: r["distance"] for p, r in zip(apart, start) if r["distance"] < 0}
    assert sorted(deep) == [(4, 6), (6, 8), (20, 22), (22, 24)] and all(-0.005 < d < -0.003 for d in deep.values())
    chosen = PR.default_pairs(model, bodies, caps)
    assert len(chosen) == 230 and PR.num_tests(bodies, chosen) == 1572
    # the study's finding: bodies inside each other at 2 of the first 4 random states
    states, _ = R.random_states(model, 8)
    hit = []
    for s in states[:4]:
        res = PR.proximity(model, s, bodies, caps, chosen)
        hit.append({p: r["distance"] for p, r in zip(chosen, res) if r["distance"] < 0})
    assert [len(h) for h in hit] == [0, 1, 0, 4]
    assert -0.12 < hit[1][(0, 2)] < -0.10 and sorted(hit[3]) == [(4, 13), (5, 13), (6, 13), (7, 13)]
    assert all(-0.15 < d < -0.04 for d in hit[3].values())


def test_the_library_exports_the_symbols():
    from trex_gym import _capi
    for sym in ("trex_batch_set_proximity_shapes", "trex_batch_proximity"):
        assert sym in _capi.SYMBOLS and hasattr(_capi.lib, sym)
    assert hasattr(_capi.Batch, "set_proximity_shapes") and hasattr(_capi.Batch, "proximity")
