"""The planner's reference and cases, qualified on the host alone (tests/planner_ref.py, tests/planner_cases.py; no device): the tap
tables' properties, the weights, that every planted mistake is caught by a case, and that every tolerance derived from the f32
run's deviation is derived from a deviation that is there."""
import numpy as np
import pytest

import planner_cases as pc
import planner_ref as ref

KIND_NAMES = {v: k for k, v in ref.KINDS.items()}
SHAPES = sorted({(c.S, c.P) for c in pc.CASES} | {(S, P) for S in (1, 2, 3, 7, 12, 16, 33, 256) for P in (1, 2, 3, 5, 6, 32) if P <= S})


def _f32_sum(w):
    total = np.float32(0)
    for x in w:
        total = np.float32(total + np.float32(x))
    return total


@pytest.mark.parametrize("kind", sorted(KIND_NAMES))
def test_tap_weights_sum_to_one_exactly(kind):
    """((w0 + w1) + w2) + w3 == 1 in f32, for every step of the interpolation table and every new knot of the shift tables; the
    indices stay inside the knots; every weight is within one rounding of a partial sum of the f64 weight it stands for"""
    for S, P in SHAPES:
        tables = [ref.tap_table(kind, S, P)] + [ref.shift_table(kind, S, P, steps) for steps in (0, 1, 2, S - 1, S + 5)]
        for idx, w in tables:
            assert idx.min() >= 0 and idx.max() < P and w.dtype == np.float32
            for row in w:
                assert _f32_sum(row) == np.float32(1), (S, P, row)
            assert np.abs(w).max() <= 1.0 + 2 ** -20 and w.sum(1).max() <= 1 + 2 ** -22


@pytest.mark.parametrize("kind", sorted(KIND_NAMES))
def test_a_constant_is_reproduced_exactly_and_a_ramp_to_rounding(kind):
    lo, hi = np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32)
    for S, P in SHAPES:
        table = ref.tap_table(kind, S, P)
        for c in (0.0, 1.0, -2.0, 0.25):          # powers of two: every product is exact, and the weights sum to 1 exactly
            knots = np.full((2, P, 3), c, np.float32)
            got = ref.actions_of(knots, table, lo, hi, True)          # the header's arithmetic: bit for bit
            assert got.shape == (S, 2, 3) and got.dtype == np.float32 and (got == c).all(), (S, P, c)
            # (in f64 the f32 weights' sum is 1 to their own rounding only)
            assert np.abs(ref.actions_of(knots, table, lo, hi, False) - c).max() <= 2 ** -23 * abs(c), (S, P, c)
        if P < 2:
            continue
        # a ramp in knot time: the value at step s is a + b s - for LINEAR everywhere, for CUBIC on the segments with both
        # neighbours (the repeated end knots flatten the first and the last one), for every kind at a step that sits on a knot
        a, b = 0.37, -0.11
        t = np.arange(P) * (S - 1) / (P - 1)
        knots = np.broadcast_to((a + b * t).astype(np.float32)[None, :, None], (1, P, 3)).copy()
        got = ref.actions_of(knots, table, lo, hi, True)[:, 0, 0].astype(np.float64)
        s = np.arange(S)
        u = s * (P - 1) / (S - 1)
        seg = np.minimum(np.floor(u), P - 2)
        on_knot = (s * (P - 1)) % (S - 1) == 0
        where = on_knot | (kind == ref.LINEAR) | ((kind == ref.CUBIC) & (seg >= 1) & (seg <= P - 3))
        err = np.abs(got - (a + b * s))
        assert (err[where] <= 8 * pc.ulp32(np.abs(knots).max())).all(), (S, P, err[where].max())
        if kind == ref.HOLD:
            assert (got == knots[0, np.minimum((s * (P - 1)) // (S - 1), P - 1), 0]).all()


def test_the_shift_by_zero_is_the_identity_and_a_long_one_holds_the_last_value():
    rng = np.random.default_rng(0)
    for kind in sorted(KIND_NAMES):
        for S, P in SHAPES:
            nominal = rng.uniform(-1, 1, (2, P, 3)).astype(np.float32)
            assert np.array_equal(ref.shift_of(nominal, kind, S, 0, True), nominal)
            far = ref.shift_of(nominal, kind, S, S + 3, True)
            assert np.array_equal(far, np.broadcast_to(nominal[:, -1:, :], far.shape))
            assert np.array_equal(far, ref.shift_of(nominal, kind, S, max(S - 1, 0), True))


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_weights_and_the_update_s_invariants(case):
    r = pc.reference(case)
    G, K = case.G, case.K
    w, R = r["weights"].reshape(G, K), r["returns"].reshape(G, K)
    for g in range(G):
        if r["best"][g] < 0:
            assert not np.isfinite(R[g]).any() and (w[g] == 0).all() and r["stats"][g, 2] == 0
            assert np.array_equal(r["nominal"][g], pc.nominal_of(case)[g])
            continue
        assert w[g, r["best"][g]] == 1 and w[g].max() == 1 and R[g, r["best"][g]] == R[g].max()
        assert (np.flatnonzero(R[g] == R[g].max())[0]) == r["best"][g]
        assert abs((w[g] / w[g].sum()).sum() - 1) < 1e-12               # the normalised weights sum to 1
        assert 1 - 1e-9 <= r["stats"][g, 2] <= K + 1e-9                 # effective sample size
        kn = r["knots"].reshape((G, K) + r["knots"].shape[1:])[g]
        assert (r["nominal"][g] >= kn.min(0) - 1e-12).all() and (r["nominal"][g] <= kn.max(0) + 1e-12).all()
        if case.temperature == 0:
            assert np.array_equal(r["nominal"][g], kn[r["best"][g]]) and w[g].sum() == 1
    # no weight in the subnormal range of f32: an exact zero is exact on every expf
    assert not ((r["weights"] > 0) & (r["weights"] < 1e-30)).any()
    if "underflow" in case.flags:
        assert (w[0, 1::2] == 0).all() and (pc.reference(case, f32=True)["weights"].reshape(G, K)[0, 1::2] == 0).all()


def test_the_cases_cover_what_they_claim():
    have = lambda f: {f(c) for c in pc.CASES}
    assert have(lambda c: c.K) >= {1, 2, 63, 64, 65, 257, 1025} and have(lambda c: c.G) == {1, 3}
    assert have(lambda c: (c.P, c.S)) >= {(1, 1), (2, 2), (5, 7), (5, 12), (1, 12), (2, 7)}
    assert have(lambda c: c.A) == {1, 4, 25, 50} and have(lambda c: c.kind) == {0, 1, 2}
    assert have(lambda c: c.temperature == 0) == {True, False} and have(lambda c: c.gamma) == {1.0, 0.9}
    assert have(lambda c: c.terminal) == {True, False} and any(c.env_offset for c in pc.CASES)
    assert any(c.step_pad and c.env_stride > 1 for c in pc.CASES)
    assert {f for c in pc.CASES for f in c.flags} == {"equal", "nan_one", "nan_group", "underflow"}
    clipped_lo = clipped_hi = zero_sigma = False
    for c in pc.CASES:
        sigma, lo, hi = pc.noise_of(c)
        k = pc.reference(c)["knots"]
        clipped_lo |= bool((k == lo.astype(np.float64)).any())
        clipped_hi |= bool((k == hi.astype(np.float64)).any())
        zero_sigma |= bool((sigma == 0).any())
        inp = pc.inputs_of(c)
        N = c.G * c.K
        assert inp.block.size >= (c.S - 1) * inp.step_stride + (N - 1) * inp.env_stride + 1 + inp.done_offset
    assert clipped_lo and clipped_hi and zero_sigma
    done_steps = set()
    for c in pc.CASES:
        d = pc.inputs_of(c).done
        done_steps |= {("first" if s == 0 else "last" if s == c.S - 1 else "mid") for s in np.flatnonzero(d.any(1)) if c.S >= 3}
    assert done_steps == {"first", "mid", "last"}


@pytest.mark.parametrize("mistake", ref.MISTAKES)
def test_every_planted_mistake_is_caught_by_a_case(mistake):
    """beyond the tolerance the device is held to: the knots beyond 4 x the Gaussian bound, the rest bitwise"""
    caught = []
    for c in pc.CASES:
        good, bad = pc.reference(c), pc.reference(c, mistake=mistake)
        knots_off = np.abs(bad["knots"] - good["knots"]).max() > 4 * pc.gaussian_bound(c)
        exact_off = any(not np.array_equal(bad[k], good[k]) for k in ("returns", "best"))
        shift_off = not np.array_equal(ref.shift_of(good["nominal"].astype(np.float32), c.kind, c.S, 1, True),
                                       ref.shift_of(good["nominal"].astype(np.float32), c.kind, c.S, 1, True, mistake))
        if knots_off or exact_off or shift_off:
            caught.append(c.name)
    assert caught, mistake


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_the_f32_run_deviates_wherever_a_tolerance_is_derived_from_it(case):
    if pc.gaussian(case).any():
        assert pc.gaussian_bound(case) > 0
    r = pc.reference(case)
    _, u32, bound, tol = pc.update_bounds(case, r["returns"].astype(np.float32), r["knots"].astype(np.float32), pc.nominal_of(case))
    if case.temperature > 0 and case.K > 1:
        assert bound["weights"] > 0 and bound["nominal"] > 0 and bound["ess"] > 0
    assert (tol["weights"] > 0).all() and (tol["nominal"] > 0).all() and (tol["ess"] > 0).all()
    # what the f32 run has exactly: best and the returns' own statistics
    assert np.array_equal(u32["best"], r["best"])
