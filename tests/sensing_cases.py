"""The cases of the sensor-model tests and the comparison they share: seeded row blocks with planted done flags, group layouts, and
compare(), which holds what a device run (tests/test_gpu_sensing.py) - or a deliberately mistaken reference
(tests/test_sensing_cases_host.py, which qualifies these cases) - must satisfy against the f64 reference tests/sensing_ref.py.
numpy only: no torch, no device. A helper, not a conftest.

The comparison, per column class:
    uncovered columns and the tail           bitwise the input
    no noise, no bias, no resolution         bitwise the delayed clean value: the delay pattern shows k, ep and the drawn delays
    uniform noise and / or bias              within 2 ulp (f32) of the largest operand - the two products, the partial sums
    Gaussian noise                           within 4 x the case's own bound: the largest deviation of the reference's f32 run from
                                             its f64 run over the case's Gaussian columns (the device's logf and cosf are not numpy's)
    with a resolution                        bitwise quantum * rintf(t) wherever the reference's unrounded t lies farther from a
                                             rounding boundary than the column's bound above (times inv_quantum, plus the rounding
                                             of the product itself); the share left out is at most 1 % per case
"""
import collections

import numpy as np

import sensing_ref as SR

G, U = SR.GAUSSIAN, SR.UNIFORM
STEPS = 20          # the 9-slot ring wraps twice
Case = collections.namedtuple("Case", "name model n D tail groups seed env_offset in_place pad done_rate")


def mixed(D):
    """six groups with one feature mix each, the rest of the row uncovered; (5, 7) straddles Philox blocks 1 and 2"""
    assert D >= 75
    return [(5, 7, G, 0.1, 0.0, 0.0, 0, 8), (12, 20, U, 0.05, 0.03, 0.0, 1, 1), (32, 8, G, 0.0, 0.0, 0.0, 8, 8),
            (40, 10, G, 0.02, 0.01, 0.01, 0, 0), (50, 12, U, 0.03, 0.0, 0.01, 0, 2), (62, 13, G, 0.0, 0.5, 0.0, 0, 0)]


def sixty_four(D):
    """64 groups that tile [0, D): widths D // 64 and one more for the first D % 64; the features cycle"""
    menu = [(G, 0.05, 0.0, 0.0, 0, 0), (U, 0.1, 0.02, 0.0, 0, 1), (G, 0.0, 0.0, 0.0, 0, 8), (G, 0.2, 0.1, 0.0, 8, 8),
            (U, 0.02, 0.0, 0.01, 1, 1), (G, 0.03, 0.0, 0.01, 0, 0), (G, 0.0, 0.0, 0.0, 0, 0)]
    out, col = [], 0
    for g in range(64):
        w = D // 64 + (1 if g < D % 64 else 0)
        out.append((col, w) + menu[g % len(menu)])
        col += w
    assert col == D
    return out


CASES = [
    Case("slab_n1", "slab", 1, 3, 2, [(0, 3, G, 0.1, 0.05, 0.0, 1, 1)], 11, 0, True, 0, 0.15),
    Case("trex_n63_mixed", "trex", 63, 75, 2, mixed(75), 12, 0, False, 3, 0.1),
    Case("locomotion_n64_one_group", "locomotion", 64, 93, 2, [(0, 93, G, 0.05, 0.02, 0.0, 0, 8)], 13, 0, True, 0, 0.1),
    Case("external_n65_64_groups", "external", 65, 512, 2, sixty_four(512), 14, 1000, False, 5, 0.1),
    Case("penalties_n257_64_groups", "penalties", 257, 75, 5, sixty_four(75), 2 ** 40 + 15, 7, True, 0, 0.1),
]


def rows_of(case, t):
    """the block of step t: [n, D + tail] f32, unit-scale values that differ from step to step, a reward, planted done flags"""
    rng = np.random.default_rng([case.seed % 2 ** 32, t, 99])
    rows = rng.normal(size=(case.n, case.D + case.tail)).astype(np.float32)
    rows[:, case.D + 1] = (rng.random(case.n) < case.done_rate).astype(np.float32)
    return rows


def reference(case, f32=False, mistake=None, steps=STEPS, env_offset=None, n=None, seed=None, inputs=None):
    """-> [Applied] over the steps; inputs: the row blocks (default rows_of)"""
    s = SR.Sensors(case.n if n is None else n, case.D, case.tail, case.groups, case.seed if seed is None else seed,
                   case.env_offset if env_offset is None else env_offset, f32=f32, mistake=mistake)
    return [s.apply(rows_of(case, t) if inputs is None else inputs[t]) for t in range(steps)], s


def column_classes(case):
    """per observation column: covered, gaussian (noise > 0), soft (bias or uniform noise > 0), quantised"""
    D = case.D
    cov, gau, soft, qua = (np.zeros(D, bool) for _ in range(4))
    for c0, w, kind, noise, bias, quantum, _, _ in case.groups:
        s = slice(c0, c0 + w)
        cov[s] = True
        gau[s] = kind == G and noise > 0
        soft[s] = bias > 0 or (kind == U and noise > 0)
        qua[s] = quantum > 0
    return cov, gau, soft, qua


_BOUNDS = {}


def gaussian_bound(case, inputs=None):
    """the largest |f32 run - f64 run| of the reference over the case's Gaussian columns, before the resolution (0 if none);
    inputs: the row blocks the case is run on (default rows_of over STEPS steps, computed once)"""
    if inputs is not None or case.name not in _BOUNDS:
        _, gau, _, _ = column_classes(case)
        steps = STEPS if inputs is None else len(inputs)
        r64, _ = reference(case, steps=steps, inputs=inputs)
        r32, _ = reference(case, f32=True, steps=steps, inputs=inputs)
        b = float(max(np.abs(a.y - b.y)[:, gau].max(initial=0.0) for a, b in zip(r64, r32)))
        if inputs is not None:
            return b
        _BOUNDS[case.name] = b
    return _BOUNDS[case.name]


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def compare(case, ref64, got, inputs=None, factor=4.0):
    """ref64: [Applied] of the f64 reference; got: [[n, D + tail] f32 arrays], one per step. -> dict(failures=[text],
    gaussian_share=largest Gaussian deviation / the bound, left_out=share of quantised values not compared, ulps=largest
    deviation of the soft columns in ulp of the largest operand)"""
    cov, gau, soft, qua = column_classes(case)
    D = case.D
    bound = factor * gaussian_bound(case, inputs)
    fails, g_share, ulps, left, total = [], 0.0, 0.0, 0, 0
    for t, (ref, g) in enumerate(zip(ref64, got)):
        g = np.asarray(g)
        assert g.dtype == np.float32 and g.shape == (case.n, D + case.tail), (g.dtype, g.shape)
        rows = rows_of(case, t) if inputs is None else inputs[t]
        g64 = g.astype(np.float64)
        plain = np.concatenate([~cov, np.ones(case.tail, bool)])
        if g[:, plain].tobytes() != rows[:, plain].tobytes():
            fails.append("step %d: an uncovered column or the tail moved" % t)
        exact = cov & ~gau & ~soft & ~qua
        if g[:, :D][:, exact].tobytes() != ref.delayed[:, exact].astype(np.float32).tobytes():
            fails.append("step %d: a delayed column differs (k, ep or a drawn delay)" % t)
        tol = 2.0 * ulp32(ref.opmax)                               # per value
        col_tol = np.where(gau[None, :], bound, tol)
        err = np.abs(g64[:, :D] - ref.y)
        sel = cov & ~qua & ~exact
        if sel.any():
            over = err[:, sel] > col_tol[:, sel]
            if over.any():
                fails.append("step %d: %d values beyond their bound (largest %.3g against %.3g)"
                             % (t, int(over.sum()), err[:, sel][over].max(), col_tol[:, sel][over].max()))
            if (sel & gau).any() and bound > 0:
                g_share = max(g_share, float(err[:, sel & gau].max() / bound))
            if (sel & ~gau).any():
                ulps = max(ulps, float((err[:, sel & ~gau] / ulp32(ref.opmax)[:, sel & ~gau]).max()))
        if qua.any():
            tt = ref.t[:, qua]
            inv = np.array([1.0 / q for q in _quanta(case)])[qua][None, :]
            margin = (np.maximum(col_tol[:, qua], ulp32(ref.y[:, qua]))) * inv + ulp32(tt)
            dist = np.abs(tt - (np.floor(tt) + 0.5))
            safe = dist > margin
            want = (np.array(_quanta(case), np.float32)[qua][None, :] * np.rint(tt).astype(np.float32)).astype(np.float32)
            bad = safe & (g[:, :D][:, qua] != want)
            if bad.any():
                fails.append("step %d: %d quantised values off their level" % (t, int(bad.sum())))
            left += int((~safe).sum())
            total += safe.size
    left_out = left / total if total else 0.0
    if left_out > 0.01:
        fails.append("%.2f %% of the quantised values lie too close to a boundary to compare" % (100 * left_out))
    return dict(failures=fails, gaussian_share=g_share, left_out=left_out, ulps=ulps)


def _quanta(case):
    q = np.ones(case.D)
    for c0, w, _, _, _, quantum, _, _ in case.groups:
        if quantum > 0:
            q[c0:c0 + w] = float(np.float32(quantum))
    return q


# ---- the action delay
def action_rows(seed, t, n, cols):
    return np.random.default_rng([seed, t, 7]).normal(size=(n, cols)).astype(np.float32)


def done_flags(seed, t, n, rate=0.15):
    return (np.random.default_rng([seed, t, 8]).random(n) < rate).astype(np.uint8)
