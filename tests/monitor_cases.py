"""The cases of the episode monitor (include/trex_monitor.h), shared by tests/test_monitor_cases_host.py - which qualifies them on
tests/monitor_ref.py alone - and tests/test_gpu_monitor.py - which sends them through the C-ABI: seeded numpy arrays of reward, done,
reason and columns for T = 40 calls, plus reset marks at one chosen call. numpy only.

Sizes: N = 1 (one team), 2, 65 (just above a wavefront), 257 (just above an accumulate workgroup of one-lane teams; a ragged last
workgroup at every team size), 600 (more than two workgroups). Windows 1, 3, 100, 1000; column blocks (0, 0), (1, 0), (5, 3),
(32, 32). Done patterns: none; every env every call; Bernoulli 0.1; every env at one call with W < N; exactly W in one call."""
import collections

import numpy as np

import monitor_ref as MR

T = 40
Case = collections.namedtuple("Case", "name n window cols_a cols_b pattern env_offset seed burst_call nan_at reset_call pad")
# pattern: none | every | bernoulli | all_at (every env at burst_call, Bernoulli elsewhere) | exactly_w (exactly W envs at burst_call,
# Bernoulli elsewhere). nan_at: (call, env) of the one NaN reward. reset_call: before that call, the envs of reset_mask are
# abandoned. pad: (reward stride, done stride, columns beyond cols_a, columns beyond cols_b) of the buffers the device run uses.
CASES = [
    Case("n1_w1_every", 1, 1, 0, 0, "every", 0, 11, None, None, None, (1, 1, 0, 0)),
    Case("n2_w3_c1_bernoulli", 2, 3, 1, 0, "bernoulli", 5, 12, None, None, 17, (3, 2, 2, 0)),
    Case("n65_w100_c5_3_bernoulli_nan_marks", 65, 100, 5, 3, "bernoulli", 1000, 13, None, (30, 40), 21, (78, 78, 3, 1)),
    Case("n257_w3_c32_32_all_at_once", 257, 3, 32, 32, "all_at", 2 ** 32 - 257, 14, 23, None, None, (2, 5, 1, 7)),
    Case("n600_w1000_c5_3_every", 600, 1000, 5, 3, "every", 0, 15, None, None, 20, (1, 1, 0, 0)),
    Case("n600_w100_c1_exactly_w", 600, 100, 1, 0, "exactly_w", 77, 16, 19, None, None, (4, 4, 5, 0)),
    Case("n257_w100_none", 257, 100, 0, 0, "none", 0, 17, None, None, 20, (1, 3, 0, 0)),
    Case("n65_w1_c32_32_every", 65, 1, 32, 32, "every", 3, 18, None, None, None, (1, 1, 0, 0)),
    Case("n600_w3_c5_3_all_at_once_marks", 600, 3, 5, 3, "all_at", 9, 19, 30, None, 34, (7, 1, 2, 2)),
    Case("n257_w1000_c5_3_bernoulli", 257, 1000, 5, 3, "bernoulli", 0, 20, None, None, 20, (1, 1, 0, 0)),
]
BY_NAME = {c.name: c for c in CASES}


def arrays(case):
    """-> reward [T, n] f32, done [T, n] f32 (0 / 1), reason [T, n] i32 in 0..7 (set for every env, finished or not: the monitor reads
    it only where done is set), cols [T, n, C] f32"""
    g = np.random.default_rng(case.seed)
    n, C = case.n, case.cols_a + case.cols_b
    reward = g.normal(0.5, 2.0, (T, n)).astype(np.float32)
    reason = g.integers(0, 8, (T, n)).astype(np.int32)
    cols = g.normal(0.0, 1.0, (T, n, C)).astype(np.float32)
    coin = g.random((T, n)) < 0.1
    if case.pattern == "none":
        done = np.zeros((T, n), bool)
    elif case.pattern == "every":
        done = np.ones((T, n), bool)
    else:
        done = coin
        if case.pattern == "all_at":
            done[case.burst_call] = True
        elif case.pattern == "exactly_w":
            done[case.burst_call] = False
            done[case.burst_call, g.choice(n, case.window, replace=False)] = True
    if case.nan_at is not None:
        reward[case.nan_at] = np.nan
    return reward, done.astype(np.float32), reason, cols


def reset_mask(case):
    """the envs abandoned before call reset_call: every other env - half of them"""
    return (np.arange(case.n) % 2 == 1) if case.n > 1 else np.ones(1, bool)


def run(case, mistake=None, calls=T):
    """the reference over the case -> ([state after every call], the summary after the last, the mean bounds, the monitor)"""
    reward, done, reason, cols = arrays(case)
    m = MR.Monitor(case.n, case.window, case.cols_a + case.cols_b, case.env_offset, mistake)
    states = []
    for t in range(calls):
        if t == case.reset_call:
            m.reset(reset_mask(case))
        m.apply(reward[t], done[t], reason[t], cols[t])
        states.append(m.state())
    return states, m.summary(), m.mean_bounds(), m


def _bits(x):
    """an array as the bytes compare it: the header's u32 arrays are i32 where a device run hands them out"""
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.uint32 else x


def same_state(a, b):
    """bitwise, key by key -> the keys that differ"""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            x, y = _bits(x), _bits(y)
            if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad


def summary_failures(got, want, bounds):
    """counts and extrema exact, means within the bound of an n-term f64 sum in any order -> [what differs]"""
    bad = []
    exact = [MR.N, MR.RET_MIN, MR.RET_MAX, MR.LEN_MIN, MR.LEN_MAX, MR.TOTAL, MR.T] + list(range(MR.WIN_REASON, MR.WIN_REASON + 4)) \
        + list(range(MR.BY_REASON, MR.BY_REASON + 4))
    for k in exact:
        if not (got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k]))):
            bad.append((k, got[k], want[k]))
    means = [(MR.RET_MEAN, bounds[0]), (MR.LEN_MEAN, bounds[1])] + [(MR.SUMMARY + c, b) for c, b in enumerate(bounds[2])]
    for k, bound in means:
        if np.isnan(want[k]) or np.isnan(got[k]):
            if not (np.isnan(want[k]) and np.isnan(got[k])):
                bad.append((k, got[k], want[k]))
        elif not abs(got[k] - want[k]) <= bound:
            bad.append((k, got[k], want[k], bound))
    return bad
