"""The episode monitor on the device (include/trex_monitor.h; csrc/monitor.hip) against tests/monitor_ref.py:
 1 through the C-ABI alone, the cases of tests/monitor_cases.py call by call: ring, running episode, episode counts, last records,
   total, by_reason and t bitwise, the summary's counts and extrema exact and its means within the bound of an n-term f64 sum;
   guard-padded outputs, strided inputs left as they were;  2 a second batch repeats the first bitwise;
 3 refusals launch nothing and change nothing;  4 eight applies captured and replayed three times equal 32 eager applies on a twin;
 5 clear and set again: every env afresh;  6 through TrexVecEnv, pair and single step form, against a host recomputation from what
   step_tensor returned;  7 fall reasons read from the batch's own buffer;  8 reset_tensor(mask), step_many_tensor, and an env
   without a monitor."""
import ctypes as C

import numpy as np
import pytest
import torch

import monitor_cases as MC
import monitor_ref as MR
from gpu_support import DEV, guarded, guards_intact, make_vec, random_action_steps, refused, same_bits

pytestmark = pytest.mark.gpu
J = 25
INVALID = -1
FILL = 3.0


def api_of(v, window, cols_a=0, cols_b=0, env_offset=0):
    from trex_gym import monitor_capi
    api = monitor_capi.BatchMonitor(v.batch)
    api.set(window, cols_a, cols_b, env_offset)
    return api


def read(api, n):
    """-> (the state as monitor_ref.Monitor.state() gives it, the summary f64 [SUMMARY + C]), through guard-padded buffers"""
    from trex_gym import monitor_capi as M
    W, Cn = api.window, api.cols
    shapes = dict(ring_cols=(W, Cn), last_cols=(n, Cn))
    bufs = {}
    for fields, count in ((M.RING_FIELDS, W), (M.ENV_FIELDS, n)):
        for name, dtype in fields:
            shape = shapes.get(name, (count,))
            if int(np.prod(shape)) == 0:
                continue
            kind = getattr(torch, dtype)
            bufs[name] = (shape, 7.0 if kind.is_floating_point else 7) + guarded(shape, fill=7.0 if kind.is_floating_point else 7, dtype=kind)
    swhole, sview = guarded((M.SUMMARY + Cn,), dtype=torch.float64)
    assert api.info(**{k: b[3] for k, b in bufs.items()}) == (W, Cn)
    api.summary(sview)
    torch.cuda.synchronize()
    assert guards_intact(swhole, (M.SUMMARY + Cn,))
    state = {}
    for name, (shape, fill, whole, view) in bufs.items():
        assert guards_intact(whole, shape, fill=fill), name
        state[name] = view.cpu().numpy()
    for name, shape in shapes.items():
        state.setdefault(name, np.zeros(shape, np.float32))
    s = sview.cpu().numpy()
    state.update(total=int(s[M.TOTAL]), by_reason=s[M.BY_REASON:M.BY_REASON + 4].astype(np.uint64), t=int(s[M.T]))
    return state, s


def device_inputs(case):
    """the case's arrays on the device as the strided, padded buffers the header allows: reward and done in the last column of a
    [T, n, stride] block, the columns in the first columns of [T, n, width + pad] blocks, every other element FILL"""
    reward, done, reason, cols = MC.arrays(case)
    rs, ds, pa, pb = case.pad
    T, n = reward.shape

    def block(values, width, last):
        b = np.full((T, n, width), FILL, np.float32)
        if values.shape[-1]:
            if last:
                b[:, :, width - values.shape[-1]:] = values
            else:
                b[:, :, :values.shape[-1]] = values
        return torch.as_tensor(b, device=DEV)
    ca = case.cols_a
    return dict(reward=block(reward[:, :, None], rs, True), done=block(done[:, :, None], ds, True),
                reason=torch.as_tensor(reason, device=DEV),
                cols_a=block(cols[:, :, :ca], ca + pa, False) if ca else None,
                cols_b=block(cols[:, :, ca:], case.cols_b + pb, False) if case.cols_b else None)


def apply_call(api, case, inp, t):
    rs, ds = case.pad[:2]
    api.apply(inp["reward"][t], inp["done"][t], inp["reason"][t], None if inp["cols_a"] is None else inp["cols_a"][t],
              None if inp["cols_b"] is None else inp["cols_b"][t], rs - 1, ds - 1)


def run_case(api, case, inp, calls=MC.T):
    got = []
    for t in range(calls):
        if t == case.reset_call:
            api.reset(torch.as_tensor(MC.reset_mask(case), device=DEV))
        apply_call(api, case, inp, t)
        got.append(read(api, case.n))
    return got


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c.name)
def test_cases_against_the_reference(case):
    v = make_vec(case.n)
    inp = device_inputs(case)
    before = {k: x.clone() for k, x in inp.items() if x is not None}
    got = run_case(api_of(v, case.window, case.cols_a, case.cols_b, case.env_offset), case, inp)
    states, summary, bounds, _ = MC.run(case)
    for t, ((state, _), want) in enumerate(zip(got, states)):
        assert not MC.same_state(want, state), (t, MC.same_state(want, state))
    bad = MC.summary_failures(got[-1][1], summary, bounds)
    err = np.abs(got[-1][1] - summary)
    print("%s: summary |device - reference| at most %.3g, bound of the return mean %.3g" % (case.name, np.nanmax(err), bounds[0]))
    assert not bad, bad
    for k, x in before.items():
        assert same_bits(x, inp[k]), k                    # the caller's blocks are as they were


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n65_w100_c5_3_bernoulli_nan_marks", "n600_w3_c5_3_all_at_once_marks"])
def test_a_second_batch_repeats_the_first_bitwise(name):
    case = MC.BY_NAME[name]
    inp = device_inputs(case)
    runs = []
    for _ in range(2):
        api = api_of(make_vec(case.n), case.window, case.cols_a, case.cols_b, case.env_offset)
        for t in range(MC.T):
            if t == case.reset_call:
                api.reset(torch.as_tensor(MC.reset_mask(case), device=DEV))
            apply_call(api, case, inp, t)
        runs.append(read(api, case.n))
    assert not MC.same_state(runs[0][0], runs[1][0]) and runs[0][1].tobytes() == runs[1][1].tobytes()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_change_nothing():
    from trex_gym import monitor_capi
    from trex_gym._capi import lib
    case = MC.BY_NAME["n65_w100_c5_3_bernoulli_nan_marks"]
    n, v = case.n, make_vec(case.n)
    inp = device_inputs(case)
    bare = monitor_capi.BatchMonitor(v.batch)
    ones = torch.ones(n, device=DEV)
    refused(INVALID, bare.apply, ones, ones)                                        # no monitor set
    refused(INVALID, bare.reset)
    refused(INVALID, bare.summary)
    refused(INVALID, bare.info, ret=torch.zeros(n, dtype=torch.float64, device=DEV))
    assert bare.info() == (0, 0)
    for w, a, b, off in ((-1, 0, 0, 0), (65537, 0, 0, 0), (10, -1, 0, 0), (10, 0, -1, 0), (10, 33, 32, 0), (10, 1, 1, 2 ** 32 - n + 1)):
        refused(INVALID, bare.set, w, a, b, off)                                    # W or C out of range, env_offset + N beyond 2^32
    api = api_of(v, case.window, case.cols_a, case.cols_b, case.env_offset)
    rs, ds, pa, pb = case.pad
    stream = v.batch._stream(None)
    p = lambda x: C.c_void_p(x.data_ptr())
    raw = lambda **kw: lib.trex_batch_monitor_apply(v.batch.h, *[kw.get(k, d) for k, d in (
        ("reward", p(inp["reward"][0])), ("rs", rs), ("done", p(inp["done"][0])), ("ds", ds), ("reason", p(inp["reason"][0])),
        ("a", p(inp["cols_a"][0])), ("sa", case.cols_a + pa), ("b", p(inp["cols_b"][0])), ("sb", case.cols_b + pb))], stream)
    host = torch.zeros(n * 80)
    for t in range(6):
        if t == 2:
            state, summary = read(api, n)
            kept = {k: x.clone() for k, x in inp.items()}
            for w, a, b, off in ((-1, 0, 0, 0), (65537, 0, 0, 0), (10, 33, 32, 0), (10, 1, 1, 2 ** 32 - n + 1)):
                refused(INVALID, monitor_capi.BatchMonitor(v.batch).set, w, a, b, off)   # a refused set: the monitor in force intact
            for bad in (dict(reward=None), dict(done=None), dict(a=None), dict(b=None),          # a missing block whose width is not 0
                        dict(rs=0), dict(ds=0), dict(ds=-1), dict(sa=case.cols_a - 1), dict(sb=case.cols_b - 1), dict(sa=0),   # strides
                        dict(reward=p(host)), dict(done=p(host)), dict(reason=p(host)), dict(a=p(host)), dict(b=p(host)),      # host memory
                        dict(rs=2 ** 26), dict(sa=2 ** 26)):                                      # a short buffer: n rows of 2^26 floats
                assert raw(**bad) == INVALID, bad
            refused(INVALID, api.apply, torch.zeros(n - 1, device=DEV), ones)                    # short buffers, by the binding
            refused(INVALID, api.apply, ones, ones, None, torch.zeros(n, case.cols_a - 1, device=DEV), inp["cols_b"][0])
            refused(INVALID, api.apply, ones, ones, torch.zeros(n - 1, dtype=torch.int32, device=DEV), inp["cols_a"][0], inp["cols_b"][0])
            refused(INVALID, api.reset, torch.ones(n - 1, dtype=torch.uint8, device=DEV))
            refused(INVALID, api.reset, torch.ones(n, dtype=torch.uint8))
            refused(INVALID, api.summary, torch.zeros(monitor_capi.SUMMARY + api.cols - 1, dtype=torch.float64, device=DEV))
            refused(INVALID, api.summary, torch.zeros(monitor_capi.SUMMARY + api.cols, dtype=torch.float64))
            refused(INVALID, api.info, ring_return=torch.zeros(case.window - 1, device=DEV))
            refused(INVALID, api.info, last_cols=torch.zeros(n * api.cols - 1, device=DEV))
            if torch.cuda.device_count() > 1:                                                     # another device's memory
                other = torch.ones(n, device="cuda:1")
                assert raw(reward=p(other), rs=1) == INVALID
            again, summary2 = read(api, n)
            assert not MC.same_state(state, again) and summary.tobytes() == summary2.tobytes()
            for k, x in kept.items():
                assert same_bits(x, inp[k]), k
        apply_call(api, case, inp, t)
    want = MC.run(case, calls=6)[0][-1]
    assert not MC.same_state(want, read(api, n)[0])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_eight_captured_applies_replayed_three_times_equal_32_eager_applies():
    """the state lives on the device, so a replay is the NEXT eight calls (gpu_support.replay_equals_eager expects one result from
    every replay - not what launches that count do; the skeleton is its own: eight eager calls that learn the buffers, the same
    eight captured on a side stream - a capture runs nothing -, three replays)"""
    case = MC.BY_NAME["n257_w1000_c5_3_bernoulli"]
    inp = device_inputs(case)
    a, b = (api_of(make_vec(case.n), case.window, case.cols_a, case.cols_b, case.env_offset) for _ in range(2))

    def eight(api):
        for t in range(8):
            apply_call(api, case, inp, t)
    for _ in range(4):
        eight(b)
    eight(a)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eight(a)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got, want = read(a, case.n), read(b, case.n)
    del graph
    assert want[0]["t"] == 32 and want[0]["total"] > case.n // 2
    assert not MC.same_state(want[0], got[0]) and want[1].tobytes() == got[1].tobytes()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_clear_and_set_again_starts_every_env_afresh():
    case = MC.BY_NAME["n65_w100_c5_3_bernoulli_nan_marks"]
    inp = device_inputs(case)
    v = make_vec(case.n)
    api = api_of(v, case.window, case.cols_a, case.cols_b, case.env_offset)
    for t in range(10):
        apply_call(api, case, inp, t)
    assert read(api, case.n)[0]["total"] > 0
    assert api.set(0) == 0 and api.info() == (0, 0)
    refused(INVALID, api.apply, torch.ones(case.n, device=DEV), torch.ones(case.n, device=DEV))
    api.set(case.window, case.cols_a, case.cols_b, case.env_offset)
    state, summary = read(api, case.n)
    assert all(not np.asarray(x).any() for x in state.values()) and np.isnan(summary[MR.RET_MEAN]) and summary[MR.N] == 0
    got = run_case(api, case, inp, calls=12)
    assert not MC.same_state(MC.run(case, calls=12)[0][-1], got[-1][0])


# 6 ------------------------------------------------------------------------------------------------------------------------
def host_records(steps, env_offset=0):
    """the records of a run recomputed on the host in f64 from what every step returned: [(rew, done, terms, reason)] ->
    [(return f32, length, reason, env, t, cols f32)] in the order they finished"""
    n = len(steps[0][0])
    ret, length, col = np.zeros(n), np.zeros(n, np.int64), np.zeros((n, steps[0][2].shape[1]))
    out = []
    for t, (rew, done, terms, reason) in enumerate(steps):
        ret += rew.astype(np.float64)
        length += 1
        col += terms.astype(np.float64)
        for e in np.flatnonzero(done):
            out.append((np.float32(ret[e]), int(length[e]), int(reason[e]), env_offset + e, t, col[e].astype(np.float32)))
            ret[e], length[e], col[e] = 0.0, 0, 0.0
    return out


def ring_records(state, count):
    """the last min(count, W) records of the ring, oldest first"""
    W = len(state["ring_return"])
    return [(state["ring_return"][j % W], int(state["ring_length"][j % W]), int(state["ring_reason"][j % W]),
             int(state["ring_env"][j % W]), int(state["ring_t"][j % W]), state["ring_cols"][j % W]) for j in range(max(0, count - W), count)]


def same_records(got, want):
    return len(got) == len(want) and all(
        np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1:5] == b[1:5] and a[5].tobytes() == b[5].tobytes()
        for a, b in zip(got, want))


@pytest.mark.parametrize("n", [66, 65], ids=["pair_n66", "single_n65"])
def test_through_the_env_against_a_host_recomputation(n):
    from trex_gym import monitor, rewards as R
    v = make_vec(n, max_episode_steps=5, rewards=[R.alive(0.5), R.joint_vel(-1.0e-4)])
    monitor.attach(v, window=1000)
    assert v.monitor == dict(window=1000, terms=True) and (v.monitor_api.cols_a, v.monitor_api.cols_b) == (2, 0)
    v.reset_tensor()
    v.set_episode_steps(torch.arange(n, device=DEV, dtype=torch.int32) % 5)
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=v.model.lower, q_upper=v.model.upper), 14, n, 5)
    steps = []
    for t in range(14):
        _, rew, done = v.step_tensor(actions[t])
        steps.append((rew.cpu().numpy().copy(), done.cpu().numpy().copy(), v.reward_terms.cpu().numpy().copy(), np.zeros(n, np.int32)))
    want = host_records(steps, v.env_lo)
    assert len(want) >= 2 * n                                   # (the condition, on the host recomputation)
    assert len({w[0].tobytes() for w in want}) > n              # returns that differ: the rewards are not constants
    state, summary = read(v.monitor_api, n)
    assert state["total"] == len(want) and state["t"] == 14
    assert same_records(ring_records(state, len(want)), want)
    stats = monitor.episode_stats(v)
    assert stats["episodes"] == len(want) and stats["end_reasons"]["limit"] == 1.0 and set(stats["terms"]) == set(v.reward_names)
    assert abs(stats["eplenmean"] - np.mean([w[1] for w in want])) < 1e-12
    last = monitor.last_episode(v)
    by_env = {w[3] - v.env_lo: w for w in want}                 # (the last record of every env)
    for e, w in by_env.items():
        assert last["return"][e].cpu().numpy().tobytes() == w[0].tobytes() and int(last["length"][e]) == w[1] and int(last["t"][e]) == w[4]
    assert last["episodes"].cpu().numpy().tolist() == [sum(1 for w in want if w[3] - v.env_lo == e) for e in range(n)]


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_fall_reasons_are_read_from_the_batch_s_own_buffer():
    """fallen start states and the thresholds of tests/termination_cases.py (computed once per process and shared with
    tests/test_gpu_termination.py through that module's cache), an episode limit of 7, staggered: within 20 steps some envs fall
    and others reach the limit. reason_dev is NULL: the monitor reads what the predicate launch left."""
    import termination_cases as TC
    from test_gpu_termination import fallen_idx, load, thr_kwargs
    from trex_gym import monitor
    n, T = 12, 20
    thr = TC.search("hulls")
    _, cases = TC.states("hulls")
    v = make_vec(n, collision="hulls", max_episode_steps=7)
    load(v, cases, fallen_idx(n, offset=5))
    v.set_termination(**thr_kwargs(thr, 1.5))
    v.set_episode_steps(torch.arange(n, device=DEV, dtype=torch.int32) % 7)
    monitor.attach(v, window=50, terms=False)
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=v.model.lower, q_upper=v.model.upper), T, n, 8)
    steps = []
    for t in range(T):
        _, rew, done = v.step_tensor(actions[t])
        steps.append((rew.cpu().numpy().copy(), done.cpu().numpy().copy(), np.zeros((n, 0), np.float32), v.termination_reason.cpu().numpy().copy()))
    want = host_records(steps)
    reasons = [w[2] for w in want]
    assert any(r == 0 for r in reasons) and any(r != 0 for r in reasons), reasons      # (the condition, on the host recomputation)
    state, summary = read(v.monitor_api, n)
    assert same_records(ring_records(state, len(want)), want[-50:])
    by_reason = [sum(1 for r in reasons if r == 0)] + [sum(1 for r in reasons if r & bit) for bit in (1, 2, 4)]
    assert state["by_reason"].tolist() == by_reason and state["total"] == len(want)
    stats = monitor.episode_stats(v)
    assert stats["end_counts"] == dict(zip(("limit", "head", "tilt", "clearance"), by_reason))


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_reset_tensor_abandons_the_running_episode():
    from trex_gym import monitor
    n = 9
    v = make_vec(n, max_episode_steps=4)
    monitor.attach(v, window=20)
    v.reset_tensor()
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=v.model.lower, q_upper=v.model.upper), 6, n, 3)
    mask = torch.arange(n, device=DEV) % 3 == 0
    steps = []
    for t in range(6):
        if t == 2:
            v.reset_tensor(mask)
        _, rew, done = v.step_tensor(actions[t])
        steps.append((rew.cpu().numpy().copy(), done.cpu().numpy().copy()))
    state, _ = read(v.monitor_api, n)
    m = mask.cpu().numpy()
    # the others end at step 3 with four rows; the marked ones started over at step 2: they end at step 5, with four rows again
    assert state["total"] == n and (state["last_length"] == 4).all() and (state["episodes"] == 1).all()
    assert (state["last_t"][m] == 5).all() and (state["last_t"][~m] == 3).all()
    for e in range(n):
        rows = range(2, 6) if m[e] else range(0, 4)
        ret = 0.0
        for t in rows:
            ret += float(steps[t][0][e])
        assert state["last_return"][e].tobytes() == np.float32(ret).tobytes()


def test_step_many_equals_six_step_calls():
    from trex_gym import monitor
    n, S = 65, 6
    a, b = make_vec(n, max_episode_steps=4), make_vec(n, max_episode_steps=4)
    for v in (a, b):
        monitor.attach(v, window=100)
        v.reset_tensor()
        v.set_episode_steps(torch.arange(n, device=DEV, dtype=torch.int32) % 4)
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=a.model.lower, q_upper=a.model.upper), S, n, 6)
    a.step_many_tensor(actions)
    for s in range(S):
        b.step_tensor(actions[s])
    (sa, ma), (sb, mb) = read(a.monitor_api, n), read(b.monitor_api, n)
    assert sa["total"] >= n and sa["t"] == S
    assert not MC.same_state(sa, sb) and ma.tobytes() == mb.tobytes()


def test_without_attach_nothing_changes():
    """the rows of 10 steps: an env that had a monitor attached and taken off again, and one with a monitor, are bitwise the rows of
    an env that never had one"""
    from trex_gym import monitor
    n = 65
    actions = None
    runs = []
    for mode in ("never", "cleared", "attached"):
        v = make_vec(n, max_episode_steps=4)
        if mode != "never":
            monitor.attach(v, window=10)
        if mode == "cleared":
            monitor.attach(v, None)
            assert v.monitor_api is None and v.monitor is None
        v.reset_tensor()
        if actions is None:
            actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=v.model.lower, q_upper=v.model.upper), 10, n, 7)
        rows = []
        for t in range(10):
            v.step_tensor(actions[t])
            rows.append(v.rows.clone())
        runs.append(torch.stack(rows))
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])
