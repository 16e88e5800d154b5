"""The motion clip on the GPU (trex_batch_set_motion / _motion_sample / _set_motion_reward / _compose_motion_reward / _motion_reset,
include/trex_motion.h) against the f64 restatement tests/motion_ref.py - itself pinned by tests/test_motion_ref.py: the sampled
reference at knots, between them, at and beyond the ends, over many cycles and along segments of 179 and 0.01 degrees; every
term kind alone and together at the 8-env workgroup's edges; the composed column as the ordered f32 sum of the breakdown; the
clock and held values through done rows; reference state initialisation under every mask, with and without warm-start records;
refusals; stream capture; the env with a clip attached, RSI included; and the trainer.

Tolerances: motion_ref.sample_bound for a sampled column, motion_ref.bound(kind, case) for a term's value, times |weight|, plus one
rounding of the product; held values (done rows) are compared bitwise with the step before. The largest deviation / bound seen is
printed (-s) and recorded in profiles/r24_motion.txt."""
import numpy as np
import pytest
import torch

import link_state_ref as L
import motion_cases as MC
import motion_ref as MR
from gpu_support import DEV, guarded, guards_intact, loaded_vec, make_vec, random_actions, refused, replay_equals_eager, same_bits
from state_sets import case_states
from tolerances import LINK_TOL

pytestmark = pytest.mark.gpu
NB, J = 26, 25
W = 13 + 2 * J
U = MR.U
INVALID = -1
KIND_NAMES = ["pose", "velocity", "end_effector", "root_pose", "root_velocity"]
WORST = {}                                  # what -> largest deviation / bound seen in this process


def worst(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def report():
    print("motion deviation / bound, largest: " + "  ".join("%s %.3f" % (k, WORST[k]) for k in sorted(WORST)))


def mapi(v):
    """the motion calls of the env's batch (trex_gym.motion_capi.BatchMotion): the env's own, or one made for a plain env"""
    if v.motion_api is None:
        from trex_gym import motion_capi
        v.motion_api = motion_capi.BatchMotion(v.batch)
    return v.motion_api


def set_clip(v, model, frames, loop=False, K=0, velocities=None, dt=MC.DT, probe_set=7):
    """the clip on the device with K end effectors -> (the reference's table, (links, points) or None)"""
    probes = None
    if K:
        ee = MC.end_effector_links(model, K)
        assert len(ee) == K
        probes = ([l for l, _ in ee], np.array([p for _, p in ee]))
        v.batch.set_link_probes(probe_set, probes[0], probes[1])
    assert mapi(v).set_motion(frames, dt, loop, velocities, probe_set if K else -1) == len(frames)
    return MR.device_table(MR.build_table(model, frames, velocities, dt, loop)), probes


def sample(v, times, K=0, J=J):
    """motion_sample into guarded buffers -> (state, points or None, phase) as numpy"""
    n, W = v.num_envs, 13 + 2 * J
    ws, s = guarded((n, W), fill=float("nan"))
    wp, p = guarded((n, max(K, 1), 3), fill=float("nan"))
    wf, f = guarded((n,), fill=float("nan"))
    mapi(v).sample(None if times is None else torch.as_tensor(times, dtype=torch.float32, device=DEV), s, p if K else None, f)
    torch.cuda.synchronize()
    assert guards_intact(ws, (n, W), fill=float("nan")) and guards_intact(wf, (n,), fill=float("nan"))
    assert guards_intact(wp, (n, max(K, 1), 3), fill=float("nan")) and (K or bool(torch.isnan(p).all()))
    return s.clone(), (p.clone() if K else None), f.clone()


def check_sample(model, tab, probes, times, state, points, phase, what="sample", J=J):
    state, phase = state.cpu().numpy().astype(np.float64), phase.cpu().numpy()
    assert np.isfinite(state).all()
    for e, t in enumerate(np.asarray(times, np.float32)):
        want, ph = MR.sample(tab, t)
        b = MR.sample_bound(tab, t)
        worst(what, (np.abs(state[e] - want) / b).max())
        assert (np.abs(state[e] - want) <= b).all(), (e, t, np.abs(state[e] - want).max())
        assert abs(float(phase[e]) - ph) <= 2.0 ** -23, (e, t, phase[e], ph)
        if probes is not None:
            pos = L.link_state(model, want, probes[0], probes[1])["position"]
            got = points[e].cpu().numpy().astype(np.float64)
            # the link query's tolerance, and the reference's own rounding carried down the chain (motion_ref.evaluate)
            reach = np.abs(pos - want[:3]).max() + 1.0
            tol = LINK_TOL["pose"] * max(1.0, np.abs(pos).max()) + (b[13:13 + J].sum() + 2 * b[3:7].sum()) * reach + b[:3].max()
            worst(what + " points", np.abs(got - pos).max() / tol)
            assert np.abs(got - pos).max() <= tol, (e, t, np.abs(got - pos).max(), tol)


def time_list(n, T, dt=MC.DT, F=33):
    """knots (exact in f32), mid-segment times, 0, T, beyond T, negative: env e takes entry e of the cycle"""
    rng = np.random.default_rng(n)
    knots = rng.integers(0, F, 6) * dt
    mids = rng.uniform(0, T, 6)
    base = np.concatenate([knots, mids, [0.0, T, 1.7 * T, -0.3, (F - 2) * dt, T - 1e-6]])
    return base[np.arange(n) % len(base)].astype(np.float32)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(1, 0), (63, 1), (64, 8), (65, 8), (257, 1)])
def test_sample_against_reference(n, K, model):
    v = make_vec(n)
    v.reset()
    frames = MC.clip_frames(model, 33, seed=n)
    tab, probes = set_clip(v, model, frames, K=K)
    info = mapi(v).info()
    assert info == dict(frames=33, duration=1.0, terms=0, probes=K)
    times = time_list(n, 1.0)
    state, points, phase = sample(v, times, K)
    check_sample(model, tab, probes, times, state, points, phase)
    # a time on a knot is that frame, up to the rounding of one product
    rows = tab["rows"]
    for e in np.flatnonzero(times * 32 == np.round(times * 32))[:4]:
        if 0 <= times[e] <= 1.0:
            assert np.abs(state[e].cpu().numpy() - rows[int(round(times[e] * 32))]).max() <= 2.0 ** -22
    # what was sampled is a state: set_state takes it, get_state returns it bit for bit
    v.set_state(state)
    assert same_bits(v.get_state(), state)
    # the env's own clock (zero after set_motion): the clip's first frame
    own, _, ph = sample(v, None, K)
    assert same_bits(own, sample(v, np.zeros(n, np.float32), K)[0]) and float(ph.abs().max()) == 0.0
    report()


def test_sample_looping_clip_over_many_cycles(model):
    n, F = 65, 17
    v = make_vec(n)
    v.reset()
    frames = MC.clip_frames(model, F, seed=3, cyclic=True)
    tab, _ = set_clip(v, model, frames, loop=True)
    T = tab["duration"]
    assert T == 0.5
    rng = np.random.default_rng(1)
    first, second, late = rng.uniform(0, T, 22), T + rng.uniform(0, T, 22), 39 * T + rng.uniform(0, T, 19)
    times = np.concatenate([first, second, late, [T, 2 * T]]).astype(np.float32)
    state, _, phase = sample(v, times)
    check_sample(model, tab, None, times, state, None, phase, "sample loop")
    s = state.cpu().numpy()
    disp = tab["disp"]
    assert disp[0] > 0.3
    assert (s[44:63, 0] > 39 * disp[0] - 1e-3).all() and (s[:22, 0] < disp[0] + 1e-3).all()      # x advances cycle by cycle
    assert np.abs(s[:, 2] - 3.0).max() < 0.06                                                   # z does not accumulate
    assert abs(s[63, 0] - disp[0]) < 1e-5 and abs(s[64, 0] - 2 * disp[0]) < 1e-5                # t = T is frame 0 of cycle 2
    report()


@pytest.mark.parametrize("angle", [179.0, 0.01])
def test_sample_two_frames_slerp_and_nlerp(angle, model):
    n = 9
    v = make_vec(n)
    v.reset()
    frames = MC.two_frame_clip(model, angle)
    tab, _ = set_clip(v, model, frames)
    times = (np.array([0.0, 0.125, 0.25, 0.5, 0.75, 0.9375, 1.0, 1.5, 0.3333]) * MC.DT).astype(np.float32)
    state, _, phase = sample(v, times)
    check_sample(model, tab, None, times, state, None, phase, "sample %g deg" % angle)
    q = state.cpu().numpy()[:, 3:7].astype(np.float64)
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 4e-7
    # equal steps in u are equal steps in angle along the arc
    ang = np.array([MR.quat_angle(tab["rows"][0, 3:7], x) for x in q])
    want = np.radians(angle) * np.minimum(times / np.float32(MC.DT), 1.0)
    assert np.abs(ang - want).max() < 2e-6
    report()


# 2 ------------------------------------------------------------------------------------------------------------------------
def offset_clip(model, s0, F=9):
    """a clip that starts AT the state s0 and leaves it by known amounts per frame: 0.02 rad on every joint (inside the limits),
    1 cm along x and y, 0.05 rad of yaw"""
    oo = model["obs_order"]
    lo, hi = model["q_lower"][oo], model["q_upper"][oo]
    frames = np.zeros((F, 7 + J))
    sign = np.where(s0[13:13 + J] < 0.5 * (lo + hi), 1.0, -1.0)
    for k in range(F):
        frames[k, :3] = s0[:3] + [0.01 * k, 0.01 * k, 0.0]
        frames[k, 3:7] = MC.quat_mul(MC.yaw_quat(0.05 * k), s0[3:7] / np.linalg.norm(s0[3:7]))
        frames[k, 7:] = np.clip(s0[13:13 + J] + 0.02 * k * sign, lo, hi)
    return frames


def spec_of(T, K):
    """T terms: every kind the clip allows first, then masks of one joint, the highest joint, a few"""
    last = 1 << (J - 1)
    spec = [(MR.POSE, 0, 0.65, 2.0, 0.0), (MR.VELOCITY, 0, 0.1, 0.1, 0.0),
            (MR.END_EFFECTOR, 0, 0.15, 40.0, 0.0) if K else (MR.POSE, 0x155, -0.5, 1.0, 0.0),
            (MR.ROOT_POSE, 0, 0.1, 10.0, 0.5), (MR.ROOT_VELOCITY, 0, -0.25, 0.05, 2.0), (MR.POSE, 1, 1.0, 5.0, 0.0),
            (MR.VELOCITY, last, 2.0, 0.01, 0.0), (MR.POSE, last, 0.3, 1.0, 0.0)]
    return spec[:T] if T > 1 else [spec[2 if K else 3]]


def compose(v, rows, T, pad=3, with_terms=True):
    """compose_motion_reward on a copy of `rows` in a guarded block with a padded stride -> (rows after, terms, guards intact?)"""
    n, Wr = rows.shape
    whole_r, r = guarded((n, Wr + pad), fill=float("nan"))
    whole_t, t = guarded((n, T))
    r[:, :Wr] = rows
    mapi(v).compose_reward(r, t if with_terms else None)
    torch.cuda.synchronize()
    ok = guards_intact(whole_r, (n, Wr + pad), fill=float("nan")) and guards_intact(whole_t, (n, T)) and bool(torch.isnan(r[:, Wr:]).all())
    return r[:, :Wr].clone(), t.clone(), ok and (with_terms or bool((t == 7.0).all()))


def check_compose(model, tab, probes, spec, step_weight, before, after, terms, state, clocks, helds, Ts, prev_terms=None, J=J):
    """every env and term against the reference (advancing clocks and held values); the column against the breakdown, bitwise"""
    before, after, terms = before.cpu().numpy(), after.cpu().numpy(), terms.cpu().numpy()
    n, T = terms.shape
    other = [c for c in range(before.shape[1]) if c != 3 * J]
    assert after[:, other].tobytes() == before[:, other].tobytes()                        # nothing but the reward column
    first = (np.float32(step_weight) * before[:, 3 * J]).astype(np.float32)
    assert after[:, 3 * J].tobytes() == MR.ordered_sum(first, terms).tobytes()            # the ordered f32 sum, bitwise
    assert np.isfinite(terms).all()
    for e in range(n):
        val, cases = MR.evaluate(model, tab, spec, state[e], before[e], clocks[e], helds[e], Ts, probes)
        for t, (s, case) in enumerate(zip(spec, cases)):
            kind, w = s[0], float(np.float32(s[2]))
            if case["held"]:
                want = np.float32(0.0) * np.float32(w) if prev_terms is None else prev_terms[e, t]
                assert np.float32(terms[e, t]).tobytes() == np.float32(want).tobytes(), (e, t, kind)
                continue
            want = w * val[t]
            b = abs(w) * MR.bound(kind, case)
            dev = abs(float(terms[e, t]) - want)
            worst(KIND_NAMES[kind], dev / b)
            assert dev <= b + 2 * U * abs(want), (e, t, KIND_NAMES[kind], dev, b, float(terms[e, t]), want)
    return terms


def stepped_cases(oracle64, model, n, **kw):
    """n envs holding case_states, stepped once: the row, and the state behind it, of one instant"""
    v = loaded_vec(case_states(oracle64, model, n), **kw)
    gen = torch.Generator(device=DEV).manual_seed(n)
    v.step_tensor(random_actions(model, n, gen))
    torch.cuda.synchronize()
    return v


def step_seconds(v):
    return MR.step_seconds(v.model.get_param("dt"), v.model.get_param("substeps"))


@pytest.mark.parametrize("n,K,T,step_weight", [(1, 0, 1, 1.0), (63, 1, 8, 0.0), (64, 8, 8, 1.0), (65, 8, 1, 0.0), (257, 0, 8, 1.0)])
def test_compose_against_reference(n, K, T, step_weight, oracle64, model):
    v = stepped_cases(oracle64, model, n)
    state = v.get_state().cpu().numpy().astype(np.float64)
    tab, probes = set_clip(v, model, offset_clip(model, state[0]), K=K)
    spec = spec_of(T, K)
    assert mapi(v).set_reward(spec, step_weight) == len(spec) and mapi(v).info()["terms"] == len(spec)
    clocks, helds = [MR.new_clock() for _ in range(n)], [np.zeros(len(spec)) for _ in range(n)]
    Ts = step_seconds(v)
    rows = v.rows.clone()
    assert not bool((rows[:, 3 * J + 1] != 0).any())
    prev = None
    for step in range(2):                                        # the clock moves on: the same state against a later reference
        after, terms, ok = compose(v, rows, len(spec), pad=3 * step)
        assert ok
        prev = check_compose(model, tab, probes, spec, step_weight, rows, after, terms, state, clocks, helds, Ts, prev)
    assert same_bits(v.get_state(), torch.as_tensor(state, dtype=torch.float32)) and all(c["k"] == 2 for c in clocks)
    if T == 8:
        t0 = prev[0] / np.array([s[2] for s in spec], np.float32)
        assert t0[0] > 0.9 and t0[5] > 0.9                       # env 0 stands two steps behind its own clip: close to 1
    report()


def test_zero_weights_leave_the_column_and_null_terms_change_nothing(oracle64, model):
    n = 17
    v = stepped_cases(oracle64, model, n)
    state = v.get_state().cpu().numpy().astype(np.float64)
    set_clip(v, model, offset_clip(model, state[3]), K=1)
    spec = spec_of(8, 1)
    rows = v.rows.clone()
    mapi(v).set_reward([(k, m, 0.0, s, a) for k, m, w, s, a in spec], 1.0)
    after, terms, ok = compose(v, rows, 8)
    assert ok and same_bits(after, rows) and float(terms.abs().max()) == 0.0          # 1 * x + 0 + ... + 0 is x
    mapi(v).set_reward(spec, 0.5)                                                   # (held values and the clock's count start anew)
    mapi(v).reset(None, torch.zeros(n, device=DEV))
    v.set_state(torch.as_tensor(state, dtype=torch.float32))
    a1, t1, ok1 = compose(v, rows, 8)
    mapi(v).reset(None, torch.zeros(n, device=DEV))
    v.set_state(torch.as_tensor(state, dtype=torch.float32))
    a2, _, ok2 = compose(v, rows, 8, with_terms=False)
    assert ok1 and ok2 and same_bits(a1, a2) and not same_bits(a1, rows)


def test_done_rows_hold_and_restart_the_clock(oracle64, model):
    n, T = 9, 8
    v = stepped_cases(oracle64, model, n)
    state = v.get_state().cpu().numpy().astype(np.float64)
    tab, probes = set_clip(v, model, offset_clip(model, state[1]), K=8)
    spec = spec_of(T, 8)
    mapi(v).set_reward(spec, 1.0)
    clocks, helds = [MR.new_clock() for _ in range(n)], [np.zeros(T) for _ in range(n)]
    Ts = step_seconds(v)
    rows = v.rows.clone()
    done_at = {0: [4], 1: [2, 5], 2: [], 3: [5, 7]}              # env 4: done with no step before; 5: twice in a row
    prev = None
    for step in range(4):
        r = rows.clone()
        r[done_at[step], 3 * J + 1] = 1.0
        after, terms, ok = compose(v, r, T)
        assert ok
        if step == 0:
            assert float(terms[4].abs().max()) == 0.0             # zeros if there was no step before
        prev = check_compose(model, tab, probes, spec, 1.0, r, after, terms, state, clocks, helds, Ts, prev)
    assert [c["k"] for c in clocks] == [4, 4, 2, 4, 3, 0, 4, 0, 4]
    # the device's clocks are the reference's: the sampled state at each env's own clock
    own, _, _ = sample(v, None, 8)
    times = np.array([MR.clock_time(c, Ts) for c in clocks], np.float32)
    assert same_bits(own, sample(v, times, 8)[0])
    report()


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [None, 0.85])
@pytest.mark.parametrize("pattern", ["none", "all", "alternate"])
def test_reset_writes_masked_envs_and_nothing_else(pattern, warm, oracle64, model):
    n, T, K = 65, 2, 1
    params = None if warm is None else {"warmstart": warm}
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    if pattern == "all":
        mask[:] = True
    elif pattern == "alternate":
        mask[::2] = True
    m = mask.cpu().numpy()
    frames = MC.clip_frames(model, 33, seed=5)
    times = torch.as_tensor(time_list(n, 1.0), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(9)
    act = random_actions(model, n, gen)
    a, b, c = [stepped_cases(oracle64, model, n, params=params) for _ in range(3)]       # a: RSI; b: set_state; c: nothing
    for v in (a, b, c):
        set_clip(v, model, frames, K=K)
        mapi(v).set_reward(spec_of(T, K), 1.0)
        v.batch.set_motors_enabled(False)
        mapi(v).compose_reward(v.rows.clone(), None)                                     # every env holds values, k = 1
    before_state, before_own = a.get_state(), sample(a, None)[0]
    whole, rows = guarded((n, 3 * J + 2 + 3), fill=float("nan"))
    rows[:, :3 * J + 2] = a.rows
    before_rows = rows.clone()
    _, held_terms, _ = compose(c, c.rows.clone().index_fill_(1, torch.tensor([3 * J + 1], device=DEV), 1.0), T)   # what every env holds
    mapi(a).reset(mask if pattern != "all" else None, times, rows)
    torch.cuda.synchronize()
    want = sample(a, times.cpu().numpy())[0]
    state = a.get_state()
    assert guards_intact(whole, (n, 3 * J + 5), fill=float("nan")) and bool(torch.isnan(rows[:, 3 * J + 2:]).all())
    assert same_bits(state[mask], want[mask]) and same_bits(state[~mask], before_state[~mask])
    assert same_bits(rows[~mask], before_rows[~mask])
    assert same_bits(rows[mask][:, :J], state[mask][:, 13:13 + J]) and same_bits(rows[mask][:, J:2 * J], state[mask][:, 13 + J:])
    assert float(rows[mask][:, 2 * J:3 * J].abs().sum()) == 0.0 if m.any() else True
    assert same_bits(rows[:, 3 * J:3 * J + 2], before_rows[:, 3 * J:3 * J + 2])          # reward and done as found
    own = sample(a, None)[0]                                                             # the clocks: t0 = time, k = 0 | untouched
    assert same_bits(own[mask], want[mask]) and same_bits(own[~mask], before_own[~mask])
    done_rows = a.rows.clone()
    done_rows[:, 3 * J + 1] = 1.0
    _, terms, _ = compose(a, done_rows, T)                                               # the held values: zero | untouched
    assert float(terms[mask].abs().sum()) == 0.0 if m.any() else True
    assert same_bits(terms[~mask], held_terms[~mask])
    # motors on, warm-start records empty - for the masked envs alone: the next step is bitwise that of a batch that was given the
    # same states by set_state (motors on, every record emptied), and for the others that of a batch nothing happened to
    mapi(a).reset(mask if pattern != "all" else None, times)                             # (the compose above reset every clock)
    b.set_state(want)
    for v in (a, b, c):
        v.step_tensor(act)
    torch.cuda.synchronize()
    assert same_bits(a.rows[mask], b.rows[mask]) and same_bits(a.rows[~mask], c.rows[~mask])
    assert same_bits(a.get_state()[mask], b.get_state()[mask]) and same_bits(a.get_state()[~mask], c.get_state()[~mask])
    if pattern == "alternate":
        assert not same_bits(a.rows[mask], c.rows[mask])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle64, model):
    n = 9
    v = stepped_cases(oracle64, model, n)
    api = mapi(v)
    frames = MC.clip_frames(model, 9, seed=1)
    out = guarded((n, W))
    refused(INVALID, api.sample, None, out[1])                                   # no clip yet
    refused(INVALID, api.set_reward, [(MR.POSE, 0, 1.0, 1.0, 0.0)])
    refused(INVALID, api.reset)
    refused(INVALID, api.compose_reward, v.rows)
    v.batch.set_link_probes(6, list(range(1, 10)))
    refused(INVALID, api.set_motion, frames, MC.DT, False, None, 6)                # 9 probes
    refused(INVALID, api.set_motion, frames, MC.DT, False, None, 5)                # an empty set
    refused(INVALID, api.set_motion, frames, MC.DT, False, None, 8)                # no such set
    refused(INVALID, api.set_motion, frames, MC.DT, False, None, -2)
    tab, probes = set_clip(v, model, frames, K=1)
    api.set_reward(spec_of(8, 1), 1.0)
    good = sample(v, np.full(n, 0.11, np.float32), 1)
    bad = frames.copy()
    bad[4, 5] = np.nan
    far = frames.copy()
    far[2, 7 + 3] = model["q_upper"][model["obs_order"]][3] + 1e-3
    zero = frames.copy()
    zero[0, 3:7] = 0.0
    for args in ((frames[:1], MC.DT), (np.zeros((4097, 7 + J)), MC.DT), (bad, MC.DT), (far, MC.DT), (zero, MC.DT), (frames, 0.0),
                 (frames, -1.0), (frames, MC.DT, False, np.full((9, 6 + J), np.inf))):
        refused(INVALID, api.set_motion, *args)
    assert api.info() == dict(frames=9, duration=0.25, terms=8, probes=1)          # the previous set is in force ...
    again = sample(v, np.full(n, 0.11, np.float32), 1)
    assert all(same_bits(x, y) for x, y in zip(good, again))                       # ... and intact
    for spec in ([(MR.POSE, 0, 1.0, 0.0, 0.0)], [(MR.POSE, 0, 1.0, -1.0, 0.0)], [(MR.ROOT_POSE, 0, 1.0, 1.0, -0.1)], [(5, 0, 1.0, 1.0, 0.0)],
                 [(MR.POSE, 0, np.nan, 1.0, 0.0)], [(MR.VELOCITY, 1 << J, 1.0, 1.0, 0.0)], [(MR.POSE, 0, 1.0, 1.0, 0.0)] * 9):
        refused(INVALID, api.set_reward, spec)
    refused(INVALID, api.set_reward, [(MR.POSE, 0, 1.0, 1.0, 0.0)], float("inf"))
    assert api.info()["terms"] == 8
    # launches: nothing is written, no clock moves
    whole, rows = guarded((n, 3 * J + 2))
    rows[:] = v.rows
    keep = rows.clone()
    own = sample(v, None, 1)[0]
    refused(INVALID, api.compose_reward, torch.zeros(n, 3 * J + 1, device=DEV))      # a stride below 3J + 2
    refused(INVALID, api.compose_reward, rows, torch.zeros(n, 7, device=DEV))        # a short breakdown
    refused(INVALID, api.compose_reward, rows.cpu())                                 # host memory
    refused(INVALID, api.reset, None, None, torch.zeros(n, 3 * J + 1, device=DEV))
    refused(INVALID, api.reset, torch.ones(n - 1, dtype=torch.uint8, device=DEV))
    refused(INVALID, api.sample, None, None, None, None)                             # nothing asked for
    refused(INVALID, api.sample, torch.zeros(n - 1, device=DEV), out[1])
    v.batch.set_link_probes(7, [1, 2])                                               # the end effectors' set changes its size
    refused(INVALID, api.compose_reward, rows)
    refused(INVALID, api.sample, None, out[1])
    refused(INVALID, api.reset)
    torch.cuda.synchronize()
    assert same_bits(rows, keep) and guards_intact(whole, (n, 3 * J + 2)) and guards_intact(out[0], (n, W))
    v.batch.set_link_probes(7, probes[0], probes[1])
    assert same_bits(sample(v, None, 1)[0], own)
    # a clip without end effectors refuses the term and the points
    api.set_motion(frames, MC.DT)
    assert api.info()["terms"] == 0                                                  # a new clip clears the terms
    refused(INVALID, api.set_reward, [(MR.END_EFFECTOR, 0, 1.0, 1.0, 0.0)])
    refused(INVALID, api.sample, None, None, torch.zeros(n, 1, 3, device=DEV))
    api.set_motion(None)                                                             # cleared: everything is refused again
    assert api.info() == dict(frames=0, duration=0.0, terms=0, probes=0)
    refused(INVALID, api.sample, None, out[1])


def test_stream_capture(oracle64, model):
    """reset, compose and sample replay inside one single-stream graph, from the second call, bitwise the eager calls"""
    n, T, K = 65, 8, 8
    v = stepped_cases(oracle64, model, n)
    state = v.get_state().cpu().numpy().astype(np.float64)
    set_clip(v, model, offset_clip(model, state[0], F=33), K=K)
    mapi(v).set_reward(spec_of(T, K), 1.0)
    src = v.rows.clone()
    times = torch.as_tensor(time_list(n, 1.0), device=DEV)
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)      # (every env: a clock that is not reset counts the calls)
    keep = v.get_state()

    def call(outs):
        rows, terms, st, pts, ph = outs
        rows.copy_(src)
        v.batch.set_state(keep)
        mapi(v).reset(mask, times, rows)
        mapi(v).compose_reward(rows, terms)
        mapi(v).sample(None, st, pts, ph)

    def change():
        times.mul_(0.5).add_(0.01)
        src[:, :2 * J].mul_(0.9)
        src[:, 3 * J].add_(1.0)

    outs = [torch.zeros(n, 3 * J + 2, device=DEV), torch.zeros(n, T, device=DEV), torch.zeros(n, W, device=DEV),
            torch.zeros(n, K, 3, device=DEV), torch.zeros(n, device=DEV)]
    replay_equals_eager(call, outs, change, replays=2)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(model):
    """an env that never had a clip, and one whose clip was attached and cleared: the same rows, bit for bit, over 20 steps"""
    from trex_gym import motion as M
    n = 17
    plain, cleared = make_vec(n, max_episode_steps=7), make_vec(n, max_episode_steps=7)
    M.attach(cleared, M.Clip(MC.clip_frames(model, 9), MC.DT), terms=M.pose(1.0), rsi=True)
    M.attach(cleared, None)
    assert cleared.motion is None and cleared.motion_api is None and cleared.motion_terms is None and cleared.motion_names == []
    gen = torch.Generator(device=DEV).manual_seed(2)
    for v in (plain, cleared):
        v.reset_tensor()
    for _ in range(20):
        act = random_actions(model, n, gen)
        for v in (plain, cleared):
            v.step_tensor(act)
        assert same_bits(plain.rows, cleared.rows)
    assert same_bits(plain.get_state(), cleared.get_state())
    with pytest.raises(ValueError):
        M.attach(plain, M.Clip(MC.clip_frames(model, 9)[:, :20], MC.DT))       # a clip of another joint count


def test_env_with_rsi_end_to_end(model):
    """64 envs, episodes of 5 steps, 12 steps: after every done the env stands where the clip is at the instant it drew, its clock
    runs from there, and motion_terms follows the reference step by step"""
    from trex_gym import motion as M
    n = 64
    frames = MC.clip_frames(model, 33, seed=8)
    ee = MC.end_effector_links(model, 2)
    v = make_vec(n, max_episode_steps=5)
    clip = M.Clip(frames, MC.DT)
    M.attach(v, clip, end_effectors=ee, rsi=True, seed=3)
    assert v.motion is clip and v.motion_names == ["motion/pose", "motion/velocity", "motion/end_effector", "motion/root_pose"]
    with pytest.raises(ValueError):
        v.step_many_tensor(torch.zeros(2, n, J, device=DEV))
    spec = [(k, 0, w, s, a) for k, w, s, a in ((0, 0.65, 2.0, 0.0), (1, 0.1, 0.1, 0.0), (2, 0.15, 40.0, 0.0), (3, 0.1, 10.0, 1.0))]
    tab = MR.device_table(MR.build_table(model, frames, None, MC.DT, False))
    probes = ([int(v._links.index(l)) for l, _ in ee], np.array([p for _, p in ee]))
    v.set_episode_steps(torch.arange(n, dtype=torch.int32, device=DEV) % 5)          # staggered: some env ends at every step
    v.reset_tensor()
    drawn = v._rsi_time.cpu().numpy().copy()
    assert same_bits(v.get_state(), sample(v, drawn, 2)[0]) and (drawn >= 0).all() and (drawn < 1.0).all() and len(set(drawn)) > 32
    v.set_episode_steps(torch.arange(n, dtype=torch.int32, device=DEV) % 5)
    clocks, helds = [dict(t0=float(t), k=0) for t in drawn], [np.zeros(4) for _ in range(n)]
    Ts = step_seconds(v)
    gen = torch.Generator(device=DEV).manual_seed(4)
    prev, ends = None, 0
    for step in range(12):
        v.step_tensor(random_actions(model, n, gen))
        done = v.done.cpu().numpy()
        ends += int(done.sum())
        rows, terms = v.rows.cpu().numpy(), v.motion_terms.cpu().numpy()
        state = v.get_state().cpu().numpy().astype(np.float64)          # (a done env's: the RSI state - its terms are held ones)
        assert (rows[:, 3 * J + 1] != 0).tolist() == done.tolist()
        for e in range(n):
            val, cases = MR.evaluate(model, tab, spec, state[e], rows[e], clocks[e], helds[e], Ts, probes)
            for t, case in enumerate(cases):
                w = float(np.float32(spec[t][2]))
                if case["held"]:
                    want = np.float32(0.0) if prev is None else prev[e, t]
                    assert np.float32(terms[e, t]).tobytes() == np.float32(want).tobytes(), (step, e, t)
                else:
                    b = abs(w) * MR.bound(spec[t][0], case)
                    worst("env " + KIND_NAMES[spec[t][0]], abs(float(terms[e, t]) - w * val[t]) / b)
                    assert abs(float(terms[e, t]) - w * val[t]) <= b + 2 * U * abs(w * val[t]), (step, e, t)
        prev = terms.copy()
        drawn = v._rsi_time.cpu().numpy()
        if done.any():
            want = sample(v, drawn, 2)[0]
            d = torch.as_tensor(done, device=DEV)
            assert same_bits(v.get_state()[d], want[d])
            assert same_bits(v.obs[d][:, :2 * J], torch.cat([want[d][:, 13:13 + J], want[d][:, 13 + J:]], 1))
            assert float(v.obs[d][:, 2 * J:].abs().sum()) == 0.0
        for e in np.flatnonzero(done):
            clocks[e].update(t0=float(drawn[e]), k=0)
    assert ends >= 2 * n
    report()


def test_channels_see_the_rsi_state(model):
    """with observation channels the composed row of an env RSI reset shows the clip's state and its phase"""
    from trex_gym import motion as M, observations as O
    n = 9
    frames = MC.clip_frames(model, 33, seed=8)
    v = make_vec(n, max_episode_steps=3, observations=O.external(2), external=M.phase_columns)
    M.attach(v, M.Clip(frames, MC.DT), rsi=True, seed=1, end_effectors=())
    assert v.motion_names == ["motion/pose", "motion/velocity", "motion/root_pose"]
    v.reset_tensor()
    gen = torch.Generator(device=DEV).manual_seed(4)
    for step in range(3):
        v.step_tensor(random_actions(model, n, gen))
    assert bool(v.done.all())
    want, _, phase = sample(v, v._rsi_time.cpu().numpy())
    assert same_bits(v.obs[:, :J], want[:, 13:13 + J]) and same_bits(v.obs[:, J:2 * J], want[:, 13 + J:])
    ang = 2 * np.pi * phase.cpu().numpy().astype(np.float64)
    assert np.abs(v.obs[:, 3 * J:].cpu().numpy() - np.stack([np.sin(ang), np.cos(ang)], 1)).max() < 1e-6
    assert v.obs.shape == (n, 3 * J + 2)


def test_recorded_rollout_becomes_a_clip(model):
    """Clip.from_states of a recorded rollout, played back: the env that repeats the rollout tracks its own clip - every term 1 at
    every step, up to the rounding the bound allows"""
    from trex_gym import motion as M
    n, steps = 1, 6
    gen = torch.Generator(device=DEV).manual_seed(6)
    acts = [random_actions(model, n, gen) for _ in range(steps)]
    v = make_vec(n)
    v.reset_tensor()
    states = [v.get_state()[0].cpu().numpy()]
    for a in acts:
        v.step_tensor(a)
        states.append(v.get_state()[0].cpu().numpy())
    Ts = step_seconds(v)
    oo = model["obs_order"]
    clip = M.Clip.from_states(np.array(states), Ts, limits=(model["q_lower"][oo], model["q_upper"][oo]))
    w = make_vec(n)
    M.attach(w, clip, terms=M.pose(1.0) + M.velocity(1.0) + M.root_pose(1.0) + M.root_velocity(1.0))
    w.reset_tensor()
    for a in acts:
        w.step_tensor(a)
        assert float((w.motion_terms - 1.0).abs().max()) < 1e-4, w.motion_terms
    assert same_bits(w.get_state(), v.get_state())


def test_trainer(tmp_path, model):
    """two updates at 64 envs with --motion and --rsi; save, load: the clip and the terms come back"""
    from trex_gym import motion as M, trex_train
    frames = MC.clip_frames(model, 33, seed=8)
    clip_path = str(tmp_path / "walk.npz")
    M.Clip(frames, MC.DT, loop=False).save(clip_path)
    args = trex_train.parse_args(["--motion", clip_path, "--rsi", "--motion_weight", "0.5"])
    env = trex_train.build_environment(64, device=DEV, max_episode_steps=20,
                                       motion=dict(clip=args.motion, rsi=args.rsi, weight=args.motion_weight))
    assert env._rsi and len(env.motion_names) == 4 and env.motion_api.info()["probes"] >= 1
    lines = []
    path = str(tmp_path / "agent.pt")
    agent, hist = trex_train.train(env, 2 * 64 * 32, 0, nsteps=32, noptepochs=1, save_path=path, log=lines.append)
    assert len(hist) == 2 and list(hist[0]["motion_terms"]) == env.motion_names
    assert all(0.0 <= x <= 0.5 * 0.65 + 1e-6 for x in [hist[1]["motion_terms"]["motion/pose"]])
    assert any("motion/pose" in l for l in lines)
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    assert again.env.motion_config == env.motion_config and again.env._rsi
    assert (again.env.motion.frames == frames).all() and again.env.motion_names == env.motion_names
    assert again.env.motion_config["terms"][0][2] == 0.5 * 0.65
    with pytest.raises(SystemExit):
        trex_train.parse_args(["--rsi"])
