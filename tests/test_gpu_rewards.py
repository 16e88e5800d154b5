"""Reward terms on the GPU (trex_batch_set_reward / trex_batch_compose_reward / trex_batch_reward_reset, include/trex_reward.h)
against the f64 restatement tests/reward_ref.py - itself pinned by tests/test_reward_ref.py: every kind alone and all together at
the 8-env workgroup's edges, the composed column as the ordered f32 sum of the breakdown, what is written and what is not, the
history rules through steps, episode ends, falls and resets, refusals, stream capture, the observation channels beside it, and
the trainer.

States: those of state_sets.case_states - landing, standing and airborne, every env with a state of its own - stepped once on the
device, so that the row, the state behind it and the contact sensor belong to one instant; the reference is fed with the GPU's own
row, state and sensor values. Tolerances: reward_ref.bound(kind, case) for the value v, times |weight|, plus one rounding of the
product; held values (done rows) are compared bitwise with the step before. The largest deviation / bound per kind is printed
(-s) and recorded in profiles/r23_rewards.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import reward_ref as RR
from conftest import ASSET_URDF
from gpu_support import DEV, guarded, guards_intact, loaded_vec, make_vec, refused, replay_equals_eager, same_bits
from state_sets import case_states

pytestmark = pytest.mark.gpu
NB, J = 26, 25
Z = (0.0, 0.0, 0.0)
U = RR.U
KIND_NAMES = ["step", "alive", "track_lin_vel", "track_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "base_height", "point_height",
              "torque", "joint_vel", "joint_acc", "action_rate", "joint_limit", "power", "joint_pose", "contact_count", "foot_air_time",
              "foot_slip"]
WORST = {}                                  # kind -> largest deviation / bound seen in this process


def term(kind, weight=1.0, link=0, mask=0, xyz=Z, p0=0.0, p1=0.0):
    return (kind, link, mask, xyz, weight, p0, p1)


def api(v):
    """the reward calls of the env's batch (trex_gym.reward_capi.BatchRewards): the env's own, or one made for a plain env"""
    if v.reward_api is None:
        from trex_gym import reward_capi
        v.reward_api = reward_capi.BatchRewards(v.batch)
    return v.reward_api


def pick(model):
    """(a toe link of either leg, the head link, the toes' bodies)"""
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    toes = [l for l in range(len(names)) if "toe" in names[l]]
    left, right = toes[0], [l for l in toes if lb[l] != lb[toes[0]]][-1]
    head = [l for l in range(len(names)) if lb[l] == int(model["head_body"])][0]
    return left, right, head


def each_kind(model):
    """one term of every kind, in kind order; weights that are not 1"""
    left, right, head = pick(model)
    lb = np.asarray(model["link_body"], int)
    return [term(RR.STEP, 0.75), term(RR.ALIVE, 2.0), term(RR.TRACK_LIN, 1.5, p0=0.25), term(RR.TRACK_ANG, 0.5, p0=0.5),
            term(RR.LIN_VEL_Z, -2.0), term(RR.ANG_VEL_XY, -0.05), term(RR.ORIENTATION, -1.0), term(RR.BASE_HEIGHT, -1.0, p0=0.6),
            term(RR.POINT_HEIGHT, 1.0, link=left, xyz=(0.1, -0.2, 0.3), p0=0.1), term(RR.TORQUE, -1e-4), term(RR.JOINT_VEL, -1e-3),
            term(RR.JOINT_ACC, -2.5e-7), term(RR.ACTION_RATE, -0.01), term(RR.JOINT_LIMIT, -1.0, p0=0.9), term(RR.POWER, -1e-3),
            term(RR.JOINT_POSE, -0.1), term(RR.CONTACT_COUNT, -1.0, mask=(1 << NB) - 2, p0=1.0),
            term(RR.FOOT_AIR_TIME, 1.0, link=left, p0=1.0, p1=0.05), term(RR.FOOT_SLIP, -0.1, link=left, xyz=(0.05, 0.0, -0.02), p0=1.0)]


def full_spec(model):
    """T = 32: the 19 kinds, then kinds again with the masks of joint 0 alone, of joint J - 1 alone, of one body, and the other foot"""
    left, right, head = pick(model)
    lb = np.asarray(model["link_body"], int)
    last = 1 << (J - 1)
    more = [term(RR.TORQUE, -1e-4, mask=1), term(RR.TORQUE, -1e-4, mask=last), term(RR.JOINT_VEL, -1e-3, mask=1),
            term(RR.JOINT_ACC, -2.5e-7, mask=last), term(RR.POWER, -1e-3, mask=1), term(RR.JOINT_POSE, -0.1, mask=last),
            term(RR.JOINT_LIMIT, -1.0, mask=1, p0=0.5), term(RR.JOINT_LIMIT, -1.0, p0=0.3), term(RR.JOINT_ACC, -2.5e-7, mask=1),
            term(RR.CONTACT_COUNT, -1.0, mask=1 << int(lb[left]), p0=5.0), term(RR.POINT_HEIGHT, 1.0, link=head, xyz=(0.3, 0.0, 0.1), p0=1.0),
            term(RR.FOOT_AIR_TIME, 1.0, link=right, p0=1.0, p1=0.0), term(RR.FOOT_SLIP, -0.1, link=right, p0=1.0)]
    spec = each_kind(model) + more
    assert len(spec) == RR.MAX_TERMS
    return spec


def step_seconds(v):
    return RR.step_seconds(v.model.get_param("dt"), v.model.get_param("substeps"))


def sensed_cases(oracle64, model, n, **kw):
    """n envs holding case_states, the contact sensor on"""
    v = loaded_vec(case_states(oracle64, model, n), **kw)
    v.enable_contact_sensor(True)
    return v


def inputs(n, seed, J=J):
    """actions well outside the joint limits (ACTION_RATE takes them as passed) and commands"""
    gen = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(n, J, generator=gen)).to(DEV), torch.randn(n, 3, generator=gen).to(DEV)


def instant(v):
    """what the reference is fed with: the GPU's own state and sensor forces (numpy)"""
    return v.get_state().cpu().numpy().astype(np.float64), v.contact_wrench()[:, :, :3].cpu().numpy()


def compose(v, rows, act, cmd, T, pad=3):
    """compose_reward on a copy of `rows` in a guarded block with a padded stride -> (rows after, terms, guards intact?)"""
    n, W = rows.shape
    whole_r, r = guarded((n, W + pad), fill=float("nan"))
    whole_t, t = guarded((n, T))
    r[:, :W] = rows
    api(v).compose_reward(r, act, cmd, t)
    torch.cuda.synchronize()
    ok = guards_intact(whole_r, (n, W + pad), fill=float("nan")) and guards_intact(whole_t, (n, T)) and bool(torch.isnan(r[:, W:]).all())
    return r[:, :W].clone(), t.clone(), ok


def check(model, spec, before, after, terms, state, force, hists, Ts, act, cmd, prev_terms=None, J=J, floor_z=RR.FLOOR_Z):
    """every env and term against the reference (advancing `hists`); the column against the breakdown, bitwise"""
    before, after, terms = before.cpu().numpy(), after.cpu().numpy(), terms.cpu().numpy()
    act, cmd = act.cpu().numpy(), cmd.cpu().numpy()
    n, T = terms.shape
    other = [c for c in range(before.shape[1]) if c != 3 * J]
    assert after[:, other].tobytes() == before[:, other].tobytes()                        # nothing but the reward column
    assert after[:, 3 * J].tobytes() == RR.ordered_sum(terms).tobytes()                   # the ordered f32 sum, bitwise
    assert np.isfinite(terms).all()
    for e in range(n):
        v, cases = RR.evaluate(model, spec, state[e], before[e], hists[e], Ts, action=act[e], command=cmd[e], force=force[e], floor_z=floor_z)
        for t, (s, case) in enumerate(zip(spec, cases)):
            kind, w = s[0], float(np.float32(s[4]))
            if case["held"]:
                want = np.float32(0.0) * np.float32(w) if prev_terms is None else prev_terms[e, t]
                assert np.float32(terms[e, t]).tobytes() == np.float32(want).tobytes(), (e, t, kind)
                continue
            want = w * v[t]
            b = abs(w) * RR.bound(kind, case)
            dev = abs(float(terms[e, t]) - want)
            if b > 0:
                WORST[kind] = max(WORST.get(kind, 0.0), dev / b)
            assert dev <= b + 2 * U * abs(want), (e, t, KIND_NAMES[kind], dev, b, float(terms[e, t]), want)
    return terms


def report():
    print("reward deviation / bound, largest per kind: " + "  ".join("%s %.3f" % (KIND_NAMES[k], WORST[k]) for k in sorted(WORST)))


def histories(n, T, J=J):
    return [RR.new_history(T, J, J) for _ in range(n)]


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 8, 9, 17])
def test_every_kind_against_reference(n, oracle64, model):
    """one slot, a full workgroup, a ragged second one, a ragged third: each kind alone on the first step's rows, then all 19
    together at T = 32 over two steps, so that the rate terms and the timers have a history. Largest deviation / bound measured
    on an MI355X over this module (profiles/r23_rewards.txt): 0.54 (JOINT_ACC), 0.30 (POINT_HEIGHT), below 0.27 for the others."""
    v = sensed_cases(oracle64, model, n)
    Ts = step_seconds(v)
    act, cmd = inputs(n, seed=n)
    v.step_tensor(act)
    rows1 = v.rows.clone()
    state1, force1 = instant(v)
    for s in each_kind(model):
        assert api(v).set_reward([s]) == 1 == api(v).reward_terms()
        after, terms, ok = compose(v, rows1, act, cmd, 1)
        assert ok
        check(model, [s], rows1, after, terms, state1, force1, histories(n, 1), Ts, act, cmd)
    spec = full_spec(model)
    assert api(v).set_reward(spec) == 32
    hists = histories(n, 32)
    after, terms, ok = compose(v, rows1, act, cmd, 32)
    assert ok
    check(model, spec, rows1, after, terms, state1, force1, hists, Ts, act, cmd)
    act2, cmd2 = inputs(n, seed=100 + n)
    v.step_tensor(act2)
    rows2 = v.rows.clone()
    state2, force2 = instant(v)
    after, terms2, ok = compose(v, rows2, act2, cmd2, 32)
    assert ok
    check(model, spec, rows2, after, terms2, state2, force2, hists, Ts, act2, cmd2)
    assert (terms2[:, 11] != 0).any() and (terms2[:, 12] != 0).all()                      # JOINT_ACC, ACTION_RATE: now with a history
    report()
    v.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_sum_breakdown_and_repeatability(oracle64, model):
    n = 9
    v = sensed_cases(oracle64, model, n)
    act, cmd = inputs(n, seed=2)
    v.step_tensor(act)
    rows = v.rows.clone()
    api(v).set_reward([term(RR.STEP, 1.0)])
    after, terms, ok = compose(v, rows, None, None, 1)
    assert ok and same_bits(after, rows) and same_bits(terms[:, 0], rows[:, 3 * J])          # a lone STEP of weight 1: the column as it was
    spec = full_spec(model)
    runs = []
    for _ in range(2):                                                                    # (set_reward starts the history afresh)
        api(v).set_reward(spec)
        runs.append(compose(v, rows, act, cmd, 32))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    assert runs[0][0][:, 3 * J].cpu().numpy().tobytes() == RR.ordered_sum(runs[0][1].cpu().numpy()).tobytes()
    # without a breakdown buffer the column is the same
    api(v).set_reward(spec)
    r = rows.clone()
    api(v).compose_reward(r, act, cmd, None)
    assert same_bits(r, runs[0][0])
    v.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_nothing_else_is_written(oracle64, model):
    """twin envs on the same actions through episode ends, one with rewards: state, every other row column, the contact wrench
    and the episode counts are bitwise the same"""
    from trex_gym import rewards as R
    n = 9
    left, right, head = pick(model)
    spec = R.step(0.5) + R.track_lin_vel() + R.orientation() + R.torque(-1e-4) + R.joint_acc(-1e-7) + R.action_rate(-0.01) + \
        R.foot_air_time(1.0, left) + R.foot_slip(-0.1, right) + R.contact_count(-1.0, [head, 0])
    cases = case_states(oracle64, model, n)
    kw = dict(max_episode_steps=5, params={"warmstart": 0.85})
    plain, rich = loaded_vec(cases, **kw), loaded_vec(cases, rewards=spec, **kw)
    plain.enable_contact_sensor(True)
    assert rich.reward_terms.shape == (n, 9) and rich.reward_names[0] == "step" and plain.reward_terms is None
    for e in (plain, rich):
        e.set_episode_steps(torch.arange(n) % 5)
    rich.commands[:] = torch.randn(n, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    gen = torch.Generator().manual_seed(4)
    ends = 0
    for t in range(8):
        a = (0.5 * torch.randn(n, J, generator=gen)).to(DEV)
        for e in (plain, rich):
            e.step_tensor(a)
        assert same_bits(plain.obs.contiguous(), rich.obs.contiguous()) and same_bits(plain.done_f, rich.done_f), t
        assert same_bits(plain.penalties.contiguous(), rich.penalties.contiguous()) and torch.equal(plain.done, rich.done), t
        assert same_bits(plain.contact_wrench(), rich.contact_wrench()), t
        assert same_bits(rich.rew, torch.tensor(RR.ordered_sum(rich.reward_terms.cpu().numpy())))
        assert same_bits(rich.reward_terms[:, 0], 0.5 * plain.rew)                         # STEP: the step's own reward
        ends += int(rich.done.sum())
    assert ends >= n
    assert same_bits(plain.get_state(), rich.get_state()) and torch.equal(plain.episode_steps, rich.episode_steps)
    with pytest.raises(ValueError, match="step_many_tensor"):
        rich.step_many_tensor(torch.zeros(2, n, J, device=DEV))
    for e in (plain, rich):
        e.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_history_rate_terms(oracle64, model):
    """three steps: ACTION_RATE and JOINT_ACC are 0 on the first, then follow the reference fed with the GPU's own rows"""
    n = 9
    spec = [term(RR.ACTION_RATE, -0.01), term(RR.JOINT_ACC, -2.5e-7), term(RR.JOINT_ACC, 1.0, mask=1 << (J - 1)), term(RR.JOINT_VEL, 1.0)]
    v = sensed_cases(oracle64, model, n)
    Ts = step_seconds(v)
    api(v).set_reward(spec)
    hists = histories(n, 4)
    for t in range(3):
        act, cmd = inputs(n, seed=40 + t)
        v.step_tensor(act)
        rows = v.rows.clone()
        state, force = instant(v)
        after, terms, ok = compose(v, rows, act, cmd, 4)
        assert ok
        check(model, spec, rows, after, terms, state, force, hists, Ts, act, cmd)
        assert bool((terms[:, :3] == 0).all()) == (t == 0) and (terms[:, 3] > 0).all()
    report()
    v.close()


def test_history_air_time_and_slip_through_a_drop(oracle64, model):
    """from the start pose the robot falls until a foot lands: the step count comes from the CPU oracle's contacts of that drop"""
    q0 = model["q_start"][model["obs_order"]]
    s = oracle64.new_state()
    oracle64.reset(s)
    first = None
    for t in range(40):
        oracle64.step(s, q0)
        if first is None and len(oracle64.contacts(s)[0]):
            first = t
        if first is not None and t >= first + 3:
            break
    assert first is not None and first >= 2, first
    steps = first + 4
    left, right, head = pick(model)
    lb = np.asarray(model["link_body"], int)
    toes = [l for l in range(len(lb)) if "toe" in model["link_names"][l]]
    feet = sorted(set(toes[:2] + toes[-2:]))                                              # toes of either leg
    spec = [s_ for l in feet for s_ in (term(RR.FOOT_AIR_TIME, 1.0, link=l, p0=1.0, p1=0.05), term(RR.FOOT_SLIP, 1.0, link=l, p0=1.0))]
    spec = spec + [term(RR.CONTACT_COUNT, 1.0, mask=(1 << NB) - 2, p0=1.0)]
    T = len(spec)
    n = 2
    v = make_vec(n)
    v.enable_contact_sensor(True)
    v.reset_tensor()
    Ts = step_seconds(v)
    api(v).set_reward(spec)
    hists = histories(n, T)
    act = torch.tensor(np.tile(q0, (n, 1)), dtype=torch.float32, device=DEV)
    cmd = torch.zeros(n, 3, device=DEV)
    landed = 0.0
    for t in range(steps):
        v.step_tensor(act)
        rows = v.rows.clone()
        state, force = instant(v)
        after, terms, ok = compose(v, rows, act, cmd, T)
        assert ok
        check(model, spec, rows, after, terms, state, force, hists, Ts, act, cmd)
        air = terms[:, 0:T - 1:2]
        if t < first - 1:
            assert (terms == 0).all(), t                                                  # in the air: no touchdown, no slip, no contact
        landed = max(landed, float(air.max()))
    assert landed > (first - 2) * Ts - 0.05                                               # a touchdown paid out the air time of the drop
    report()
    v.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_done_rows_episode_limit(oracle64, model):
    """episode limit 3 with staggered counts: in every launch some envs end and others go on. A done row repeats the step before
    (bitwise) but for STEP; the step after has no rate terms and a restarted timer - the reference's rules, checked by check()"""
    n = 9
    left, right, head = pick(model)
    spec = [term(RR.STEP, 0.5), term(RR.JOINT_VEL, -1e-3), term(RR.JOINT_ACC, -2.5e-7), term(RR.ACTION_RATE, -0.01),
            term(RR.FOOT_AIR_TIME, 1.0, link=left, p0=1e6, p1=0.0), term(RR.ORIENTATION, -1.0), term(RR.FOOT_AIR_TIME, 1.0, link=right, p0=-1e6)]
    v = sensed_cases(oracle64, model, n, max_episode_steps=3)
    v.set_episode_steps(torch.arange(n) % 3)
    Ts = step_seconds(v)
    api(v).set_reward(spec)
    hists = histories(n, len(spec))
    prev, ended, mixed = None, 0, 0
    for t in range(6):
        act, cmd = inputs(n, seed=50 + t)
        v.step_tensor(act)
        rows = v.rows.clone()
        done = (rows[:, 3 * J + 1] != 0).cpu().numpy()
        state, force = instant(v)
        after, terms, ok = compose(v, rows, act, cmd, len(spec))
        assert ok
        terms = check(model, spec, rows, after, terms, state, force, hists, Ts, act, cmd, prev_terms=prev)
        assert same_bits(torch.tensor(terms[:, 0]), 0.5 * rows[:, 3 * J].cpu())              # STEP comes from the row, done or not
        if prev is not None and done.any():
            assert terms[done, 1:].tobytes() == prev[done, 1:].tobytes()
        # (the timer of a foot that never "touches" - threshold 1e6 - restarts with every episode: the reference's timers)
        assert all(hists[e]["timer"][4] == 0.0 for e in range(n) if done[e]) and any(hists[e]["timer"][4] > Ts for e in range(n)) == (t >= 1)
        ended += int(done.sum())
        mixed += int(done.any() and not done.all())
        prev = terms
    assert ended >= 2 * n - 3 and mixed >= 4
    report()
    v.close()


def test_done_rows_fall_termination(oracle64, model):
    """fall termination with a penalty: the fallen envs' rows are done rows, and the penalty shows in STEP"""
    n = 9
    spec = [term(RR.STEP, 1.0), term(RR.JOINT_VEL, -1e-3), term(RR.ACTION_RATE, -0.01)]
    term_kw = dict(max_tilt=0.6)
    cases = [(s.copy(), ms) for s, ms in case_states(oracle64, model, n)]
    for e in (1, 4, 7):                                                                   # three envs lie on their side: they end at once
        cases[e][0][3:7] = np.float32([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)])
    a, b = (loaded_vec(cases, terminate=dict(penalty=p, **term_kw)) for p in (0.0, 2.5))
    b.enable_contact_sensor(True)
    Ts = step_seconds(b)
    api(b).set_reward(spec)
    hists = histories(n, 3)
    prev, fell = None, 0
    for t in range(3):
        act, cmd = inputs(n, seed=60 + t)
        act = 0.1 * act
        for e in (a, b):
            e.step_tensor(act)
        rows = b.rows.clone()
        done = rows[:, 3 * J + 1] != 0
        assert torch.equal(done, a.done)
        state, force = instant(b)
        after, terms, ok = compose(b, rows, act, cmd, 3)
        assert ok
        terms = check(model, spec, rows, after, terms, state, force, hists, Ts, act, cmd, prev_terms=prev)
        d = done.cpu().numpy()
        want = np.where(d, (a.rew.cpu().numpy() - np.float32(2.5)).astype(np.float32), a.rew.cpu().numpy())
        assert terms[:, 0].tobytes() == want.tobytes() == rows[:, 3 * J].cpu().numpy().tobytes()
        fell += int(d.sum())
        prev = terms
    assert 3 <= fell < 3 * n
    for e in (a, b):
        e.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_reset_tensor_mask(oracle64, model):
    """reset_tensor(mask): the masked envs lose their history - no rate terms on their next step, held values zero -, the others
    keep theirs"""
    from trex_gym import rewards as R
    n = 9
    spec = R.action_rate(1.0) + R.joint_acc(1e-6) + R.joint_vel(1.0)
    v = loaded_vec(case_states(oracle64, model, n), rewards=spec, max_episode_steps=100)
    gen = torch.Generator().manual_seed(7)
    for t in range(2):
        v.step_tensor((0.5 * torch.randn(n, J, generator=gen)).to(DEV))
    assert (v.reward_terms[:, :2] > 0).all()
    mask = (torch.arange(n) % 2 == 0).to(DEV)
    v.reset_tensor(mask)
    v.step_tensor((0.5 * torch.randn(n, J, generator=gen)).to(DEV))
    assert (v.reward_terms[mask][:, :2] == 0).all() and (v.reward_terms[~mask][:, :2] > 0).all() and (v.reward_terms[:, 2] > 0).all()
    # held values: end every episode at the next step; the masked envs of a second reset repeat zeros, the others their values
    before = v.reward_terms.clone()
    v.reward_api.reward_reset(mask)
    v.set_episode_steps(torch.full((n,), 99, dtype=torch.int32))
    v.step_tensor((0.5 * torch.randn(n, J, generator=gen)).to(DEV))
    assert v.done.all()
    assert (v.reward_terms[mask] == 0).all() and same_bits(v.reward_terms[~mask], before[~mask])
    v.reset_tensor()
    v.step_tensor((0.5 * torch.randn(n, J, generator=gen)).to(DEV))
    assert (v.reward_terms[:, :2] == 0).all()
    v.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(model):
    """every TREX_E_INVALID case of the header: nothing written, the previous specification still in force"""
    from trex_gym import _capi
    E = _capi.E_INVALID
    left, right, head = pick(model)
    n = 32768                               # (buffers of 32768 envs: larger than the allocation a small tensor lives in)
    v = make_vec(n)
    v.reset_tensor()
    b, rb = v.batch, api(v)
    raw = _capi.lib.trex_batch_compose_reward
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(rows, stride, act, cmd, terms):
        _capi.check(raw(b.h, p(rows) if hasattr(rows, "data_ptr") else rows, stride, p(act) if hasattr(act, "data_ptr") else act,
                        p(cmd) if hasattr(cmd, "data_ptr") else cmd, p(terms) if hasattr(terms, "data_ptr") else terms, None))

    W = 3 * J + 2
    rows = torch.full((n, W), 7.0, device=DEV)
    rows[:, 3 * J + 1] = 0.0
    keep = rows.clone()
    act, cmd = torch.zeros(n, J, device=DEV), torch.zeros(n, 3, device=DEV)
    terms = torch.full((n, 32), 7.0, device=DEV)
    short = torch.full((100,), 7.0, device=DEV)
    host = C.c_void_p(np.zeros(n * W, np.float32).ctypes.data)
    refused(E, call, rows, W, act, cmd, terms)                                             # no terms set
    refused(E, rb.reward_reset)
    assert rb.reward_terms() == 0
    good = [term(RR.ALIVE, 3.0), term(RR.TRACK_LIN, p0=0.25), term(RR.ACTION_RATE), term(RR.FOOT_SLIP, link=left, p0=1.0)] + \
        [term(RR.ALIVE)] * 28                                                             # (32 terms: a [n, T] block of 4 MB)
    assert rb.set_reward(good) == 32
    nl = len(model["link_names"])
    for bad in ([term(RR.KINDS)], [term(-1)], [term(RR.POINT_HEIGHT, link=nl)], [term(RR.FOOT_SLIP, link=-1)], [term(RR.ALIVE, float("nan"))],
                [term(RR.BASE_HEIGHT, p0=float("inf"))], [term(RR.FOOT_AIR_TIME, link=left, p1=float("nan"))],
                [term(RR.FOOT_SLIP, link=left, xyz=(0.0, float("nan"), 0.0))], [term(RR.TRACK_LIN, p0=0.0)], [term(RR.TRACK_ANG, p0=-1.0)],
                [term(RR.JOINT_LIMIT, p0=0.0)], [term(RR.JOINT_LIMIT, p0=1.5)], [term(RR.TORQUE, mask=1 << J)],
                [term(RR.CONTACT_COUNT, mask=1 << NB)], [term(RR.ALIVE)] * 33):
        refused(E, rb.set_reward, bad)
        assert rb.reward_terms() == 32                                                     # the previous set intact
    refused(E, call, rows, W, act, cmd, terms)                                             # a contact kind, the sensor off
    assert "sensor is off" in _capi.lib.trex_last_error().decode()
    v.enable_contact_sensor(True)
    refused(E, call, rows, W - 1, act, cmd, terms)                                         # a stride below 3J + tail
    refused(E, call, rows, W, act, None, terms)                                            # command missing
    refused(E, call, rows, W, None, cmd, terms)                                            # actions missing
    refused(E, call, None, W, act, cmd, terms)
    refused(E, call, host, W, act, cmd, terms)                                             # host memory
    refused(E, call, rows, W, host, cmd, terms)
    refused(E, call, rows, W, act, host, terms)
    refused(E, call, rows, W, act, cmd, host)
    refused(E, call, short, W, act, cmd, terms)                                            # short buffers
    refused(E, call, rows, W, short, cmd, terms)
    refused(E, call, rows, W, act, cmd, short)
    refused(E, rb.compose_reward, rows, act, cmd, terms[:, :3].contiguous())                # (the Python layer's own checks)
    refused(E, rb.compose_reward, rows.cpu(), act, cmd, terms)
    v.batch.set_penalties_in_rows(True)
    refused(E, call, rows, W, act, cmd, terms)                                             # 3J + 5 with penalties in rows
    v.batch.set_penalties_in_rows(False)
    b.set_stiffness_actions(True, 1.0)
    refused(E, call, rows, W, act, cmd, terms)                                             # the action width changed
    assert "wide" in _capi.lib.trex_last_error().decode()
    b.set_stiffness_actions(False, 1.0)
    torch.cuda.synchronize()
    assert same_bits(rows, keep) and (terms == 7.0).all() and (short == 7.0).all()
    # the batch keeps answering, with the specification that was in force
    call(rows, W, act, cmd, terms)
    torch.cuda.synchronize()
    assert (terms[:, 0] == 3.0).all() and (terms[:, 4:] == 1.0).all() and torch.isfinite(rows[:, 3 * J]).all()
    assert rb.set_reward([]) == 0 and rb.reward_terms() == 0
    v.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_stream_capture(oracle64, model):
    """set_state + reward_reset + two x (step + compose_reward) + compose_rows, captured on a side stream and replayed on another
    state, is bitwise the eager run"""
    from trex_gym import observations as O
    n = 9
    left, right, head = pick(model)
    cases = case_states(oracle64, model, 2 * n)
    states = torch.tensor(np.array([c[0] for c in cases], np.float32), device=DEV)
    v = make_vec(n)
    v.enable_contact_sensor(True)
    v.reset_tensor()
    spec = full_spec(model)
    api(v).set_reward(spec)
    E = v.batch.set_observation([(0, 0, Z, 1.0), (7, left, Z, 1.0), (8, 0, Z, 1.0)])
    state = states[:n].clone()
    act, cmd = inputs(n, seed=8)
    act2 = 0.5 * act
    rows = torch.zeros(n, 3 * J + 2, device=DEV)
    pen = torch.zeros(n, 3, device=DEV)

    def call(outs):
        wide, terms = outs
        v.batch.set_state(state)
        api(v).reward_reset(None)
        for a in (act, act2):
            v.batch.step_rows(a, rows, pen)
            api(v).compose_reward(rows, a, cmd, terms)
        v.batch.compose_rows(rows, wide, a)

    outs = [torch.zeros(n, 3 * J + E + 2, device=DEV), torch.zeros(n, 32, device=DEV)]
    replay_equals_eager(call, outs, lambda: state.copy_(states[n:]), replays=2)
    assert (outs[1][:, 12] != 0).all()                                                    # ACTION_RATE had its history inside the graph
    assert same_bits(outs[0][:, 3 * J + E], torch.tensor(RR.ordered_sum(outs[1].cpu().numpy())))
    v.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_with_observations(model):
    """the locomotion observation preset and the locomotion reward preset together: the extended row's reward column is the
    composed one, the observation columns are bitwise those of an env without rewards"""
    from trex_gym import _capi, observations as O, rewards as R
    from trex_gym.vec_env import TrexVecEnv
    n = 9
    m = _capi.Model(ASSET_URDF)
    obs, rew = O.locomotion(m, DEV), R.locomotion(m, DEV)
    kinds = [c.kind for c in rew]
    assert kinds[0] == "step" and rew[0].weight == 0.0 and kinds.count("foot_air_time") == 2 and kinds.count("foot_slip") == 2
    assert {"track_lin_vel", "track_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "torque", "joint_acc", "action_rate",
            "contact_count"} <= set(kinds) and len(rew) <= R.MAX_TERMS
    kw = dict(urdf_path=ASSET_URDF, device=DEV, max_episode_steps=6)
    plain = TrexVecEnv(n, observations=obs, **kw)
    both = TrexVecEnv(n, observations=obs + O.external(3), external=lambda env: env.commands, rewards=rew, **kw)
    assert both.obs_dim == plain.obs_dim + 3 == 96 and both.reward_names == R.names(rew) and both.reward_terms.shape == (n, len(rew))
    both.commands[:] = torch.tensor([0.5, 0.0, 0.25], device=DEV)
    for e in (plain, both):
        e.reset_tensor()
        e.set_episode_steps(torch.arange(n) % 6)
    gen = torch.Generator().manual_seed(9)
    D = plain.obs_dim
    for t in range(8):
        a = (0.3 * torch.randn(n, J, generator=gen)).to(DEV)
        for e in (plain, both):
            e.step_tensor(a)
        assert same_bits(plain.obs.contiguous(), both.obs[:, :D].contiguous()) and same_bits(plain.done_f, both.done_f), t
        assert torch.equal(both.obs[:, D:], both.commands)
        assert same_bits(both.rew, torch.tensor(RR.ordered_sum(both.reward_terms.cpu().numpy()))), t
        assert (both.reward_terms[:, 0] == 0).all() and torch.isfinite(both.reward_terms).all()
        assert not torch.equal(both.rew, plain.rew)
    for e in (plain, both):
        e.close()


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_trainer(tmp_path):
    """two PPO iterations at 64 envs with rewards="locomotion" and captured graphs: finite losses, a per-term log line, and a
    checkpoint that carries the specification and the command"""
    from trex_gym import trex_train
    args = trex_train.parse_args(["--rewards", "locomotion", "--command", "0.5", "0", "0.1", "--observations", "locomotion", "--graphs"])
    env = trex_train.build_environment(64, device=DEV, observations=args.observations, rewards=args.rewards, command=args.command,
                                       max_episode_steps=40)
    assert env.obs_dim == 96 and env.reward_terms is not None and torch.equal(env.commands[5].cpu(), torch.tensor([0.5, 0.0, 0.1]))
    path = str(tmp_path / "policy.pt")
    lines = []
    agent, hist = trex_train.train(env, 2 * 64 * 32, 0, nsteps=32, noptepochs=1, save_path=path, log=lines.append, use_graphs=True)
    assert len(hist) == 2 and agent.kern.D == 96
    for h in hist:
        assert all(np.isfinite(h[k]) for k in ("policy_loss", "value_loss", "entropy", "mean_step_reward"))
        assert list(h["reward_terms"]) == env.reward_names and np.isfinite(list(h["reward_terms"].values())).all()
        assert abs(sum(h["reward_terms"].values()) - h["mean_step_reward"]) <= 1e-3 * max(1.0, abs(h["mean_step_reward"]))
    assert hist[0]["reward_terms"] != hist[1]["reward_terms"]
    assert sum("reward terms/step" in l and "track_lin_vel" in l for l in lines) == 2
    env.close()
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    assert again.env.rewards == env.rewards and again.env.observations == env.observations and again.env.obs_dim == 96
    assert again.env.reward_names == env.reward_names and torch.equal(again.env.commands[3].cpu(), torch.tensor([0.5, 0.0, 0.1]))
    _, rewards = trex_train.play(again, 3, log=lambda *a: None)
    assert np.isfinite(rewards).all()
    again.env.close()
    with pytest.raises(ValueError, match="--rewards"):
        trex_train.build_environment(4, device=DEV, rewards="no_such_preset")


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_bullet_env_reports_the_breakdown():
    """TrexBulletEnv(rewards=, command=): the reward of step() is the composed one, info carries weight x value per term"""
    from trex_gym import rewards as R
    from trex_gym.trex_env import TrexBulletEnv
    env = TrexBulletEnv(urdf_path=ASSET_URDF, device=DEV, rewards=R.alive(2.0) + R.track_lin_vel(1.0, 0.25) + R.joint_vel(-1e-3),
                        command=(0.5, 0.0, 0.0))
    assert torch.equal(env._vec.commands.cpu(), torch.tensor([[0.5, 0.0, 0.0]]))
    for _ in range(2):
        _, reward, _, info = env.step(np.zeros(J, np.float32))
        terms = info["reward_terms"]
        assert list(terms) == ["alive", "track_lin_vel", "joint_vel"] and terms["alive"] == 2.0 and 0.0 < terms["track_lin_vel"] <= 1.0
        assert np.float32(reward) == RR.ordered_sum(np.array([list(terms.values())], np.float32))[0]
    env.close()
    plain = TrexBulletEnv(urdf_path=ASSET_URDF, device=DEV)
    assert "reward_terms" not in plain.step(np.zeros(J, np.float32))[3]
    plain.close()


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_air_time_timer_restarts_with_an_episode_end_and_a_reset(oracle64, model):
    """Three envs drop from the start pose. Env 0's episode ends in mid-air (the limit inside the step launch puts it back on the
    start pose), env 2 is reset in mid-air by reset_tensor(mask), env 1 falls undisturbed. When the feet land, the GPU's
    FOOT_AIR_TIME pays the time since the restart - not since the first drop began: the timers went to zero with the done row and
    with trex_batch_reward_reset. The expected payout counts, from the GPU's own sensor, the steps without contact since the
    restart; (steps + 2) 2^-23 of it is the f32 sum's bound (reward_ref.bound)."""
    from trex_gym import rewards as R
    q0 = model["q_start"][model["obs_order"]]
    s = oracle64.new_state()
    oracle64.reset(s)
    first = None
    for t in range(40):
        oracle64.step(s, q0)
        if len(oracle64.contacts(s)[0]):
            first = t
            break
    assert first is not None and first >= 6, first
    half = first // 2                                                                     # the restarts: well before anything lands
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    toes = [l for l in range(len(names)) if "toe" in names[l]]
    feet = sorted(set(toes[:2] + toes[-2:]))
    offset = 0.05
    n, L = 3, 1000
    v = make_vec(n, rewards=[c for l in feet for c in R.foot_air_time(1.0, l, threshold=1.0, offset=offset)], max_episode_steps=L)
    v.reset_tensor()
    v.set_episode_steps(torch.tensor([L - half, 0, 0], dtype=torch.int32))
    Ts, p1 = step_seconds(v), float(np.float32(offset))
    act = torch.tensor(np.tile(q0, (n, 1)), dtype=torch.float32, device=DEV)
    count = np.zeros((n, len(feet)), int)                                                 # steps without contact since the restart
    since = np.zeros(n, int)                                                              # steps since the env's restart
    paid = [[] for _ in range(n)]
    for t in range(half + first + 6):
        if t == half:
            v.reset_tensor(torch.tensor([0, 0, 1], dtype=torch.uint8, device=DEV))
            count[2], since[2] = 0, 0
        v.step_tensor(act)
        terms = v.reward_terms.cpu().numpy()
        fz = v.contact_wrench()[:, lb[feet], 2].cpu().numpy()
        done = v.done.cpu().numpy()
        assert bool(done[0]) == (t == half - 1) and not done[1:].any()
        for e in range(n):
            if done[e]:
                assert (terms[e] == 0).all()                                              # held values: nothing was paid in the air
                count[e], since[e] = 0, 0
                continue
            since[e] += 1
            for k in range(len(feet)):
                if fz[e, k] > 1.0:
                    want = count[e, k] * Ts - p1 if count[e, k] > 0 else 0.0
                    assert abs(terms[e, k] - want) <= (count[e, k] + 2) * 2 * U * count[e, k] * Ts + 2 * U * abs(want), (t, e, k, terms[e, k], want)
                    if count[e, k] > 0:
                        paid[e].append((t, count[e, k], since[e]))
                    count[e, k] = 0
                else:
                    assert terms[e, k] == 0
                    count[e, k] += 1
    # every env landed; the restarted ones later than env 1, and each was paid its own fall: as long as env 1's, not longer
    assert all(paid[e] for e in range(n)), paid
    t1, c1, _ = paid[1][0]
    for e in (0, 2):
        te, ce, se = paid[e][0]
        assert te >= t1 + half - 2 and ce <= se < te + 1 and abs(ce - c1) <= 2, (paid[1][0], paid[e][0])
    v.close()
