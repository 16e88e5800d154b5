"""The per-env state of the row features on the GPU at the shapes where a wrong offset in its layout (csrc/host_tables.cpp:
reward_hist_layout, motion_clock_layout, motion_held_layout, sense_counter_layout, sense_hist_layout, rand_state_layout) would show:
n = 3 - an odd count of 4-byte members behind one another - with every count at its limit: 32 reward terms on 2J-wide actions,
8 motion terms with 8 end effectors, 64 sensing groups with every column late and with none, the action delay on 2J columns,
16 randomisation terms with 4 pushes and with none. Each feature takes three steps with a done raised for env 0 in the second,
then a reset of env 1 alone and a fourth step that shows it, against the numpy references and with the comparisons and
tolerances of its own suite (tests/test_gpu_rewards.py, _motion, _sensing, _randomize; bitwise where they are bitwise); what
sensing_info and randomization_info copy out is compared after every step. tests/test_sensing_tables_host.py and its kin check
the same layouts on the CPU."""
import numpy as np
import pytest
import torch

import motion_ref as MR
import randomize_cases as RC
import randomize_ref as RND
import reward_ref as RR
import sensing_cases as SC
import sensing_ref as SR
import test_gpu_motion as TM
import test_gpu_randomize as TZ
import test_gpu_rewards as TR
import test_gpu_sensing as TS
from gpu_support import DEV, guarded, guards_intact, make_vec, refused
from randomize_ref import COMMAND, FRICTION, KD, KP, MASS, MAX_FORCE, PUSH

pytestmark = pytest.mark.gpu
N, J, NB = 3, 25, 26
INVALID = -1
DONE_STEP, DONE_ENV, RESET_STEP, RESET_ENV = 1, 0, 3, 1
RESET_MASK = (np.arange(N) == RESET_ENV).astype(np.uint8)


def reset_mask():
    return torch.as_tensor(RESET_MASK, device=DEV)


def test_rewards_32_terms_on_2J_actions(oracle64, model):
    A = 2 * J
    v = TR.sensed_cases(oracle64, model, N, variable_stiffness=True)
    assert v.A == A
    spec = TR.full_spec(model)
    assert TR.api(v).set_reward(spec) == RR.MAX_TERMS == 32
    Ts = TR.step_seconds(v)
    hists = [RR.new_history(32, J, A) for _ in range(N)]
    prev = None
    for t in range(4):
        if t == RESET_STEP:
            TR.api(v).reward_reset(reset_mask())
            RR.reset_history(hists[RESET_ENV])
        act, cmd = TR.inputs(N, seed=70 + t, J=A)
        act[:, J:] = 0.01 * act[:, J:].abs()                                       # the stiffness columns
        v.step_tensor(act)
        rows = v.rows.clone()
        rows[:, 3 * J + 1] = 0.0
        if t == DONE_STEP:
            rows[DONE_ENV, 3 * J + 1] = 1.0
        state, force = TR.instant(v)
        after, terms, ok = TR.compose(v, rows, act, cmd, 32)
        assert ok
        prev = TR.check(model, spec, rows, after, terms, state, force, hists, Ts, act, cmd, prev_terms=prev)
    assert (prev[[0, 2], 12] != 0).all() and prev[RESET_ENV, 12] == 0              # ACTION_RATE: the reset env has no history
    v.close()


def test_motion_8_terms_8_end_effectors(oracle64, model):
    T, K = 8, 8
    v = TM.stepped_cases(oracle64, model, N)
    state = v.get_state().cpu().numpy().astype(np.float64)
    tab, probes = TM.set_clip(v, model, TM.offset_clip(model, state[1]), K=K)
    spec = TM.spec_of(T, K)
    assert TM.mapi(v).set_reward(spec, 1.0) == T
    clocks, helds = [MR.new_clock() for _ in range(N)], [np.zeros(T) for _ in range(N)]
    Ts = TM.step_seconds(v)
    rows = v.rows.clone()
    rows[:, 3 * J + 1] = 0.0
    prev = None
    for t in range(4):
        if t == RESET_STEP:                                                         # env 1 alone: its clock starts at 0.05 s, its state is the clip's
            when = np.float32(0.05)
            TM.mapi(v).reset(reset_mask().bool(), torch.full((N,), float(when), device=DEV))
            torch.cuda.synchronize()
            after_reset = v.get_state().cpu().numpy().astype(np.float64)
            assert after_reset[[0, 2]].tobytes() == state[[0, 2]].tobytes() and after_reset[1].tobytes() != state[1].tobytes()
            state = after_reset
            clocks[RESET_ENV] = dict(t0=float(when), k=0)
            helds[RESET_ENV][:] = 0.0
        r = rows.clone()
        if t == DONE_STEP:
            r[DONE_ENV, 3 * J + 1] = 1.0
        after, terms, ok = TM.compose(v, r, T)
        assert ok
        prev = TM.check_compose(model, tab, probes, spec, 1.0, r, after, terms, state, clocks, helds, Ts, prev)
    assert [c["k"] for c in clocks] == [2, 1, 4]                                    # restarted by the done row, by the reset, never
    own, _, _ = TM.sample(v, None, K)                                               # the device's clocks are the reference's
    times = np.array([MR.clock_time(c, Ts) for c in clocks], np.float32)
    assert own.cpu().numpy().tobytes() == TM.sample(v, times, K)[0].cpu().numpy().tobytes()


def sixty_four_groups(late):
    """64 groups over the 75 columns: every one of them with a delay to draw (all 75 columns have a history), or none"""
    return [g[:6] + ((g[6], max(g[7], 1)) if late else (0, 0)) for g in SC.sixty_four(3 * J)]


@pytest.mark.parametrize("late", [True, False], ids=["every_column_late", "no_column_late"])
def test_sensing_64_groups_and_the_action_delay_on_2J_columns(late):
    D, A, seed, offset = 3 * J, 2 * J, 31, 9
    groups = sixty_four_groups(late)
    case = SC.Case("layout_n3_late%d" % late, "trex", N, D, 2, groups, seed, offset, True, 0, 0.0)
    v = make_vec(N, variable_stiffness=True)
    assert v.batch.observation_dim() == D and v.A == A
    api = TS.api_of(v)
    assert api.set_sensing(groups, seed, offset) == 64
    api.set_action_delay(0, 8)
    assert api.info() == dict(groups=64, delayed_columns=D if late else 0, action_delay=(0, 8))
    sens, delay = SR.Sensors(N, D, 2, groups, seed, offset), SR.ActionDelay(N, A, 0, 8, seed, offset)
    inputs, want, got = [], [], []
    whole_d, drawn = guarded((N, 64), fill=7, dtype=torch.int32)
    whole_a, drawn_act = guarded((N,), fill=7, dtype=torch.int32)
    whole_o, out = guarded((N, A), fill=float("nan"))
    done_prev = None
    for t in range(4):
        if t == RESET_STEP:
            api.reset(reset_mask())
            sens.reset(RESET_MASK)
            delay.reset(RESET_MASK != 0)
        rows = SC.rows_of(case, t)
        rows[DONE_ENV, D + 1] = float(t == DONE_STEP)
        dev = torch.as_tensor(rows, device=DEV)
        api.apply(dev)
        acts = SC.action_rows(seed, t, N, A)
        api.delay_actions(torch.as_tensor(acts, device=DEV), out, None if done_prev is None else torch.as_tensor(done_prev, device=DEV))
        api.info(delays=drawn, action_delays=drawn_act)
        torch.cuda.synchronize()
        inputs.append(rows)
        want.append(sens.apply(rows))
        got.append(dev.cpu().numpy())
        assert (drawn.cpu().numpy() == sens.delay[:, :64]).all(), t
        assert out.cpu().numpy().tobytes() == delay.step(acts, done_prev).tobytes(), t
        assert (drawn_act.cpu().numpy() == delay.delay).all(), t
        assert guards_intact(whole_d, (N, 64), fill=7) and guards_intact(whole_a, (N,), fill=7) and guards_intact(whole_o, (N, A), fill=float("nan"))
        done_prev = (rows[:, D + 1] != 0).astype(np.uint8)
    r = SC.compare(case, want, got, inputs=inputs)
    assert not r["failures"], r["failures"][:6]
    assert r["left_out"] <= 0.01
    assert sens.ep.tolist() == [2, 2, 1]                                            # restarted by the done row, by the reset, never


def bits(*elements):
    return sum(1 << i for i in elements)


def sixteen_without_pushes():
    return [(MASS, bits(0), 0, 1, 0.9, 1.1, 0, 0, 0.0), (MASS, bits(*range(1, 9)), 0, 0, 0.8, 1.2, 0, 0, 0.0),
            (MASS, bits(*range(9, 17)), 0, 0, 0.7, 1.3, 0, 0, 0.0), (MASS, bits(*range(17, 26)), 0, 1, 0.5, 2.0, 0, 0, 0.0),
            (FRICTION, 0, 0, 0, 0.4, 1.0, 0, 0, 0.0),
            (KP, bits(*range(0, 8)), 0, 0, 0.8, 1.2, 0, 0, 0.0), (KP, bits(*range(8, 16)), 0, 1, 0.9, 1.1, 0, 0, 0.0),
            (KP, bits(*range(16, 25)), 0, 0, 0.7, 1.3, 0, 0, 0.0),
            (KD, bits(*range(0, 25, 3)), 0, 0, 0.8, 1.2, 0, 0, 0.0), (KD, bits(*range(1, 25, 3)), 0, 0, 1.0, 1.0, 0, 0, 0.0),
            (KD, bits(*range(2, 25, 3)), 0, 1, 0.5, 1.5, 0, 0, 0.0),
            (MAX_FORCE, bits(*range(0, 12)), 0, 0, 0.5, 1.0, 0, 0, 0.0), (MAX_FORCE, bits(*range(12, 25)), 0, 1, 0.9, 1.1, 0, 0, 0.0),
            (COMMAND, 0, 0, 0, -1.0, 1.5, 4, 0, 0.5), (COMMAND, 0, 1, 0, -0.3, 0.3, 0, 0, 0.0), (COMMAND, 0, 2, 0, -0.5, 0.5, 4, 0, 0.0)]


@pytest.mark.parametrize("pushes", [4, 0], ids=["4_pushes", "no_push"])
def test_randomization_16_terms(pushes):
    terms = RC._sixteen() if pushes else sixteen_without_pushes()
    assert len(terms) == 16 and sum(t[0] == PUSH for t in terms) == pushes
    seed, offset = 41, 2 ** 32 - N                                                  # the last three global indices there are
    api = TZ.api_of(make_vec(N), terms, seed, offset)
    r32, r64 = (RND.Randomizer(N, NB, J, terms, seed, offset, f32=f) for f in (True, False))
    whole_c, command = guarded((N, 3))
    command.zero_()
    whole_v, values = guarded((N, 16, 32))
    whole_f, force = guarded((N, max(pushes, 1), 3))
    whole_l, left = guarded((N, max(pushes, 1)), fill=7, dtype=torch.int32)
    if not pushes:
        refused(INVALID, api.info, None, force)
        refused(INVALID, api.info, None, None, left)
    run = []
    for t in range(4):
        if t == RESET_STEP:
            api.reset(reset_mask())
            r32.reset(RESET_MASK)
            r64.reset(RESET_MASK)
        done = np.zeros(N, np.float32)
        done[DONE_ENV] = float(t == DONE_STEP)
        api.apply(torch.as_tensor(done, device=DEV), command)
        assert api.info(values, force if pushes else None, left if pushes else None) == 16
        torch.cuda.synchronize()
        run.append((r32.apply(done), r64.apply(done), values.cpu().numpy(), force.cpu().numpy(), left.cpu().numpy(), command.cpu().numpy()))
    assert guards_intact(whole_c, (N, 3)) and guards_intact(whole_v, (N, 16, 32))
    assert guards_intact(whole_f, (N, max(pushes, 1), 3)) and guards_intact(whole_l, (N, max(pushes, 1)), fill=7)
    # the comparison of randomize_cases.compare, on this run's own f32 and f64 references
    dev = max(float(np.abs(a.push_force.astype(np.float64) - b.push_force).max(initial=0.0)) for a, b, *_ in run)
    bound = max(4.0 * dev, 2.0 * RC.ulp32(max([x[5] for x in terms if x[0] == PUSH], default=0.0)))
    for t, (a, b, got_values, got_force, got_left, got_command) in enumerate(run):
        assert got_values.tobytes() == a.values.astype(np.float32).tobytes(), t
        assert got_command.tobytes() == a.command.astype(np.float32).tobytes(), t
        if pushes:
            assert np.array_equal(got_left.astype(np.int64), a.push_left), t
            assert (got_force[b.push_force == 0] == 0).all(), t
            assert float(np.abs(got_force.astype(np.float64) - b.push_force).max()) <= bound, t
    assert not pushes or any((b.push_force != 0).any() for _, b, *_ in run)         # a push was under way in these rows
