"""The composed env on the GPU: TrexVecEnv with EVERY row feature attached at once - channels with the commands and the previous
action, reward terms, a motion clip, episode randomisation, the monitor, the joint sensor, the sensor model with an action delay,
the privileged critic's row, fall termination and an episode limit - on the scenario of tests/pipeline_cases.py, which
tests/test_pipeline_cases_host.py qualifies on the CPU.

 1 the chain: after the reset, every step and the masked reset, what the device left is compared stage by stage with the feature's
   own numpy reference, each fed the DEVICE's output of the stage before - with the comparison and the bound of the feature's own
   suite: the delayed action and the drawn delays bitwise (test_gpu_sensing.test_delay_actions_against_the_reference);
   reward_terms by test_gpu_rewards.check; motion_terms by test_gpu_motion.check_compose; randomisation values, commands and
   push_left bitwise and the push force within the bound of randomize_cases.compare as test_gpu_state_layouts restates it; the
   monitor by monitor_cases.same_state and test_gpu_monitor.same_records; the joint sensor bitwise against the bare query
   (test_gpu_joint_wrench.test_attached_sensor_is_the_bare_query); the clean block by test_gpu_observations.check_rows; rows by
   sensing_cases.compare; critic_rows bitwise (test_gpu_critic.test_privileged_rows_follow_the_env); the step's own 3J columns and
   the terminal observations bitwise against a plain twin given the reported randomisation values
   (test_gpu_randomize.test_a_twin_given_the_reported_values_steps_the_same_rows).
   The references that walk the kinematic tree in Python (reward terms, motion terms, channels) are evaluated for the envs of ENVS -
   both ends of the batch, both sides of the 8-env workgroup's edge, reset and not -; everything else for all 33.
 2 twins with exactly one feature left off differ only in what that feature owns;  3 a captured step_tensor replays as the eager
   one;  4 the trainer with every flag, eager and with graphs;  5 attach orders either work or are refused at attach time, and
   taking every feature off again leaves a plain env."""
import numpy as np
import pytest
import torch

import monitor_cases as MCASES
import monitor_ref as MON
import motion_ref as MR
import pipeline_cases as PC
import randomize_cases as RC
import randomize_ref as RND
import reward_ref as RR
import sensing_cases as SC
import sensing_ref as SR
import test_gpu_monitor as TMON
import test_gpu_motion as TM
import test_gpu_observations as TO
import test_gpu_randomize as TZ
import test_gpu_rewards as TR
from gpu_support import DEV, make_vec, same_bits

pytestmark = pytest.mark.gpu
N, J, NB = PC.N, PC.J, PC.NB
ENVS = [0, 1, 7, 8, 9, 15, 16, 31, 32]


@pytest.fixture(scope="module")
def sc(oracle64, model):
    return PC.scenario(oracle64, model)


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=DEV)


def test_the_specifications_are_the_presets(sc, model):
    """what pipeline_cases derives on the oracle is what the presets find with their query on the device"""
    from trex_gym import _capi, observations as O, rewards as R
    m = _capi.Model()
    assert O.as_tuples(O.locomotion(m, DEV)) == O.as_tuples(sc.locomotion)
    assert R.as_tuples(R.locomotion(m, DEV)) == R.as_tuples(sc.rewards)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def random_inputs(env, base=None):
    """what a plain twin is given before a step so that it steps as the randomised env does: mass scale, friction, the three gains
    and the wrench, from _info and the nominal (the construction of test_gpu_randomize.twin_inputs for the scenario's terms)"""
    n, terms = env.num_envs, env.randomization["terms"]
    values, force, left = (dev(x, torch.int32 if i == 2 else torch.float32) for i, x in enumerate(TZ.read(env.random_api, n)))
    kind = lambda k: [t for t, x in enumerate(terms) if x[0] == k]
    gains = []
    for k, name in ((RND.KP, "motor_kp"), (RND.KD, "motor_kd"), (RND.MAX_FORCE, "motor_max_force")):
        t = kind(k)[0]
        assert terms[t][1] == 0                                                     # (no mask: every joint is covered)
        nominal = torch.full((n, J), env.model.get_param(name), dtype=torch.float32, device=DEV)
        gains.append((nominal * values[:, t, :J]).contiguous())
    wrench = torch.zeros(n, NB, 6, device=DEV) if base is None else base.clone()
    for p, t in enumerate(kind(RND.PUSH)):
        body = terms[t][2]
        on = (left[:, p] > 0)[:, None]
        wrench[:, body, :3] = torch.where(on, wrench[:, body, :3] + force[:, p], wrench[:, body, :3])
    return values[:, kind(RND.MASS)[0], :NB].contiguous(), values[:, kind(RND.FRICTION)[0], 0].contiguous(), gains, wrench


def give(probe, inputs):
    mass, friction, gains, wrench = inputs
    probe.batch.set_domain(mass, friction)
    probe.batch.set_motor_gains(*gains)
    probe.batch.set_external_wrench(wrench)


class Stages:
    """the references of one env, and the comparison of every stage after a reset and after a step"""

    def __init__(self, env, sc, model, variant):
        from trex_gym import joint_wrench_capi
        self.env, self.sc, self.model, self.variant = env, sc, model, variant
        n = self.n = env.num_envs
        self.channels = variant != "no_channels"
        self.tail = 5 if variant == "penalties_in_rows" else 2
        self.D = env.obs_dim
        self.groups = sc.groups if self.channels else sc.groups_3j
        assert [tuple(g) for g in env.sensing["groups"]] == [tuple(g) for g in self.groups] and env.env_lo == 0
        assert [tuple(t) for t in env.randomization["terms"]] == [tuple(t) for t in sc.random_terms]
        self.delay = SR.ActionDelay(n, J, PC.ACTION_DELAY[0], PC.ACTION_DELAY[1], PC.SENSE_SEED, 0)
        self.sensors = SR.Sensors(n, self.D, self.tail, self.groups, PC.SENSE_SEED, 0)
        self.r32, self.r64 = (RND.Randomizer(n, NB, J, sc.random_terms, PC.RAND_SEED, 0, f32=f) for f in (True, False))
        T, Tm = len(sc.reward_terms), len(sc.motion_terms)
        assert env.reward_terms.shape == (n, T) and env.motion_terms.shape == (n, Tm) and env._rew_actions
        self.monitor = MON.Monitor(n, PC.WINDOW, T + Tm, 0)
        self.hists = {e: RR.new_history(T, J, J) for e in ENVS}
        self.clocks, self.helds = {e: MR.new_clock() for e in ENVS}, {e: np.zeros(Tm) for e in ENVS}
        self.prev_reward = self.prev_motion = None
        self.Ts = TR.step_seconds(env)
        self.joint_api = joint_wrench_capi.BatchJointWrench(env.batch)
        self.inv_dt = torch.tensor(1.0 / (env.model.get_param("dt") * env.model.get_param("substeps")), dtype=torch.float32, device=DEV)
        self.sense_log = dict(inputs=[], want=[], got=[])
        self.random_log = []
        self.counts = dict(late=0, limit=0, fall=0, both=0, moved=0, delays=set(), pushing=0)
        self.probe = make_vec(n)
        self.probe.reset_tensor()
        self.probe_rows = torch.zeros(n, 3 * J + 2, device=DEV)
        self.last_velocity = None

    # -- the small readers
    def velocity(self, state):
        return torch.cat([state[:, 7:13], state[:, 13 + J:13 + 2 * J]], 1)

    def step_rows(self):
        env = self.env
        return (env._step_rows if self.channels else env.clean_rows).clone()

    def drawn(self):
        n, G = self.n, len(self.groups)
        delays, action = torch.zeros(n, G, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        self.env.sense_api.info(delays=delays, action_delays=action)
        return delays.cpu().numpy(), action.cpu().numpy()

    # -- the stages that follow the step call, shared by a reset and a step
    def randomisation(self, done):
        env = self.env
        a, b = self.r32.apply(done), self.r64.apply(done)
        values, force, left = TZ.read(env.random_api, self.n)
        assert values.tobytes() == a.values.astype(np.float32).tobytes(), "randomisation values"
        assert env.commands.cpu().numpy().tobytes() == a.command.astype(np.float32).tobytes(), "commands"
        assert np.array_equal(left.astype(np.int64), a.push_left), "push_left"
        self.random_log.append((a, b, force))
        self.counts["pushing"] += int((a.push_left > 0).sum())

    def joint_sensor(self, state, done):
        env = self.env
        now = self.velocity(state)
        acc = torch.zeros_like(now) if done is None else (now - self.last_velocity) * self.inv_dt
        if done is not None:
            acc[done] = 0.0
        self.last_velocity = now
        base = torch.zeros(self.n, 6, device=DEV)
        want = self.joint_api.joint_wrench(acc, env.contact_wrench(), None, "link", None, base)
        assert same_bits(env.joint_reaction, want) and same_bits(env.joint_base_residual, base), "joint sensor"

    def composed(self, rows, state, action):
        """clean block, rows, critic's row"""
        env, sc, n, D = self.env, self.sc, self.n, self.D
        clean = env.clean_rows
        if self.channels:
            TO.check_rows(self.model, sc.chans, clean, rows, state, action, env.commands, env.contact_wrench()[:, :, 2], envs=ENVS)
            assert same_bits(clean[:, 3 * J + 18:3 * J + 21], env.commands)           # the command in force from now on, every env
            shown = torch.zeros(n, J, device=DEV) if action is None else torch.where((rows[:, 3 * J + 1] != 0)[:, None], torch.zeros_like(action), action)
            assert same_bits(clean[:, D - J:D], shown), "prev_action: the policy's own action; zeros for a new episode"
        else:
            assert same_bits(clean, rows)
        block = clean.cpu().numpy().copy()
        self.sense_log["inputs"].append(block)
        self.sense_log["want"].append(self.sensors.apply(block))
        self.sense_log["got"].append(env.rows.cpu().numpy().copy())
        assert same_bits(env.rows[:, D:], clean[:, D:]), "the tail columns pass the sensors"
        delays, _ = self.drawn()
        assert (delays == self.sensors.delay[:, :len(self.groups)]).all(), "sensing delays"
        self.critic(clean)

    def critic(self, clean):
        env, n = self.env, self.n
        got, col = env.critic_rows, 0
        values, force, _ = (dev(x) for x in TZ.read(env.random_api, n))
        for kind, arg in env.critic_spec["sources"]:
            if kind == "clean":
                want = clean[:, :self.D]
            elif kind == "random":
                want = values[:, arg[0]][:, arg[1]]
            elif kind == "push_force":
                want = force[:, :, :2].reshape(n, -1)
            else:
                assert kind == "contact"
                want = env.contact_wrench()[:, [int(b) for b in env._link_bodies(arg)], :3].reshape(n, -1)
            assert same_bits(got[:, col:col + want.shape[1]], want), "critic source %s" % kind
            col += want.shape[1]
        assert col == got.shape[1]

    # -- a reset
    def after_reset(self, mask=None, before=None):
        """mask: numpy uint8 or None; before: the state before a masked reset"""
        env, n = self.env, self.n
        marked = np.ones(n, bool) if mask is None else mask != 0
        state = env.get_state()
        if before is not None:
            assert same_bits(state[dev(~marked, torch.bool)], before[dev(~marked, torch.bool)]), "the other envs' state is untouched"
        if env._rsi:
            want = TM.sample(env, env._rsi_time.cpu().numpy(), len(self.sc.feet))[0]
            assert same_bits(state[dev(marked, torch.bool)], want[dev(marked, torch.bool)]), "the RSI state"
        for e in ENVS:
            if marked[e]:
                RR.reset_history(self.hists[e])
                t0 = float(env._rsi_time[e]) if env._rsi else 0.0
                self.clocks[e], self.helds[e][:] = dict(t0=t0, k=0), 0.0
        for r in (self.r32, self.r64, self.delay, self.sensors, self.monitor):
            r.reset(mask if r is not self.delay else marked)
        assert not bool(env.done[dev(marked, torch.bool)].any())
        self.randomisation(np.zeros(n, np.float32))
        self.joint_sensor(state, None)
        rows = self.step_rows()
        assert float(rows[dev(marked, torch.bool)][:, 3 * J:3 * J + 2].abs().max()) == 0.0
        self.composed(rows, state, None)
        got, _ = TMON.read(env.monitor_api, n)
        assert not MCASES.same_state(self.monitor.state(), got), MCASES.same_state(self.monitor.state(), got)

    # -- a step
    def step(self, action):
        env, sc, n, model = self.env, self.sc, self.n, self.model
        done_prev = env.done.cpu().numpy().astype(np.uint8)
        commands_before = env.commands.clone()
        state_before = env.get_state()
        give(self.probe, random_inputs(env))
        env.step_tensor(action)
        torch.cuda.synchronize()
        # the action the motors got
        applied = self.delay.step(action.cpu().numpy(), done_prev)
        assert env._delayed_actions.cpu().numpy().tobytes() == applied.tobytes(), "delayed action"
        _, drawn = self.drawn()
        assert (drawn == self.delay.delay).all(), "action delays"
        self.counts["delays"] |= set(drawn.tolist())
        self.counts["late"] += int((applied != action.cpu().numpy()).any(axis=1).sum())
        rows, state = self.step_rows(), env.get_state()
        done = rows[:, 3 * J + 1] != 0
        done_np, reason = done.cpu().numpy(), env.termination_reason.cpu().numpy().copy()
        assert same_bits(done, env.done) and not (reason[~done_np] != 0).any()
        limit, fall = done_np & (reason == 0), reason != 0
        for k, v in (("limit", limit.sum()), ("fall", fall.sum()), ("both", limit.any() and fall.any())):
            self.counts[k] += int(v)
        # the step's own columns and the terminal observations: a plain twin at the state before, given the reported values
        self.probe.set_state(state_before)
        self.probe.batch.step_rows(dev(applied), self.probe_rows)
        keep = ~done
        assert same_bits(rows[keep][:, :3 * J], self.probe_rows[keep][:, :3 * J]), "the step's rows under the reported randomisation"
        if fall.any():
            f = dev(fall, torch.bool)
            assert same_bits(env.terminal_obs[f], self.probe_rows[f][:, :3 * J]), "terminal observations are clean"
        # reward terms: the state of the row's instant, the POLICY's action, the command from BEFORE the redraw
        force = env.contact_wrench()[:, :, :3].cpu().numpy()
        state64 = state.cpu().numpy().astype(np.float64)
        idx = dev(ENVS, torch.long)
        terms = env.reward_terms.clone()
        column = dev(RR.ordered_sum(terms.cpu().numpy()))
        before = rows.clone()
        before[:, 3 * J] = 0.0                                                       # (the step's own reward: a term of weight 0)
        after = before.clone()
        after[:, 3 * J] = column
        prev = None if self.prev_reward is None else self.prev_reward[ENVS]
        TR.check(model, sc.reward_terms, before[idx], after[idx], terms[idx], state64[ENVS], force[ENVS], [self.hists[e] for e in ENVS],
                 self.Ts, action[idx], commands_before[idx], prev_terms=prev)
        if self.prev_reward is not None and done_np.any():                           # a done row holds the step before, every env
            assert same_bits(terms[done][:, 1:], dev(self.prev_reward)[done][:, 1:])
        self.prev_reward = terms.cpu().numpy()
        # motion terms, and the reward column behind them
        mterms = env.motion_terms.clone()
        prevm = None if self.prev_motion is None else self.prev_motion[ENVS]
        TM.check_compose(model, sc.tab, sc.probes, sc.motion_terms, 1.0, after[idx], rows[idx], mterms[idx], state64[ENVS],
                         [self.clocks[e] for e in ENVS], [self.helds[e] for e in ENVS], self.Ts, prevm)
        final = MR.ordered_sum(column.cpu().numpy(), mterms.cpu().numpy())
        assert rows[:, 3 * J].cpu().numpy().tobytes() == final.tobytes(), "the reward column: rewards' compose, then motion's"
        self.prev_motion = mterms.cpu().numpy()
        if env._rsi:
            drawn_t = env._rsi_time.cpu().numpy()
            for e in ENVS:
                if done_np[e]:
                    self.clocks[e].update(t0=float(drawn_t[e]), k=0)
            if done_np.any():
                want = TM.sample(env, drawn_t, len(sc.feet))[0]
                assert same_bits(state[done], want[done]), "the RSI state"
        # randomisation, driven by the device's done column
        self.randomisation(rows[:, 3 * J + 1].cpu().numpy())
        moved = (env.commands - commands_before).abs().max(dim=1).values > 0.1
        self.counts["moved"] += int((moved & done).sum())
        # the monitor: the reward column AFTER the motion terms, the done column, the batch's reasons, the two blocks
        self.monitor.apply(final, rows[:, 3 * J + 1].cpu().numpy(), reason, np.concatenate([terms.cpu().numpy(), mterms.cpu().numpy()], 1))
        got, _ = TMON.read(env.monitor_api, n)
        want = self.monitor.state()
        assert not MCASES.same_state(want, got), MCASES.same_state(want, got)
        assert TMON.same_records(TMON.ring_records(got, got["total"]), TMON.ring_records(want, want["total"]))
        self.joint_sensor(state, done)
        self.composed(rows, state, action)
        assert same_bits(env.rew, env.rows[:, self.D]) and env.rew.cpu().numpy().tobytes() == final.tobytes()

    # -- the end of the run
    def finish(self, loose=True):
        env, c = self.env, self.counts
        case = SC.Case("pipeline_" + self.variant, "locomotion", self.n, self.D, self.tail, self.groups, PC.SENSE_SEED, 0, True, 0, 0.0)
        log = self.sense_log
        r = SC.compare(case, log["want"], log["got"], inputs=log["inputs"])
        print("%s: sensing Gaussian deviation %.3f of the allowed bound, soft columns %.2f ulp, left out %.3f %%"
              % (self.variant, r["gaussian_share"], r["ulps"], 100 * r["left_out"]))
        assert not r["failures"], r["failures"][:6]
        assert not same_bits(env.obs, env.clean_obs)
        # the push forces: the comparison of randomize_cases.compare on this run's own f32 and f64 references
        dev_ = max(float(np.abs(a.push_force.astype(np.float64) - b.push_force).max(initial=0.0)) for a, b, _ in self.random_log)
        bound = max(4.0 * dev_, 2.0 * RC.ulp32(max(x[5] for x in self.sc.random_terms if x[0] == RND.PUSH)))
        for t, (a, b, got) in enumerate(self.random_log):
            assert (got[b.push_force == 0] == 0).all(), t
            assert float(np.abs(got.astype(np.float64) - b.push_force).max()) <= bound, t
        TR.report()
        TM.report()
        print("%s: %s" % (self.variant, c))
        if loose:                                    # the scenario's conditions, at the loose end of the host test's margins
            assert c["delays"] == {1, 2} and c["late"] >= 1 and c["limit"] >= 1 and c["fall"] >= 1 and c["moved"] >= 1 and c["pushing"] >= 1
            assert c["both"] >= 1 or self.variant == "rsi"      # (RSI starts the episodes elsewhere than the host's run does)
        self.probe.close()


def run_chain(oracle64, model, sc, variant, steps=PC.STEPS, order=PC.ORDER, loose=True):
    env = PC.build_env(oracle64, model, variant, order=order)
    if variant != "no_channels":
        assert env.obs_dim == 3 * J + 18 + 3 + J and env.clean_rows is not env.rows
    assert env.monitor_api.cols == len(sc.reward_terms) + len(sc.motion_terms) and env._rsi == (variant == "rsi")
    assert "clean" in [s[0] for s in env.critic_spec["sources"]] and (variant != "no_channels" or env.critic_spec["left_out"] == [])
    st = Stages(env, sc, model, variant)
    env.reset_tensor()
    st.after_reset()
    actions = dev(sc.actions)
    mask = PC.reset_mask()
    for t in range(steps):
        if t == PC.RESET_AFTER:
            before = env.get_state()
            env.reset_tensor(dev(mask, torch.uint8))
            st.after_reset(mask, before)
        st.step(actions[t])
    st.finish(loose)
    env.close()


@pytest.mark.parametrize("variant", PC.VARIANTS)
def test_chain_against_the_references(variant, oracle64, model, sc):
    run_chain(oracle64, model, sc, variant)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def everything(env):
    """every tensor of the env and the state, cloned"""
    out = dict(rows=env.rows, state=env.get_state(), done=env.done, reward_terms=env.reward_terms, commands=env.commands)
    for k in ("clean_rows", "motion_terms", "critic_rows", "joint_reaction", "joint_base_residual", "_delayed_actions", "_step_rows"):
        if getattr(env, k, None) is not None:
            out[k] = getattr(env, k)
    if env._term_on:
        out.update(reason=env.termination_reason, terminal_obs=env.terminal_obs)
    return {k: v.clone() for k, v in out.items()}


OWNED = dict(monitor=(), critic=("critic_rows",), joint_sensor=("joint_reaction", "joint_base_residual"))


@pytest.mark.parametrize("off", ["monitor", "critic", "joint_sensor", "sensing_groups", "action_delay", "motion", "randomize"])
def test_taking_one_feature_off_changes_only_what_it_owns(off, oracle64, model, sc):
    steps = 16
    variant = "full"
    full = PC.build_env(oracle64, model, variant)
    twin = PC.build_env(oracle64, model, variant, off=(off,))
    actions = dev(sc.actions)
    for v in (full, twin):
        v.reset_tensor()
    D = full.obs_dim
    differed = 0
    if off == "randomize":
        twin.commands.copy_(full.commands)
    for t in range(steps):
        fed = actions[t]
        if off == "randomize":          # the twin is given what the full env reports, and its commands
            give(twin, random_inputs(full))
        full.step_tensor(actions[t])
        if off == "action_delay":
            fed = full._delayed_actions
        if off == "randomize":
            old = twin.commands.clone()
        twin.step_tensor(fed)
        a, b = everything(full), everything(twin)
        if off in OWNED:
            for k in a:
                if k not in OWNED[off]:
                    assert same_bits(a[k], b[k]), (t, k)
            assert all(k not in b for k in OWNED[off])
        elif off == "sensing_groups":
            assert twin.clean_rows is twin.rows and same_bits(twin.rows, full.clean_rows), t
            assert same_bits(a["state"], b["state"]) and same_bits(a["critic_rows"][:, :D], b["critic_rows"][:, :D])
            differed += int(not same_bits(full.rows, full.clean_rows))
        elif off == "action_delay":
            assert same_bits(a["state"], b["state"]) and same_bits(a["_step_rows"][:, :3 * J], b["_step_rows"][:, :3 * J]), t
            assert same_bits(a["done"], b["done"]) and same_bits(a["motion_terms"], b["motion_terms"]) and same_bits(a["commands"], b["commands"])
            differed += int(not same_bits(fed, actions[t]))
        elif off == "motion":
            assert same_bits(a["state"], b["state"]) and same_bits(a["reward_terms"], b["reward_terms"]), t
            want = MR.ordered_sum(twin._step_rows[:, 3 * J].cpu().numpy(), full.motion_terms.cpu().numpy())
            assert full._step_rows[:, 3 * J].cpu().numpy().tobytes() == want.tobytes(), t
            assert same_bits(a["clean_rows"][:, :D], b["clean_rows"][:, :D]) and same_bits(a["commands"], b["commands"])
            differed += int(not same_bits(full.rew, twin.rew))
        else:
            # (the twin's step ran under the values of the step; its channels then show ITS commands: given behind the step, they
            # show from the next compose on - so the command columns are compared with the commands the twin held)
            keep = [c for c in range(D) if not 3 * J + 18 <= c < 3 * J + 21]
            assert same_bits(a["_step_rows"][:, :3 * J], b["_step_rows"][:, :3 * J]) and same_bits(a["state"], b["state"]), t
            assert same_bits(a["clean_rows"][:, keep], b["clean_rows"][:, keep]) and same_bits(b["clean_rows"][:, 3 * J + 18:3 * J + 21], old), t
            assert same_bits(a["done"], b["done"]) and same_bits(a["reason"], b["reason"]) and same_bits(a["reward_terms"], b["reward_terms"])
            twin.commands.copy_(full.commands)
            differed += int(bool((full.commands != old).any()))
    assert differed >= 3 or off in OWNED
    assert int(full.episode_steps.max()) < steps                                     # episodes ended on the way
    for v in (full, twin):
        v.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_captured_chain_replays_as_eager(oracle64, model, sc):
    """two warm-up steps, one step_tensor captured on a side stream, 12 replays with the action buffer refilled in place, against
    an eager twin: bitwise. (RSI off: tests/test_gpu_motion.py captures the motion launches, not a step with RSI's draw.) The
    chain is linear; nothing about queues or how graphs are replayed is set."""
    from trex_gym import randomize_capi
    eager, captured = (PC.build_env(oracle64, model, "full") for _ in range(2))
    actions = dev(sc.actions)
    act = torch.zeros(N, J, device=DEV)
    for v in (eager, captured):
        v.reset_tensor()
    for t in range(2):
        act.copy_(actions[t])
        eager.step_tensor(actions[t])
        captured.step_tensor(act)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured.step_tensor(act)

    def more(v):
        n, G = v.num_envs, len(v.sensing["groups"])
        delays, action = torch.zeros(n, G, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        v.sense_api.info(delays=delays, action_delays=action)
        state, summary = TMON.read(v.monitor_api, n)
        return [delays, action, v.episode_steps] + [dev(x) for x in TZ.read(v.random_api, n)], state, summary

    ends = 0
    for t in range(2, 14):
        act.copy_(actions[t])
        graph.replay()
        eager.step_tensor(actions[t])
        torch.cuda.synchronize()
        a, b = everything(eager), everything(captured)
        for k in a:
            assert same_bits(a[k], b[k]), (t, k)
        (xa, sa, ma), (xb, sb, mb) = more(eager), more(captured)
        assert all(same_bits(x, y) for x, y in zip(xa, xb)), t
        assert not MCASES.same_state(sa, sb) and ma.tobytes() == mb.tobytes(), t
        ends += int(eager.done.sum())
    assert ends >= N                                                                 # the replays cross an episode end of every env
    del graph
    for v in (eager, captured):
        v.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
TRAIN_N, NSTEPS, TRAIN_LIMIT, TRAIN_WINDOW = 64, 8, 6, 100


def trainer_env(tmp_path, model):
    from trex_gym import motion as M, observations as O, trex_train
    import motion_cases as MC
    clip = str(tmp_path / "clip.npz")
    M.Clip(MC.clip_frames(model, 33, seed=8), MC.DT).save(clip)
    # (channels narrower than the locomotion preset's: with the commands' and the phase's columns the row stays within the 96
    # columns the native learner stages)
    channels = O.as_tuples(O.gravity() + O.base_velocity() + O.base_height())
    return trex_train.build_environment(
        TRAIN_N, device=DEV, max_episode_steps=TRAIN_LIMIT, observations=channels, rewards="locomotion", motion=dict(clip=clip, rsi=False),
        sensing=dict(preset="typical", obs_delay=(0, 2), action_delay=(1, 2)), randomize=dict(preset="typical", push=100.0, command_interval=3),
        monitor=dict(window=TRAIN_WINDOW, terms=True), critic="privileged", terminate=dict(max_tilt=1.0))


def test_trainer_with_everything(tmp_path, model):
    """the form of tests/test_gpu_monitor_train.py: eprewmean / eplenmean are the host's recomputation from b_rew / b_done within
    the bound of the summary's means, and the eager and the graph run agree as that test requires"""
    from trex_gym import trex_train
    from trex_gym.ppo import PPO
    got = {}
    for graphs in (False, True):
        env = trainer_env(tmp_path, model)
        assert env.obs_dim == 3 * J + 10 + 3 + 2 and env.critic_rows.shape[1] <= 96 and env._term_on
        assert all(c is not None for c in (env.motion_config, env.sensing_config, env.randomize_config, env.monitor_config, env.critic_config))
        agent = PPO(env, nsteps=NSTEPS, nminibatches=8, noptepochs=1, seed=3, use_graphs=graphs, critic=True)
        rollouts = []

        def log(line):
            if line.startswith("it "):
                rollouts.append((agent.b_rew.cpu().numpy().copy(), agent.b_done.cpu().numpy().copy()))
        hist = agent.learn(2 * TRAIN_N * NSTEPS, log=log)
        assert len(hist) == 2 and len(rollouts) == 2
        ret, length, records = np.zeros(TRAIN_N), np.zeros(TRAIN_N, np.int64), []
        for h, (rew, done) in zip(hist, rollouts):
            for t in range(NSTEPS):
                ret += rew[t].astype(np.float64)
                length += 1
                for e in np.flatnonzero(done[t]):
                    records.append((np.float64(np.float32(ret[e])), int(length[e])))
                    ret[e], length[e] = 0.0, 0
            last = records[-TRAIN_WINDOW:]
            r = np.array([x[0] for x in last])
            bound = 2.0 ** -53 * np.abs(r).sum()
            print("graphs %s: eprewmean %.17g, host %.17g, bound %.3g; eplenmean %.17g" % (graphs, h["eprewmean"], r.sum() / len(last), bound, h["eplenmean"]))
            assert abs(h["eprewmean"] - r.sum() / len(last)) <= bound
            assert abs(h["eplenmean"] - np.mean([x[1] for x in last])) < 1e-12 and h["episodes"] == len(records) >= TRAIN_N
        got[graphs] = hist
        env.close()
    a, b = got[True][0], got[False][0]
    print("first iteration: eprewmean with graphs %.9g, eager %.9g" % (a["eprewmean"], b["eprewmean"]))
    assert (a["episodes"], a["eplenmean"]) == (b["episodes"], b["eplenmean"])
    assert abs(a["eprewmean"] - b["eprewmean"]) <= 2e-3 * abs(b["eprewmean"])


def test_checkpoint_stores_every_specification(tmp_path, model):
    from trex_gym import trex_train
    env = trainer_env(tmp_path, model)
    path = str(tmp_path / "agent.pt")
    agent, hist = trex_train.train(env, 2 * TRAIN_N * NSTEPS, 0, nsteps=NSTEPS, noptepochs=1, save_path=path, log=lambda *_: None, use_graphs=True)
    assert len(hist) == 2
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    for name in ("motion_config", "sensing_config", "randomize_config", "monitor_config"):
        assert getattr(again.env, name) == getattr(env, name) is not None, name
    assert again.critic_config["spec"] == env.critic_spec and again.env.observations == env.observations and again.env.rewards == env.rewards
    assert again.env.obs_dim == env.obs_dim
    env.close(); again.env.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_attach_orders_work_or_are_refused(oracle64, model, sc):
    from trex_gym import monitor, motion as M, sensing as S
    # the monitor before the motion clip or the reward terms: its term columns would be sized without them - refused by name
    env = PC.build_env(oracle64, model, "full", off=("motion",), order=("monitor",))
    with pytest.raises(ValueError, match="monitor"):
        M.attach(env, M.Clip(sc.frames, PC.CLIP_DT), end_effectors=sc.end_effectors)
    with pytest.raises(ValueError, match="monitor"):
        env._set_rewards(sc.rewards)
    monitor.attach(env, None)
    M.attach(env, M.Clip(sc.frames, PC.CLIP_DT), end_effectors=sc.end_effectors)      # the monitor off: the clip attaches
    monitor.attach(env, window=PC.WINDOW)
    assert env.monitor_api.cols == len(sc.reward_terms) + len(sc.motion_terms)
    env.close()
    # sensing before the channels: its groups and its clean block would be the old row's - refused by name
    env = make_vec(N, max_episode_steps=PC.LIMIT, rewards=sc.rewards)
    S.attach(env, S.from_tuples(sc.groups_3j), action_delay=PC.ACTION_DELAY, seed=PC.SENSE_SEED)
    env._external = lambda e: e.commands
    with pytest.raises(ValueError, match="sensing"):
        env._set_observations(sc.channels)
    assert env.obs_dim == 3 * J and env.observations is None
    env.close()
    # the critic before sensing: its clean source is looked up at every fill - the 3-step chain passes
    order = ("motion", "randomize", "monitor", "joint_sensor", "critic", "sensing")
    run_chain(oracle64, model, sc, "full", steps=3, order=order, loose=False)


def test_every_feature_taken_off_again_is_a_plain_env(oracle64, model, sc):
    """test_off_is_off for the whole set at once: after attach(env, None) of every feature the env steps bitwise like an env of
    the same constructor arguments that never had them, from the same state"""
    from trex_gym import critic as C, joint_sensor, monitor, motion as M, randomize as Z, sensing as S
    cleared = PC.build_env(oracle64, model, "full")
    plain = PC.build_env(oracle64, model, "full", order=())
    actions = dev(sc.actions)
    cleared.reset_tensor()
    for t in range(9):                                                               # (an episode limit passes: every per-env state has moved)
        cleared.step_tensor(actions[t])
    C.attach(cleared, None)
    joint_sensor.detach(cleared)
    monitor.attach(cleared, None)
    Z.attach(cleared, None)
    S.attach(cleared, None)
    M.attach(cleared, None)
    for v in (cleared, plain):
        v.commands.zero_()                                                           # (the randomisation's last draw: the caller's again)
        v.reset_tensor()
    assert same_bits(cleared.get_state(), plain.get_state()) and same_bits(cleared.rows, plain.rows)
    ends = falls = 0
    for t in range(9, 19):
        for v in (cleared, plain):
            v.step_tensor(actions[t])
        ends += int(plain.done.sum())
        a, b = everything(cleared), everything(plain)
        assert sorted(a) == sorted(b)
        fell = a["reason"] != 0      # (terminal_obs keeps an env's most recent fall: the cleared env's may date from before the clearing)
        falls += int(fell.sum())
        for k in a:
            assert same_bits(a[k][fell], b[k][fell]) if k == "terminal_obs" else same_bits(a[k], b[k]), (t, k)
    assert ends > 0 and falls > 0                                                    # episodes ended on the way, some by a fall
    for v in (cleared, plain):
        v.close()
