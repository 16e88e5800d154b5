"""The scenario of tests/test_gpu_pipeline.py - the T-rex env with EVERY row feature attached at once - in one place, generated from
seeds and the same on the CPU and the GPU side: the specifications (channels, reward terms, clip, sensing groups, randomisation
terms), the actions, the masked reset, the fall threshold; the run on the f64 oracle that tests/test_pipeline_cases_host.py
qualifies the scenario with (host_run); and the reference chain (chain): one row of the composed env from the per-feature numpy
references, in the launch order of TrexVecEnv.step_tensor - or with one of MISTAKES planted in that order. A helper, not a conftest.

The presets rewards.locomotion / observations.locomotion find the feet with a query on the device; here the same rule
(trex_gym.termination: the bodies within contact_margin of the robot's lowest point in the reset state) is evaluated on the oracle
with tests/termination_ref.py, and the GPU test asserts that the two specifications are equal."""
import types

import numpy as np

from parity_helpers import oracle_wrench

import motion_ref as MR
import observation_ref as OR
import randomize_ref as RND
import reward_ref as RR
import sensing_ref as SR
import termination_ref as TRF

N, STEPS, LIMIT, RESET_AFTER = 33, 30, 7, 16       # envs, steps, episode limit, the masked reset comes after this many steps
J, NB = 25, 26
SENSE_SEED, RAND_SEED, RSI_SEED, ACTION_SEED = 9, 2, 3, 6
ACTION_DELAY, OBS_DELAY = (1, 2), (0, 2)
COMMAND_INTERVAL = 3
PUSH_BODIES = (0, 13)
WINDOW = 256                                       # the monitor's: more than the N * (STEPS // LIMIT + 2) episodes a run can end
# the fall threshold: chosen on the CPU (host_run; tests/test_pipeline_cases_host.py asserts what it gives, with margins)
MAX_TILT = 0.07
CLIP_DT, CLIP_FRAMES = 1.0 / 32.0, 9
VARIANTS = ("full", "no_channels", "two_row_buffers", "penalties_in_rows", "rsi")
MISTAKES = ("reward_gets_delayed_action", "command_before_reward", "monitor_before_motion", "sensing_before_compose",
            "prev_action_gets_delayed_action", "critic_reads_sensed_block")


def limits(model):
    oo = model["obs_order"]
    return np.asarray(model["q_lower"], np.float64)[oo], np.asarray(model["q_upper"], np.float64)[oo]


def actions(model, n=N, steps=STEPS, seed=ACTION_SEED):
    """[steps, n, J] f32: the bounded random actions of test_gpu_sensing.py::test_env_end_to_end - a quarter of the joint range
    around one pose per env -, drawn on the host"""
    lo, hi = limits(model)
    rng = np.random.default_rng(seed)
    mid = lo + (hi - lo) * rng.random((n, J))
    return (mid[None] + 0.25 * (lo + (hi - lo) * rng.random((steps, n, J)) - mid[None])).astype(np.float32)


def reset_mask(n=N):
    return (np.arange(n) % 3 == 0).astype(np.uint8)


def terminate_kwargs():
    return dict(max_tilt=MAX_TILT)


# ---- the feet, by the rule of trex_gym.termination, on the oracle
def reset_state(orc):
    s = orc.new_state()
    orc.reset(s)
    return orc.get_state(s)


def feet(orc, model):
    """(one URDF link per foot, the bodies of the feet's limbs): termination.foot_links / foot_bodies on the oracle's reset state"""
    c = TRF.evaluate(orc, model, reset_state(orc))["clearance"]
    support = [int(b) for b in np.flatnonzero(c < c[np.isfinite(c)].min() + float(orc.params["contact_margin"]))]
    parent = np.asarray(model["parent"], int)
    nb = len(parent)
    kids = [[k for k in range(nb) if parent[k] == b] for b in range(nb)]
    link_body = np.asarray(model["link_body"], int)
    first, limbs = {}, set()
    for b in support:
        top = b
        while parent[top] > 0 and len(kids[top]) < 2:
            top = parent[top]
        first.setdefault(top, b)
        stack = [top]
        while stack:
            x = stack.pop()
            limbs.add(int(x))
            stack += kids[x]
    return [int(np.flatnonzero(link_body == first[top])[0]) for top in sorted(first)], sorted(limbs)


# ---- the specifications
def channel_spec(foot_links):
    """observations.locomotion for these feet, the commands' three columns, the previous action"""
    from trex_gym import observations as O
    spec = O.gravity() + O.base_velocity() + O.base_height()
    for l in foot_links:
        spec += O.contact_force(l) + O.point(l)
    return spec, spec + O.external(3) + O.prev_action()


def reward_spec(model, foot_links, limbs):
    """rewards.locomotion for these feet"""
    from trex_gym import rewards as R
    first_link = {}
    for l, b in enumerate(np.asarray(model["link_body"], int)):
        first_link.setdefault(int(b), l)
    others = [first_link[b] for b in range(model["nb"]) if b not in limbs and b in first_link]
    spec = R.step(0.0) + R.track_lin_vel(1.0, 0.25) + R.track_ang_vel(0.5, 0.25)
    spec += R.lin_vel_z(-2.0) + R.ang_vel_xy(-0.05) + R.orientation(-1.0) + R.torque(-2e-12) + R.joint_acc(-2.5e-7) + R.action_rate(-0.01)
    for l in foot_links:
        spec += R.foot_air_time(1.0, l, threshold=1.0, offset=0.3) + R.foot_slip(-0.1, l, threshold=1.0)
    return spec + R.contact_count(-1.0, others, threshold=1.0)


def resolved_rewards(model, spec):
    """the terms as BatchRewards.set_reward takes them and reward_ref reads them (TrexVecEnv._set_rewards on the oracle's model)"""
    from trex_gym import rewards as R
    names = list(model["obs_joint_names"])
    link_names = list(model["link_names"])
    link_index = lambda l: link_names.index(l) if isinstance(l, str) else int(l)
    joint_index = lambda j: names.index(j) if isinstance(j, str) else int(j)
    return R.resolve(spec, link_index, joint_index, lambda l: int(model["link_body"][l]))[0]


def resolved_channels(spec, action_cols=J):
    from trex_gym import observations as O
    return O.resolve(spec, lambda l: int(l), action_cols)[0]


def clip_frames(model, start):
    """a clip made the way tests/test_gpu_motion.py makes one (offset_clip): it starts AT the reset state and leaves it by 0.02 rad
    per frame on every joint, 1 cm along x and y and 0.05 rad of yaw - the base stays upright, so that RSI starts no env fallen"""
    import motion_cases as MC
    lo, hi = limits(model)
    frames = np.zeros((CLIP_FRAMES, 7 + J))
    sign = np.where(start[13:13 + J] < 0.5 * (lo + hi), 1.0, -1.0)
    for k in range(CLIP_FRAMES):
        frames[k, :3] = start[:3] + [0.01 * k, 0.01 * k, 0.0]
        frames[k, 3:7] = MC.quat_mul(MC.yaw_quat(0.05 * k), start[3:7] / np.linalg.norm(start[3:7]))
        frames[k, 7:] = np.clip(start[13:13 + J] + 0.02 * k * sign, lo, hi)
    return frames


def motion_spec():
    """motion.imitation with end effectors, resolved: (kind, mask, weight, scale, aux)"""
    from trex_gym import motion as M
    return M.resolve(M.imitation(None, end_effectors=True), lambda j: int(j))[0]


def sensing_spec(channels, with_channels=True):
    """sensing.typical(env, delay=OBS_DELAY) and - typical leaves external columns clean - a noisy, late sensor on the three command
    columns: merged groups as tuples. Without channels: the groups of q and qd alone."""
    from trex_gym import observations as O, sensing as S
    env = types.SimpleNamespace(J=J, A=J, observations=O.as_tuples(channels) if with_channels else None)
    spec = S.typical(env, delay=OBS_DELAY)
    if with_channels:
        cmd = S.columns(env, "external")
        spec = spec + S.noise(cmd, std=0.02) + S.latency(cmd, OBS_DELAY)
    return [tuple(g) for g in S.merge(spec)]


def randomize_spec():
    """randomize.typical with its push and the commands resampled every COMMAND_INTERVAL steps, but for the friction: typical's
    0.5 .. 1.25 is two to five times this model's 0.25, and under it the toes that touch the floor are thrown to hundreds of rad/s
    (the f64 oracle shows the same), which the bound of the sensing comparison, set by the largest value, follows - here 0.2 ..
    0.3; and - typical's push comes every 200 steps - a second push, on a heavy body other than typical's (the twin of the GPU
    test adds one force per body), that acts within the run"""
    from trex_gym import randomize as Z
    env = types.SimpleNamespace(rewards=True)
    spec = [t._replace(lo=0.2, hi=0.3) if t.kind == Z.FRICTION else t for t in Z.typical(env, command_interval=COMMAND_INTERVAL)]
    return Z.merge(spec, Z.push(PUSH_BODIES[1], 50.0, 150.0, 4, 2, 1.0))


def scenario(orc, model):
    """everything the two sides share, computed once per (orc, model)"""
    key = id(model)
    if key not in _SCENARIOS:
        links, limbs = feet(orc, model)
        loco, channels = channel_spec(links)
        rewards = reward_spec(model, links, limbs)
        start = reset_state(orc)
        frames = clip_frames(model, start)
        terms = [tuple(t) for t in randomize_spec()]
        _SCENARIOS[key] = types.SimpleNamespace(
            feet=links, limbs=limbs, locomotion=loco, channels=channels, rewards=rewards, reward_terms=resolved_rewards(model, rewards),
            chans=resolved_channels(channels), frames=frames, motion_terms=motion_spec(), end_effectors=[(l, (0.0, 0.0, 0.0)) for l in links],
            tab=MR.device_table(MR.build_table(model, frames, None, CLIP_DT, False)),
            probes=(list(links), np.zeros((len(links), 3))),
            groups=sensing_spec(channels), groups_3j=sensing_spec(channels, False), random_terms=terms,
            actions=actions(model), start=start)
    return _SCENARIOS[key]


_SCENARIOS = {}


# ---- the run on the f64 oracle
def host_run(orc, model, max_tilt=MAX_TILT, steps=STEPS):
    """The scenario's run with the physics of the f64 oracle: the motors get the delayed actions (sensing_ref.ActionDelay on the
    previous done flags), an episode ends at LIMIT steps or when tests/termination_ref.py finds the base tipped by more than
    max_tilt, the masked reset comes after RESET_AFTER steps. The oracle steps the nominal robot: the randomised masses, gains and
    pushes are the device's, which is what the margins of the host test are for. -> a list over reset + steps of dicts: policy /
    applied action, done, reason, cos_tilt of the finished state, the state and row [3J + 2] (obs | reward | done) after the
    auto-reset, the delays drawn and the contact force on every body (the mean over the step's substeps; zeros for an env that was reset)."""
    sc = scenario(orc, model)
    delay = SR.ActionDelay(N, J, ACTION_DELAY[0], ACTION_DELAY[1], SENSE_SEED, 0)
    sims = [orc.new_state() for _ in range(N)]
    obs = np.array([orc.reset(s) for s in sims])
    count = np.zeros(N, int)
    done_prev = np.zeros(N, np.uint8)
    out = [dict(state=np.array([orc.get_state(s) for s in sims]), row=np.concatenate([obs, np.zeros((N, 2))], 1))]
    for t in range(steps):
        masked = None
        if t == RESET_AFTER:
            masked = reset_mask()
            for e in np.flatnonzero(masked):
                obs[e] = orc.reset(sims[e])
            count[masked != 0] = 0
            done_prev[masked != 0] = 0
            delay.reset(masked != 0)
        applied = delay.step(sc.actions[t], done_prev)
        row, done, reason, tilt = np.zeros((N, 3 * J + 2)), np.zeros(N, np.uint8), np.zeros(N, int), np.zeros(N)
        force = np.zeros((N, NB, 3))
        for e in range(N):
            wrench, _ = oracle_wrench(orc, model, None, applied[e], oracle_state=sims[e])      # (one env-step, in place)
            o, r, force[e] = orc.observe(sims[e]), 0.0, wrench[:, :3]
            count[e] += 1
            vals = TRF.values(TRF.evaluate(orc, model, orc.get_state(sims[e])))
            tilt[e] = vals[1]
            if count[e] >= LIMIT:
                done[e] = 1
            elif TRF.reason(vals, max_tilt=max_tilt):
                done[e], reason[e] = 1, TRF.reason(vals, max_tilt=max_tilt)
            if done[e]:
                o = orc.reset(sims[e])
                count[e], force[e] = 0, 0.0
            row[e] = np.concatenate([o, [r, float(done[e])]])
        out.append(dict(action=sc.actions[t], applied=applied, done=done, reason=reason, cos_tilt=tilt, masked=masked, row=row,
                        state=np.array([orc.get_state(s) for s in sims]), action_delay=delay.delay.copy(), force=force))
        done_prev = done
    return out


# ---- the reference chain
class Chain:
    """One composed env of n envs, row by row, from the references of the features - reward terms, motion terms, randomisation,
    monitor, channels, sensor model, critic row - in the launch order of TrexVecEnv.step_tensor (with channels). reset(row, state,
    mask) and step(row, state, action, applied): the step's own row block [n, 3J + 2] and the state behind it (after the resets of
    the step call) come from the caller - the oracle on the CPU -, as does the action the motors got; everything behind the step
    call is computed here. `mistake`: one of MISTAKES, planted in the order. The contact forces are zeros: the run's episodes are
    over before the robot, hung over the floor, lands (the host test asserts that of the oracle's states).
    What a call leaves: reward_terms, motion_terms, reward (the column after each compose), commands, values, monitor (its state),
    clean [n, D + 2], rows (the sensed block, an Applied), critic [n, Dv]."""

    def __init__(self, model, sc, n=N, mistake=None):
        import monitor_ref as MON
        assert mistake is None or mistake in MISTAKES
        self.model, self.sc, self.n, self.mistake = model, sc, n, mistake
        self.Ts = RR.step_seconds()
        T = len(sc.reward_terms)
        self.hists = [RR.new_history(T, J, J) for _ in range(n)]
        self.clocks, self.helds = [MR.new_clock() for _ in range(n)], [np.zeros(len(sc.motion_terms)) for _ in range(n)]
        self.random = RND.Randomizer(n, NB, J, sc.random_terms, RAND_SEED, 0)
        self.monitor = MON.Monitor(n, WINDOW, T + len(sc.motion_terms), 0)
        self.D = 3 * J + OR.extra_dim(sc.chans, J)
        self.sensors = SR.Sensors(n, self.D, 2, sc.groups, SENSE_SEED, 0)
        self.early = SR.Sensors(n, 3 * J, 2, sc.groups_3j, SENSE_SEED, 0)      # (the mistake: sensing on the step's own rows)
        self.prev_reward = self.prev_motion = None
        self.friction = [i for i, t in enumerate(sc.random_terms) if t[0] == RND.FRICTION][0]
        self.foot_bodies = [int(model["link_body"][l]) for l in sc.feet]

    def _compose(self, row, state, action, force):
        n, sc = self.n, self.sc
        force = np.zeros((n, NB, 3)) if force is None else force
        src = row
        if self.mistake == "sensing_before_compose":
            src = self.early.apply(row.astype(np.float32)).out
        clean = np.zeros((n, self.D + 2))
        for e in range(n):
            clean[e] = OR.compose(self.model, state[e], sc.chans, src[e], 2, action=None if action is None else action[e],
                                  extern=self.commands[e], contact_fz=force[e][:, 2])
        self.clean = clean.astype(np.float32)
        if self.mistake == "sensing_before_compose":
            self.rows = types.SimpleNamespace(out=self.clean.astype(np.float64))
            self.early_out = src
        else:
            self.rows = self.sensors.apply(self.clean)
        sensed = self.rows.out[:, :self.D].astype(np.float32)
        source = sensed if self.mistake == "critic_reads_sensed_block" else self.clean[:, :self.D]
        self.critic = np.concatenate([source, self.values[:, self.friction, :1].astype(np.float32),
                                      self.push_force[:, :, :2].reshape(n, -1).astype(np.float32),
                                      force[:, self.foot_bodies].reshape(n, -1).astype(np.float32)], 1)

    def _randomize(self, done):
        r = self.random.apply(done)
        self.values, self.push_force, self.commands = r.values, r.push_force, r.command.astype(np.float32)

    def reset(self, row, state, mask=None, force=None):
        marked = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        for e in np.flatnonzero(marked):
            RR.reset_history(self.hists[e])
            self.clocks[e], self.helds[e][:] = MR.new_clock(), 0.0
        self.random.reset(mask)
        self._randomize(np.zeros(self.n))
        self.sensors.reset(mask)
        self.early.reset(mask)
        self._compose(np.asarray(row, np.float64), state, None, force)
        self.monitor.reset(mask)

    def step(self, row, state, action, applied, force=None):
        n, sc, model = self.n, self.sc, self.model
        force = np.zeros((n, NB, 3)) if force is None else force
        row = np.asarray(row, np.float64).copy()
        done = row[:, 3 * J + 1]
        if self.mistake == "command_before_reward":
            self._randomize(done)
        act = applied if self.mistake == "reward_gets_delayed_action" else action
        terms, bounds = np.zeros((n, len(sc.reward_terms)), np.float32), np.zeros((n, len(sc.reward_terms)))
        for e in range(n):
            v, cases = RR.evaluate(model, sc.reward_terms, state[e], row[e], self.hists[e], self.Ts, action=act[e],
                                   command=self.commands[e], force=force[e])
            for t, (s, case) in enumerate(zip(sc.reward_terms, cases)):
                if case["held"]:
                    terms[e, t] = 0.0 if self.prev_reward is None else self.prev_reward[e, t]
                else:
                    terms[e, t] = np.float32(np.float32(s[4]) * np.float32(v[t]))
                    bounds[e, t] = abs(float(np.float32(s[4]))) * RR.bound(s[0], case)
        self.reward_terms, self.reward_bounds, self.prev_reward = terms, bounds, terms
        column = RR.ordered_sum(terms)
        row[:, 3 * J] = column
        mterms = np.zeros((n, len(sc.motion_terms)), np.float32)
        for e in range(n):
            v, cases = MR.evaluate(model, sc.tab, sc.motion_terms, state[e], row[e], self.clocks[e], self.helds[e], self.Ts, sc.probes)
            for t, (s, case) in enumerate(zip(sc.motion_terms, cases)):
                if case["held"]:
                    mterms[e, t] = 0.0 if self.prev_motion is None else self.prev_motion[e, t]
                else:
                    mterms[e, t] = np.float32(np.float32(s[2]) * np.float32(v[t]))
        self.motion_terms, self.prev_motion = mterms, mterms
        final = MR.ordered_sum(column, mterms)
        row[:, 3 * J] = final
        self.reward = final
        if self.mistake != "command_before_reward":
            self._randomize(done)
        self.monitor.apply(column if self.mistake == "monitor_before_motion" else final, done, None, np.concatenate([terms, mterms], 1))
        shown = applied if self.mistake == "prev_action_gets_delayed_action" else action
        self._compose(row, state, shown, force)


# ---- the env on the device
ORDER = ("motion", "sensing", "randomize", "monitor", "joint_sensor", "critic")     # the order of trex_train.build_environment


def build_env(orc, model, variant="full", off=(), n=N, order=ORDER, limit=LIMIT):
    """The full env of `variant` on the device, the features attached in `order` (observations, rewards and termination are the
    constructor's); off: features left off - of ORDER, or "sensing_groups" (the action delay kept), "action_delay" (the groups kept)."""
    from gpu_support import make_vec
    from trex_gym import critic as C, joint_sensor, monitor, motion as M, randomize as Z, sensing as S
    assert variant in VARIANTS and set(off) <= set(ORDER) | {"sensing_groups", "action_delay", "rsi"}
    sc = scenario(orc, model)
    channels = variant != "no_channels"
    kw = dict(max_episode_steps=limit, terminate=terminate_kwargs(), rewards=sc.rewards)
    if channels:
        kw.update(observations=sc.channels, external=lambda env: env.commands)
    if variant == "two_row_buffers":
        kw["row_buffers"] = 2
    if variant == "penalties_in_rows":
        kw["penalties_in_rows"] = True
    env = make_vec(n, **kw)
    for feature in order:
        if feature in off:
            continue
        if feature == "motion":
            M.attach(env, M.Clip(sc.frames, CLIP_DT), end_effectors=sc.end_effectors, rsi=variant == "rsi" and "rsi" not in off, seed=RSI_SEED)
        elif feature == "sensing":
            groups = [] if "sensing_groups" in off else S.from_tuples(sc.groups if channels else sc.groups_3j)
            S.attach(env, groups, action_delay=0 if "action_delay" in off else ACTION_DELAY, seed=SENSE_SEED)
        elif feature == "randomize":
            Z.attach(env, Z.from_tuples(sc.random_terms), seed=RAND_SEED)
        elif feature == "monitor":
            monitor.attach(env, window=WINDOW, terms=True)
        elif feature == "joint_sensor":
            joint_sensor.attach(env)
        else:
            C.privileged(env, max_width=126)     # (the policy object's limit: the clean row with its channels is 121 wide)
    return env
