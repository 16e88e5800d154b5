"""Batched T-rex env on one MI355X: N independent copies of TrexBulletEnv advanced by one HIP kernel
launch per step (C-ABI: include/trex_batch.h).

Surface = baselines' VecEnv, which is what ppo2.learn drives in the reference (trex_train.py:41-49:
DummyVecEnv([make_env]) -> VecNormalize): num_envs, observation_space, action_space, reset(),
step_async(), step_wait(), step(), close(); plus tensor-native variants that keep everything in HBM
(step_tensor) for an on-device policy.  Episodes never terminate in the reference
(should_terminate() is constant False, trex_env.py:183-184); a time limit, if any, is the
harness's: `max_episode_steps` (None = never) auto-resets like a VecEnv does and reports done=True -
inside the step launch itself (trex_batch_set_episode_limit).

Outputs live in ONE row block `rows` [n, 3J+2] f32 = obs | reward | done (written by the kernel in that layout:
trex_batch_step_rows; with penalties_in_rows [n, 3J+5]: the three penalties behind done); `obs`, `rew`, `done_f` are views
into it; `done` holds the flags as bool, `penalties` [n, 3] the three reward terms. With `observations=` (trex_gym.observations)
the block is [n, 3J + E + 2]: E more observation columns, composed on the device by one more launch per step and reset. With `rewards=` (trex_gym.rewards) the reward column is
composed on the device from a specification of terms, by one more launch per step: `reward_terms` [n, T] holds the breakdown.

Multi-GPU: one process per GPU, env ids sharded by contiguous range (trex_gym.sharding); the only
exchange is the all-gather of that row block (all_gather_rows / all_gather_rows_pipelined).
"""
import collections  # noqa: F401 - no longer used here; one of this module's public names (tests/golden/python_surface.json)
import time

import numpy as np
import torch

from . import _capi, actuators, sharding, spaces
# the read-only queries are vec_queries.VecQueries; their result types stay importable from here
from .vec_queries import AXES, Centroidal, ClosestPoints, IkInfo, LinkProbes, LinkState, ProximityShapes  # noqa: F401
from .vec_queries import VecQueries as _VecQueries

REWARD_DEFAULTS = dict(distance_weight=1.0, energy_weight=0.005, drift_weight=0.002)  # trex_env.py:42-44


class TrexVecEnv(_VecQueries, spaces.Env):   # gym.Env where gym is importable; the surface is baselines' VecEnv
    """This file holds what a step or reset launch depends on: construction, the observation channels, the tensor-native and
    numpy step calls, the gathers, and the setters the step kernels read (gains, domain, wrench, contact sensor, termination).
    The calls that only read the state are inherited from vec_queries.VecQueries."""
    metadata = {"render.modes": ["human", "rgb_array"], "video.frames_per_second": 50}  # trex_env.py:33-36

    def __init__(self, num_envs, urdf_path=None, collisions_dir=None, device=None, action_repeat=1,
                 distance_weight=1.0, energy_weight=0.005, drift_weight=0.002,
                 max_episode_steps=None, starting_configuration=None, params=None,
                 rank=0, world_size=1, process_group=None, collision="hulls", primitive_max_radius=0.2, row_buffers=1,
                 penalties_in_rows=False, pushes=None, control_mode=None, variable_stiffness=False,
                 kp_max=actuators.DEFAULT_KP_MAX, terminate=None, observations=None, external=None, rewards=None):
        """num_envs is the GLOBAL env count; this process owns sharding.shard_range(num_envs, rank, world_size).
        row_buffers=2: successive steps write two row blocks in turn (`rows`, `obs`, `rew`, `done_f` always name the
        block of the LAST step), which lets the pipelined all-gather read a block in place.
        pushes: a trex_gym.perturb.RandomPushes over this process's n envs; step_tensor / step_wait draw its pushes before
        each step launch and apply them, on top of the wrench of set_external_wrench / apply_external_force.
        control_mode: "position" (default), "velocity", "torque", a sequence of J of them or {joint_name: mode} - what a joint's
        action means (include/trex_batch.h; pybullet's setJointMotorControlArray modes). variable_stiffness: actions are [2J],
        J commands then J stiffnesses kp in [0, kp_max] (the reference's intended action space, trex_env.py:30).
        terminate: dict(head_height=, max_tilt=, keep_clear=, penalty=) - the arguments of set_termination(): episodes end
        when the robot falls, decided inside the step calls.
        observations: a list of trex_gym.observations channels (e.g. observations.locomotion(model)): E extra observation columns
        behind the 3J, computed on the device from the state of the row's own instant by one more launch per step and reset
        (trex_batch_compose_rows). `rows` is then [n, 3J + E + 2 (or 5)] = obs | reward | done, `obs` its first D' = 3J + E
        columns, and observation_space is D' wide. None (default): nothing changes - not a launch, not a byte.
        external: with observations.external(k) channels, their columns: a tensor [n, X] read at every compose, or a callable
        env -> such a tensor, called after every step and reset.
        rewards: a list of trex_gym.rewards terms (e.g. rewards.locomotion(model)): the reward column becomes the sum of weight *
        value over the terms, evaluated on the device at the row's own instant by one more launch per step
        (trex_batch_compose_reward) that runs after the step and before the channels are composed. `commands` [n, 3] (vx, vy in
        base axes, yaw rate; zeros) is a device tensor to write in place, `reward_terms` [n, T] the weighted value of every term
        at the last step (a tensor the caller may replace by another [n, T] block, e.g. a slice of a rollout buffer), `reward_names` their names, `reward_api` the batch's calls (reward_capi.BatchRewards). The commands join the observations through
        observations.external(3) with external=lambda env: env.commands. None (default): nothing changes - not a launch, not a byte.
        A motion clip with its tracking terms is attached to a constructed env by trex_gym.motion.attach(env, clip, ...), a sensor
        model - noise, bias, resolution and latency on what the policy reads, latency on its actions - by
        trex_gym.sensing.attach(env, spec, ...), episode randomisation - mass scale, friction, motor gains, pushes and commands
        redrawn on the device - by trex_gym.randomize.attach(env, spec, ...), start-state randomisation - the state an episode
        starts in, perturbed on the device and placed on the floor - by trex_gym.start_state.attach(env, spec, ...)."""
        self.global_num_envs = int(num_envs)
        self.rank, self.world_size, self.process_group = int(rank), int(world_size), process_group
        self.env_lo, self.env_hi = sharding.shard_range(self.global_num_envs, self.rank, self.world_size)
        self.num_envs = self.env_hi - self.env_lo
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _capi.TrexError(-5, "TrexVecEnv needs a HIP device; the physics step has no CPU fallback")
        if self.device.index is None:   # "cuda" without an index means the CURRENT device, for batch and buffers alike
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.model = _capi.Model(urdf_path, collisions_dir)
        # NUM_SUBSTEPS = 5 physics substeps per action repeat (trex_env.py:18,71-73)
        self.model.set_param("substeps", 5 * int(action_repeat))
        for k, v in (params or {}).items():
            self.model.set_param(k, v)
        if collision == "primitives":   # capsules / spheres fitted to the hulls
            self.model.use_primitive_collision(primitive_max_radius)
        elif collision != "hulls":
            raise ValueError("collision must be 'hulls' or 'primitives'")
        for name, angle in (starting_configuration or {}).items():
            self.model.set_start_angle(name, angle)  # unknown name raises, like KeyError at trex_robot.py:307
        self.batch = _capi.Batch(self.model, self.num_envs, self.device.index)
        self.batch.set_reward_weights(distance_weight, energy_weight, drift_weight)
        J = self.J = self.model.num_joints
        lo, hi = self.model.lower.astype(np.float32), self.model.upper.astype(np.float32)
        self.control_modes = actuators.resolve_control_modes(control_mode, self.model.joint_names)
        self.variable_stiffness, self.kp_max = bool(variable_stiffness), float(kp_max)
        if any(self.control_modes):
            self.batch.set_control_mode(self.control_modes)
        if self.variable_stiffness:
            self.batch.set_stiffness_actions(True, self.kp_max)
        alo, ahi = actuators.action_bounds(self.control_modes, lo, hi, self.model.get_param("max_coordinate_velocity"),
                                           self.model.get_param("motor_max_force"), self.variable_stiffness, self.kp_max)
        self.action_space = spaces.Box(low=alo, high=ahi, dtype=np.float32)  # trex_robot.py:424-433 for position control
        big = np.full(2 * J, 1.0e12, np.float32)                            # trex_robot.py:348-357
        self.observation_space = spaces.Box(low=np.concatenate([lo, -big]), high=np.concatenate([hi, big]),
                                            dtype=np.float32)
        n = self.num_envs
        # obs | reward | done. row_buffers=2: the steps write two blocks in turn, so that a block can be gathered in
        # place while the next step runs (all_gather_rows_pipelined without a staging copy)
        # penalties_in_rows: [n, 3J+5] rows that carry the three penalties behind done (one message for a consumer that
        # wants them); default [n, 3J+2] + a `penalties` tensor of its own. (The 80-column form was MEASURED to cost
        # more HBM write traffic, not less - 8.1 against 3.7 MB per launch of 4096 envs, PMC WRITE_SIZE: DESIGN.md 6.)
        self._pen_in_rows = bool(penalties_in_rows)
        self.batch.set_penalties_in_rows(self._pen_in_rows)      # (explicit: a wide row stride alone writes nothing beyond column 3J + 1)
        self._row_blocks = [torch.zeros(n, 3 * J + (5 if self._pen_in_rows else 2), device=self.device) for _ in range(int(row_buffers))]
        self._penalties = None if self._pen_in_rows else torch.zeros(n, 3, device=self.device)
        # observation channels: the step keeps writing a [n, 3J + tail] block of its own (_step_rows); the composed rows are the
        # env's row blocks, so that everything that reads `rows` - the trainer in place, the gathers - reads the extended row
        self.observations, self.obs_dim, self._step_rows, self._external = None, 3 * J, None, external
        self.rewards, self.reward_names, self.reward_terms, self.reward_api = None, [], None, None
        self.commands = None                    # [n, 3] with rewards: made by _set_rewards
        self._rew_actions = False
        self.motion, self.motion_api, self.motion_terms, self.motion_names = None, None, None, []
        self._rsi = False
        self.sensing, self.sense_api, self.clean_rows, self.clean_obs = None, None, None, None
        self._clean_block, self._delayed_actions = None, None
        self.randomization, self.random_api, self.random_values = None, None, None
        self._no_done = None
        self.start_state, self.start_api, self.start_values, self._start_no_done = None, None, None, None
        self.monitor, self.monitor_api = None, None
        # the privileged critic row (trex_gym.critic.attach): [n, Dv], its column names, the recorded sources, and the call that
        # refills it behind every step and reset
        self.critic_rows, self.critic_names, self.critic_spec, self._critic_fill = None, [], None, None
        # the joint force/torque sensor (trex_gym.joint_sensor.attach): the batch's calls, the readings [n, J, 6] and [n, 6], and the
        # call that refreshes them behind every step and reset
        self.joint_api, self.joint_reaction, self.joint_base_residual, self._joint_fill = None, None, None, None
        self.collision = collision
        self._init_queries()                    # the link table and the caches of the read-only queries (vec_queries.py)
        if observations is not None and len(observations):
            self._set_observations(observations)
        elif external is not None:
            raise ValueError("external: there is no observations.external(k) channel to take it")
        if rewards is not None and len(rewards):
            self._set_rewards(rewards)
        self._row_k = 0
        self._point_at(0)
        self.done = torch.zeros(n, dtype=torch.bool, device=self.device)   # the same flags as bytes (written by the kernel too)
        self.max_episode_steps = max_episode_steps
        if max_episode_steps is not None:
            # the step launch itself resets an env whose episode is over (no reset launch between two steps)
            self.batch.set_episode_limit(int(max_episode_steps))
        self.gains = None                       # a trex_gym.perturb.RandomGains: redrawn at every reset() / reset_tensor()
        self._actions = None
        self._gather_buf = None
        self._pipe = None
        self._copy_pipe = None
        self._ep_ret = self._ep_len = None      # episode statistics of the numpy API (step_wait)
        self._wrench = None                     # the caller's external wrench [n, num_bodies, 6] (None: none)
        self.pushes = pushes
        if pushes is not None and pushes.num_envs != n:
            raise ValueError("pushes: RandomPushes over %d envs, the env has %d" % (pushes.num_envs, n))
        self._term_on, self._term_buf = False, None   # fall termination: on?, (reason, values, terminal_obs) buffers of the env
        if terminate:
            self.set_termination(**terminate)

    # ---- episode randomisation (trex_batch_set_randomization and its kin, include/trex_randomize.h; trex_gym.randomize builds
    # specifications)
    def _set_randomization(self, spec, seed=0):
        """What trex_gym.randomize.attach(env, ...) does (the constructor's signature is a recorded one): the terms of `spec`
        (trex_gym.randomize; merged, link names of push terms resolved to bodies) go to the batch, and one more launch per step
        (trex_batch_apply_randomization) - behind the step call, the reward compose and the motion step, before the channels'
        compose - redraws them for the envs whose done column is set: the finished step is rewarded against the old command, the
        first row of the new episode shows the new one. reset_tensor marks the envs it resets and applies at the same place.
        `random_api` is the batch's calls (randomize_capi.BatchRandomization), `random_values` a [n, T, 32] tensor for its info(),
        `randomization` the recorded specification: dict(terms=, seed=). Command terms write `commands` (made here where the env has
        none). The Philox key is `seed`, the env offset `env_lo`. ValueError while the env has `pushes` or `gains`: one owner per
        buffer. spec None clears the batch's terms - gains, wrench, mass scale and friction go back - and takes all of this off
        the env again. Never called, or cleared: nothing changes - not a launch, not a byte."""
        from . import randomize as R, randomize_capi
        if spec is None:
            if self.random_api is not None:
                self.random_api.set(())
            self.randomization, self.random_api, self.random_values, self._no_done = None, None, None, None
            return
        if self.pushes is not None or self.gains is not None:
            raise ValueError("randomisation: the env has pushes or gains of trex_gym.perturb - one owner per buffer")
        terms = []
        for t in R.merge(spec):
            if isinstance(t.index, str):
                t = t._replace(index=int(self._links.link_body[self._links.index(t.index)]))
            terms.append(t)
        api = randomize_capi.BatchRandomization(self.batch)
        api.set([tuple(t) for t in terms], seed, self.env_lo)
        self.random_api = api
        self.randomization = dict(terms=R.as_tuples(terms), seed=int(seed))
        self.random_values = torch.zeros(self.num_envs, max(len(terms), 1), randomize_capi.ELEMENTS, device=self.device)
        self._no_done = torch.zeros(self.num_envs, device=self.device)      # what a reset applies with: only the marked envs start
        if self.commands is None and any(t.kind == randomize_capi.COMMAND for t in terms):
            self.commands = torch.zeros(self.num_envs, 3, device=self.device)

    # ---- start-state randomisation (trex_batch_set_start_state and its kin, include/trex_start_state.h; trex_gym.start_state builds
    # specifications)
    def _set_start_state(self, spec, seed=0):
        """What trex_gym.start_state.attach(env, ...) does (the constructor's signature is a recorded one): the terms of `spec`
        (trex_gym.start_state; merged, joint names resolved to observation slots) go to the batch, and one more launch per step
        (trex_batch_apply_start_state) - behind the step call, the reward compose, the motion step and RSI, before the
        randomisation - perturbs the state of the envs whose done column is set and patches the first 3J columns of their rows:
        noise lands on the RSI state, and the monitor, the joint sensor, the channels, the sensor model and the critic's row all
        see the final state. reset_tensor marks the envs it resets and applies at the same place. `start_api` is the batch's
        calls (start_state_capi.BatchStartState), `start_values` a [n, T, 32] tensor for its info(), `start_state` the recorded
        specification: dict(terms=, seed=). The Philox key is `seed`, the env offset `env_lo`. Nothing here is sized by the row
        or by another feature: it attaches in any order with the others. spec None clears the batch's terms and takes all of
        this off the env again. Never called, or cleared: nothing changes - not a launch, not a byte."""
        from . import start_state as S, start_state_capi
        if spec is None:
            if self.start_api is not None:
                self.start_api.set(())
            self.start_state, self.start_api, self.start_values, self._start_no_done = None, None, None, None
            return
        names = list(self.model.joint_names)
        terms = S.resolve(spec, names.index)
        if not terms:
            raise ValueError("start state: an empty specification (None takes the feature off)")
        api = start_state_capi.BatchStartState(self.batch)
        api.set([tuple(t) for t in terms], seed, self.env_lo)
        self.start_api = api
        self.start_state = dict(terms=S.as_tuples(terms), seed=int(seed))
        self.start_values = torch.zeros(self.num_envs, len(terms), start_state_capi.ELEMENTS, device=self.device)
        self._start_no_done = torch.zeros(self.num_envs, device=self.device)  # what a reset applies with: only the marked envs start

    # ---- episode monitor (trex_batch_set_monitor and its kin, include/trex_monitor.h; trex_gym.monitor reads it)
    def _set_monitor(self, window=100, terms=True):
        """What trex_gym.monitor.attach(env, ...) does (the constructor's signature is a recorded one): the batch keeps every
        episode's return, length, end reason and - with terms - the per-episode sums of the env's `reward_terms` and `motion_terms`
        blocks, and a window of the last `window` finished episodes. Two more launches per step (trex_batch_monitor_apply) behind
        the step call, the reward compose and the motion step read the step's own rows - columns 3J and 3J + 1 - and the two
        blocks as they are at that call: the trainer points them at its rollout buffers, so they are arguments, not settings.
        reset_tensor(mask) abandons the running episode of the envs it resets. `monitor_api` is the batch's calls
        (monitor_capi.BatchMonitor), `monitor` the recorded settings: dict(window=, terms=). The env offset is `env_lo`. The term
        columns are sized here, from the blocks the env has: attach the monitor BEHIND rewards and motion - attaching either behind
        a monitor with terms is a ValueError (take the monitor off first). window None or 0 clears the batch's monitor and takes all of this off the env again. Never called, or cleared: nothing changes -
        not a launch, not a byte."""
        from . import monitor_capi
        if not window:
            if self.monitor_api is not None:
                self.monitor_api.set(0)
            self.monitor, self.monitor_api = None, None
            return
        cols_a = int(self.reward_terms.shape[1]) if terms and self.reward_terms is not None else 0
        cols_b = int(self.motion_terms.shape[1]) if terms and self.motion_terms is not None else 0
        api = monitor_capi.BatchMonitor(self.batch)
        api.set(int(window), cols_a, cols_b, self.env_lo)
        self.monitor_api = api
        self.monitor = dict(window=int(window), terms=bool(terms))

    # ---- observation channels (trex_batch_set_observation / trex_batch_compose_rows; trex_gym.observations builds specifications)
    def _set_observations(self, spec):
        """The channels are the constructor's (observations=). ValueError behind trex_gym.sensing.attach: the groups and the clean
        block of a sensor model are sized for the row it found - attach sensing after the row has its final width."""
        from . import observations as O
        if self.sense_api is not None:
            raise ValueError("observations: the env has a sensor model (trex_gym.sensing.attach), set for the row as it was - attach sensing behind the channels")
        J, n = self.J, self.num_envs
        chans, extra, contact, ext_cols = O.resolve(spec, self._links.index, self.A)
        if len(chans) > O.MAX_CHANNELS or 3 * J + extra > O.MAX_DIM:
            raise ValueError("observations: %d channels and %d columns; at most %d channels and %d columns"
                             % (len(chans), 3 * J + extra, O.MAX_CHANNELS, O.MAX_DIM))
        if (ext_cols > 0) != (self._external is not None):
            raise ValueError("observations: external(k) channels and the external= argument go together")
        if contact:
            self.batch.set_contact_sensor(True)
        added = self.batch.set_observation(chans)
        assert added == extra, (added, extra)
        self.observations = O.as_tuples(spec)
        self.obs_dim = self.batch.observation_dim()
        tail = 5 if self._pen_in_rows else 2
        self._step_rows = self._row_blocks[0]
        self._row_blocks = [torch.zeros(n, self.obs_dim + tail, device=self.device) for _ in self._row_blocks]
        big = np.full(extra, 1.0e12, np.float32)      # the bounds of the velocity columns
        sp = self.observation_space
        self.observation_space = spaces.Box(low=np.concatenate([sp.low, -big]), high=np.concatenate([sp.high, big]), dtype=np.float32)

    def _compose(self, actions, out=None):
        ext = self._external(self) if callable(self._external) else self._external
        self.batch.compose_rows(self._step_rows, self.rows if out is None else out, actions, None if ext is None else self._dev(ext))

    # ---- reward terms (trex_batch_set_reward / trex_batch_compose_reward; trex_gym.rewards builds specifications)
    def _set_rewards(self, spec):
        """The reward terms are the constructor's (rewards=). ValueError behind a monitor that sums terms: see _set_monitor."""
        from . import reward_capi, rewards as R
        self._refuse_late_terms("rewards")
        L = self._links
        names = list(self.model.joint_names)
        terms, contact, _, self._rew_actions = R.resolve(spec, L.index, lambda j: names.index(j) if isinstance(j, str) else int(j),
                                                         lambda l: int(L.link_body[l]))
        if contact:
            self.batch.set_contact_sensor(True)
        self.reward_api = reward_capi.BatchRewards(self.batch)    # (trex_batch_set_reward and its kin: include/trex_reward.h)
        self.reward_api.set_reward(terms)
        self.rewards, self.reward_names = R.as_tuples(spec), R.names(spec)
        self.reward_terms = torch.zeros(self.num_envs, len(terms), device=self.device)
        self.commands = torch.zeros(self.num_envs, 3, device=self.device)

    def _refuse_late_terms(self, what):
        if self.monitor is not None and self.monitor["terms"]:
            raise ValueError("%s: the env has a monitor (trex_gym.monitor.attach) whose term columns were sized without them - "
                             "attach the monitor behind rewards and motion" % what)

    def _compose_reward(self, rows, actions):
        self.reward_api.compose_reward(rows, actions if self._rew_actions else None, self.commands, self.reward_terms)

    # ---- motion clip (trex_batch_set_motion and its kin, include/trex_motion.h; trex_gym.motion builds clips and specifications)
    def _set_motion(self, clip, terms=None, end_effectors=(), rsi=False, step_weight=1.0, probe_set=7, seed=0):
        """What trex_gym.motion.attach(env, ...) does (the constructor's signature is a recorded one and takes no `motion`):
        clip - a trex_gym.motion.Clip or the path of a saved one - goes to the device, and the tracking terms against it
        (trex_gym.motion; default motion.imitation) are added to the reward column by one more launch per step
        (trex_batch_compose_motion_reward) behind the rewards' compose: reward = step_weight * the column found + the weighted
        terms. end_effectors: [(link name or index, xyz in the link frame)], at most 8, kept as link-probe set probe_set.
        rsi: an env whose episode ends starts the next one at an instant of the clip drawn uniformly in [0, T) by a generator
        of the env's own seeded with `seed` - one more launch per step (trex_batch_motion_reset), before the channels are
        composed. `motion` then is the Clip, `motion_api` the batch's calls (motion_capi.BatchMotion), `motion_terms` [n, T] the
        weighted value of every term at the last step, `motion_names` their names. ValueError behind a monitor that sums terms
        (_set_monitor). clip None clears the batch's clip and takes all of this off the env again. Never called, or cleared: nothing changes - not a launch, not a byte."""
        from . import motion as M, motion_capi
        if clip is None:
            if self.motion_api is not None:
                self.motion_api.set_motion(None)
            self.motion, self.motion_api, self.motion_terms, self.motion_names, self._rsi = None, None, None, [], False
            return
        self._refuse_late_terms("motion")
        if isinstance(clip, str):
            clip = M.Clip.load(clip)
        if clip.num_joints != self.J:
            raise ValueError("motion: the clip has %d joints, the model %d" % (clip.num_joints, self.J))
        end_effectors = list(end_effectors or ())
        if len(end_effectors) > M.MAX_END_EFFECTORS:
            raise ValueError("motion: %d end effectors, at most %d" % (len(end_effectors), M.MAX_END_EFFECTORS))
        if end_effectors:
            self.batch.set_link_probes(int(probe_set), [self._links.index(l) for l, _ in end_effectors], [xyz for _, xyz in end_effectors])
        spec = M.imitation(self.model, end_effectors=bool(end_effectors)) if terms is None else M.flatten(terms)
        names = list(self.model.joint_names)
        resolved, effectors = M.resolve(spec, lambda j: names.index(j) if isinstance(j, str) else int(j))
        if effectors and not end_effectors:
            raise ValueError("motion: an end_effector term and no end_effectors")
        self.motion_api = motion_capi.BatchMotion(self.batch)
        self.motion_api.set_motion(clip.frames, clip.frame_dt, clip.loop, clip.velocities, int(probe_set) if end_effectors else -1)
        self.motion_api.set_reward(resolved, step_weight)
        self.motion, self.motion_names = clip, M.names(spec)
        self.motion_terms = torch.zeros(self.num_envs, len(resolved), device=self.device)
        self._motion_spec = M.as_tuples(spec)
        self._rsi = bool(rsi)
        self._rsi_gen = torch.Generator(device=self.device).manual_seed(int(seed))
        self._rsi_time = torch.zeros(self.num_envs, device=self.device)   # the instants the envs drew last
        self._rsi_span = self.motion_api.info()["duration"]

    def _motion_step(self, rows):
        """behind the step call and the rewards' compose: the tracking terms into the reward column; with rsi, the envs whose
        episode ended start at an instant of the clip"""
        if self.motion_terms.shape[1]:
            self.motion_api.compose_reward(rows, self.motion_terms)
        if self._rsi:
            self._motion_rsi(rows, self.done)

    def _motion_rsi(self, rows, mask):
        self._rsi_time.uniform_(0.0, self._rsi_span, generator=self._rsi_gen)
        self.motion_api.reset(mask, self._rsi_time, rows)

    # ---- sensor model (trex_batch_set_sensing and its kin, include/trex_sensing.h; trex_gym.sensing builds specifications)
    def _set_sensing(self, spec, action_delay=0, seed=0):
        """What trex_gym.sensing.attach(env, ...) does (the constructor's signature is a recorded one and takes no `sensing`):
        the groups of `spec` (trex_gym.sensing; merged) go to the batch, and every row the env composes passes through them by
        one more launch per step and reset (trex_batch_apply_sensing) behind the last compose: the env composes into a block of
        its own, `clean_rows` (`clean_obs` its observation columns), and `rows` / `obs` - what the policy, the trainer and the
        gathers read - hold the sensors' view. action_delay - steps or (min, max) - delays the actions by one more launch before
        the step call (trex_batch_delay_actions); the reward terms and the prev_action channel keep reading the policy's own
        action. `sense_api` is the batch's calls (sensing_capi.BatchSensing), `sensing` the recorded specification:
        dict(groups=, action_delay=, seed=). The Philox key is `seed`, the env offset `env_lo`. An empty spec sets only the action
        delay (`clean_rows` is `rows` then). spec None clears the batch's groups and delay and takes all of this off the env
        again. Never called, or cleared: nothing changes - not a launch, not a byte."""
        from . import sensing as S, sensing_capi
        if spec is None:
            if self.sense_api is not None:
                self.sense_api.set_sensing(())
                self.sense_api.set_action_delay(0, 0)
            self.sensing, self.sense_api, self.clean_rows, self.clean_obs = None, None, None, None
            self._clean_block, self._delayed_actions = None, None
            return
        groups = S.merge(spec)
        lo, hi = S.delay_range(action_delay)
        api = sensing_capi.BatchSensing(self.batch)
        api.set_sensing([tuple(g) for g in groups], seed, self.env_lo)
        api.set_action_delay(lo, hi)
        self.sense_api = api
        self.sensing = dict(groups=S.as_tuples(groups), action_delay=[lo, hi], seed=int(seed))
        self._clean_block = torch.zeros_like(self.rows) if groups else None
        self._delayed_actions = torch.zeros(self.num_envs, self.A, device=self.device) if hi > 0 else None
        if self._clean_block is not None:
            self._clean_block.copy_(self.rows)
        self._point_at(self._row_k)

    def _dev(self, t, dtype=torch.float32):
        """t as a contiguous `dtype` tensor on the env's device: t ITSELF where it is one already - no copy, no launch."""
        if t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
            t = t.to(device=self.device, dtype=dtype).contiguous()
        return t

    # ---- tensor-native API (stays on device, stream-ordered, no host sync)
    def reset_tensor(self, mask=None):
        """Reset all envs (mask=None) or those with mask != 0 (uint8 or bool [n], e.g. the `done` of the last step).
        Returns obs [n, 3J]; the reward / done columns and `done` of the envs that were reset read 0 afterwards.
        With observations: obs [n, 3J + E], every env's channels recomposed at the current state, prev_action() columns zero."""
        out = self.rows if self._clean_block is None else self._clean_block      # (with sensing: the clean block)
        rows = out if self._step_rows is None else self._step_rows
        if self.motion is not None and not self._rsi:     # clocks and held values of the envs to 0 (the state it writes is replaced next)
            self.motion_api.reset(mask)
        self.batch.reset_rows(rows, mask)
        if self._rsi:
            self._motion_rsi(rows, mask)
        if self.start_api is not None:          # the envs that were reset start from a perturbed state: on the reset's or RSI's, before all that reads it
            self.start_api.reset(mask)
            self.start_api.apply(self._start_no_done, rows)
        if self.random_api is not None:         # the envs that were reset start an episode: their draws, before the compose shows them
            self.random_api.reset(mask)
            self.random_api.apply(self._no_done, self.commands)
        if self._joint_fill is not None:        # the joint sensor at the state the reset left: before the compose and the critic's row, which may read it
            self._joint_fill(None)
        if self._step_rows is not None:
            self._compose(None, out)
        if self._clean_block is not None or self._delayed_actions is not None:   # the envs that were reset start an episode of their sensors and of their action history
            self.sense_api.reset(mask)
            if self._clean_block is not None:   # the sensors' view of the clean block into the block the policy reads
                self.sense_api.apply(out, self.rows)
        if self._critic_fill is not None:       # behind the sensing launch: the critic's row of the reset state
            self._critic_fill()
        if self.rewards is not None:            # the envs that were reset have no previous step: their reward history starts afresh
            self.reward_api.reward_reset(mask)
        if self.gains is not None:              # the envs that were reset draw new motor gains
            self.set_motor_gains(**self.gains.draw(mask))
        if self.monitor_api is not None:        # the running episode of the envs that were reset is abandoned, not recorded
            self.monitor_api.reset(mask)
        if mask is None:
            self.done.zero_()
        else:
            self.done.logical_and_(mask == 0)     # (also correct for mask is self.done)
        return self.obs

    @property
    def episode_steps(self):
        """[n] int32: env-steps since each env's last reset (kept by the batch when an episode limit is set)."""
        out = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.batch.get_episode_steps(out)
        return out

    def set_episode_steps(self, steps):
        """Set the per-env step counts (e.g. to stagger the episodes of a benchmark)."""
        self.batch.set_episode_limit(int(self.max_episode_steps or 0), self._dev(steps, torch.int32))

    def step_tensor(self, actions):
        """actions [n, J] f32 on device -> (obs [n,3J], reward [n], done [n] bool). Views into buffers
        that the next call overwrites.

        The launch order, each launch only where its feature is attached (tests/test_gpu_pipeline.py pins it; the same with and
        without channels, where the step's block is the clean block itself): (1) the action delay - the motors get the action of
        some steps ago, `done` still holding the flags of the step before; (2) the step call on the delayed action: step, fall
        predicate, reset of the envs that fell or reached the limit - done = 1, the reward of the finished step, the observation
        of the new episode, the last one of a fallen env in terminal_obs, which no later launch touches; (3) the reward terms,
        on the POLICY's action and the commands as they are, into the reward column; (4) the motion terms added to that column,
        then RSI, which writes the state of the envs whose episode ended; (4b) the start-state terms, which perturb the state of
        those envs as the reset or RSI left it, place it on the floor and patch the first 3J columns of their rows; (5) the
        randomisation, which redraws for those envs -
        commands included: the finished step was rewarded against the old command, the row of the new episode shows the new one;
        (6) the monitor, on the reward column as (3) and (4) left it, the done column and the two term blocks; (7) the joint
        sensor, at the state (4) and (4b) left; (8) the channels' compose into the clean block, with the policy's action for prev_action
        and the commands of (5); (9) the sensor model, from the clean block - channel and command columns included - into `rows`;
        (10) the critic's row, whose clean source is the clean block. reset_tensor runs (4)'s reset, (4b), (5), (7) - (10) in that order,
        then starts the reward history and the monitor's episode of the envs it reset afresh."""
        actions = self._dev(actions)
        if tuple(actions.shape) != (self.num_envs, self.A):
            raise ValueError("actions must have shape (%d, %d), got %s" % (self.num_envs, self.A, tuple(actions.shape)))
        # (with max_episode_steps the launch also resets the envs whose episode ends with this step: done = 1,
        # reward of the finished step, observation of the new episode - VecEnv semantics, no second launch)
        if self.random_api is not None and (self.pushes is not None or self.gains is not None):
            raise ValueError("randomisation: the env has pushes or gains of trex_gym.perturb - one owner per buffer")
        if self.pushes is not None:   # this step's pushes (those of envs that ended their episode last step are dropped)
            w = self.pushes.wrench(self.model.num_bodies, self.done).to(self.device)
            self.batch.set_external_wrench(w if self._wrench is None else w + self._wrench)
        if len(self._row_blocks) > 1:
            self._point_at(1 - self._row_k)
        # (with set_termination the call is three launches: step, fall predicate, reset of the fallen - done = 1, the reward of
        # the finished step less the penalty, observation of the new episode)
        applied = actions
        if self._delayed_actions is not None:
            self.sense_api.delay_actions(actions, self._delayed_actions, self.done)
            applied = self._delayed_actions
        out = self.rows if self._clean_block is None else self._clean_block
        if self._step_rows is None:
            self.batch.step_rows(applied, out, self._penalties, done=self.done)   # (None: the penalties ride in the row block)
            if self.rewards is not None:
                self._compose_reward(out, actions)
            if self.motion is not None:
                self._motion_step(out)
            if self.start_api is not None:
                self.start_api.apply(out, out, 3 * self.J + 1)
            if self.random_api is not None:
                self.random_api.apply(out, self.commands, 3 * self.J + 1)
            if self.monitor_api is not None:
                self.monitor_api.apply(out, out, None, self.reward_terms, self.motion_terms, 3 * self.J, 3 * self.J + 1)
            if self._joint_fill is not None:
                self._joint_fill(out)
        else:   # (observation channels: the step keeps a block of its own, and (8) composes the env's)
            self.batch.step_rows(applied, self._step_rows, self._penalties, done=self.done)
            if self.rewards is not None:
                self._compose_reward(self._step_rows, actions)
            if self.motion is not None:
                self._motion_step(self._step_rows)
            if self.start_api is not None:
                self.start_api.apply(self._step_rows, self._step_rows, 3 * self.J + 1)
            if self.random_api is not None:
                self.random_api.apply(self._step_rows, self.commands, 3 * self.J + 1)
            if self.monitor_api is not None:
                self.monitor_api.apply(self._step_rows, self._step_rows, None, self.reward_terms, self.motion_terms, 3 * self.J, 3 * self.J + 1)
            if self._joint_fill is not None:
                self._joint_fill(self._step_rows)
            self._compose(actions, out)
        if self._clean_block is not None:
            self.sense_api.apply(out, self.rows)
        if self._critic_fill is not None:
            self._critic_fill()
        if self._term_on and self.gains is not None:   # the envs that fell start their episode with new motor gains
            self.set_motor_gains(**self.gains.draw(self.termination_reason != 0))
        return self.obs, self.rew, self.done

    def step_many_tensor(self, actions, rows=None):
        """Open-loop rollout: actions [S, n, J] f32 on device -> rows [S, n, 3J+2] (obs | reward | done of every step), S
        env-steps in ONE launch (trex_batch_step_many; bitwise S calls of step_tensor). `rows`, `obs`, `rew`, `done_f`
        and `done` then hold the last step. sharding.split_rows(rows[s]) cuts a step's block into the three.
        ValueError with observations, rewards, motion, sensing, randomisation, start-state terms or the joint sensor: an open-loop launch has no compose between its steps.
        With a monitor attached its applies follow the launch, one per step block (not together with fall termination)."""
        if self.random_api is not None:
            raise ValueError("step_many_tensor: not with randomisation - the open-loop launch has no per-step launch of the redraws")
        if self.start_api is not None:
            raise ValueError("step_many_tensor: not with start-state terms - the open-loop launch has no per-step launch of the perturbation")
        if self.monitor_api is not None and self._term_on:
            raise ValueError("step_many_tensor: not with a monitor and fall termination - the batch keeps the last step's reasons only")
        if self._joint_fill is not None:
            raise ValueError("step_many_tensor: not with the joint sensor - the open-loop launch has no per-step launch of its query")
        if self.sense_api is not None:
            raise ValueError("step_many_tensor: not with sensing - the open-loop launch has no per-step launch of the sensor model")
        if self.motion is not None:
            raise ValueError("step_many_tensor: not with motion - the open-loop launch has no per-step compose of the tracking terms")
        if self.rewards is not None:
            raise ValueError("step_many_tensor: not with rewards - the open-loop launch has no per-step compose of the reward terms")
        if self._step_rows is not None:
            raise ValueError("step_many_tensor: not with observations - the open-loop launch has no per-step compose of the channels")
        actions = self._dev(actions)
        if actions.dim() != 3 or tuple(actions.shape[1:]) != (self.num_envs, self.A):
            raise ValueError("actions must have shape (S, %d, %d), got %s" % (self.num_envs, self.A, tuple(actions.shape)))
        S = int(actions.shape[0])
        if rows is None:
            rows = torch.empty(S, self.num_envs, self.rows.shape[1], device=self.device)
        # (the three reward terms of every step: in the rows when penalties_in_rows, else in `penalties_many` [S, n, 3]; `penalties`
        # then holds the last step's, like the other views - it used to keep the values from BEFORE the call)
        self.penalties_many = None if self._pen_in_rows else torch.empty(S, self.num_envs, 3, device=self.device)
        self.batch.step_many(actions, rows, self.penalties_many)
        if self.monitor_api is not None:        # once per step block, behind the launch: the monitor needs nothing between the steps
            for s in range(S):
                self.monitor_api.apply(rows[s], rows[s], None, None, None, 3 * self.J, 3 * self.J + 1)
        self.rows.copy_(rows[-1])
        if not self._pen_in_rows:
            self._penalties.copy_(self.penalties_many[-1])
        self.done.copy_(self.done_f != 0)
        return rows

    @property
    def A(self):
        """columns of an action row: J, or 2J with stiffness actions (the batch's own count)"""
        return self.batch.A

    def _point_at(self, k):
        D = self.obs_dim        # 3J, or 3J + E with observation channels
        self._row_k = k
        self.rows = self._row_blocks[k]
        self.obs, self.rew, self.done_f = self.rows[:, :D], self.rows[:, D], self.rows[:, D + 1]
        # lifting_com, station_keeping, energy (trex_env.py:193-195)
        self.penalties = self.rows[:, D + 2:D + 5] if self._pen_in_rows else self._penalties
        if self.sense_api is not None:          # (with sensing: the block the env composes, before the sensors)
            self.clean_rows = self.rows if self._clean_block is None else self._clean_block
            self.clean_obs = self.clean_rows[:, :D]

    def all_gather_rows(self, rows=None):
        """[global N, 3J+2] = obs | reward | done of EVERY env, on every rank: the one collective of the path
        (RCCL all-gather over xGMI; gloo in the CPU tests). sharding.split_rows(rows, 3 * J) cuts it back."""
        rows = self.rows if rows is None else rows
        if self.world_size == 1:
            return rows
        self._gather_buf = sharding.all_gather_rows(rows, self.global_num_envs, self.world_size,
                                                    self.process_group, out=self._gather_buf)
        return self._gather_buf

    def all_gather_rows_pipelined(self, rows=None, wait=True, join="stream"):
        """Like all_gather_rows, but the collective overlaps the next step: returns the rows gathered by the
        PREVIOUS call (None on the first). See sharding.PipelinedGather."""
        rows = self.rows if rows is None else rows
        if self.world_size == 1:
            return rows
        if self._pipe is None:
            if self.global_num_envs != self.num_envs * self.world_size:
                raise ValueError("pipelined gather needs equal shards")
            self._pipe = sharding.PipelinedGather(self.num_envs, rows.shape[1], self.world_size, rows.dtype,
                                                  self.device, self.process_group)
        return self._pipe.push(rows, copy=not (rows is self.rows and len(self._row_blocks) > 1), wait=wait, join=join)

    def all_gather_rows_copy(self, signal_group=None, sync="barrier"):
        """The pipelined exchange by peer copies instead of a collective kernel (sharding.CopyGather; needs
        row_buffers=2): returns the rows gathered from the PREVIOUS step (None on the first call)."""
        if self.world_size == 1:
            return self.rows
        if len(self._row_blocks) < 2 or self.global_num_envs != self.num_envs * self.world_size:
            raise ValueError("the copy exchange reads the row block in place: row_buffers=2 and equal shards")
        if self._copy_pipe is None:
            self._copy_pipe = sharding.CopyGather(self.num_envs, self.rows.shape[1], self.world_size, self.rank, self.rows.dtype,
                                                  self.device, self.process_group, signal_group, sync)
        return self._copy_pipe.push(self.rows)

    def all_gather_obs(self):
        """[global N, 3J] (with observations: 3J + E): the observation columns of all_gather_rows()."""
        return self.all_gather_rows()[:, :self.obs_dim]

    # ---- baselines VecEnv API (host numpy in/out)
    def reset(self):
        if self._ep_ret is not None:
            self._ep_ret[:] = 0.0
            self._ep_len[:] = 0
        return self.reset_tensor().cpu().numpy()

    def step_async(self, actions):
        actions = np.asarray(actions, np.float32)
        if actions.shape != (self.num_envs, self.A):
            raise ValueError("actions must have shape (%d, %d), got %s" % (self.num_envs, self.A, actions.shape))
        self._actions = torch.as_tensor(actions).to(self.device, non_blocking=True)

    def set_motor_gains(self, kp=None, kd=None, max_force=None):
        """Per-env, per-joint motor gains: each a scalar, [J] or [n, J] (observation order), None = the model parameter; all
        three None clears (trex_batch_set_motor_gains). Kept over resets."""
        n, J = self.num_envs, self.J
        g = [actuators.broadcast_gains(v, n, J, k) for k, v in (("kp", kp), ("kd", kd), ("max_force", max_force))]
        self.batch.set_motor_gains(*[None if t is None else self._dev(t) for t in g])

    def step_wait(self):
        """-> obs, rewards, dones, infos as numpy / dicts. The reference wraps its env in baselines' bench.Monitor
        (trex_train.py:41-42), whose info['episode'] = {'r': episode return, 'l': length, 't': seconds since the monitor was
        made} is what ppo2.learn averages into eprewmean / eplenmean: the env whose episode ENDS with this step (the harness's
        time limit inside the launch, or a contained env) carries that entry here too."""
        obs, rew, done = self.step_tensor(self._actions)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        if self._ep_ret is None:
            self._ep_ret, self._ep_len = np.zeros(self.num_envs, np.float64), np.zeros(self.num_envs, np.int64)
            self._t_start = time.time()
        self._ep_ret += rew          # (Monitor sums Python floats: f64)
        self._ep_len += 1
        infos = [{} for _ in range(self.num_envs)]
        if self._term_on:   # a fallen env: why, and the last observation of its episode (obs holds the new episode's first)
            reason = self.termination_reason.cpu().numpy()
            fallen = np.flatnonzero(reason)
            if len(fallen):
                tobs = self.terminal_obs.cpu().numpy()
                for i in fallen:
                    infos[i]["terminal_observation"] = tobs[i].copy()
                    infos[i]["termination"] = int(reason[i])
        for i in np.flatnonzero(done):
            infos[i]["episode"] = {"r": round(float(self._ep_ret[i]), 6), "l": int(self._ep_len[i]),
                                   "t": round(time.time() - self._t_start, 6)}
            self._ep_ret[i] = 0.0
            self._ep_len[i] = 0
        return obs, rew, done, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        # the batch caches the device allocations it has validated; the buffers of this env go back to torch's allocator now
        self.batch.forget_buffers()
        self.batch.close()

    def seed(self, seed=None):
        return [seed]  # the env is deterministic; np_random is never consumed (trex_env.py:124-126)

    # ---- state access for tests / checkpointing
    def get_state(self):
        out = torch.zeros(self.num_envs, self.batch.state_width, device=self.device)
        self.batch.get_state(out)
        return out

    def set_state(self, state, motors_enabled=True):
        state = self._dev(state)
        assert tuple(state.shape) == (self.num_envs, self.batch.state_width)
        self.batch.set_state(state)
        self.batch.set_motors_enabled(motors_enabled)

    def set_domain(self, mass_scale=None, friction=None):
        """Per-env domain randomisation (BASELINE config 5): mass_scale [n, num_bodies], friction [n]."""
        if mass_scale is not None:
            mass_scale = self._dev(mass_scale)
            assert tuple(mass_scale.shape) == (self.num_envs, self.model.num_bodies)
        if friction is not None:
            friction = self._dev(friction)
            assert tuple(friction.shape) == (self.num_envs,)
        self.batch.set_domain(mass_scale, friction)

    # ---- external forces (trex_batch_set_external_wrench; trex_gym.perturb)
    def set_external_wrench(self, wrench):
        """wrench [n, num_bodies, 6]: force at each moving body's COM and torque about it, world axes (N, N m). Held for
        every substep of every later step until replaced or cleared - not for the settle substep of a reset. None clears."""
        if wrench is None:
            return self.clear_external_wrench()
        wrench = self._dev(wrench)
        if tuple(wrench.shape) != (self.num_envs, self.model.num_bodies, 6):
            raise ValueError("wrench must have shape (%d, %d, 6), got %s" % (self.num_envs, self.model.num_bodies, tuple(wrench.shape)))
        self._wrench = wrench.clone()
        self.batch.set_external_wrench(self._wrench)

    def apply_external_force(self, link, force, position=None, frame="world", env_ids=None):
        """pybullet's applyExternalForce for link `link` (index or name): force [3] or [n, 3] at `position` (None: the
        body's COM), both in world coordinates (frame="world") or the link's frame (frame="link"), on the envs env_ids
        (None: all). ADDS to the held wrench (clear_external_wrench() removes it) and holds it for the whole env-step,
        every later step - pybullet's lasts one stepSimulation. The moment arm is taken at the current state."""
        from .perturb import link_wrench
        w = link_wrench(self._links, self.link_transforms(), link, force, position, frame)
        if env_ids is not None:
            keep = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
            keep[torch.as_tensor(env_ids, device=self.device, dtype=torch.long)] = True
            w = torch.where(keep.view(-1, 1, 1), w, torch.zeros_like(w))
        self.set_external_wrench(w if self._wrench is None else self._wrench + w)
        return self._wrench

    def clear_external_wrench(self):
        self._wrench = None
        self.batch.set_external_wrench(None)

    # ---- contact sensor (trex_batch_set_contact_sensor; the readings are vec_queries.contact_wrench() and its kin)
    def enable_contact_sensor(self, on=True):
        """on: every later step and reset records each env's floor-contact wrench per body (contact_wrench()); off: the
        default kernels again. The physics is bitwise the same either way."""
        self.batch.set_contact_sensor(on)

    # ---- fall termination (trex_batch_set_termination; what the predicate left is read in vec_queries.py)
    def set_termination(self, head_height=None, max_tilt=None, keep_clear=None, penalty=0.0):
        """End an env's episode when the robot falls (trex_batch_set_termination): the head point lower than head_height above
        the floor; the base tipped more than max_tilt rad from its start orientation; a body of keep_clear closer to the floor
        than allowed - keep_clear is {link name or index: least clearance} or a sequence of links, which must then stay clear of
        the floor by the model's contact_margin: "touches" (trex_gym.termination.support_bodies names the feet to leave out).
        Each None = off; all None switches the feature off. penalty is taken from the reward of the step in which the env falls.
        The step calls then decide on the device: done = 1, reward less penalty, the env reset at once - its observation is the
        new episode's first, the last of the old one is in terminal_obs."""
        cm = None
        if keep_clear is not None and len(keep_clear):
            cm = np.full(self.model.num_bodies, np.nan, np.float32)
            if isinstance(keep_clear, dict):
                links, mins = list(keep_clear.keys()), [float(v) for v in keep_clear.values()]
            else:
                links = list(keep_clear)
                mins = [self.model.get_param("contact_margin")] * len(links)
            for b, v in zip(self._link_bodies(links), mins):
                cm[b] = v if np.isnan(cm[b]) else max(cm[b], v)   # (two links of one body: the stricter)
        self.batch.set_termination(head_height, max_tilt, cm, penalty)
        self._term_on = head_height is not None or max_tilt is not None or cm is not None
        if self._term_on and self._term_buf is None:
            n = self.num_envs
            self._term_buf = (torch.zeros(n, dtype=torch.int32, device=self.device), torch.zeros(n, 3, device=self.device),
                              torch.zeros(n, 3 * self.J, device=self.device))
