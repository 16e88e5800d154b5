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
the block is [n, 3J + E + 2]: E more observation columns, composed on the device by one more launch per step and reset.

Multi-GPU: one process per GPU, env ids sharded by contiguous range (trex_gym.sharding); the only
exchange is the all-gather of that row block (all_gather_rows / all_gather_rows_pipelined).
"""
import collections
import time

import numpy as np
import torch

from . import _capi, actuators, sharding, spaces

REWARD_DEFAULTS = dict(distance_weight=1.0, energy_weight=0.005, drift_weight=0.002)  # trex_env.py:42-44


class Centroidal:
    """Named view of the [n, 16] block of trex_batch_centroidal (include/trex_batch.h); numpy or torch alike."""

    def __init__(self, data):
        self.data = data
        self.com, self.com_velocity = data[..., 0:3], data[..., 3:6]
        self.momentum, self.angular_momentum = data[..., 6:9], data[..., 9:12]
        self.kinetic, self.potential, self.mass = data[..., 12], data[..., 13], data[..., 14]


LinkState = collections.namedtuple("LinkState", "position orientation linear_velocity angular_velocity linear_acceleration "
                                                "angular_acceleration")
AXES = {"world": 0, "link": 1, "base": 2}
IkInfo = collections.namedtuple("IkInfo", "position_error orientation_error iterations initial_error")
ProximityShapes = collections.namedtuple("ProximityShapes", "bodies capsules pairs")
ClosestPoints = collections.namedtuple("ClosestPoints", "distance point_a point_b normal capsule")


class LinkProbes:
    """A set of points fixed in URDF links, held on the device by a TrexVecEnv (TrexVecEnv.link_probes): what link_state()
    evaluates in one launch. links: the link indices [K]; positions: [K, 3] in the link frames. close() gives the env's set slot
    back (an env holds 8)."""

    def __init__(self, env, slot, links, positions):
        self.env, self.slot = env, slot
        self.links, self.positions = links, positions
        self.num_probes = len(links)

    def close(self):
        if self.slot is not None:
            self.env._release_probes(self)
            self.slot = None

    def __len__(self):
        return self.num_probes


class TrexVecEnv(spaces.Env):       # gym.Env where gym is importable; the surface is baselines' VecEnv
    metadata = {"render.modes": ["human", "rgb_array"], "video.frames_per_second": 50}  # trex_env.py:33-36

    def __init__(self, num_envs, urdf_path=None, collisions_dir=None, device=None, action_repeat=1,
                 distance_weight=1.0, energy_weight=0.005, drift_weight=0.002,
                 max_episode_steps=None, starting_configuration=None, params=None,
                 rank=0, world_size=1, process_group=None, collision="hulls", primitive_max_radius=0.2, row_buffers=1,
                 penalties_in_rows=False, pushes=None, control_mode=None, variable_stiffness=False,
                 kp_max=actuators.DEFAULT_KP_MAX, terminate=None, observations=None, external=None):
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
        env -> such a tensor, called after every step and reset."""
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
        self.observations, self.obs_dim, self._step_rows, self._external, self._link_table = None, 3 * J, None, external, None
        if observations is not None and len(observations):
            self._set_observations(observations)
        elif external is not None:
            raise ValueError("external: there is no observations.external(k) channel to take it")
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
        self._link_table = None
        self._ray_out = (None, None)            # ray_test's output buffers of the last (R, positions, normals)
        self._probe_sets = [None] * 8           # the LinkProbes handle in each of the batch's probe-set slots
        self._probe_cache = (None, None)        # link_state()'s one-off set of the last links given directly
        self.collision = collision
        self._prox, self._prox_out = None, (None, None)   # the ProximityShapes in force; closest_points()'s output buffers
        self.pushes = pushes
        if pushes is not None and pushes.num_envs != n:
            raise ValueError("pushes: RandomPushes over %d envs, the env has %d" % (pushes.num_envs, n))
        self._term_on, self._term_buf = False, None   # fall termination: on?, (reason, values, terminal_obs) buffers of the env
        if terminate:
            self.set_termination(**terminate)

    # ---- observation channels (trex_batch_set_observation / trex_batch_compose_rows; trex_gym.observations builds specifications)
    def _set_observations(self, spec):
        from . import observations as O
        from .perturb import LinkTable
        if self._link_table is None:
            self._link_table = LinkTable.from_model(self.model)
        J, n = self.J, self.num_envs
        chans, extra, contact, ext_cols = O.resolve(spec, self._link_table.index, self.A)
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

    def _compose(self, actions):
        ext = self._external(self) if callable(self._external) else self._external
        if ext is not None and (ext.dtype != torch.float32 or not ext.is_contiguous() or ext.device != self.device):
            ext = ext.to(device=self.device, dtype=torch.float32).contiguous()
        self.batch.compose_rows(self._step_rows, self.rows, actions, ext)

    # ---- tensor-native API (stays on device, stream-ordered, no host sync)
    def reset_tensor(self, mask=None):
        """Reset all envs (mask=None) or those with mask != 0 (uint8 or bool [n], e.g. the `done` of the last step).
        Returns obs [n, 3J]; the reward / done columns and `done` of the envs that were reset read 0 afterwards.
        With observations: obs [n, 3J + E], every env's channels recomposed at the current state, prev_action() columns zero."""
        self.batch.reset_rows(self.rows if self._step_rows is None else self._step_rows, mask)
        if self._step_rows is not None:
            self._compose(None)
        if self.gains is not None:              # the envs that were reset draw new motor gains
            self.set_motor_gains(**self.gains.draw(mask))
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
        self.batch.set_episode_limit(int(self.max_episode_steps or 0), steps.to(device=self.device, dtype=torch.int32).contiguous())

    def step_tensor(self, actions):
        """actions [n, J] f32 on device -> (obs [n,3J], reward [n], done [n] bool). Views into buffers
        that the next call overwrites."""
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(actions.shape) != (self.num_envs, self.A):
            raise ValueError("actions must have shape (%d, %d), got %s" % (self.num_envs, self.A, tuple(actions.shape)))
        # (with max_episode_steps the launch also resets the envs whose episode ends with this step: done = 1,
        # reward of the finished step, observation of the new episode - VecEnv semantics, no second launch)
        if self.pushes is not None:   # this step's pushes (those of envs that ended their episode last step are dropped)
            w = self.pushes.wrench(self.model.num_bodies, self.done).to(self.device)
            self.batch.set_external_wrench(w if self._wrench is None else w + self._wrench)
        if len(self._row_blocks) > 1:
            self._point_at(1 - self._row_k)
        # (with set_termination the call is three launches: step, fall predicate, reset of the fallen - done = 1, the reward of
        # the finished step less the penalty, observation of the new episode)
        if self._step_rows is None:
            self.batch.step_rows(actions, self.rows, self._penalties, done=self.done)   # (None: the penalties ride in the row block)
        else:   # (observation channels: one more launch, after the resets of the step call - the row of the new episode's state)
            self.batch.step_rows(actions, self._step_rows, self._penalties, done=self.done)
            self._compose(actions)
        if self._term_on and self.gains is not None:   # the envs that fell start their episode with new motor gains
            self.set_motor_gains(**self.gains.draw(self.termination_reason != 0))
        return self.obs, self.rew, self.done

    def step_many_tensor(self, actions, rows=None):
        """Open-loop rollout: actions [S, n, J] f32 on device -> rows [S, n, 3J+2] (obs | reward | done of every step), S
        env-steps in ONE launch (trex_batch_step_many; bitwise S calls of step_tensor). `rows`, `obs`, `rew`, `done_f`
        and `done` then hold the last step. sharding.split_rows(rows[s]) cuts a step's block into the three.
        ValueError with observations: an open-loop launch has no compose between its steps."""
        if self._step_rows is not None:
            raise ValueError("step_many_tensor: not with observations - the open-loop launch has no per-step compose of the channels")
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if actions.dim() != 3 or tuple(actions.shape[1:]) != (self.num_envs, self.A):
            raise ValueError("actions must have shape (S, %d, %d), got %s" % (self.num_envs, self.A, tuple(actions.shape)))
        S = int(actions.shape[0])
        if rows is None:
            rows = torch.empty(S, self.num_envs, self.rows.shape[1], device=self.device)
        # (the three reward terms of every step: in the rows when penalties_in_rows, else in `penalties_many` [S, n, 3]; `penalties`
        # then holds the last step's, like the other views - it used to keep the values from BEFORE the call)
        self.penalties_many = None if self._pen_in_rows else torch.empty(S, self.num_envs, 3, device=self.device)
        self.batch.step_many(actions, rows, self.penalties_many)
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
        self.batch.set_motor_gains(*[None if t is None else t.to(self.device).contiguous() for t in g])

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

    # ---- rendering (trex_batch_render: a ray caster over the collision hulls, include/trex_batch.h)
    def render_tensor(self, env_ids=None, width=84, height=84, camera=None, depth=False, segmentation=False):
        """Pixel observations on the device: rgb [V, H, W, 3] uint8 of the envs env_ids (host sequence, None = all n), plus
        depth [V, H, W] float32 (linear eye-space metres) and / or seg [V, H, W] int32 (body index, -1 floor, -2 nothing)
        when asked - then a tuple (rgb, depth?, seg?). camera: trex_gym.render.Camera (default: the reference's, following
        each env's base). One launch, stream-ordered, no host sync; the state is only read."""
        from .render import Camera
        camera = Camera() if camera is None else camera
        V = self.num_envs if env_ids is None else len(env_ids)
        rgb = torch.empty(V, height, width, 3, dtype=torch.uint8, device=self.device)
        dep = torch.empty(V, height, width, dtype=torch.float32, device=self.device) if depth else None
        seg = torch.empty(V, height, width, dtype=torch.int32, device=self.device) if segmentation else None
        self.batch.render(camera, width, height, env_ids, rgb, dep, seg)
        if not depth and not segmentation:
            return rgb
        return (rgb,) + ((dep,) if depth else ()) + ((seg,) if segmentation else ())

    def get_images(self, width=None, height=None, camera=None, env_ids=None):
        """baselines' VecEnv.get_images: a list of H x W x 3 uint8 numpy frames, one per env (default 720 x 960, the
        reference's frame size: mind the memory for large batches - render_tensor keeps them on the device)."""
        from .render import RENDER_HEIGHT, RENDER_WIDTH
        rgb = self.render_tensor(env_ids, width or RENDER_WIDTH, height or RENDER_HEIGHT, camera)
        return list(rgb.cpu().numpy())

    def render(self, mode="rgb_array"):
        """'rgb_array': ONE near-square tile (baselines' tile_images) of the first min(n, 16) envs at 720 x 960 each - not
        of all n: 4 096 full frames would be 8 GB. 'human' raises NotImplementedError (no display)."""
        from .render import tile_images
        if mode == "human":
            raise NotImplementedError("render('human'): there is no display; use 'rgb_array' or render_tensor()")
        if mode != "rgb_array":
            raise ValueError("render mode must be 'rgb_array' or 'human'")
        return tile_images(np.stack(self.get_images(env_ids=list(range(min(self.num_envs, 16))))))

    def seed(self, seed=None):
        return [seed]  # the env is deterministic; np_random is never consumed (trex_env.py:124-126)

    # ---- state access for tests / checkpointing
    def get_state(self):
        out = torch.zeros(self.num_envs, self.batch.state_width, device=self.device)
        self.batch.get_state(out)
        return out

    def set_state(self, state, motors_enabled=True):
        state = state.to(device=self.device, dtype=torch.float32).contiguous()
        assert tuple(state.shape) == (self.num_envs, self.batch.state_width)
        self.batch.set_state(state)
        self.batch.set_motors_enabled(motors_enabled)

    def head_position(self):
        out = torch.zeros(self.num_envs, 3, device=self.device)
        self.batch.head_position(out)
        return out

    def link_transforms(self):
        """World pose of every URDF link frame, [n, L, 7] = xyz + quaternion xyzw (rollout export for
        rendering, the step after the path: trex_env.py:156-181)."""
        L = len(self.model.links())
        out = torch.empty(self.num_envs, L, 7, device=self.device)
        self.batch.link_transforms(out)
        return out

    def visual_transforms(self):
        """World pose of every <visual> mesh of the URDF, [n, V, 7] = xyz + quaternion xyzw (252 meshes for trex.urdf;
        `model.visuals()` names them): what a renderer places the meshes with - the table pybullet keeps for
        getCameraImage (trex_env.py:164-176)."""
        V = len(self.model.visuals())
        out = torch.empty(self.num_envs, V, 7, device=self.device)
        self.batch.visual_transforms(out)
        return out

    def set_domain(self, mass_scale=None, friction=None):
        """Per-env domain randomisation (BASELINE config 5): mass_scale [n, num_bodies], friction [n]."""
        if mass_scale is not None:
            mass_scale = mass_scale.to(device=self.device, dtype=torch.float32).contiguous()
            assert tuple(mass_scale.shape) == (self.num_envs, self.model.num_bodies)
        if friction is not None:
            friction = friction.to(device=self.device, dtype=torch.float32).contiguous()
            assert tuple(friction.shape) == (self.num_envs,)
        self.batch.set_domain(mass_scale, friction)

    # ---- external forces (trex_batch_set_external_wrench; trex_gym.perturb)
    def set_external_wrench(self, wrench):
        """wrench [n, num_bodies, 6]: force at each moving body's COM and torque about it, world axes (N, N m). Held for
        every substep of every later step until replaced or cleared - not for the settle substep of a reset. None clears."""
        if wrench is None:
            return self.clear_external_wrench()
        wrench = wrench.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(wrench.shape) != (self.num_envs, self.model.num_bodies, 6):
            raise ValueError("wrench must have shape (%d, %d, 6), got %s" % (self.num_envs, self.model.num_bodies, tuple(wrench.shape)))
        self._wrench = wrench.clone()
        self.batch.set_external_wrench(self._wrench)

    def apply_external_force(self, link, force, position=None, frame="world", env_ids=None):
        """pybullet's applyExternalForce for link `link` (index or name): force [3] or [n, 3] at `position` (None: the
        body's COM), both in world coordinates (frame="world") or the link's frame (frame="link"), on the envs env_ids
        (None: all). ADDS to the held wrench (clear_external_wrench() removes it) and holds it for the whole env-step,
        every later step - pybullet's lasts one stepSimulation. The moment arm is taken at the current state."""
        from .perturb import LinkTable, link_wrench
        if self._link_table is None:
            self._link_table = LinkTable.from_model(self.model)
        w = link_wrench(self._link_table, self.link_transforms(), link, force, position, frame)
        if env_ids is not None:
            keep = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
            keep[torch.as_tensor(env_ids, device=self.device, dtype=torch.long)] = True
            w = torch.where(keep.view(-1, 1, 1), w, torch.zeros_like(w))
        self.set_external_wrench(w if self._wrench is None else self._wrench + w)
        return self._wrench

    def clear_external_wrench(self):
        self._wrench = None
        self.batch.set_external_wrench(None)

    # ---- contact sensor (trex_batch_set_contact_sensor / trex_batch_contact_wrench; no host sync)
    def enable_contact_sensor(self, on=True):
        """on: every later step and reset records each env's floor-contact wrench per body (contact_wrench()); off: the
        default kernels again. The physics is bitwise the same either way."""
        self.batch.set_contact_sensor(on)

    def contact_wrench(self, out=None):
        """[n, num_bodies, 6] on the device: floor-contact force at each body's COM and torque about it, world axes (N, N m),
        the mean over the substeps of the last step (a reset env: its settle substep; a contained env: zeros)."""
        return self.batch.contact_wrench(out)

    # ---- dynamics queries (trex_batch_inverse_dynamics / _mass_matrix / _jacobian / _centroidal / _forward_dynamics /
    # _solve_mass; no host sync)
    # Generalised velocity [D = 6 + J]: base linear v(3), base angular w(3), world axes, then qd in observation order - the
    # velocity part of get_state(); forces are its duals (base force, base torque about the base origin, joint torques).
    def inverse_dynamics(self, accel=None, out=None):
        """[n, D] generalised force M(q) a + h(q, qd) for the accelerations accel [n, D] (None: zeros) at the current state.
        Rigid-body terms only: no joint damping, link damping, motors, limits or contacts (pybullet's calculateInverseDynamics)."""
        if accel is not None:
            accel = torch.as_tensor(accel).to(device=self.device, dtype=torch.float32).contiguous()
        return self.batch.inverse_dynamics(accel, out)

    def gravity_compensation(self):
        """[n, J] joint torques of inverse_dynamics() with zero accelerations: what holds the joints against gravity (and the
        velocity-product terms of a moving state), ready to add to the actions of TORQUE-mode joints."""
        return self.batch.inverse_dynamics(None, None)[:, 6:]

    def mass_matrix(self, out=None):
        """[n, D, D] joint-space inertia matrix M(q), symmetric (pybullet's calculateMassMatrix)."""
        return self.batch.mass_matrix(out)

    def jacobian(self, link, position=None, out=None):
        """[n, 6, D] Jacobian of the point `position` (link frame; None: the link origin) of link `link` (index or name):
        rows 0..2 its world linear velocity, rows 3..5 the link's world angular velocity (pybullet's calculateJacobian)."""
        from .perturb import LinkTable
        if self._link_table is None:
            self._link_table = LinkTable.from_model(self.model)
        return self.batch.jacobian(self._link_table.index(link), position, out)

    def centroidal(self, out=None):
        """Whole-body quantities as a Centroidal of device tensors: com [n, 3], com_velocity, momentum, angular_momentum (about
        the COM), kinetic [n], potential (sum m g z), mass (the env's mass scale included); `.data` is the [n, 16] block."""
        return Centroidal(self.batch.centroidal(out))

    def forward_dynamics(self, force=None, tau=None, out=None):
        """[n, D] accelerations M(q)^-1 (force - h(q, qd)) that the generalised force `force` [n, D] produces at the current
        state (None: zeros - free motion under gravity): the inverse of inverse_dynamics, rigid-body terms only. tau [n, J] is
        shorthand for a force with a zero base block; giving both is an error."""
        if force is not None and tau is not None:
            raise ValueError("forward_dynamics: give force or tau, not both")
        if tau is not None:
            tau = torch.as_tensor(tau).to(device=self.device, dtype=torch.float32)
            force = torch.cat([torch.zeros(tau.shape[0], 6, dtype=torch.float32, device=self.device), tau], 1)
        elif force is not None:
            force = torch.as_tensor(force).to(device=self.device, dtype=torch.float32).contiguous()
        return self.batch.forward_dynamics(force, out)

    def solve_mass(self, rhs=None, out=None):
        """[n, K, D] = M(q)^-1 applied to the K force-like rows rhs[e, k, :] of every env, K <= 64 ([n, D]: one row, returns
        [n, D]); None: the identity, M^-1 itself. solve_mass(jacobian(link)) is (M^-1 J^T)^T. Depends on q alone."""
        if rhs is not None:
            rhs = torch.as_tensor(rhs).to(device=self.device, dtype=torch.float32).contiguous()
        return self.batch.solve_mass(rhs, out)

    def inverse_mass_matrix(self, out=None):
        """[n, D, D] M(q)^-1 (symmetric up to rounding)."""
        return self.batch.solve_mass(None, out)

    def operational_space_inertia(self, link, position=None):
        """[n, 6, 6] task-space inertia inv(J M^-1 J^T) of the point `position` of link `link` (as jacobian()): one Jacobian
        launch, one solve launch and a batched 6 x 6 inverse."""
        Jm = self.jacobian(link, position)
        return torch.linalg.inv(Jm @ self.batch.solve_mass(Jm).transpose(1, 2))

    # ---- link kinematics (trex_batch_set_link_probes / trex_batch_link_state; one launch for all probes, no host sync)
    def link_probes(self, links, positions=None):
        """A LinkProbes handle for the points `positions` [K, 3] (link frames; None: the link origins) of the links `links` (K
        names or indices, or one). It takes one of the env's 8 probe-set slots until its close(); RuntimeError when none is free."""
        from .perturb import LinkTable
        if self._link_table is None:
            self._link_table = LinkTable.from_model(self.model)
        if isinstance(links, (str, int, np.integer)):
            links = [links]
            if positions is not None:
                positions = np.asarray(positions, np.float64).reshape(1, 3)
        idx = [self._link_table.index(l) for l in links]
        pos = np.zeros((len(idx), 3)) if positions is None else np.asarray(positions, np.float64)
        if pos.shape != (len(idx), 3):
            raise ValueError("positions must have shape (%d, 3), got %s" % (len(idx), pos.shape))
        if not idx:
            raise ValueError("link_probes: no link given")
        free = [k for k, h in enumerate(self._probe_sets) if h is None]
        if not free:
            raise RuntimeError("link_probes: all %d probe sets of this env are in use; close() one first" % len(self._probe_sets))
        self.batch.set_link_probes(free[0], idx, pos)
        h = LinkProbes(self, free[0], idx, pos)
        self._probe_sets[free[0]] = h
        return h

    def _release_probes(self, h):
        if self._probe_sets[h.slot] is h:
            self.batch.set_link_probes(h.slot, [])
            self._probe_sets[h.slot] = None
        if self._probe_cache[1] is h:
            self._probe_cache = (None, None)

    def link_state(self, probes, accel=None, axes="world", proper=False, velocity=True, acceleration=False):
        """Kinematics of the K probes of `probes` - a LinkProbes handle, or a link / a list of links (their origins; kept as a
        one-off set until other links are given) - at the current state, as a LinkState of device tensors:
        position [n, K, 3] of the points and orientation [n, K, 4] (xyzw, w >= 0) of their link frames; with `velocity`
        linear_velocity of the points and angular_velocity of the links; with `acceleration` linear_acceleration (classical,
        d2p/dt2) and angular_acceleration at the generalised accelerations accel [n, D] (None: zeros - the bias acceleration
        Jdot qd). Parts not asked for are None.
        axes: "world", "link" (each probe's own link frame) or "base" (URDF link 0's frame): the axes the velocities and
        accelerations - still relative to the world - are expressed in; with "base" the pose is relative to that frame too.
        proper: + g z (world) on the linear acceleration: the specific force an accelerometer at the point reads."""
        if axes not in AXES:
            raise ValueError("axes must be one of %s" % sorted(AXES))
        if not isinstance(probes, LinkProbes):
            key = tuple(probes) if isinstance(probes, (list, tuple)) else (probes,)
            if self._probe_cache[0] != key:
                if self._probe_cache[1] is not None:
                    self._probe_cache[1].close()
                self._probe_cache = (key, self.link_probes(list(key)))
            probes = self._probe_cache[1]
        if probes.env is not self or probes.slot is None:
            raise ValueError("link_state: the probes are closed or belong to another env")
        n, K = self.num_envs, probes.num_probes
        if accel is not None:
            accel = torch.as_tensor(accel).to(device=self.device, dtype=torch.float32).contiguous()
        pose = torch.empty(n, K, 7, device=self.device)
        vel = torch.empty(n, K, 6, device=self.device) if velocity else None
        acc = torch.empty(n, K, 6, device=self.device) if acceleration else None
        self.batch.link_state(probes.slot, AXES[axes], proper, accel, pose, vel, acc, probes=K)
        return LinkState(pose[..., :3], pose[..., 3:], None if vel is None else vel[..., :3], None if vel is None else vel[..., 3:],
                         None if acc is None else acc[..., :3], None if acc is None else acc[..., 3:])

    def bias_acceleration(self, link, position=None):
        """[n, 6] = Jdot qd of the point `position` of link `link` (as jacobian(), and in its row order: linear, angular; world
        axes): the point's acceleration at zero generalised accelerations - with operational_space_inertia(), jacobian() and
        inverse_dynamics() what a task-space controller needs."""
        key = ("bias", link, None if position is None else tuple(float(x) for x in position))
        if self._probe_cache[0] != key:
            if self._probe_cache[1] is not None:
                self._probe_cache[1].close()
            self._probe_cache = (key, self.link_probes(link, position))
        h = self._probe_cache[1]
        acc = torch.empty(self.num_envs, 1, 6, device=self.device)
        self.batch.link_state(h.slot, 0, False, None, None, None, acc, probes=1)
        return acc[:, 0]

    # ---- inverse kinematics (trex_batch_inverse_kinematics: pybullet's calculateInverseKinematics; one launch for every env, all
    # targets and all iterations, no host sync)
    def inverse_kinematics(self, probes, positions=None, orientations=None, frame="world", q_init=None, joints=None,
                           iterations=20, damping=0.01, gain=0.1, max_step=0.2, tol=(0.0, 0.0)):
        """Joint angles that bring the K <= 8 probes of `probes` (a LinkProbes of link_probes()) to per-env targets, by damped
        least squares at the envs' current base poses: (q [n, J] in observation order, IkInfo of device tensors).
        positions [n, K, 3] (or [K, 3], every env alike): where the probe points are to be; orientations [n, K, 4] (xyzw): the
        orientations of their link frames; either may be None, and a row with a NaN in it means "not constrained" - rows are
        read on the host once to find them, so every env constrains the same parts. frame: "world", or "base": targets relative
        to URDF link 0's frame, as link_state(axes="base") reports poses. q_init [n, J]: where the solve starts (None: the
        current joint angles). joints: the names or observation indices of the joints that may move (None: all); the others
        come back as they went in. tol = (metres, radians): stop an env early once both residuals are at or below them.
        info: position_error [n] and orientation_error [n] (the largest residuals at q), iterations [n], initial_error [n]
        (the norm of the stacked error at the start). step(joint_targets_to_actions(q)) commands the result."""
        if frame not in ("world", "base"):
            raise ValueError("frame must be 'world' or 'base'")
        if not isinstance(probes, LinkProbes) or probes.env is not self or probes.slot is None:
            raise ValueError("inverse_kinematics: probes must be an open LinkProbes of this env")
        n, J, K = self.num_envs, self.J, probes.num_probes
        if positions is None and orientations is None:
            raise ValueError("inverse_kinematics: give positions, orientations or both")

        def rows(t, width, what):
            if t is None:
                return None, np.zeros(K, bool)
            t = torch.as_tensor(t, dtype=torch.float32)
            if t.dim() == 2:
                t = t.unsqueeze(0).expand(n, K, width)
            if tuple(t.shape) != (n, K, width):
                raise ValueError("%s must have shape (%d, %d, %d) or (%d, %d), got %s" % (what, n, K, width, K, width, tuple(t.shape)))
            t = t.to(self.device)
            return t, (~torch.isnan(t).any(2).any(0)).cpu().numpy()

        pos, has_p = rows(positions, 3, "positions")
        ori, has_o = rows(orientations, 4, "orientations")
        modes = has_p * 1 + has_o * 2
        if (modes == 0).any():
            raise ValueError("inverse_kinematics: probe %d is not constrained at all" % int(np.argmin(modes)))
        target = torch.zeros(n, K, 7, device=self.device)
        target[..., 6] = 1.0
        if pos is not None:
            target[..., :3] = pos
        if ori is not None:
            target[..., 3:] = ori
        if joints is None:
            mask = (1 << J) - 1
        else:
            names = self.model.joint_names
            mask = 0
            for j in ([joints] if isinstance(joints, (str, int, np.integer)) else joints):
                k = names.index(j) if isinstance(j, str) else int(j)
                if not 0 <= k < J:
                    raise IndexError("joint index %d out of range [0, %d)" % (k, J))
                mask |= 1 << k
        if q_init is not None:
            q_init = torch.as_tensor(q_init, dtype=torch.float32).to(self.device).expand(n, J).contiguous()
        q, info = torch.empty(n, J, device=self.device), torch.empty(n, 4, device=self.device)
        self.batch.inverse_kinematics(probes.slot, modes, target.contiguous(), q, AXES[frame], q_init, mask, info, iterations, damping,
                                      gain, max_step, tol[0], tol[1])
        return q, IkInfo(info[:, 0], info[:, 1], info[:, 2].to(torch.int32), info[:, 3])

    def joint_targets_to_actions(self, q):
        """Action rows [n, A] that command the joint angles q [n, J] (observation order; e.g. inverse_kinematics()' result): the
        inverse of the env's action scaling. A POSITION-mode joint's action IS its target angle, clipped by the step to the
        joint's limits as it is here; a VELOCITY- or TORQUE-mode joint has no position target: its column is 0. With stiffness
        actions the J stiffness columns carry the model's motor_kp, clipped to kp_max."""
        q = torch.as_tensor(q, dtype=torch.float32).to(self.device)
        lo = torch.as_tensor(self.model.lower.astype(np.float32), device=self.device)
        hi = torch.as_tensor(self.model.upper.astype(np.float32), device=self.device)
        position = torch.as_tensor(np.asarray(self.control_modes) == 0, device=self.device)
        a = torch.where(position, torch.minimum(torch.maximum(q, lo), hi), torch.zeros_like(q))
        if self.variable_stiffness:
            kp = min(float(self.model.get_param("motor_kp")), self.kp_max)
            a = torch.cat([a, torch.full_like(a, kp)], -1)
        return a

    # ---- proximity between bodies (trex_batch_set_proximity_shapes / trex_batch_proximity: pybullet's getClosestPoints between
    # links of the robot; one launch for all pairs, no host sync)
    def proximity_shapes(self, capsules=None, pairs=None, max_radius=0.2, max_divisions=3, min_points=4, exclude_adjacent=True,
                         exclude_start_overlaps=True):
        """Set the env's proximity table and return what it holds, as ProximityShapes(bodies [C], capsules [C, 7], pairs [P, 2]).
        capsules: (bodies [C], [C, 7] = p0 xyz, p1 xyz, radius in the body frames); None: every convex hull fitted with
        Model.fit_hull_primitives(max_radius, max_divisions, min_points) - or, with collision="primitives", the model's spheres
        as capsules of length 0: what the physics collides with (the cylinder between a capsule's ends is absent there too).
        pairs: [P, 2] body pairs (A, B); None: all pairs of bodies with geometry, minus parent-child pairs (exclude_adjacent),
        minus the pairs that already overlap at the start pose (exclude_start_overlaps; found with one query on a reset batch of
        one env). capsules=() frees the table."""
        m = self.model
        if capsules is None:
            hs = m.array("hull_start").astype(int)
            if self.collision == "primitives":
                xyz, rad = m.array("hull_xyz").reshape(-1, 3), m.array("hull_radius")
                bodies = np.repeat(np.arange(m.num_bodies), np.diff(hs)).astype(np.int32)
                caps = np.concatenate([xyz, xyz, rad[:, None]], 1)
            else:
                gs = m.array("hull_group_start").astype(int)
                bodies, caps = [], []
                for b in range(m.num_bodies):
                    for g in range(len(gs) - 1):
                        if hs[b] <= gs[g] < hs[b + 1] and gs[g + 1] > gs[g]:
                            for p0, p1, r in m.fit_hull_primitives(g, max_radius, max_divisions, min_points):
                                bodies.append(b)
                                caps.append(np.concatenate([p0, p1, [r]]))
                bodies, caps = np.array(bodies, np.int32), np.array(caps, np.float64).reshape(-1, 7)
        else:
            bodies, caps = capsules if len(capsules) else ((), ())
            bodies, caps = np.asarray(bodies, np.int32).reshape(-1), np.asarray(caps, np.float64).reshape(-1, 7)
        if len(bodies) == 0:
            self.batch.set_proximity_shapes([])
            self._prox, self._prox_out = None, (None, None)
            return None
        if pairs is None:
            have = sorted(set(int(b) for b in bodies))
            parent = m.array("parent").astype(int)
            pairs = [(a, b) for i, a in enumerate(have) for b in have[i + 1:]
                     if not (exclude_adjacent and (parent[b] == a or parent[a] == b))]
            if exclude_start_overlaps and pairs:
                probe = _capi.Batch(m, 1, self.device.index)
                try:
                    probe.reset()
                    probe.set_proximity_shapes(bodies, caps, pairs)
                    d = torch.empty(1, len(pairs), device=self.device)
                    probe.proximity(d, pairs=len(pairs))
                    keep = (~(d[0] < 0)).cpu().numpy()
                finally:
                    probe.forget_buffers()
                    probe.close()
                pairs = [p for p, k in zip(pairs, keep) if k]
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        self.batch.set_proximity_shapes(bodies, caps, pairs)
        self._prox, self._prox_out = ProximityShapes(bodies, caps, pairs), (None, None)
        return self._prox

    def closest_points(self, points=False):
        """Signed distance [n, P] between the bodies of every pair of proximity_shapes() (made with its defaults on first use) at
        the current state: the smallest over the capsules of the two bodies, negative = overlap depth. points: a ClosestPoints
        instead, adding point_a, point_b [n, P, 3] (world; on the surfaces of A and B), normal [n, P, 3] (unit, from B to A:
        pybullet's contactNormalOnB) and capsule [n, P, 2] int32 (table indices of the two winning capsules). The tensors are
        buffers of the env, reused by the next call."""
        if self._prox is None:
            self.proximity_shapes()
        n, P = self.num_envs, len(self._prox.pairs)
        key = (P, bool(points))
        if self._prox_out[0] != key:
            f = lambda *s: torch.empty(*s, device=self.device)
            self._prox_out = (key, (f(n, P),) + ((f(n, P, 3), f(n, P, 3), f(n, P, 3), torch.empty(n, P, 2, dtype=torch.int32, device=self.device))
                                                 if points else (None,) * 4))
        out = self._prox_out[1]
        self.batch.proximity(*out, pairs=P)
        return ClosestPoints(*out) if points else out[0]

    def self_collision_distance(self):
        """[n]: the smallest distance over the pairs of proximity_shapes(); negative: two bodies of the env overlap by that much."""
        return self.closest_points().min(dim=1).values

    def in_self_collision(self, margin=0.0):
        """[n] bool: some pair of proximity_shapes() is closer than `margin`."""
        return self.self_collision_distance() < margin

    # ---- floor clearance and fall termination (trex_batch_body_clearance / trex_batch_set_termination; no host sync)
    def _link_bodies(self, links):
        """links: names or indices of URDF links -> their bodies [K] (numpy int64)"""
        from .perturb import LinkTable
        if self._link_table is None:
            self._link_table = LinkTable.from_model(self.model)
        return np.array([self._link_table.link_body[self._link_table.index(l)] for l in links], np.int64)

    def body_clearance(self, links=None, lowest=False):
        """Height of the lowest collision point above the floor, exact over the collision geometry of the physics, at the
        current state: [n, num_bodies] for every body (links=None), or [n, K] for the bodies of the links `links` (names or
        indices; one link: [n]). +inf for a body without collision geometry; negative: that deep in the floor. lowest: a tuple
        (clearance, point [..., 3]) with the world position of that lowest point. One launch, device tensors."""
        n, nb = self.num_envs, self.model.num_bodies
        clr = torch.empty(n, nb, device=self.device)
        low = torch.empty(n, nb, 3, device=self.device) if lowest else None
        self.batch.body_clearance(clr, low)
        if links is not None:
            one = isinstance(links, (str, int, np.integer))
            idx = torch.as_tensor(self._link_bodies([links] if one else list(links)), device=self.device)
            clr = clr[:, idx[0]] if one else clr[:, idx]
            if lowest:
                low = low[:, idx[0]] if one else low[:, idx]
        return (clr, low) if lowest else clr

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

    def _term_info(self, k):
        if self._term_buf is None:
            raise RuntimeError("termination is not enabled (set_termination)")
        out = self._term_buf[k]
        self.batch.termination_info(*[out if i == k else None for i in range(3)])
        return out

    @property
    def termination_reason(self):
        """[n] int32 on the device: why each env fell in the last step - bits 1 head height, 2 tilt, 4 clearance; 0: it did not.
        A buffer of the env, rewritten by the next read."""
        return self._term_info(0)

    @property
    def termination_values(self):
        """[n, 3] on the device, what the last step's decision compared: head height above the floor, cos of the base's tilt,
        least (clearance - allowed) over the watched bodies (+inf: none watched)."""
        return self._term_info(1)

    @property
    def terminal_obs(self):
        """[n, 3J] on the device: for an env that fell, the last observation of that episode (the row of an env that did not
        fall in the last step holds the one of its most recent fall, zeros before the first). With observations it stays the 3J
        base columns: the channels of the state that fell are not kept."""
        return self._term_info(2)

    # ---- ray casts (trex_batch_ray_test: pybullet's rayTestBatch; no host sync; trex_gym.sensors builds patterns)
    def ray_test(self, rays, link=None, positions=False, normals=False, bodies=None, floor=True):
        """Cast rays [n, R, 6] (or [R, 6]: one pattern for every env) - from xyz, to xyz, in the frame of link `link` (name or
        index; None: the world) - against the collision geometry render_tensor() draws, at the current state. bodies: an
        iterable of body indices that may be hit (None: all); floor: whether the floor may be.
        -> (fraction [n, R], body [n, R] int32[, position [n, R, 3]][, normal [n, R, 3]]) on the device: fraction of the
        segment at the nearest hit (1.0: none), body index (-1 the floor, -2 a miss), world hit point (a miss: the segment's
        end) and unit normal (a miss: zeros). The tensors are buffers of the env, reused by the next call of the same shape."""
        from .perturb import LinkTable
        if link is None:
            k = -1
        else:
            if self._link_table is None:
                self._link_table = LinkTable.from_model(self.model)
            k = self._link_table.index(link)
        rays = torch.as_tensor(rays)
        if rays.dtype != torch.float32 or not rays.is_contiguous() or rays.device != self.device:
            rays = rays.to(device=self.device, dtype=torch.float32).contiguous()
        if rays.dim() not in (2, 3) or rays.shape[-1] != 6:
            raise ValueError("rays must have shape (%d, R, 6) or (R, 6), got %s" % (self.num_envs, tuple(rays.shape)))
        mask = 0xFFFFFFFF
        if bodies is not None:
            mask = 0
            for b in bodies:
                if not 0 <= int(b) < self.model.num_bodies:
                    raise IndexError("body index %d out of range [0, %d)" % (int(b), self.model.num_bodies))
                mask |= 1 << int(b)
        n, R = self.num_envs, int(rays.shape[-2])
        key = (R, bool(positions), bool(normals))
        if self._ray_out[0] != key:   # (one shape is kept: a caller that sweeps R does not pile up device memory)
            self._ray_out = (None, None)
            self._ray_out = (key, (torch.empty(n, R, device=self.device), torch.empty(n, R, dtype=torch.int32, device=self.device),
                                   torch.empty(n, R, 3, device=self.device) if positions else None,
                                   torch.empty(n, R, 3, device=self.device) if normals else None))
        frac, body, pos, nrm = self._ray_out[1]
        self.batch.ray_test(rays, k, None, mask, floor, frac, body, pos, nrm)
        return (frac, body) + ((pos,) if positions else ()) + ((nrm,) if normals else ())

    def contact_forces(self, links):
        """[n, K, 3] floor-contact force on URDF links: links = K entries, each a link name / index or a list of them (the
        force summed over their distinct bodies), e.g. contact_forces(["foot_L", "foot_R"])."""
        from .perturb import LinkTable, link_contact_forces
        if self._link_table is None:
            self._link_table = LinkTable.from_model(self.model)
        return link_contact_forces(self._link_table, self.contact_wrench(), links)

    def in_contact(self, threshold=0.0):
        """[n, num_bodies] bool: the floor pushes the body with more than `threshold` N (normal force)."""
        from .perturb import contact_flags
        return contact_flags(self.contact_wrench(), threshold)
