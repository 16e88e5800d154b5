"""A sampling-based planner around a TrexVecEnv: MPPI, or predictive sampling with temperature 0 (include/trex_planner.h states the
arithmetic; planner_capi.PlannerHandle binds it). `plant` holds the G robots that are controlled; the planner builds a sim env of
its own with G K envs on the same model, engine parameters and control mode, and per control step copies every robot's state into
its K sample envs, perturbs the nominal action sequence K ways, rolls all of them out open-loop, averages the sequences by their
returns, plays the first action and shifts.

Deviations: there is no pybullet counterpart. The sim env runs without an episode limit and with a cold solve (warmstart 0: a
warm-start record is not part of get_state, so a warm sim could not start where the plant is); its model is the planner's own
copy - set_domain / set_motor_gains below set the SIM's, the plant keeps whatever its owner gave it. Nothing here claims control
quality."""
import numpy as np
import torch

from . import _capi, planner_capi
from .vec_env import TrexVecEnv

ROLLOUTS = ("many", "steps")
_OPEN_LOOP_REFUSES = ("observations", "rewards", "external")      # what step_many_tensor has no per-step launch for


class Planner:
    def __init__(self, plant, samples, horizon, knots=None, interpolation="cubic", sigma=0.1, temperature=0.1, gamma=1.0, iterations=1,
                 seed=0, terminal_value=None, rollout="many", use_graphs=False, sim_kwargs=None):
        """plant: a TrexVecEnv of G envs (stepped by step() only; plan() reads its state). samples K, horizon S, knots P (default
        min(S, 6)), interpolation "hold" / "linear" / "cubic". sigma: a scalar or [A], the noise of a knot; the knots are clipped
        to the plant's action space. temperature 0: predictive sampling. iterations: sample - rollout - update rounds per plan().
        terminal_value: a callable rows [N, row width] -> [N] f32 on the device, the value of the state behind the last step
        (e.g. a trex_gym.distill.Teacher's value), discounted by gamma^S and added where no step was done.
        rollout "many": one step_many_tensor launch and the step's own reward. rollout "steps": S step_tensor calls on a sim env
        built with sim_kwargs - observations=, rewards=, terminate= of TrexVecEnv -, whose composed reward and done columns are
        copied into [S, N] buffers: the reward terms can be the cost. sim_kwargs may also carry collisions_dir= and
        primitive_max_radius=, which a TrexVecEnv does not keep. use_graphs: one planning iteration is captured during the second
        one and replayed from then on."""
        if rollout not in ROLLOUTS:
            raise ValueError("rollout %r: expected one of %s" % (rollout, ROLLOUTS))
        sim_kwargs = dict(sim_kwargs or {})
        if rollout == "many":
            bad = [k for k in _OPEN_LOOP_REFUSES if sim_kwargs.get(k) is not None]
            if bad:
                raise ValueError("rollout='many' with sim_kwargs %s: step_many_tensor has no per-step compose - use rollout='steps'" % bad)
        if int(iterations) < 1:
            raise ValueError("iterations: at least 1")
        self.plant, self.rollout, self.iterations = plant, rollout, int(iterations)
        self.G, self.K, self.S = plant.num_envs, int(samples), int(horizon)
        self.P = min(self.S, 6) if knots is None else int(knots)
        self.A, self.N = plant.A, self.G * self.K
        self.temperature, self.gamma, self.terminal_value = float(temperature), float(gamma), terminal_value
        self.device = plant.device
        self.handle = planner_capi.PlannerHandle(self.G, self.K, self.S, self.P, self.A, interpolation, self.device.index)
        params = {name: plant.model.get_param(name) for name in _capi.PARAM_NAMES}      # (warmstart stays 0: the cold solve)
        self.sim = TrexVecEnv(self.N, urdf_path=plant.model.urdf_path, device=self.device, params=params, collision=plant.collision,
                              control_mode=plant.control_modes, variable_stiffness=plant.variable_stiffness, kp_max=plant.kp_max,
                              max_episode_steps=None, penalties_in_rows=True, **sim_kwargs)
        if self.sim.batch.state_width != plant.batch.state_width or self.sim.A != self.A:
            raise ValueError("the sim env's state or action width (%d, %d) is not the plant's (%d, %d)"
                             % (self.sim.batch.state_width, self.sim.A, plant.batch.state_width, self.A))
        self.sim.reset_tensor()
        lo, hi = plant.action_space.low, plant.action_space.high
        self.handle.set_noise(sigma, lo, hi, seed, plant.env_lo * self.K)
        dev, f32 = self.device, torch.float32
        self.actions = torch.zeros(self.S, self.N, self.A, device=dev)
        self.returns, self.weights = torch.zeros(self.N, device=dev), torch.zeros(self.N, device=dev)
        self.best, self.stats = torch.zeros(self.G, dtype=torch.int32, device=dev), torch.zeros(self.G, 4, device=dev)
        self._state = torch.zeros(self.G, plant.batch.state_width, device=dev)
        self._sim_state = torch.zeros(self.N, plant.batch.state_width, device=dev)
        self._action = torch.zeros(self.G, self.A, device=dev)
        self._terminal = None if terminal_value is None else torch.zeros(self.N, device=dev, dtype=f32)
        W = self.sim.rows.shape[1]
        if rollout == "many":
            self.rows = torch.zeros(self.S, self.N, W, device=dev)
            col = 3 * self.sim.J
            flat = self.rows.view(-1)
            self._reward, self._done, self._strides = flat[col:], flat[col + 1:], (self.N * W, W)
        else:
            self.rows = None
            self._reward, self._done = torch.zeros(self.S, self.N, device=dev), torch.zeros(self.S, self.N, device=dev)
            self._strides = (self.N, 1)
        self.use_graphs, self._graph, self._iterations_run = bool(use_graphs), None, 0

    # ---- one planning iteration: state -> sample -> rollout -> update (every buffer preallocated: capturable)
    def _iterate(self):
        self.plant.batch.get_state(self._state)
        self._sim_state.view(self.G, self.K, -1).copy_(self._state[:, None, :])
        self.sim.set_state(self._sim_state, motors_enabled=True)
        self.handle.sample(self.actions)
        if self.rollout == "many":
            self.sim.step_many_tensor(self.actions, self.rows)
            last = self.rows[-1]
        else:
            for s in range(self.S):
                self.sim.step_tensor(self.actions[s])
                self._reward[s].copy_(self.sim.rew)
                self._done[s].copy_(self.sim.done_f)
            last = self.sim.rows
        if self._terminal is not None:
            self._terminal.copy_(self.terminal_value(last).reshape(self.N))
        self.handle.update(self._reward, self._strides[0], self._strides[1], self._done, self._terminal, self.gamma, self.temperature,
                           self.returns, self.weights, self.best, self.stats)

    def plan(self):
        """`iterations` rounds from the plant's current state; afterwards `returns`, `weights` [N], `best` [G] and `stats` [G, 4]
        (R_max, mean return, effective sample size, the nominal's return) hold the last round's. Returns stats."""
        for _ in range(self.iterations):
            if not self.use_graphs or self._iterations_run == 0:
                self._iterate()                       # (the first one is always eager: tables are built, buffers are learnt)
            else:
                if self._graph is None:
                    torch.cuda.synchronize()
                    side, self._graph = torch.cuda.Stream(device=self.device), torch.cuda.CUDAGraph()
                    with torch.cuda.stream(side):
                        with torch.cuda.graph(self._graph, stream=side):
                            self._iterate()
                self._graph.replay()
            self._iterations_run += 1
        return self.stats

    def action(self, step=0):
        """[G, A]: the nominal's clipped action at `step` (a buffer the next call overwrites)"""
        return self.handle.action(self._action, step)

    def shift(self, steps=1):
        self.handle.shift(steps)

    def step(self):
        """plan(), play the first action on the plant, shift by one step -> what plant.step_tensor returned"""
        self.plan()
        out = self.plant.step_tensor(self.action(0))
        self.shift(1)
        return out

    def record(self, steps):
        """`steps` calls of step(): the plant's states BEFORE each [T, G, state width], for trex_gym.motion.Clip.from_states"""
        states = []
        for _ in range(int(steps)):
            states.append(self.plant.get_state())
            self.step()
        return torch.stack(states)

    @property
    def nominal(self):
        return self.handle.get_nominal()

    def _expand(self, t, name):
        if t is None:
            return None
        t = torch.as_tensor(np.asarray(t, np.float32)) if not isinstance(t, torch.Tensor) else t
        if t.dim() < 1 or t.shape[0] != self.G:
            raise ValueError("%s: expected [%d, ...] - one row per plant env -, got shape %s" % (name, self.G, tuple(t.shape)))
        return t.to(self.device, torch.float32).repeat_interleave(self.K, 0).contiguous()

    def set_domain(self, mass_scale=None, friction=None):
        """The SIM's domain: mass_scale [G, num_bodies], friction [G], each robot's row for its K samples"""
        self.sim.set_domain(self._expand(mass_scale, "mass_scale"), self._expand(friction, "friction"))

    def set_motor_gains(self, kp=None, kd=None, max_force=None):
        """The SIM's motor gains: each [G, J] (None: the model parameter), each robot's row for its K samples"""
        self.sim.set_motor_gains(self._expand(kp, "kp"), self._expand(kd, "kd"), self._expand(max_force, "max_force"))

    def close(self):
        self._graph = None
        self.handle.close()
        self.sim.close()
