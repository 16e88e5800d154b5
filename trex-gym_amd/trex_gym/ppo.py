"""On-device PPO2 driver for TrexVecEnv (BASELINE config 3).

The reference trains with baselines' ppo2.learn on DummyVecEnv -> VecNormalize (trex_train.py:35-63). baselines /
TensorFlow are not installed here, so this is an equivalent that keeps the WHOLE loop in HBM: observations, actions,
advantages and the policy never leave the GPU, and the env is stepped through step_tensor() (no host sync per step).

The per-step caller work - VecNormalize's running statistics, the policy / value MLPs, the Gaussian sample and its
log-probability - runs in the hand-written HIP kernels of include/trex_policy.h (csrc/policy_step.hip, called through
csrc/capi_policy.cpp: two launches per env step instead of ~30 framework kernels), GAE(lambda) and the optimiser step (global-norm clip + Adam in
TensorFlow's form, as ppo2 applies it) in one launch each. There is no fallback: without libtrex_hip.so this module
does not import. PyTorch keeps one job: autograd over the minibatch loss, on parameters that are VIEWS into the flat
f32 vector the kernels read (weights stored [in, out]).

Kept from the reference (trex_train.py:49-61): MlpPolicy (2 x 64 tanh, separate value net, state-independent
log-std), lam 0.95, gamma 0.99, lr 3e-4, cliprange 0.2, ent_coef 0.0, nminibatches 32, VecNormalize's running
normalisation of observations and of discounted returns (clip 10). Different on purpose: nsteps (4096 steps x 4096
envs would be 16.7 M samples per batch) and noptepochs default to smaller values; both are constructor arguments and
are printed by the trainer. The arithmetic is restated in f64 by oracle/ppo_oracle.py (tests/test_gpu_policy.py).
"""
import math
import time

import torch
from torch import nn

from . import _capi

POLICY_MAX_OBS_DIM = 126     # trex_policy_create (include/trex_policy.h)
LEARNER_MAX_OBS_DIM = 96     # trex_policy_minibatch_step: the observation columns it stages per sample


class MlpPolicy(nn.Module):
    """baselines MlpPolicy: pi and vf are separate 2 x 64 tanh MLPs, diagonal Gaussian with a free log-std. The
    parameters are views into ONE flat f32 vector laid out as include/trex_policy.h says (weights [in, out]); their
    gradients are views into a second flat vector, so that the optimiser step is one kernel over both. With a privileged
    critic the layout's vf.W1 has Dv rows (critic_capi.PolicyCritic.layout) and value() takes the critic observation."""

    def __init__(self, layout, param_count, device):
        super().__init__()
        self.theta = torch.zeros(param_count, device=device)
        self.grad = torch.zeros(param_count, device=device)
        self._names = list(layout)
        for name, (off, shape) in layout.items():
            n = math.prod(shape)
            p = nn.Parameter(self.theta[off:off + n].view(shape))
            p.grad = self.grad[off:off + n].view(shape)      # autograd accumulates in place: the views stay
            self.register_parameter(name.replace(".", "_"), p)
        with torch.no_grad():
            for net, gain_out in (("pi", 0.01), ("vf", 1.0)):
                for k, gain in ((1, math.sqrt(2)), (2, math.sqrt(2)), (3, gain_out)):
                    w = self.p("%s.W%d" % (net, k))
                    w.copy_(nn.init.orthogonal_(torch.empty(w.shape[1], w.shape[0], device=device), gain).t())

    def p(self, name):
        return getattr(self, name.replace(".", "_"))

    def _mlp(self, net, x):
        h = torch.tanh(torch.addmm(self.p(net + ".b1"), x, self.p(net + ".W1")))
        h = torch.tanh(torch.addmm(self.p(net + ".b2"), h, self.p(net + ".W2")))
        return torch.addmm(self.p(net + ".b3"), h, self.p(net + ".W3"))

    def mean(self, obs):
        return self._mlp("pi", obs)

    def dist(self, obs):
        return torch.distributions.Normal(self.mean(obs), self.logstd.exp(), validate_args=False)   # the check syncs: not capturable

    def value(self, obs):
        """obs: what the value net reads - the policy's observation, or the critic observation [.., Dv] of an asymmetric layout"""
        return self._mlp("vf", obs).squeeze(-1)


def merge_running_moments(prefix, parts):
    """VecNormalize's running statistics across data-parallel ranks. All ranks start a rollout with the SAME statistics
    `prefix` = (mean, var, count); during the rollout rank r's statistics kernel folds in its own envs' observations and
    ends with parts[r] = (mean_r, var_r, count_r). The statistics of everything seen - the prefix and every rank's new
    data once - by Chan's parallel formula, in rank order (f64; the same on every rank):
      new data of rank r: n_r = count_r - c0, mean and M2 by un-merging the prefix from rank r's statistics;
      merged = prefix (+) new_0 (+) new_1 ...     with (a (+) b): delta = mean_b - mean_a, n = n_a + n_b,
               mean = mean_a + delta n_b / n, M2 = M2_a + M2_b + delta^2 n_a n_b / n."""
    import numpy as np
    m0, v0, c0 = (np.asarray(x, np.float64) for x in prefix)
    mean, M2, cnt = m0.copy(), v0 * c0, float(c0)
    for mr, vr, cr in parts:
        mr, vr, cr = np.asarray(mr, np.float64), np.asarray(vr, np.float64), float(cr)
        nb = cr - float(c0)
        if nb <= 0:
            continue
        mb_ = (cr * mr - c0 * m0) / nb                                   # mean of rank r's new data
        M2b = vr * cr - v0 * c0 - (mb_ - m0) ** 2 * c0 * nb / cr         # its sum of squared deviations
        delta = mb_ - mean
        tot = cnt + nb
        M2 = M2 + M2b + delta ** 2 * cnt * nb / tot
        mean = mean + delta * nb / tot
        cnt = tot
    return mean, M2 / cnt, cnt


def dp_minibatch_stats(adv, perm, nminibatches, mb, world, out, group=None):
    """mean and 1 / (std + 1e-8) (population std) of the advantages of every GLOBAL minibatch - this rank's share
    perm[k mb : (k + 1) mb) together with the other ranks' - from f64 sums, ONE all-reduce per epoch -> out [nminibatches, 2]."""
    import torch.distributed as dist
    a = adv[perm[: nminibatches * mb]].view(nminibatches, mb).double()
    s = torch.stack([a.sum(1), (a * a).sum(1)], 1)
    dist.all_reduce(s, group=group)
    n = float(mb * world)
    mean = s[:, 0] / n
    var = (s[:, 1] / n - mean * mean).clamp_min(0.0)
    out.copy_(torch.stack([mean, 1.0 / (var.sqrt() + 1e-8)], 1).float())


def dp_minibatch_step(kern, theta, grad, m, v, srcs, perm, first, mb, stats_row, world, group=None, cliprange=0.2, ent_coef=0.0,
                      vf_coef=0.5, lr=3e-4, max_grad_norm=0.5, loss_sums=None):
    """One data-parallel minibatch step: this rank's gradient / ranks (trex_policy_minibatch_grad), summed over the ranks (the
    one collective of the trainer: 21 112 floats), then global-norm clip + TF-form Adam on every rank (trex_policy_adam) - the
    update of the concatenated minibatch, the same on every rank."""
    import torch.distributed as dist
    obs, act, logp0, val0, adv, ret = srcs
    kern.minibatch_grad(theta, grad, obs, act, logp0, val0, adv, ret, perm, first, mb, stats_row, cliprange, ent_coef, vf_coef,
                        1.0 / world, loss_sums)
    dist.all_reduce(grad, group=group)
    kern.adam(theta, grad, m, v, lr=lr, eps=1e-5, max_grad_norm=max_grad_norm)


class PPO:
    _symmetry = (None, None, 1.0)      # (mode, mirror, sym_coef): trex_gym.symmetry.MirrorPPO sets it on the instance before this __init__ runs

    def __init__(self, env, nsteps=32, nminibatches=32, noptepochs=4, gamma=0.99, lam=0.95, lr=3e-4,
                 cliprange=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, clip_obs=10.0, clip_rew=10.0,
                 seed=0, use_graphs=False, native_learner=True, critic=None):
        """native_learner: the minibatch step is three HIP launches (trex_policy_minibatch_step: forward + analytic
        backward on the matrix cores, then ordered partial sums, then clip + Adam) instead of ~90 autograd kernels; False keeps
        the PyTorch autograd path (the f32 reference the native step is tested against).
        use_graphs: capture the whole nsteps rollout (policy kernel + env step + statistics kernel per step) and
        one epoch of minibatch updates as HIP graphs and replay them - everything launched is stream-ordered, so it
        is capture-safe (tests/test_gpu_invariants.py).
        critic: True trains an asymmetric actor-critic (include/trex_policy_critic.h): the value net reads env.critic_rows
        (trex_gym.critic.attach), normalised by running moments of its own, the policy net keeps env.rows; `b_obs_v` is the second
        rollout buffer. Single process only: the moment merge of a data-parallel run is not written. No training benefit is
        claimed: that takes long runs nobody has made.
        Mirror symmetry: trex_gym.symmetry.MirrorPPO, a subclass, sets `_symmetry` to (mode, a Mirror of this env, sym_coef)
        (include/trex_symmetry.h); its docstring says what "augment", "loss" and "both" allocate and launch. PPO itself
        allocates and launches nothing of this."""
        self.env = env
        self.dev = env.device
        # DATA-PARALLEL (BASELINE config 3 on N GPUs; SURVEY 8e: "only PPO gradient all-reduce remains"): one process per GPU, env
        # sharded as the env itself is (TrexVecEnv(rank=, world_size=)): every rank rolls out its own envs with its own replica of
        # the policy; per minibatch step the ranks SUM their gradients (one all-reduce of the flat 21 112-float vector between the
        # reduce launch and the Adam launch), per epoch the advantage statistics of the minibatches, per rollout the VecNormalize
        # moments (Chan's formula) - so that every rank applies the update of the concatenated minibatch and keeps identical
        # parameters and statistics. Unmeasured on more than one GPU.
        self.rank, self.world = int(getattr(env, "rank", 0)), int(getattr(env, "world_size", 1))
        self.group = getattr(env, "process_group", None)
        if self.world > 1 and (use_graphs or not native_learner):
            raise ValueError("the data-parallel trainer runs the native learner, eagerly (collectives inside a captured graph are not supported here)")
        self.nsteps, self.nminibatches, self.noptepochs = nsteps, nminibatches, noptepochs
        symmetry, mirror, sym_coef = self._symmetry
        if symmetry not in (None, "augment", "loss", "both"):
            raise ValueError("symmetry: expected None, \"augment\", \"loss\" or \"both\", got %r" % (symmetry,))
        if symmetry and mirror is None:
            raise ValueError("symmetry: a trex_gym.symmetry.Mirror of the env is required")
        if symmetry and self.world > 1:
            raise ValueError("symmetry: not written for the data-parallel trainer")
        if symmetry in ("loss", "both") and critic:
            raise ValueError("symmetry: the mirror loss is refused together with critic=, as distillation is")
        if symmetry and critic and getattr(mirror, "critic_table", None) is None:
            raise ValueError("symmetry: critic= needs the mirror's critic table (trex_gym.symmetry.MirrorPPO builds it)")
        self.symmetry, self.mirror, self.sym_coef = symmetry, mirror if symmetry else None, float(sym_coef)
        self._augment, self._mirror_loss = symmetry in ("augment", "both"), symmetry in ("loss", "both")
        if self._mirror_loss and not native_learner:
            raise ValueError("symmetry: the mirror loss is a launch of the native learner (native_learner=True)")
        self._steps = nminibatches * (2 if self._augment else 1)      # optimiser steps of an epoch
        self.gamma, self.lam, self.cliprange, self.lr = gamma, lam, cliprange, lr
        self.ent_coef, self.vf_coef, self.max_grad_norm = ent_coef, vf_coef, max_grad_norm
        self.clip_obs, self.clip_rew = clip_obs, clip_rew
        torch.manual_seed(seed)
        n, od, ad = env.num_envs, env.observation_space.shape[0], env.action_space.shape[0]
        # (an env with observation channels is wider than the reference's 3J = 75: the kernels' limits are met here, by name, not
        # as a refused launch inside the first update)
        if od > POLICY_MAX_OBS_DIM:
            raise ValueError("the observation is %d columns wide; the policy kernel takes at most %d" % (od, POLICY_MAX_OBS_DIM))
        if native_learner and od > LEARNER_MAX_OBS_DIM:
            raise ValueError("the observation is %d columns wide; the native learner stages at most %d per sample "
                             "(native_learner=False trains up to %d)" % (od, LEARNER_MAX_OBS_DIM, POLICY_MAX_OBS_DIM))
        self.kern = _capi.Policy(n, od, ad, 64, self.dev.index)       # VecNormalize state + the kernels
        self.crit, self.critic_dim = None, 0
        if critic:
            from . import critic_capi
            if self.world > 1:
                raise ValueError("critic: the data-parallel trainer does not merge the critic moments across ranks (world_size 1 only)")
            if getattr(env, "critic_rows", None) is None:
                raise ValueError("critic: the env has no critic row (trex_gym.critic.attach)")
            dv = int(env.critic_rows.shape[1])
            if native_learner and dv > critic_capi.LEARNER_MAX_CRITIC_DIM:
                raise ValueError("the critic row is %d columns wide; the native learner stages at most %d per sample "
                                 "(native_learner=False trains up to %d)" % (dv, critic_capi.LEARNER_MAX_CRITIC_DIM, critic_capi.MAX_CRITIC_DIM))
            self.crit, self.critic_dim = critic_capi.PolicyCritic(self.kern), dv
            self.crit.set(dv)
        lay, count = (self.crit.layout, self.crit.param_count) if self.crit else (self.kern.layout, self.kern.param_count)
        self.policy = MlpPolicy(lay, count, self.dev)
        self.adam_m = torch.zeros_like(self.policy.theta)
        self.adam_v = torch.zeros_like(self.policy.theta)
        self.use_graphs, self.native_learner = use_graphs, native_learner
        self._rollout_graph = self._update_graph = None
        self.mb_stats = torch.zeros(self._steps, 2, device=self.dev)
        self.loss_sums = torch.zeros(2, device=self.dev)
        self.total_env_steps = 0
        if self.world > 1:      # same initial parameters everywhere (seeded above), different exploration noise per rank
            import torch.distributed as dist
            dist.broadcast(self.policy.theta.data, 0, group=self.group)
            torch.manual_seed(seed + 1000003 * (self.rank + 1))
        T = nsteps
        if symmetry and (mirror.obs_dim != od or mirror.act_table.width != ad):
            raise ValueError("symmetry: the mirror's tables are %d and %d columns wide, the policy's rows %d and %d"
                             % (mirror.obs_dim, mirror.act_table.width, od, ad))
        self._rows_T = 2 * T if self._augment else T            # steps' worth of samples the learner reads
        self.noise = torch.empty(T, n, ad, device=self.dev)
        self.actions = torch.empty(n, ad, device=self.dev)
        T, T_rollout = self._rows_T, T                           # (the mirrored samples lie behind the rollout's, in every buffer)
        self.b_obs = torch.empty(T, n, od, device=self.dev)
        self.b_obs_v = torch.empty(T, n, self.critic_dim, device=self.dev) if self.crit else None   # the NORMALISED critic observation
        self.b_act = torch.empty(T, n, ad, device=self.dev)
        self.b_logp = torch.empty(T, n, device=self.dev)
        # (GAE reads the bootstrap value in row T_rollout; the augment launch behind it overwrites that row with mirrored samples)
        self.b_val = torch.empty(max(T_rollout + 1, T), n, device=self.dev)
        self.b_adv = torch.empty(T, n, device=self.dev)
        self.b_ret = torch.empty(T, n, device=self.dev)
        T = T_rollout
        self.b_rew = torch.empty(T, n, device=self.dev)          # RAW rewards; GAE applies scale[t] and the clip
        self.b_scale = torch.empty(T, device=self.dev)
        self.b_done = torch.empty(T, n, device=self.dev)
        self._raw_sum = 0.0
        if self._mirror_loss:
            # the proximal mirror target M_a mu_old(M_o s) of every sample the learner reads, the scratch of its two act calls, the
            # second gradient and the loss sums of the distillation launch
            from . import distill_capi
            self._distill = distill_capi.PolicyDistill(self.kern)
            self.b_tgt = torch.zeros(self._rows_T, n, ad, device=self.dev)
            self._rows_m = torch.zeros_like(env.rows)
            self._zero_noise = torch.zeros(n, ad, device=self.dev)
            self._mean = torch.zeros(n, ad, device=self.dev)
            self.grad_sym = torch.zeros_like(self.policy.theta)
            self.sym_sums = torch.zeros(2, device=self.dev)
        # reward terms (TrexVecEnv(rewards=...)): the weighted value of every term summed over the rollout, on the device
        rt = getattr(env, "reward_terms", None)
        self.term_names = list(getattr(env, "reward_names", [])) if rt is not None else []
        # (the env's compose launch writes each step's breakdown straight into b_terms[t]: no launch per step is added; ONE sum per
        # rollout folds them)
        self.b_terms = torch.zeros(nsteps, n, rt.shape[1], device=self.dev) if rt is not None else None
        self.term_sum = torch.zeros(rt.shape[1], device=self.dev) if rt is not None else None
        self.mean_terms = None
        # motion terms (trex_gym.motion.attach): the same, in a block of their own
        mt = getattr(env, "motion_terms", None)
        self.motion_names = list(getattr(env, "motion_names", [])) if mt is not None else []
        self.b_motion = torch.zeros(nsteps, n, mt.shape[1], device=self.dev) if mt is not None else None
        self.motion_sum = torch.zeros(mt.shape[1], device=self.dev) if mt is not None else None
        self.mean_motion = None
        self.episode_stats, self._monitor_out = None, None      # the episode monitor's window (trex_gym.monitor.attach), per rollout
        env.reset_tensor()
        self.kern.observe(env.rows, with_reward=False)           # VecNormalize.reset: the statistics see the first obs
        if self.crit:
            self.crit.observe(env.critic_rows)
        self._symmetrize()

    @property
    def obs(self):
        """The normalised observation the policy saw at the last step of the last rollout (diagnostics)."""
        return self.b_obs[self.nsteps - 1]

    def _mirror_targets(self, t):
        """b_tgt[t] = M_a mu_old(M_o s) on the rows the policy is acting on: the rows mirrored, a second act call with zero noise
        - its action IS its mean -, the mean mirrored. With the mirrored samples ("both") their target too, M_a mu_old(s): a third
        act call, on the rows themselves."""
        m, k, th = self.mirror, self.kern, self.policy.theta
        m.rows(self.env.rows, self._rows_m)
        k.act(th, self._rows_m, self._zero_noise, self._mean, clip_obs=self.clip_obs)
        m.actions(self._mean, self.b_tgt[t])
        if self._augment:
            k.act(th, self.env.rows, self._zero_noise, self._mean, clip_obs=self.clip_obs)
            m.actions(self._mean, self.b_tgt[self.nsteps + t])

    def _symmetrize(self):
        """In EVERY symmetry mode the running observation moments become those of the stream that holds every row and its image.
        "augment" needs it to mirror the stored normalised observations; "loss" needs it as much: its target M_a mu_old(M_o s)
        normalises the mirrored RAW rows, and only with symmetric moments is that the policy at the mirror image of the
        observation the learner reads - else the loss would ask a symmetric policy to be asymmetric (for symmetrize_theta'd
        parameters it would not be zero). The policy then trains under the symmetrised normalisation; a checkpoint stores it."""
        if self.symmetry:
            from . import symmetry_capi
            symmetry_capi.symmetrize_stats(self.kern, self.mirror.obs_table, self.mirror.critic_table if self.crit else None)

    @torch.no_grad()
    def _rollout(self):
        """nsteps env steps with the current policy + GAE, everything into the preallocated buffers. Per step: ONE
        policy launch (normalise, both MLPs on the matrix cores, sample, log-prob), the env's step launch, ONE
        statistics launch (VecNormalize)."""
        T, env, k, th, c = self.nsteps, self.env, self.kern, self.policy.theta, self.crit
        self.noise.normal_()
        for t in range(T):
            if c:       # (the same launch shape: the vf workgroups read the critic row and its moments)
                c.act(th, env.rows, env.critic_rows, self.noise[t], self.actions, self.b_obs[t], self.b_obs_v[t], self.b_act[t],
                      self.b_logp[t], self.b_val[t], clip_obs=self.clip_obs)
            else:
                k.act(th, env.rows, self.noise[t], self.actions, self.b_obs[t], self.b_act[t], self.b_logp[t], self.b_val[t],
                      clip_obs=self.clip_obs)
            if self._mirror_loss:
                self._mirror_targets(t)
            if self.b_terms is not None:
                env.reward_terms = self.b_terms[t]
            if self.b_motion is not None:
                env.motion_terms = self.b_motion[t]
            env.step_tensor(self.actions)       # the env clips to the joint limits (trex_env.py:147)
            k.observe(env.rows, True, self.gamma, self.b_rew[t], self.b_done[t], self.b_scale[t:t + 1])
            if c:
                c.observe(env.critic_rows)
            self._symmetrize()
        if self.b_terms is not None:
            torch.sum(self.b_terms, dim=(0, 1), out=self.term_sum)
        if self.b_motion is not None:
            torch.sum(self.b_motion, dim=(0, 1), out=self.motion_sum)
        if c:
            c.act(th, None, env.critic_rows, None, None, value_out=self.b_val[T], clip_obs=self.clip_obs, value_only=True)
        else:
            k.act(th, env.rows, None, None, value_out=self.b_val[T], clip_obs=self.clip_obs, value_only=True)
        k.gae(self.b_rew, self.b_scale, self.b_done, self.b_val, self.b_adv, self.b_ret, self.gamma, self.lam, self.clip_rew)
        if self._augment:       # ONE launch: the samples [T n, 2 T n) of the six buffers from the samples [0, T n)
            from . import symmetry_capi
            symmetry_capi.augment(self.mirror.obs_table, self.mirror.act_table, self.b_obs, self.b_act, self.b_logp, self.b_val,
                                  self.b_adv, self.b_ret, T * env.num_envs, critic_table=self.mirror.critic_table if c else None,
                                  obs_v=self.b_obs_v if c else None)

    @torch.no_grad()
    def collect(self):
        T, n = self.nsteps, self.env.num_envs
        if len(getattr(self.env, "_row_blocks", [0])) != 1:
            raise ValueError("the trainer reads env.rows in place: TrexVecEnv(row_buffers=1)")
        if self.use_graphs:
            if self._rollout_graph is None:
                torch.cuda.synchronize()
                self._rollout_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._rollout_graph):
                    self._rollout()
            self._rollout_graph.replay()
        else:
            self._rollout()
        self.total_env_steps += T * n * self.world
        if self.world > 1:
            self._merge_statistics()
        R = self._rows_T        # (T, or 2 T with the mirrored samples)
        flat = lambda x: x.reshape(R * n, *x.shape[2:])
        raw = self.kern.get_stats()["raw_reward_sum"]            # (the one host read-back per rollout)
        mean_rew, self._raw_sum = (raw - self._raw_sum) / (T * n), raw
        if self.term_sum is not None:                            # (behind that read-back: the stream is drained, one small copy)
            self.mean_terms = [x / (T * n) for x in self.term_sum.tolist()]
        if self.motion_sum is not None:
            self.mean_motion = [x / (T * n) for x in self.motion_sum.tolist()]
        mon = getattr(self.env, "monitor_api", None)
        if mon is not None:     # (the episode monitor's window: one launch and one small copy; its applies ran inside the rollout)
            self._monitor_out = mon.summary(self._monitor_out)
            summary = self._monitor_out.tolist()
            if self.world > 1:
                summary = self._merge_monitor(summary)
            from . import monitor
            self.episode_stats = monitor.stats_from_summary(summary, monitor.column_names(self.env))
        return (flat(self.b_obs), flat(self.b_act), flat(self.b_logp), flat(self.b_val[:R]), flat(self.b_adv), flat(self.b_ret),
                mean_rew)

    def _merge_statistics(self):
        """Once per rollout: every rank's VecNormalize moments (observations, returns) merged into the same statistics."""
        import numpy as np
        import torch.distributed as dist
        st = self.kern.get_stats()
        prev = getattr(self, "_stats_prefix", None)
        mine = {k: st[k] for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count") if k in st}
        everyone = [None] * self.world
        dist.all_gather_object(everyone, mine, group=self.group)
        if prev is None:      # first rollout: the statistics started from the reset's first observation on every rank
            prev = dict(obs_mean=np.zeros_like(np.asarray(st["obs_mean"], np.float64)), obs_var=np.ones_like(np.asarray(st["obs_var"], np.float64)),
                        obs_count=1e-4, ret_mean=0.0, ret_var=1.0, ret_count=1e-4)
        om, ov, oc = merge_running_moments((prev["obs_mean"], prev["obs_var"], prev["obs_count"]),
                                           [(e["obs_mean"], e["obs_var"], e["obs_count"]) for e in everyone])
        st.update(obs_mean=om, obs_var=ov, obs_count=oc)
        if "ret_count" in mine:
            rm, rv, rc = merge_running_moments((prev["ret_mean"], prev["ret_var"], prev["ret_count"]),
                                               [(e["ret_mean"], e["ret_var"], e["ret_count"]) for e in everyone])
            st.update(ret_mean=float(rm), ret_var=float(rv), ret_count=rc)
        self.kern.set_stats(st)
        self._stats_prefix = {k: (np.array(st[k], np.float64) if hasattr(st[k], "__len__") else float(st[k])) for k in mine}

    def _merge_monitor(self, summary):
        """Once per rollout, beside _merge_statistics: the window of the episode monitor is per rank; every rank's window sums,
        counts and extrema merged into one summary (trex_gym.monitor.merge_summaries)."""
        import torch.distributed as dist
        from . import monitor
        everyone = [None] * self.world
        dist.all_gather_object(everyone, list(summary), group=self.group)
        return monitor.merge_summaries(everyone)

    def _dp_minibatch_stats(self, adv, perm, mb):
        dp_minibatch_stats(adv, perm, self.nminibatches, mb, self.world, self.mb_stats, self.group)

    def dp_minibatch_step(self, srcs, perm, first, mb, stats_row):
        dp_minibatch_step(self.kern, self.policy.theta, self.policy.grad, self.adam_m, self.adam_v, srcs, perm, first, mb, stats_row,
                          self.world, self.group, self.cliprange, self.ent_coef, self.vf_coef, self.lr, self.max_grad_norm, self.loss_sums)

    def _loss(self, obs, act, logp0, val0, adv, ret, obs_v=None):
        a = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)       # numpy's std: population
        d = self.policy.dist(obs)
        logp = d.log_prob(act).sum(-1)
        ratio = (logp - logp0).exp()
        pg = torch.max(-a * ratio, -a * ratio.clamp(1 - self.cliprange, 1 + self.cliprange)).mean()
        v = self.policy.value(obs if obs_v is None else obs_v)
        vclip = val0 + (v - val0).clamp(-self.cliprange, self.cliprange)
        vf = 0.5 * torch.max((v - ret) ** 2, (vclip - ret) ** 2).mean()
        ent = d.entropy().sum(-1).mean()
        return pg - self.ent_coef * ent + self.vf_coef * vf, pg, vf, ent

    def _minibatch_step(self, obs, act, logp0, val0, adv, ret, obs_v=None):
        loss, pg, vf, ent = self._loss(obs, act, logp0, val0, adv, ret, obs_v)
        loss.backward()          # accumulates into the flat gradient vector (zeroed by the optimiser kernel)
        (self.crit or self.kern).adam(self.policy.theta, self.policy.grad, self.adam_m, self.adam_v, lr=self.lr, eps=1e-5,
                                      max_grad_norm=self.max_grad_norm)     # (with a critic: lengths of the layout in force)
        return pg.detach(), vf.detach(), ent.detach()

    def _epoch(self, srcs, N, mb):
        """One epoch: a fresh permutation, nminibatches optimiser steps (twice as many over the mirrored samples too); returns the
        summed (pg, vf, ent)."""
        perm = torch.rand(N, device=self.dev).argsort()     # (capturable: no host round trip, unlike randperm's size logic)
        if self.native_learner:
            obs, act, logp0, val0, adv, ret = srcs[:6]
            k, pol = self.kern, self.policy
            self.loss_sums.zero_()
            if self.world > 1:
                self._dp_minibatch_stats(adv, perm, mb)
                for i in range(self._steps):
                    self.dp_minibatch_step(srcs, perm, i * mb, mb, self.mb_stats[i])
                import torch.distributed as dist
                dist.all_reduce(self.loss_sums, group=self.group)
                ent = (pol.logstd.detach() + 0.5 * (math.log(2 * math.pi) + 1.0)).sum() * self._steps
                return torch.cat([self.loss_sums, ent.reshape(1)])
            k.minibatch_stats(adv, perm, self._steps, mb, self.mb_stats)
            for i in range(self._steps):
                if self.crit:
                    self.crit.minibatch_step(pol.theta, pol.grad, self.adam_m, self.adam_v, obs, srcs[6], act, logp0, val0, adv, ret,
                                             perm, i * mb, mb, self.mb_stats[i], self.cliprange, self.ent_coef, self.vf_coef, self.lr,
                                             0.9, 0.999, 1e-5, self.max_grad_norm, self.loss_sums)
                    continue
                if self._mirror_loss:
                    # PPO's gradient, the mirror loss' - sym_coef (1 / mb) sum (mu - target)^2 / 2, the distillation launch at its
                    # output layer - into a second buffer, their sum, then clip + Adam
                    k.minibatch_grad(pol.theta, pol.grad, obs, act, logp0, val0, adv, ret, perm, i * mb, mb, self.mb_stats[i],
                                     self.cliprange, self.ent_coef, self.vf_coef, 1.0, self.loss_sums)
                    self._distill.minibatch_grad(pol.theta, self.grad_sym, obs, self.b_tgt, val0, None, perm, i * mb, mb, "mse", 0.0,
                                                 self.sym_coef, self.sym_sums)
                    pol.grad.add_(self.grad_sym)
                    k.adam(pol.theta, pol.grad, self.adam_m, self.adam_v, self.lr, 0.9, 0.999, 1e-5, self.max_grad_norm)
                    continue
                k.minibatch_step(pol.theta, pol.grad, self.adam_m, self.adam_v, obs, act, logp0, val0, adv, ret, perm, i * mb, mb,
                                 self.mb_stats[i], self.cliprange, self.ent_coef, self.vf_coef, self.lr, 0.9, 0.999, 1e-5,
                                 self.max_grad_norm, self.loss_sums)
            ent = (pol.logstd.detach() + 0.5 * (math.log(2 * math.pi) + 1.0)).sum() * self._steps   # (of the updated policy)
            return torch.cat([self.loss_sums, ent.reshape(1)])
        acc = torch.zeros(3, device=self.dev)
        for k in range(self._steps):
            idx = perm[k * mb:(k + 1) * mb]
            out = self._minibatch_step(*[x.index_select(0, idx) for x in srcs])
            acc = acc + torch.stack(out)
        return acc

    def _mb(self, N):
        """the minibatch size of N samples: with the mirrored samples N is twice the rollout's and the steps are twice as many"""
        return N // self._steps

    def update(self, batch):
        obs, act, logp0, val0, adv, ret, _ = batch
        srcs = (obs, act, logp0, val0, adv, ret)
        if self.crit:       # (the critic observation of the same samples: the second rollout buffer, behind the six)
            srcs += (self.b_obs_v.reshape(-1, self.critic_dim),)
        N = obs.shape[0]
        mb = self._mb(N)
        if self.use_graphs:
            # ONE graph per epoch (a permutation + all its minibatch steps)
            if self._update_graph is None:
                self._srcs = srcs              # views of the persistent rollout buffers: same addresses every iteration
                keep = self.policy.theta.clone()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):      # warm-up outside the capture (library set-up, autograd buffers, workspace)
                    if self.native_learner:
                        self._epoch(srcs, N, mb)
                    else:
                        for _ in range(3):
                            self._minibatch_step(*[x[:mb] for x in srcs])
                    torch.rand(N, device=self.dev).argsort()
                torch.cuda.current_stream().wait_stream(side)
                with torch.no_grad():              # undo the warm-up: same parameters and a fresh Adam state
                    self.policy.theta.copy_(keep)
                    self.adam_m.zero_(); self.adam_v.zero_(); self.policy.grad.zero_()
                    self.kern.adam_reset()
                torch.cuda.synchronize()
                self._update_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._update_graph):
                    self._epoch_out = self._epoch(srcs, N, mb)
            assert all(a.data_ptr() == b.data_ptr() for a, b in zip(srcs, self._srcs)), "rollout buffers moved"
            total = torch.zeros(3, device=self.dev)
            for _ in range(self.noptepochs):
                self._update_graph.replay()
                total += self._epoch_out
        else:
            total = torch.zeros(3, device=self.dev)
            for _ in range(self.noptepochs):
                total += self._epoch(srcs, N, mb)
        pg, vf, ent = (total / (self.noptepochs * self._steps)).tolist()
        return dict(policy_loss=pg, value_loss=vf, entropy=ent)

    def learn(self, total_timesteps, log=print):
        t0 = time.perf_counter()
        it = 0
        history = []
        while self.total_env_steps < total_timesteps:
            batch = self.collect()
            info = self.update(batch)
            it += 1
            info.update(iteration=it, env_steps=self.total_env_steps, mean_step_reward=batch[-1],
                        env_steps_per_s=self.total_env_steps / (time.perf_counter() - t0))
            history.append(info)
            if log:
                log("it %3d  env-steps %9d  mean reward/step %12.4f  pg %.4f  vf %.4f  ent %.3f  %.0f env-steps/s"
                    % (it, info["env_steps"], info["mean_step_reward"], info["policy_loss"], info["value_loss"],
                       info["entropy"], info["env_steps_per_s"]))
            if self.mean_terms is not None:
                info["reward_terms"] = dict(zip(self.term_names, self.mean_terms))
            if self.mean_motion is not None:
                info["motion_terms"] = dict(zip(self.motion_names, self.mean_motion))
            if log and (self.mean_terms is not None or self.mean_motion is not None):   # (the motion terms beside the reward terms)
                both = list(info.get("reward_terms", {}).items()) + list(info.get("motion_terms", {}).items())
                log("        reward terms/step  " + "  ".join("%s %.4g" % kv for kv in both))
            stats = self.episode_stats
            if stats is not None:       # (baselines' eprewmean / eplenmean, and why the window's episodes ended)
                info.update(eprewmean=stats["eprewmean"], eplenmean=stats["eplenmean"], episodes=stats["episodes"],
                            end_reasons=stats["end_reasons"])
                if log:
                    log("        eprewmean %.4f  eplenmean %.2f  episodes %d  ended by  " % (stats["eprewmean"], stats["eplenmean"], stats["episodes"])
                        + "  ".join("%s %.3f" % kv for kv in stats["end_reasons"].items()))
        return history
