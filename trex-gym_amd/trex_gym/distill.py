"""Policy distillation for TrexVecEnv (include/trex_policy_distill.h): the second stage of the two-stage sim-to-real recipe. A
teacher that was trained on the clean or the privileged row exists already; the student, which reads the sensors' row (`env.rows`),
is regressed onto the teacher's action distribution on states that its own rollouts visit more and more (DAgger).

    teacher = Teacher(env, "teacher.ckpt", rows="clean")       # frozen: a second policy object, its moments set once
    agent = Distill(env, teacher, loss="kl", beta=1.0, beta_decay=0.9)
    agent.learn(total_timesteps)

Per rollout step the student's act call samples and writes b_obs, the teacher's - with an all-zero noise buffer, so that its
action IS its mean - writes b_tmean and b_tval, and the env is stepped with the teacher's mean in the envs of a Bernoulli(beta)
mask drawn once per rollout and the student's sample elsewhere. The update is trex_policy_distill_minibatch_step per minibatch: the
PPO learner's three launches with another loss at the output layer. What comes out is an ordinary student: `policy.theta` and the
student's running moments, which trex_train's checkpoint stores, --play runs and trex_gym.ppo.PPO fine-tunes.

Distill is PPO's driver with another rollout and another epoch: the buffers, the graph capture of a rollout and of an epoch, the
per-rollout read-backs (mean reward, reward terms, episode monitor) are PPO's own. Single process. No training benefit is claimed:
that takes long runs nobody has made."""
import torch

from . import _capi, distill_capi
from .ppo import POLICY_MAX_OBS_DIM, PPO

ROW_CHOICES = ("clean", "critic", "rows")


def _layout_count(D, A, H=64):
    """parameters of a symmetric policy (include/trex_policy.h: 13 blocks, each on a multiple of 4 floats)"""
    o = 0
    for n in (D * H, H, H * H, H, H * A, A, D * H, H, H * H, H, H, 1, A):
        o = (o + n + 3) & ~3
    return o


class Teacher:
    """A frozen policy: a second _capi.Policy of the teacher's own obs_dim with its moments set once (trex_policy_observe is never
    called on it). source: a checkpoint path (trex_train's) or (theta, stats) - stats as _capi.Policy.get_stats gives them. rows:
    what the teacher reads - "clean" env.clean_rows (env.rows without a sensor model), "critic" env.critic_rows, "rows" env.rows,
    or a caller's [n, >= obs_dim] device tensor, read at every act."""

    def __init__(self, env, source, rows="clean", clip_obs=10.0):
        self.env, self.path, self.clip_obs = env, None, float(clip_obs)
        dev = env.device
        if isinstance(source, str):
            ck = torch.load(source, map_location=dev, weights_only=True)
            if ck.get("critic") is not None:
                raise ValueError("teacher %s was trained with a privileged critic: its parameters have that layout, not a policy's" % source)
            theta = ck["theta"]
            stats = dict(obs_mean=ck["obs_mean"].cpu().numpy(), obs_var=ck["obs_var"].cpu().numpy(), obs_count=float(ck["obs_count"]),
                         ret_mean=0.0, ret_var=float(ck["ret_var"]), ret_count=1.0)
            self.path = source
        else:
            theta, stats = source
        n, A, D = env.num_envs, int(env.action_space.shape[0]), len(stats["obs_mean"])
        if D > POLICY_MAX_OBS_DIM:
            raise ValueError("the teacher's observation is %d columns wide; the policy kernel takes at most %d" % (D, POLICY_MAX_OBS_DIM))
        if theta.numel() != _layout_count(D, A):
            other = [a for a in range(1, 33) if _layout_count(D, a) == theta.numel()]
            raise ValueError("the teacher has %s actions (%d parameters at obs_dim %d), the env %d"
                             % (other[0] if other else "another number of", theta.numel(), D, A))
        self.rows_choice = rows if isinstance(rows, str) else "tensor"
        if isinstance(rows, str):
            if rows not in ROW_CHOICES:
                raise ValueError("teacher rows %r: expected one of %s or a tensor" % (rows, ", ".join(ROW_CHOICES)))
            if rows == "critic":
                if getattr(env, "critic_rows", None) is None:
                    raise ValueError("teacher rows 'critic': the env has no critic row (trex_gym.critic.attach)")
                width = int(env.critic_rows.shape[1])
            else:
                width = int(env.observation_space.shape[0])
            if width != D:
                raise ValueError("the teacher reads %d columns, the env's %s row has %d" % (D, rows, width))
            self._tensor = None
        else:
            if not hasattr(rows, "dim") or rows.dim() != 2 or rows.shape[0] != n or rows.shape[1] < D or rows.device != dev:
                raise ValueError("teacher rows: expected a [%d, %d or more] tensor on %s" % (n, D, dev))
            self._tensor = rows
        self.obs_dim, self.act_dim = D, A
        self.kern = _capi.Policy(n, D, A, 64, dev.index)
        self.theta = theta.detach().to(dev).float().contiguous().clone()
        self.kern.set_stats(stats)
        off, _ = self.kern.layout["logstd"]
        self.logstd = self.theta[off:off + A]                 # [A] on the device: what the KL loss reads
        self.zero_noise = torch.zeros(n, A, device=dev)

    def rows(self):
        env = self.env
        if self._tensor is not None:
            return self._tensor
        if self.rows_choice == "critic":
            return env.critic_rows
        if self.rows_choice == "clean" and env.clean_rows is not None:
            return env.clean_rows
        return env.rows

    def act(self, mean_out, value_out=None, stream=None):
        """the teacher's mean [n, A] and value [n] on its row as it is now (trex_policy_act, zero noise: the action is the mean)"""
        self.kern.act(self.theta, self.rows(), self.zero_noise, mean_out, value_out=value_out, clip_obs=self.clip_obs, stream=stream)


class Distill(PPO):
    def __init__(self, env, teacher, nsteps=32, nminibatches=32, noptepochs=4, lr=3e-4, loss="kl", vf_coef=0.5, beta=1.0,
                 beta_decay=0.9, max_grad_norm=0.5, seed=0, use_graphs=False):
        """loss: "kl" (KL(teacher || student) of the two diagonal Gaussians) or "mse" (half the squared error of the means; the
        student's logstd then stays where it is). beta: the probability that an env follows the teacher's mean during a rollout,
        drawn per env once per rollout and multiplied by beta_decay after each; the mask lives in a preallocated buffer that is
        refilled outside the capture, so use_graphs captures the rollout and an epoch as PPO does."""
        if int(getattr(env, "world_size", 1)) > 1:
            raise ValueError("distillation: single process only (world_size 1): the data-parallel form is not written")
        if teacher.env is not env or teacher.act_dim != env.action_space.shape[0]:
            raise ValueError("distillation: the teacher was made for another env")
        self.kind = distill_capi.kind_of(loss)
        if self.kind not in (distill_capi.MSE, distill_capi.KL):
            raise ValueError("distillation loss %r: expected 'kl' or 'mse'" % (loss,))
        super().__init__(env, nsteps=nsteps, nminibatches=nminibatches, noptepochs=noptepochs, lr=lr, vf_coef=vf_coef,
                         max_grad_norm=max_grad_norm, seed=seed, use_graphs=use_graphs)
        self.teacher, self.loss, self.beta, self.beta_decay = teacher, loss, float(beta), float(beta_decay)
        self.distill = distill_capi.PolicyDistill(self.kern)
        T, n, ad = nsteps, env.num_envs, env.action_space.shape[0]
        self.student_actions = torch.empty(n, ad, device=self.dev)       # the student's sample of the step
        self.b_tmean = torch.empty(T, n, ad, device=self.dev)            # the teacher's mean and value on the rollout's samples
        self.b_tval = torch.empty(T, n, device=self.dev)
        self.mask = torch.zeros(n, 1, dtype=torch.bool, device=self.dev)  # True: the env follows the teacher in this rollout
        self.last_beta = self.beta

    @torch.no_grad()
    def _rollout(self):
        T, env, k, th = self.nsteps, self.env, self.kern, self.policy.theta
        self.noise.normal_()
        for t in range(T):
            k.act(th, env.rows, self.noise[t], self.student_actions, self.b_obs[t], clip_obs=self.clip_obs)
            self.teacher.act(self.b_tmean[t], self.b_tval[t])
            torch.where(self.mask, self.b_tmean[t], self.student_actions, out=self.actions)
            if self.b_terms is not None:
                env.reward_terms = self.b_terms[t]
            if self.b_motion is not None:
                env.motion_terms = self.b_motion[t]
            env.step_tensor(self.actions)
            k.observe(env.rows, True, self.gamma)       # (the student alone: the teacher's moments are frozen)
        if self.b_terms is not None:
            torch.sum(self.b_terms, dim=(0, 1), out=self.term_sum)
        if self.b_motion is not None:
            torch.sum(self.b_motion, dim=(0, 1), out=self.motion_sum)

    @torch.no_grad()
    def collect(self, mask=None):
        """One rollout. mask: an [n] or [n, 1] bool tensor to follow instead of this rollout's Bernoulli(beta) draw."""
        if mask is None:
            self.mask.copy_(torch.rand(self.mask.shape, device=self.dev) < self.beta)
        else:
            self.mask.copy_(mask.reshape(self.mask.shape))
        self.last_beta = self.beta
        self.beta *= self.beta_decay
        return super().collect()

    def _epoch(self, srcs, N, mb):
        perm = torch.rand(N, device=self.dev).argsort()
        pol, A = self.policy, self.b_tmean.shape[2]
        tlog = self.teacher.logstd if self.kind == distill_capi.KL else None
        self.loss_sums.zero_()
        for i in range(self.nminibatches):
            self.distill.minibatch_step(pol.theta, pol.grad, self.adam_m, self.adam_v, srcs[0], self.b_tmean.view(N, A), self.b_tval.view(N),
                                        tlog, perm, i * mb, mb, self.kind, self.vf_coef, self.lr, 0.9, 0.999, 1e-5, self.max_grad_norm,
                                        self.loss_sums)
        return torch.cat([self.loss_sums, self.loss_sums.new_zeros(1)])

    def update(self, batch):
        info = super().update(batch)
        return dict(policy_loss=info["policy_loss"], value_loss=info["value_loss"], beta=self.last_beta)

    def learn(self, total_timesteps, log=print):
        import time
        t0, it, history = time.perf_counter(), 0, []
        while self.total_env_steps < total_timesteps:
            batch = self.collect()
            info = self.update(batch)
            it += 1
            info.update(iteration=it, env_steps=self.total_env_steps, mean_step_reward=batch[-1],
                        env_steps_per_s=self.total_env_steps / (time.perf_counter() - t0))
            history.append(info)
            if log:
                log("it %3d  env-steps %9d  mean reward/step %12.4f  L_pi %.5f  L_vf %.5f  beta %.3f  %.0f env-steps/s"
                    % (it, info["env_steps"], info["mean_step_reward"], info["policy_loss"], info["value_loss"], info["beta"],
                       info["env_steps_per_s"]))
            stats = self.episode_stats
            if stats is not None:
                info.update(eprewmean=stats["eprewmean"], eplenmean=stats["eplenmean"], episodes=stats["episodes"],
                            end_reasons=stats["end_reasons"])
                if log:
                    log("        eprewmean %.4f  eplenmean %.2f  episodes %d" % (stats["eprewmean"], stats["eplenmean"], stats["episodes"]))
        return history
