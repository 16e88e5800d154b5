// Trainer (include/trex_policy.h, trex_policy_critic.h, trex_policy_distill.h): the kernel argument blocks and the launches that
// capi_policy.cpp shares with policy_step.hip and ppo_learner.hip. A launcher computes its grid, block and LDS bytes from the
// block it is given and returns the launch's error; the limits and the parameter layout are policy_limits.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_limits.h"

// ---------------------------------------------------------------- policy_step.hip
struct ActArgs {
  const float *theta, *rows, *norm, *noise;
  float *actions, *obs_out, *act_out, *logp_out, *value_out;
  int n, row_stride, value_only;
  float clip_obs;
  trex_policy::PolicyLayout lay;
};
// With a privileged critic (include/trex_policy_critic.h) the value net has a row block, a width, moments and a rollout copy of its
// own: a per-net choice of pointers and of D in the vf workgroups (CRITIC = true). The plain launch is the CRITIC = false instantiation,
// whose argument block and instructions are the ones it had before the template (profiles/r31_critic.txt).
struct ActArgsV : ActArgs {
  const float *rows_v, *norm_v;
  float *obs_v_out;
  int stride_v, Dv;
};

// stats (f64): [0, D) obs mean, [D, 2D) obs var, [2D] obs count, [2D+1] ret mean, [2D+2] ret var, [2D+3] ret count,
//              [2D+4] sum of raw rewards.  norm (f32): [0, D) mean, [D, 2D) 1/sqrt(var + eps), [2D] reward scale.
struct ObserveArgs {
  const float *rows;
  double *stats, *partial;     // partial [G][D + 2][2]: per workgroup and column: sum and sum of squares about the running mean
  float *norm, *ret, *raw_rew_out, *done_out, *rew_scale_out;
  unsigned *counter;           // null: no kernel has read it since round 4. Kept: without it every member behind it moves in the argument block
  int n, row_stride, D, with_reward;
  float gamma, epsilon;
};

// (host side only: the two kernels take these member by member)
struct GaeArgs {
  const float *raw_rew, *scale, *done, *val;
  float *adv, *ret;
  int T, n;
  float gamma, lam, clip_rew;
};
struct AdamArgs {
  float *theta, *grad, *m, *v;
  int P, *step;
  float lr, b1, b2, eps, max_norm, *norm_out;
};

extern "C" hipError_t trex_launch_policy_act(const ActArgs &args, hipStream_t stream);
// both nets, or the policy alone when the block names no critic rows
extern "C" hipError_t trex_launch_policy_critic_act(const ActArgsV &args, hipStream_t stream);
// the observe pair: the per-workgroup partial sums of ceil(n / OBS_ROWS) workgroups, then their merge
extern "C" hipError_t trex_launch_policy_observe(const ObserveArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_policy_refresh_norm(const double *stats, float *norm, int D, float epsilon, hipStream_t stream);
extern "C" hipError_t trex_launch_policy_gae(const GaeArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_policy_adam(const AdamArgs &args, hipStream_t stream);

// ---------------------------------------------------------------- ppo_learner.hip
struct LearnArgs {
  const float *theta, *obs, *act, *logp0, *val0, *adv, *ret;
  const long long *perm;
  const float *adv_stats;      // [2]: mean and 1 / (std + 1e-8) of the minibatch's advantages
  float *partial;              // [tiles][stride]
  int first, mb, stride;
  float cliprange, vf_coef;
  trex_policy::PolicyLayout lay;
};
// With a privileged critic (include/trex_policy_critic.h) the vf workgroups read a rollout buffer and a width of their own (CRITIC =
// true); the plain launch is the CRITIC = false instantiation, the kernel as it was before the template (profiles/r31_critic.txt).
struct LearnArgsV : LearnArgs {
  const float *obs_v;
  int Dv;
};
// LOSS_DISTILL (include/trex_policy_distill.h) regresses onto a teacher - `act` carries the teacher's mean, `ret` its value, and
// logp0 / val0 / adv / adv_stats are null and never loaded.
struct LearnArgsD : LearnArgs {
  const float *teacher_logstd;   // [A] (MSE: any A readable floats, not used)
  int kind;                      // TREX_DISTILL_MSE / _KL
  int has_value;                 // 0: `ret` is a stand-in address, the value head's target is its own output
};

struct ApplyArgs {
  const float *partial;
  float *theta, *grad, *m, *v, *losses;     // losses [2]: running sums of the surrogate / value loss MEANS per minibatch
  double *red;                              // [LEARN_RED_DOUBLES]: the workgroups' partial squared norms, the Adam step size last
  unsigned *counter;                        // null: no kernel has read it since round 4. Kept: see ObserveArgs
  int *step;
  int tiles, stride, count, logstd_off, A;
  float ent_coef, lr, b1, b2, eps, max_norm, inv_mb;
  float grad_scale;      // the gradient (entropy term included) and the loss sums are multiplied by this: 1 / ranks for a data-parallel step
  int advance;           // != 0: workgroup 0 advances the Adam step count and forms its step size (the Adam launch follows)
};

extern "C" hipError_t trex_launch_policy_adv_stats(const float *adv, const long long *perm, int num_minibatches, int mb, float *out,
                                                   hipStream_t stream);
// learn_grad_kernel on ceil(mb / TILE) tiles of both nets: the plain, the critic and the distillation instantiation
extern "C" hipError_t trex_launch_policy_learn_grad(const LearnArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_policy_learn_grad_critic(const LearnArgsV &args, hipStream_t stream);
extern "C" hipError_t trex_launch_policy_learn_grad_distill(const LearnArgsD &args, hipStream_t stream);
// the partial rows -> the gradient; then the clip and Adam (the same block)
extern "C" hipError_t trex_launch_policy_learn_reduce(const ApplyArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_policy_learn_adam(const ApplyArgs &args, hipStream_t stream);
