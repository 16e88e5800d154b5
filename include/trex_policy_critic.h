/*
 * trex_policy_critic.h - C-ABI of the privileged critic of a TrexPolicy (include/trex_policy.h, whose conventions hold here: return
 * codes, pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable). trex_policy.h
 * includes this header at its end; including either one declares both.
 *
 * An asymmetric actor-critic: the policy net keeps the row the deployed policy will see (sensor noise, latency and all), the value
 * net, which exists during training alone, reads a second row of its own - the clean observation plus whatever the simulator knows.
 *
 * Semantics (ONE definition). A policy object may have a critic width Dv, 1 <= Dv <= 126, independent of obs_dim = D.
 *   theta keeps the 13 blocks of trex_policy.h, same order, same 4-float alignment; only vf.W1 changes, to [Dv, H]
 *   (trex_policy_param_count and trex_policy_param_offsets report the layout in force).
 *   The critic has running moments of its own, f64: mean [Dv], var [Dv], count; fresh: mean 0, var 1, count 1e-4, as the
 *   observation block. trex_policy_critic_observe folds the columns [0, Dv) of a row block rows_v [N, stride_v] into them by
 *   Chan's formula, exactly as trex_policy_observe folds the observations; it reads no other column and touches neither the return
 *   statistics, the raw-reward sum nor the discounted returns.
 *   value = vf(clip((rows_v[:, :Dv] - mean_v) * rstd_v, +-clip_obs)), rstd_v = 1 / sqrt(var_v + 1e-8); the policy mean, the sample,
 *   the log-probability and obs_out come from rows exactly as in trex_policy_act.
 *   The learner takes a second rollout buffer obs_v [num_samples, Dv], the normalised critic observation the act call wrote: the
 *   value net's workgroups read it, the policy net's read obs. Loss, advantage normalisation, clipping, entropy, the ordered
 *   reduction and Adam are those of trex_policy_minibatch_step. The native learner stages 96 columns per sample and net:
 *   Dv <= 96 there (TREX_E_INVALID beyond; a caller's own autograd path still trains such a critic).
 * While a critic width is set, trex_policy_act and trex_policy_minibatch_grad / _step refuse the object by name; without one, every
 * call below but the set and the width query does.
 */
#ifndef TREX_POLICY_CRITIC_H
#define TREX_POLICY_CRITIC_H

#include "trex_policy.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Set (1 .. 126) or clear (0) the critic width. Synchronises the device; the critic moments start afresh; the learner workspace,
 * whose row stride is the parameter count, is dropped (the next minibatch call allocates: not inside a capture). The Adam step
 * count, the observation and return statistics are not touched. Another width: TREX_E_INVALID, the object unchanged. */
int trex_policy_set_critic(TrexPolicy *policy, int critic_dim, void *stream);
/* the width in force, 0 without a critic */
int trex_policy_critic_dim(const TrexPolicy *policy);

/* The critic moments, host f64: mean [Dv], var [Dv], count = 2 Dv + 1 doubles. Synchronise the stream. */
int trex_policy_critic_get_stats(TrexPolicy *policy, double *stats_host, void *stream);
int trex_policy_critic_set_stats(TrexPolicy *policy, const double *stats_host, void *stream);

/* Fold rows_v_dev [N, stride_v >= Dv] into the critic moments (two launches, stream-ordered, capturable). */
int trex_policy_critic_observe(TrexPolicy *policy, const float *rows_v_dev, int stride_v, void *stream);

/* trex_policy_act with a critic row: rows_v_dev [N, stride_v >= Dv] raw, normalised here with the critic moments;
 * obs_v_out [N, Dv] (nullable): the normalised critic row, the rollout buffer the learner reads.
 *   rows_v_dev == NULL: the policy alone - only the policy net's workgroups are launched, value_out and obs_v_out must be NULL
 *   (playing a trained policy needs no critic row).
 *   value_only != 0: only the value net's workgroups do work, only value_out is written; rows_dev, noise_dev, actions_dev may be NULL. */
int trex_policy_critic_act(TrexPolicy *policy, const float *theta_dev, const float *rows_dev, int row_stride,
                           const float *rows_v_dev, int stride_v, float clip_obs, const float *noise_dev, float *actions_dev,
                           float *obs_out, float *obs_v_out, float *act_out, float *logp_out, float *value_out, int value_only,
                           void *stream);

/* trex_policy_minibatch_grad / _step with obs_v_dev [num_samples, Dv] behind obs_dev; every other argument as there. */
int trex_policy_critic_minibatch_grad(TrexPolicy *policy, const float *theta_dev, float *grad_dev, const float *obs_dev,
                                      const float *obs_v_dev, const float *act_dev, const float *logp_dev, const float *val_dev,
                                      const float *adv_dev, const float *ret_dev, int64_t num_samples, const int64_t *perm_dev,
                                      int first, int mb, const float *adv_stats_dev, float cliprange, float ent_coef, float vf_coef,
                                      float grad_scale, float *loss_sums_dev, void *stream);
int trex_policy_critic_minibatch_step(TrexPolicy *policy, float *theta_dev, float *grad_dev, float *m_dev, float *v_dev,
                                      const float *obs_dev, const float *obs_v_dev, const float *act_dev, const float *logp_dev,
                                      const float *val_dev, const float *adv_dev, const float *ret_dev, int64_t num_samples,
                                      const int64_t *perm_dev, int first, int mb, const float *adv_stats_dev, float cliprange,
                                      float ent_coef, float vf_coef, float lr, float beta1, float beta2, float eps,
                                      float max_grad_norm, float *loss_sums_dev, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_POLICY_CRITIC_H */
