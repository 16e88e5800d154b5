/*
 * trex_policy_distill.h - C-ABI of policy distillation on a TrexPolicy (include/trex_policy.h, whose conventions hold here: return
 * codes, pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable). trex_policy.h
 * includes this header at its end; including either one declares both.
 *
 * The second stage of the two-stage recipe ("learning by cheating"): a teacher that reads the clean or privileged row exists
 * already; the student, which reads the sensors' row, is regressed onto the teacher's action distribution on states its own
 * rollouts visit. The learner is the one of trex_policy_minibatch_step - forward on the matrix cores, analytic backward pass,
 * ordered reduction, global-norm clip, Adam - with another loss at the output layer. There is no act call here: the teacher's mean
 * and value are what trex_policy_act writes (actions_dev with an all-zero noise buffer, value_out) on a second policy object.
 *
 * Semantics (ONE definition). mu_s, V_s, ls_s: the student's mean [A], value and logstd [A] on a sample's obs row; mu_t, V_t, ls_t
 * the teacher's; sd = exp(ls). Sums run over the mb samples i of the minibatch perm[first .. first + mb) and the actions a < A.
 *   TREX_DISTILL_MSE   L_pi = (1 / mb) sum_i sum_a (mu_s - mu_t)^2 / 2
 *                      dL/dmu_s = (mu_s - mu_t) / mb;  dL/dls_s = 0 exactly (teacher_logstd is not read)
 *   TREX_DISTILL_KL    L_pi = (1 / mb) sum_i sum_a [ ls_s - ls_t + (sd_t^2 + (mu_t - mu_s)^2) / (2 sd_s^2) - 1 / 2 ]
 *                      = KL(teacher || student) of the two diagonal Gaussians
 *                      dL/dmu_s = (mu_s - mu_t) / sd_s^2 / mb;  dL/dls_s = (1 / mb) sum_i (1 - (sd_t^2 + (mu_t - mu_s)^2) / sd_s^2)
 *   both               L_vf = (1 / mb) sum_i (V_s - V_t)^2 / 2;  L = L_pi + vf_coef L_vf; no entropy term.
 *                      vf_coef == 0: the vf blocks of the gradient are exact zeros (teacher_value may then be NULL, and L_vf
 *                      is reported as 0).
 * The means are compared as the nets give them, unclipped (the env clips an action to the joint limits later).
 * Buffers: obs_dev [num_samples, D] the student's NORMALISED observations (obs_out of its act call); teacher_mean_dev
 * [num_samples, A]; teacher_value_dev [num_samples]; teacher_logstd_dev [A] (required for KL, may be NULL for MSE); perm_dev, first,
 * mb, grad_dev, grad_scale and loss_sums_dev (L_pi and L_vf are ADDED, times grad_scale) exactly as in trex_policy_minibatch_grad.
 * Limits: obs_dim <= 96 as there; a policy object with a critic width set (trex_policy_set_critic) is refused.
 */
#ifndef TREX_POLICY_DISTILL_H
#define TREX_POLICY_DISTILL_H

#include "trex_policy.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define TREX_DISTILL_MSE 0
#define TREX_DISTILL_KL 1

/* The minibatch's gradient (UNclipped) times grad_scale -> grad_dev [P]: two launches; no clip, no Adam, the step count stays. */
int trex_policy_distill_minibatch_grad(TrexPolicy *policy, const float *theta_dev, float *grad_dev, const float *obs_dev,
                                       const float *teacher_mean_dev, const float *teacher_value_dev,
                                       const float *teacher_logstd_dev, int64_t num_samples, const int64_t *perm_dev, int first,
                                       int mb, int kind, float vf_coef, float grad_scale, float *loss_sums_dev, void *stream);
/* One distillation step: that gradient, then the global-norm clip and Adam of trex_policy_minibatch_step (three launches); the
 * policy object's Adam step count advances by one. */
int trex_policy_distill_minibatch_step(TrexPolicy *policy, float *theta_dev, float *grad_dev, float *m_dev, float *v_dev,
                                       const float *obs_dev, const float *teacher_mean_dev, const float *teacher_value_dev,
                                       const float *teacher_logstd_dev, int64_t num_samples, const int64_t *perm_dev, int first,
                                       int mb, int kind, float vf_coef, float lr, float beta1, float beta2, float eps,
                                       float max_grad_norm, float *loss_sums_dev, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_POLICY_DISTILL_H */
