/*
 * trex_reward.h - C-ABI of the reward terms of a TrexBatch (include/trex_batch.h, whose conventions hold here: return codes,
 * pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable from the second call with
 * the same buffers on). trex_batch.h includes this header at its end; including either one declares both.
 */
#ifndef TREX_REWARD_H
#define TREX_REWARD_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- reward terms (no reference counterpart: the reference's reward is its three terms alone, trex_batch_set_reward_weights):
 * a specification of up to 32 terms, evaluated on the device by ONE more launch per step at the instant of the row, and composed
 * into the reward column the step wrote:
 *   rows row e [3J] = sum over t of weight_t * v_t   (f32, in term order, starting from the first product: a lone STEP term of
 *                                                    weight 1 leaves the column bitwise as it was)
 *   terms_dev [e][t] = weight_t * v_t                (the breakdown, if asked for)
 * row: the env's row as the step call wrote it, q, qd, tau its columns [0, J), [J, 2J), [2J, 3J); v, w, g: linear and angular
 * velocity of URDF link 0 and the projected gravity, in base axes, exactly the BASE_LINEAR_VELOCITY, BASE_ANGULAR_VELOCITY and
 * PROJECTED_GRAVITY observation channels; h: the BASE_HEIGHT / POINT_HEIGHT channel; f_b: the contact sensor's force on body b;
 * Ts = dt * substeps; c: the env's command (vx, vy in base axes, yaw rate). "sum_mask": over the joints j (observation order) whose
 * bit is set in `mask`, 0 = all joints.
 *   STEP            row[3J] as found: the reference reward, less any fall penalty
 *   ALIVE           1
 *   TRACK_LIN_VEL   exp(-((v_x - c0)^2 + (v_y - c1)^2) / p0), p0 > 0
 *   TRACK_ANG_VEL   exp(-(w_z - c2)^2 / p0), p0 > 0
 *   LIN_VEL_Z       v_z^2
 *   ANG_VEL_XY      w_x^2 + w_y^2
 *   ORIENTATION     g_x^2 + g_y^2
 *   BASE_HEIGHT     (h_base - p0)^2
 *   POINT_HEIGHT    (h(link, local_xyz) - p0)^2
 *   TORQUE          sum_mask tau_j^2
 *   JOINT_VEL       sum_mask qd_j^2
 *   JOINT_ACC       sum_mask ((qd_j - qd_prev_j) / Ts)^2
 *   ACTION_RATE     sum over all A action columns of (a - a_prev)^2, the actions as passed (not clipped)
 *   JOINT_LIMIT     sum_mask max(0, lo_j + m_j - q_j) + max(0, q_j - (hi_j - m_j)), m_j = (1 - p0) (hi_j - lo_j) / 2, 0 < p0 <= 1
 *   POWER           sum_mask |tau_j qd_j|
 *   JOINT_POSE      sum_mask (q_j - q_start_j)^2, q_start the model's start angles
 *   CONTACT_COUNT   the number of moving bodies b with bit b of `mask` set and |f_b| > p0
 *   FOOT_AIR_TIME   for the body of `link`, contact meaning f_b.z > p0: a timer per env and term gains Ts on a step without
 *                   contact; on the first step with contact after air v = timer - p1 and the timer is zeroed; otherwise v = 0
 *   FOOT_SLIP       [f_b.z > p0] * |world xy velocity of the point (link, local_xyz)|^2
 * History - per env the previous actions, the previous qd, one timer and the last evaluated v_t per term, a valid flag - belongs to
 * the batch; trex_batch_set_reward allocates it, zeroed, for the terms it sets. Rules:
 *   1. a row whose done column is non-zero: the state behind it is already the new episode's, so every term but STEP repeats the
 *      value it had on the step before (zeros if none) and STEP comes from the row; then the env's history is invalidated: flag 0,
 *      timers 0;
 *   2. any other row: the terms are evaluated, JOINT_ACC and ACTION_RATE being 0 while the flag is 0; then the actions, qd and the
 *      v_t are stored and the flag is set;
 *   3. trex_batch_reward_reset invalidates the history of the envs with mask != 0 (NULL: all envs) and zeroes their held values;
 *   4. nothing else touches history: not trex_batch_set_state, not trex_batch_set_domain.
 * trex_batch_compose_reward runs ONCE after a step call, on the rows that call wrote; CALLING IT TWICE FOR ONE STEP ADVANCES THE
 * HISTORY TWICE (and composes the already composed column). With observation channels it runs before trex_batch_compose_rows,
 * which then carries the new reward along in the tail. */
#define TREX_REW_STEP 0
#define TREX_REW_ALIVE 1
#define TREX_REW_TRACK_LIN_VEL 2
#define TREX_REW_TRACK_ANG_VEL 3
#define TREX_REW_LIN_VEL_Z 4
#define TREX_REW_ANG_VEL_XY 5
#define TREX_REW_ORIENTATION 6
#define TREX_REW_BASE_HEIGHT 7
#define TREX_REW_POINT_HEIGHT 8
#define TREX_REW_TORQUE 9
#define TREX_REW_JOINT_VEL 10
#define TREX_REW_JOINT_ACC 11
#define TREX_REW_ACTION_RATE 12
#define TREX_REW_JOINT_LIMIT 13
#define TREX_REW_POWER 14
#define TREX_REW_JOINT_POSE 15
#define TREX_REW_CONTACT_COUNT 16
#define TREX_REW_FOOT_AIR_TIME 17
#define TREX_REW_FOOT_SLIP 18
#define TREX_REW_KINDS 19
typedef struct TrexRewardTerm {
  int32_t  kind, link;     /* link: URDF link index where the kind names one */
  uint32_t mask;           /* joint-sum kinds: bit j = joint j in observation order, 0 = all joints;
                              CONTACT_COUNT: bit b = moving body b */
  float    local_xyz[3];   /* a point in the link's frame where the kind names one */
  float    weight, p0, p1;
} TrexRewardTerm;
/* Set the batch's reward terms (host values, copied; synchronises the device; replaces the previous set and starts its history
 * afresh); num_terms 0 clears. ACTION_RATE takes the batch's action width of this moment. TREX_E_INVALID, the previous set intact:
 * an unknown kind, a link out of range, a weight, p0, p1 or local_xyz that is not finite, p0 <= 0 on a tracking term, p0 outside
 * (0, 1] on JOINT_LIMIT, a mask bit at or beyond J (CONTACT_COUNT: at or beyond the body count), more than 32 terms. */
int trex_batch_set_reward(TrexBatch *batch, const TrexRewardTerm *terms_host, int num_terms);
/* T, the number of terms set; 0 while none are */
int trex_batch_reward_terms(const TrexBatch *batch);
/* Evaluate the terms (above) for all N envs: rows_dev is what a step call wrote (row e at + e * row_stride, row_stride >= 3J +
 * tail), actions_dev [N, A] the actions of that step (nullable unless ACTION_RATE is set), command_dev [N, 3] (nullable unless a
 * tracking term is set), terms_dev [N, T] (nullable). One launch, asynchronous on `stream`, capturable from the second call with
 * the same buffers on. Writes column 3J of every row, terms_dev and the batch's reward history, and nothing else: not the other
 * columns, not the state, not the contact sensor. TREX_E_INVALID, nothing launched: no terms set, a stride too small, a contact
 * kind (CONTACT_COUNT, FOOT_AIR_TIME, FOOT_SLIP) with the sensor off, a missing command_dev or actions_dev that a term needs, host
 * memory or another device's, a short buffer, an action width that is no longer the one the terms were set with. */
int trex_batch_compose_reward(TrexBatch *batch, float *rows_dev, int row_stride, const float *actions_dev,
                              const float *command_dev, float *terms_dev, void *stream);
/* Rule 3 above: mask_dev [N] u8 (nullable = all envs). TREX_E_INVALID while no terms are set. */
int trex_batch_reward_reset(TrexBatch *batch, const uint8_t *mask_dev, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_REWARD_H */
