/*
 * trex_sensing.h - C-ABI of the sensor model of a TrexBatch (include/trex_batch.h, whose conventions hold here: return codes,
 * pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable from the second call with
 * the same buffers on). trex_batch.h includes this header at its end; including either one declares both.
 */
#ifndef TREX_SENSING_H
#define TREX_SENSING_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- sensor model (no reference counterpart): what the policy reads is the row the launches before composed, seen through
 * sensors - white noise, a bias held through an episode, a resolution, a latency of whole env-steps - and what the motors get is
 * the policy's action some env-steps late. ONE launch per step rewrites the observation columns (trex_batch_apply_sensing), one
 * more delays the actions (trex_batch_delay_actions). The step kernels see none of this; the state, the terminal observations of
 * the termination and everything the reward and motion launches read stay clean. Nothing set: not a launch, not a byte.
 *
 * Semantics (ONE definition). The batch keeps per env an episode count ep (u32) and a row count k within the episode (u32).
 *   A row is the FIRST of an episode when its done column is non-zero (the step launch reset the env), or the env was marked by
 *   trex_batch_sensing_reset, or it is the env's first apply since trex_batch_set_sensing. Then ep += 1, k = 0, and the delay of
 *   every group and the biases of the episode are drawn. Any other row: k += 1. Nothing of the old episode reaches the new one.
 *   Per covered column c of group g, with d the env's delay of g in this episode:
 *     clean   = the row's value as found
 *     delayed = the clean value of row max(k - d, 0) of this episode: a sensor holds its first reading until its delay has elapsed
 *     y       = (delayed + bias_g * b(e, ep, c)) + noise_g * z(e, ep, k, c)       every product and sum rounded to f32, no fma;
 *               a bias or noise of 0 adds nothing - not even a signed zero: such a group leaves the value bit for bit
 *     quantum_g > 0:  y = quantum_g * rintf(y * inv_quantum_g), inv_quantum = (float)(1.0 / (double)quantum) made on the host
 *   Values are not validated: a NaN passes through.
 * Random numbers: Philox4x32-10 (Salmon et al., Random123), counter-based - there is no generator state; a graph replay advances
 * only k and ep, which live on the device.
 *   key     = (low half of seed, high half of seed)
 *   counter = (env_offset + e, k, (stream << 16) | block, ep)                     e the env's index in this batch
 *   streams: TREX_SENSE_STREAM_WHITE 0 (noise), _BIAS 1 (k = 0), _DELAY 2 (k = 0, block = the group's index, output 0),
 *            _ACTION 3 (k = 0, block = 0, output 0, ep = the env's action episode count)
 *   block = c >> 2: the four outputs r0..r3 serve columns 4 block .. 4 block + 3, so the numbers of a column do not depend on
 *   how the groups are cut.
 *   u = (r >> 8) * 2^-24 in [0, 1), u' = ((r >> 8) + 1) * 2^-24 in (0, 1]; uniform noise and bias: 2u - 1 (exact in f32).
 *   Gaussian: (r0, r1) give columns 4 block and 4 block + 1 as R cosf(a) and R sinf(a), R = sqrtf(-2 logf(u'(r0))),
 *   a = 6.2831855f * u(r1) rounded to f32; (r2, r3) give the other two columns the same way. The precise logf, sinf, cosf, sqrtf.
 *   An integer in [lo, hi]: lo + mulhi32(r, hi - lo + 1). */

#define TREX_SENSE_GAUSSIAN 0
#define TREX_SENSE_UNIFORM 1
#define TREX_SENSE_KINDS 2
#define TREX_SENSE_MAXDELAY 8
#define TREX_SENSE_MAXGROUPS 64
#define TREX_SENSE_STREAM_WHITE 0
#define TREX_SENSE_STREAM_BIAS 1
#define TREX_SENSE_STREAM_DELAY 2
#define TREX_SENSE_STREAM_ACTION 3
typedef struct TrexSenseGroup {
  int32_t col0, width;            /* observation columns [col0, col0 + width) of the final row, 3J + E wide */
  int32_t noise_kind;             /* TREX_SENSE_GAUSSIAN: noise is the standard deviation; TREX_SENSE_UNIFORM: the half-width */
  float   noise;
  float   bias;                   /* half-width of a uniform offset per env and column, drawn at the start of an episode */
  float   quantum;                /* the resolution; 0: none */
  int32_t delay_min, delay_max;   /* env-steps, 0 <= delay_min <= delay_max <= TREX_SENSE_MAXDELAY; drawn per env and episode */
} TrexSenseGroup;

/* Set up to 64 groups (host values, copied; synchronises the device; replaces the previous groups and starts every env afresh:
 * ep = 0, the next applied row is a first one). Columns in no group pass through unchanged. seed: the Philox key. env_offset: the
 * global index of this batch's env 0, so that a sharded run and a whole run draw the same numbers. The history - 9 slots of the
 * columns whose group has delay_max > 0, laid out [slot][env][delayed column] - exists only while such a group is set.
 * num_groups 0 clears the groups and frees their tables; seed and env_offset are kept either way (trex_batch_delay_actions draws
 * from them). TREX_E_INVALID, the previous groups intact: more than 64 groups, a width below 1, a range outside [0, 3J + E), two
 * groups that overlap, an unknown noise_kind, a noise, bias or quantum that is negative or not finite, a quantum whose inverse
 * is not finite in f32, a delay outside [0, 8] or delay_min > delay_max, env_offset + N beyond 2^32. The groups are set for the
 * observation dimension of that moment (trex_batch_observation_dim): once it has changed, trex_batch_apply_sensing returns
 * TREX_E_INVALID until the groups are set again. */
int trex_batch_set_sensing(TrexBatch *batch, const TrexSenseGroup *groups_host, int num_groups, uint64_t seed, uint32_t env_offset);
/* Apply the groups to all N envs in ONE launch, once per step and once per reset, behind the last compose of the row: out row =
 * the covered columns as defined above, the uncovered columns and the tail (reward, done, the penalties when they ride in the
 * rows) as found. out_rows_dev == rows_dev with out_stride == row_stride (in place) is allowed, so are disjoint blocks; a partial
 * overlap is refused. Writes those 3J + E + tail columns of every out row and the batch's own sensing state, and nothing else.
 * CALLING IT TWICE FOR ONE ROW ADVANCES k TWICE. TREX_E_INVALID, nothing launched: no groups set, the observation dimension has
 * changed since the set, a stride below 3J + E + 2 (+ 5 with penalties in rows), host memory or another device's, a short buffer,
 * a partial overlap. */
int trex_batch_apply_sensing(TrexBatch *batch, const float *rows_dev, int row_stride, float *out_rows_dev, int out_stride,
                             void *stream);
/* Mark the envs with mask_dev[e] != 0 (u8 [N]; NULL: all): their next applied row is the first of an episode, and their action
 * history starts afresh at the next trex_batch_delay_actions. The counterpart of trex_batch_reward_reset. One launch. Needs
 * groups or an action delay to be set. */
int trex_batch_sensing_reset(TrexBatch *batch, const uint8_t *mask_dev, void *stream);

/* Actuation latency: every env draws d_e in [delay_min, delay_max] (env-steps, within [0, 8]) per episode, stream ACTION with the
 * seed and env_offset of the last trex_batch_set_sensing (0, 0 if never called). Allocates the action history [9][N][A], A the
 * batch's current action width (J, or 2J with stiffness actions), and starts every env afresh. 0, 0 clears and frees.
 * Synchronises the device. TREX_E_INVALID: a delay outside [0, 8], delay_min > delay_max. */
int trex_batch_set_action_delay(TrexBatch *batch, int delay_min, int delay_max);
/* ONE launch: out row e = the action row env e was given d_e calls ago in this episode; while fewer than d_e calls of the episode
 * exist, the episode's first action (a motor holds the first command; it is not fed zeros). done_prev_dev (u8 [N], nullable): the
 * done flags of the previous step; a set flag, a mark of trex_batch_sensing_reset or the env's first call starts the env's action
 * history afresh: d_e is drawn again. actions_dev, out_actions_dev [N, A]; out == actions is allowed, a partial overlap refused.
 * The caller passes out_actions_dev to the step call. TREX_E_INVALID, nothing launched: no action delay set, the action width has
 * changed since the set, the usual buffer checks. */
int trex_batch_delay_actions(TrexBatch *batch, const float *actions_dev, const uint8_t *done_prev_dev, float *out_actions_dev,
                             void *stream);
/* What is set: the number of groups, the number of delayed columns (those the history holds), the action-delay range (0, 0: none);
 * each pointer nullable. delays_dev (i32 [N, groups], nullable; needs groups): the delays the envs drew for their current episode,
 * zeros before an env's first row; action_delay_dev (i32 [N], nullable; needs an action delay): the same for the actions.
 * Stream-ordered device copies. */
int trex_batch_sensing_info(const TrexBatch *batch, int *num_groups, int *delayed_columns, int *action_delay_min,
                            int *action_delay_max, int32_t *delays_dev, int32_t *action_delay_dev, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_SENSING_H */
