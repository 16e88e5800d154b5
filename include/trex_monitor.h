/*
 * trex_monitor.h - C-ABI of the episode monitor of a TrexBatch (include/trex_batch.h, whose conventions hold here: return codes,
 * pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable from the second call with
 * the same buffers on). trex_batch.h includes this header at its end; including either one declares both.
 */
#ifndef TREX_MONITOR_H
#define TREX_MONITOR_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- episode monitor (baselines' bench.Monitor, whose last-100 window ppo2 logs as eprewmean / eplenmean): what every episode
 * amounted to - its return, its length, why it ended, the sums of up to 64 caller-supplied columns (the reward terms' and the motion
 * terms' breakdowns) -, kept on the device. TWO launches per step (trex_batch_monitor_apply) behind the last launch that writes
 * the reward column read the rows as found and write the monitor's own state and nothing else. Nothing set: not a launch, not a
 * byte.
 *
 * Semantics (ONE definition). State per env e: ret (f64), len (i32), col[C] (f64), episodes (u32) and the env's last finished
 *   record. State per batch: a call count t (u32), total (u64: episodes finished since the set), by_reason[4] (u64) and a ring of W
 *   records, structure of arrays: return (f32), length (i32), reason (i32), env (u32: the global index env_offset + e), t (u32),
 *   cols [W][C] (f32). C = cols_a + cols_b; column c < cols_a is column c of block a, the others follow from block b.
 * One trex_batch_monitor_apply call, for env e, in this order: (1) ret += (double)reward, len += 1, col[c] += (double)cols[c];
 *   (2) if done != 0, the record {(float)ret, len, reason, env_offset + e, t, (float)col[..]} becomes the env's last record,
 *   (3) episodes[e] += 1 and (4) ret, len and col go to 0. The records of one call enter the ring in ascending e; the j-th record
 *   ever finished (0-based) lies in slot j % W. When one call finishes more than W episodes only its last W are written, each slot
 *   once. Then total += the call's count of records, all of them, and by_reason: bucket 0 counts the records with reason 0 (the
 *   episode limit, or containment), bucket 1 those with TREX_TERM_HEAD set, bucket 2 TREX_TERM_TILT, bucket 3
 *   TREX_TERM_CLEARANCE; a record with two bits set counts in both. Then t += 1.
 * Values are not validated: a NaN reward accumulates as NaN. Every sum has a fixed order: results are bitwise repeatable. */

#define TREX_MON_MAXWINDOW 65536
#define TREX_MON_MAXCOLS   64
/* the fields of the summary, f64 each; TREX_MON_SUMMARY of them, then the C column means */
#define TREX_MON_N            0   /* n = min(total, W): the valid ring entries everything below "window" is taken over */
#define TREX_MON_RET_MEAN     1   /* window: mean, minimum, maximum of the returns */
#define TREX_MON_RET_MIN      2
#define TREX_MON_RET_MAX      3
#define TREX_MON_LEN_MEAN     4   /* window: the same of the lengths */
#define TREX_MON_LEN_MIN      5
#define TREX_MON_LEN_MAX      6
#define TREX_MON_WIN_REASON   7   /* window: 4 counts, bucketed as by_reason is */
#define TREX_MON_TOTAL       11
#define TREX_MON_BY_REASON   12   /* 4 totals since the set */
#define TREX_MON_T           16
#define TREX_MON_SUMMARY     17

/* Set the monitor: window W in [1, TREX_MON_MAXWINDOW], cols_a, cols_b >= 0 with C = cols_a + cols_b <= TREX_MON_MAXCOLS;
 * env_offset: the global index of the batch's env 0. Synchronises the device, allocates, and starts every env afresh: all state
 * above zero. window 0 clears and frees (cols_a, cols_b and env_offset are then ignored). TREX_E_INVALID, the monitor in force
 * intact: window or a width out of range, env_offset + N beyond 2^32. */
int trex_batch_set_monitor(TrexBatch *batch, int window, int cols_a, int cols_b, uint32_t env_offset);
/* Once per step, behind the last launch that writes the reward column: reward_dev[e * reward_stride] and done_dev[e * done_stride]
 * are f32 - the two tail columns of the rows, or any arrays. reason_dev [N] i32, nullable: NULL is the batch's own reason buffer
 * while termination is enabled (trex_batch_set_termination), read in place with no copy, and zeros otherwise. cols_a_dev: column c
 * of env e at [e * stride_a + c], f32; cols_b_dev likewise. The caller's buffers are only read. CALLING IT TWICE FOR ONE ROW
 * COUNTS THE ROW TWICE. TREX_E_INVALID, nothing launched: no monitor set, reward_dev or done_dev NULL, a missing block whose width
 * is not 0, a stride below the width or below 1 (of a block whose width is 0 neither pointer nor stride is looked at), host memory
 * or another device's, a short buffer. */
int trex_batch_monitor_apply(TrexBatch *batch, const float *reward_dev, int reward_stride, const float *done_dev, int done_stride,
                             const int32_t *reason_dev, const float *cols_a_dev, int stride_a, const float *cols_b_dev, int stride_b,
                             void *stream);
/* The running episode of the envs with mask_dev[e] != 0 (u8 [N]; NULL: all) is abandoned: ret, len and col go to 0. Nothing is
 * recorded, nothing counted. One launch. */
int trex_batch_monitor_reset(TrexBatch *batch, const uint8_t *mask_dev, void *stream);
/* out_dev: f64 [TREX_MON_SUMMARY + C], a stream-ordered device result over the n = min(total, W) valid ring entries, laid out as
 * the TREX_MON_* indices say, then the C column means. Sums in f64. n == 0: means and extrema are NaN (baselines' safemean). One
 * launch; once per rollout, not on the hot path. */
int trex_batch_monitor_summary(TrexBatch *batch, double *out_dev, void *stream);
/* What is set: window and cols (each nullable; 0, 0 without a monitor) and stream-ordered device copies, each nullable, each
 * needing a monitor: the ring - ring_return [W], ring_length [W], ring_reason [W], ring_env [W], ring_t [W], ring_cols [W, C] -,
 * and per env ret [N] f64 and len [N] of the running episode, episodes [N], and the last finished record: last_return [N],
 * last_length [N], last_reason [N], last_t [N], last_cols [N, C] (zeros before the env's first). */
int trex_batch_monitor_info(const TrexBatch *batch, int *window, int *cols, float *ring_return_dev, int32_t *ring_length_dev,
                            int32_t *ring_reason_dev, uint32_t *ring_env_dev, uint32_t *ring_t_dev, float *ring_cols_dev, double *ret_dev,
                            int32_t *len_dev, uint32_t *episodes_dev, float *last_return_dev, int32_t *last_length_dev,
                            int32_t *last_reason_dev, uint32_t *last_t_dev, float *last_cols_dev, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_MONITOR_H */
