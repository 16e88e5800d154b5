/*
 * trex_start_state.h - C-ABI of the start-state randomisation of a TrexBatch (include/trex_batch.h, whose conventions hold here:
 * return codes, pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable from the second
 * call with the same buffers on). trex_batch.h includes this header at its end; including either one declares both.
 */
#ifndef TREX_START_STATE_H
#define TREX_START_STATE_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- start-state randomisation (no reference counterpart): the state an episode starts IN - joint angles, joint velocities, base
 * attitude, base velocity, base position - perturbed on the device for every env whose episode has just started, and the robot
 * then optionally placed on the floor. ONE launch per step and per reset (trex_batch_apply_start_state) behind the step call
 * PERTURBS THE STATE IT FINDS - the model's start pose behind a plain reset, an instant of a motion clip behind
 * trex_batch_motion_reset - and patches the row of the new episode. The step kernels see none of this. Nothing set: not a launch,
 * not a byte.
 *
 * Semantics (ONE definition). The batch keeps per env an episode count ep (u32), as the episode randomisation does
 *   (include/trex_randomize.h). A row is the FIRST of an episode when done_dev[e * done_stride] != 0, or the env was marked by
 *   trex_batch_start_state_reset, or it is the env's first apply since trex_batch_set_start_state. Then ep += 1 and the env's state
 *   is perturbed. An env that is not starting is untouched, bit for bit.
 * Uniform value: v = lo + (hi - lo) * u, u = (r >> 8) * 2^-24 in [0, 1); every product and sum rounded to f32, no fma. lo == hi
 *   gives lo bit for bit.
 * Random numbers: Philox4x32-10 with the key and the counter of include/trex_sensing.h,
 *   counter = (env_offset + e, 0, (TREX_START_STREAM << 16) | block, ep), stream 7 beside the sensor model's 0..3 and the episode
 *   randomisation's 4..6. Term t, element i (a joint in observation order; 0 for a shared term and for every base kind) uses block
 *   8 t + (i >> 2), output i & 3: a value does not depend on which other elements the mask holds. There is no generator state: a
 *   sharded run draws what the whole run draws, a captured graph replays.
 * The operations run in this order, whatever the order of the terms; every sum and product below is rounded to f32, no fma:
 *   (1) JOINT_POSITION: q = min(max(q_found + v, lower), upper) with the model's limits;
 *   (2) JOINT_VELOCITY: qd = qd_found + v;
 *   (3) BASE_RPY: R = Rz(yaw) Ry(pitch) Rx(roll), applied about the base inertial origin - the base position the state carries -
 *       to the whole found state: with the quaternion r = (sr cp cy - cr sp sy, cr sp cy + sr cp sy, cr cp sy - sr sp cy,
 *       cr cp cy + sr sp sy) (x y z w; c, s the precise cosf, sinf of HALF the angle), quat = r (x) quat_found, renormalised
 *       (divided by its norm); the base's linear and angular world velocities become R v and R w, R the matrix of r. Without a
 *       BASE_RPY term nothing of this runs: quaternion and velocities are as found;
 *   (4) BASE_LINEAR_VELOCITY, BASE_ANGULAR_VELOCITY: v[index] += value, world axes;
 *   (5) BASE_POSITION: pos[index] += value;
 *   (6) FLOOR_CLEARANCE: last of all, on the final state: base z = (floor_z + v) - h, h the height relative to the base origin of
 *       the lowest point of the collision geometry - hull vertices, or sphere centres and capsule ends less their radius after
 *       trex_model_use_primitive_collision - with the point arithmetic and the tie rule (the earlier point wins) of
 *       trex_batch_body_clearance. A model without collision points: no shift.
 * For a starting env, rows_dev (nullable) gets columns [0, 2J) = the new q and qd in observation order, [2J, 3J) = zeros; reward
 *   and done stay as found: what trex_batch_motion_reset does. The env's warm-start record, if the batch has them, is emptied. The
 *   motors-enabled flag and the episode step count stay as the reset left them; the contact sensor's record is stale until the next
 *   step, as after trex_batch_motion_reset. NO settle substep is run again, and without a FLOOR_CLEARANCE term penetration of the
 *   floor is the caller's to avoid. */

#define TREX_START_JOINT_POSITION         0  /* mask: joints, observation order (0 = all). shared != 0: one draw for all, else one each */
#define TREX_START_JOINT_VELOCITY         1  /* the same addressing */
#define TREX_START_BASE_RPY               2  /* index: 0 roll, 1 pitch, 2 yaw (rad) */
#define TREX_START_BASE_LINEAR_VELOCITY   3  /* index: 0..2, world axes, added after the rotation */
#define TREX_START_BASE_ANGULAR_VELOCITY  4  /* index: 0..2, world axes, added after the rotation */
#define TREX_START_BASE_POSITION          5  /* index: 0..2 */
#define TREX_START_FLOOR_CLEARANCE        6  /* at most one: lo, hi the clearance of the lowest collision point (m) */
#define TREX_START_KINDS                  7
#define TREX_START_MAXTERMS              16
#define TREX_START_STREAM                 7
typedef struct TrexStartTerm { int32_t kind; uint32_t mask; int32_t index, shared; float lo, hi; } TrexStartTerm;

/* Set up to 16 terms (host values, copied; synchronises the device; replaces the previous terms) and start every env afresh:
 * ep = 0, the next applied row is a first one. num_terms 0 clears and frees the state; seed and env_offset are kept.
 * TREX_E_INVALID, the previous terms intact: more than 16 terms, an unknown kind, lo > hi or a bound that is not finite, a mask
 * bit beyond the model's joints, two terms of one kind whose masks overlap or that name the same index, two FLOOR_CLEARANCE terms,
 * an index out of range, env_offset + N beyond 2^32. */
int trex_batch_set_start_state(TrexBatch *batch, const TrexStartTerm *terms_host, int num_terms, uint64_t seed, uint32_t env_offset);
/* ONE launch for all N envs, once per step behind the step call and once per reset: done_dev[e * done_stride] is the env's done
 * flag (the done column of the rows, or any f32 array). rows_dev: nullable; the rows of the step call, row_stride floats apart.
 * Writes the state of the starting envs, their rows' first 3J columns, their warm-start records and the batch's own state, and
 * nothing else. TREX_E_INVALID, nothing launched: no terms set, done_dev NULL, done_stride < 1, rows_dev given with row_stride <
 * 3J + 2 (3J + 5 with penalties in rows), host memory or another device's, a short buffer. */
int trex_batch_apply_start_state(TrexBatch *batch, const float *done_dev, int done_stride, float *rows_dev, int row_stride, void *stream);
/* Mark the envs with mask_dev[e] != 0 (u8 [N]; NULL: all): their next applied row is the first of an episode. One launch. */
int trex_batch_start_state_reset(TrexBatch *batch, const uint8_t *mask_dev, void *stream);
/* What is set: num_terms (nullable) and stream-ordered device copies, each nullable, each needing terms:
 * values_dev [N, num_terms, 32]: the draws of each env's current episode by element - a shared term repeats its one value, a base
 *   kind and FLOOR_CLEARANCE hold theirs at element 0, elements outside the mask read 0;
 * shift_dev [N]: the z shift the floor placement applied; lowest_dev [N]: the collision point that decided it. They read 0 / -1 for
 *   an env that has not started an episode since the set, without a FLOOR_CLEARANCE term, and for a model without collision points. */
int trex_batch_start_state_info(const TrexBatch *batch, int *num_terms, float *values_dev, float *shift_dev, int32_t *lowest_dev,
                                void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_START_STATE_H */
