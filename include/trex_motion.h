/*
 * trex_motion.h - C-ABI of the motion clip of a TrexBatch (include/trex_batch.h, whose conventions hold here: return codes,
 * pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable from the second call with
 * the same buffers on). trex_batch.h includes this header at its end; including either one declares both.
 */
#ifndef TREX_MOTION_H
#define TREX_MOTION_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- motion clip (no reference counterpart): ONE clip of F frames at a fixed frame interval, shared by all envs and kept on the
 * device as F rows of the state layout of trex_batch_get_state [pos 3 | quat xyzw 4 | v 3 | w 3 | q J | qd J] in f32; a clock per
 * env; the reference state at a time (trex_batch_motion_sample); tracking terms against the reference at the env's clock, composed
 * into the reward column (trex_batch_compose_motion_reward); and reference state initialisation (trex_batch_motion_reset).
 *
 * Time -> reference (ONE definition, all f32 on the device; dt = (float)frame_dt, T = (float)((F - 1) dt), 1/dt and 1/T rounded
 * to f32 on the host, products by them instead of divisions):
 *   a time that is not > 0 (negative, NaN) counts as 0;
 *   loop == 0: tw = min(t, T), c = 0: past its end the clip holds its last frame, velocities included (they are NOT zeroed);
 *   loop != 0: c = floor(t / T) completed cycles, tw = t - c T in [0, T); the base x and y gain c * (pos[F-1] - pos[0]); z and
 *              the orientation DO NOT accumulate: a clip that turns or climbs over a cycle jumps back at the wrap;
 *   segment k = min(floor(tw / dt), F - 2), u = tw / dt - k in [0, 1];
 *   positions, q and ALL velocities: (1 - u) row[k] + u row[k + 1]. The velocities are per-frame values, continuous across knots;
 *   quaternion: shortest-arc slerp of the two rows' quaternions, normalised lerp where their dot product exceeds 0.9995;
 *   phase = tw / T in [0, 1].
 * Clock: per env a start time t0 (f32) and a step count k (i32); the env's reference time is t0 + k Ts, Ts = (float)(dt_sim *
 * substeps), the reward terms' step_seconds. trex_batch_set_motion zeroes every clock. */

/* Set the clip (host values, copied; synchronises the device; replaces the previous clip, clears the motion terms and zeroes the
 * clocks). frames_host [F, 7 + J] f64: base position, base quaternion xyzw, q in observation order. velocities_host [F, 6 + J]
 * f64 or NULL: base linear and angular world velocity, qd. NULL: derived in f64 by central differences over 2 frame_dt -
 * one-sided at the two ends of a clip that does not loop; on a looping clip frame F-1 is frame 0 of the next cycle, the
 * differences wrap and the base position carries the cycle's displacement -, the angular velocity being the world-frame rotation
 * vector of q[k+1] o q[k-1]^-1 over the time span. Every quaternion is normalised, and negated where that brings it into the
 * hemisphere of the frame before. probe_set: a set of trex_batch_set_link_probes whose K <= 8 points are the end effectors, -1 =
 * none; K is recorded, and a compose, sample or reset that finds the set with another K returns TREX_E_INVALID (set the clip
 * again). num_frames 0 clears the clip, its terms and its tables. TREX_E_INVALID, the previous clip intact: F == 1 or F > 4096, a
 * value that is not finite, a quaternion of norm 0, frame_dt <= 0, a q outside its joint's limits by more than 1e-6, a probe set
 * out of range or empty or of more than 8 probes. */
int trex_batch_set_motion(TrexBatch *batch, const double *frames_host, const double *velocities_host, int num_frames,
                          double frame_dt, int loop, int probe_set);
/* What is set: F (0: no clip), T in seconds, the number of motion terms, K (0: no end effectors). Each pointer nullable. */
int trex_batch_motion_info(const TrexBatch *batch, int *frames, double *duration, int *num_terms, int *probes);
/* The reference at time_dev [N] (NULL: each env's own clock): state_out [N, 13 + 2J], the interpolated state in the layout of
 * trex_batch_get_state (what trex_batch_set_state takes); points_out [N, K, 3], the world position of every end effector AT THE
 * REFERENCE POSE (forward kinematics over the reference q and base pose); phase_out [N]. Each output nullable, not all three;
 * points_out needs a clip with a probe set. One launch; reads only: no clock moves. */
int trex_batch_motion_sample(TrexBatch *batch, const float *time_dev, float *state_out, float *points_out, float *phase_out,
                             void *stream);

/* Tracking terms. Hats mark the reference at the env's clock; "sum_mask": over the joints j (observation order) whose bit is set
 * in `mask`, 0 = all joints.
 *   POSE            exp(-scale * sum_mask (q_j - q^_j)^2)     (hinge angles, not DeepMimic's quaternion differences)
 *   VELOCITY        exp(-scale * sum_mask (qd_j - qd^_j)^2)
 *   END_EFFECTOR    exp(-scale * sum_k |r_k - r^_k|^2), r_k: probe k relative to URDF link 0's origin in its axes - the TREX_AXES_BASE
 *                   pose columns of trex_batch_link_state -, at the actual and at the reference state: a drift of the base does not enter
 *   ROOT_POSE       exp(-scale * (|p - p^|^2 + aux * theta^2)), p the base position, theta in [0, pi] the angle of base^-1 o base^
 *   ROOT_VELOCITY   exp(-scale * (|v - v^|^2 + aux * |w - w^|^2)), the world velocities of the state layout */
#define TREX_MOT_POSE 0
#define TREX_MOT_VELOCITY 1
#define TREX_MOT_END_EFFECTOR 2
#define TREX_MOT_ROOT_POSE 3
#define TREX_MOT_ROOT_VELOCITY 4
#define TREX_MOT_KINDS 5
typedef struct TrexMotionTerm {
  int32_t  kind;
  uint32_t mask;
  float    weight, scale, aux;
} TrexMotionTerm;
/* Set up to 8 terms (host values, copied; synchronises the device) and the weight the column found keeps; allocates the held values
 * [N][T], zeroed. num_terms 0 clears. TREX_E_INVALID, the previous terms intact: no clip set, more than 8 terms, an unknown kind,
 * scale <= 0, aux < 0, a weight, scale, aux or step_weight that is not finite, a mask bit at or beyond J, END_EFFECTOR with no
 * probe set in the clip. */
int trex_batch_set_motion_reward(TrexBatch *batch, const TrexMotionTerm *terms_host, int num_terms, float step_weight);
/* Evaluate the terms for all N envs in ONE launch, at the instant of the row (the rule of trex_batch_compose_reward):
 *   a row whose done column is non-zero has the new episode's state behind it: its terms repeat the values held from the step
 *     before (zeros if none); then the env's clock goes to t0 = 0, k = 0 and its held values to zero;
 *   any other row: k += 1, then the terms at the new clock - q, qd from the row's columns [0, J), [J, 2J), the base and the end
 *     effectors from the batch's state -, then the values are held.
 * Then row[3J] = step_weight * row[3J] + sum_t weight_t v_t, an f32 sum of rounded products in term order that starts from the
 * rounded product step_weight * row[3J]; terms_dev [N, T] (nullable) receives weight_t v_t. Writes that column, terms_dev, the
 * clocks and the held values, and nothing else. Runs ONCE after a step call, behind trex_batch_compose_reward if that is used
 * and before trex_batch_compose_rows; CALLING IT TWICE FOR ONE STEP ADVANCES THE CLOCK TWICE (and composes the composed column).
 * TREX_E_INVALID, nothing launched: no terms set, a stride below 3J + 2 (3J + 5 with penalties in rows), host memory or another
 * device's, a short buffer, a probe set that no longer has the K the clip recorded. */
int trex_batch_compose_motion_reward(TrexBatch *batch, float *rows_dev, int row_stride, float *terms_dev, void *stream);
/* Reference state initialisation. For every env with mask_dev[e] != 0 (u8 [N]; NULL: all): the clip's state at time_dev[e] (NULL:
 * 0) becomes the env's state - bitwise what trex_batch_motion_sample gives -, its motors are enabled (the episode starts in
 * motion), its warm-start record, if the batch has them, is emptied, its clock becomes t0 = time (as mapped above: not > 0 is 0),
 * k = 0, its held values zero; with rows_dev, the row's columns [0, 2J) become q, qd and [2J, 3J) zeros, reward and done as found.
 * Envs outside the mask: untouched, bit for bit. ONE launch. NOT touched: the episode step count (a step launch has already
 * zeroed it for an env it reset); the contact sensor's record, which for a reset env is stale until the next step. Needs a clip;
 * terms need not be set. */
int trex_batch_motion_reset(TrexBatch *batch, const uint8_t *mask_dev, const float *time_dev, float *rows_dev, int row_stride,
                            void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_MOTION_H */
