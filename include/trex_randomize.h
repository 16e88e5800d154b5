/*
 * trex_randomize.h - C-ABI of the episode randomisation of a TrexBatch (include/trex_batch.h, whose conventions hold here: return
 * codes, pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable from the second call
 * with the same buffers on). trex_batch.h includes this header at its end; including either one declares both.
 */
#ifndef TREX_RANDOMIZE_H
#define TREX_RANDOMIZE_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- episode randomisation (no reference counterpart): what a training loop redraws when an episode starts - mass scale,
 * friction, motor gains - or at an interval inside it - pushes, the velocity command -, drawn on the device. ONE launch per step
 * (trex_batch_apply_randomization) reads the rows' done column and writes the buffers the step launches already read; the step
 * kernels themselves see none of this. Nothing set: not a launch, not a byte.
 *
 * Semantics (ONE definition). The batch keeps per env an episode count ep (u32) and a row count k within the episode (u32), as
 *   the sensor model does (include/trex_sensing.h). A row is the FIRST of an episode when done_dev[e * done_stride] != 0, or the env
 *   was marked by trex_batch_randomization_reset, or it is the env's first apply since trex_batch_set_randomization. Then ep += 1,
 *   k = 0, push_left = 0. Any other row: k += 1.
 * Uniform value: v = lo + (hi - lo) * u, u = (r >> 8) * 2^-24 in [0, 1); every product and sum rounded to f32, no fma. lo == hi
 *   gives lo bit for bit.
 * Random numbers: Philox4x32-10 with the key and the counter of include/trex_sensing.h,
 *   counter = (env_offset + e, k, (stream << 16) | block, ep), and three streams beside the sensor model's 0..3:
 *   TREX_RAND_STREAM_EPISODE 4: first rows only, k = 0. Term t, element i (a body, or a joint in observation order; 0 for a shared
 *     term, for FRICTION and for COMMAND) uses block 8 t + (i >> 2), output i & 3: a value does not depend on which other elements
 *     the mask holds. A PUSH term draws its phase off = draw_int(r0 of block 8 t, 0, interval - 1) here; a COMMAND term its first
 *     value: r0 the zero test, r1 the value.
 *   TREX_RAND_STREAM_PUSH 5: at the row's k, block t. r0 the start test u < probability, r1 the angle, r2 the magnitude.
 *   TREX_RAND_STREAM_COMMAND 6: at the row's k, block t; used at rows with k > 0, interval > 0 and k % interval == 0. r0 the zero
 *     test (u < probability gives the value +0), r1 the value.
 * MASS, FRICTION: a first row writes v into the env's mass scale / friction coefficient (what trex_batch_set_domain sets).
 * KP, KD, MAX_FORCE: a first row writes nominal * v for the covered joints (a negative product as 0, as trex_batch_set_motor_gains
 *   does). The nominal is a device snapshot of the batch's gains taken at trex_batch_set_randomization: the model parameters if
 *   none were set. A LATER trex_batch_set_motor_gains WRITES THE LIVE BUFFER AS ALWAYS; FOR COVERED JOINTS IT IS OVERWRITTEN FROM
 *   THE SNAPSHOT AT THE ENV'S NEXT EPISODE START.
 * PUSH: row k's launch decides the wrench of the step that follows row k, in this order: (1) on a first row push_left = 0;
 *   (2) otherwise, if push_left > 0, push_left -= 1; (3) if push_left == 0 and (k + off) % interval == 0, draw: on a start
 *   a = 6.2831855f * u(r1), m the uniform value of r2, force = (m cosf(a), m sinf(a), 0) with the precise functions, push_left =
 *   duration. A push acts on exactly `duration` steps and ends with its episode. The push body's six columns of the wrench the step
 *   launches read hold base + (push_left > 0 ? force : 0): force at the body's COM, world axes, no torque; base what the caller last
 *   set through trex_batch_set_external_wrench (zeros if nothing), which keeps a copy of the push bodies' columns while push terms
 *   are set; a NULL wrench then makes the base zeros and leaves the wrench switched on.
 * COMMAND: component `index` of command_dev[e] is written on first rows and at the resample rows, and at no other row. */

#define TREX_RAND_MASS       0  /* mask: bodies (0 = all). shared != 0: one draw for all, else one per body. mass_scale[e][b] = v */
#define TREX_RAND_FRICTION   1  /* friction[e] = v (the coefficient itself) */
#define TREX_RAND_KP         2  /* mask: joints, observation order (0 = all); shared as above; gain = nominal * v */
#define TREX_RAND_KD         3
#define TREX_RAND_MAX_FORCE  4
#define TREX_RAND_PUSH       5  /* index: body; lo, hi: magnitude (N); interval, duration (env-steps); probability */
#define TREX_RAND_COMMAND    6  /* index: component 0..2 of command_dev; lo, hi; interval (0: per episode only); probability of an exact 0 */
#define TREX_RAND_KINDS      7
#define TREX_RAND_MAXTERMS  16
#define TREX_RAND_MAXPUSHES  4
#define TREX_RAND_STREAM_EPISODE 4
#define TREX_RAND_STREAM_PUSH 5
#define TREX_RAND_STREAM_COMMAND 6
typedef struct TrexRandomTerm { int32_t kind; uint32_t mask; int32_t index, shared; float lo, hi; int32_t interval, duration; float probability; } TrexRandomTerm;

/* Set up to 16 terms (host values, copied; synchronises the device; replaces the previous terms - whose effects are taken back
 * first, as num_terms 0 does - and starts every env afresh: ep = 0, the next applied row is a first one). Flips the host-side
 * switches its terms need, so that a graph captured afterwards sees one launch form: MASS / FRICTION the per-env domain arrays,
 * KP / KD / MAX_FORCE the actuator model with the gains buffer in place, PUSH the external wrench with its buffer in place.
 * num_terms 0 clears: gains, wrench, mass scale and friction go back to their values at set time (mass scale and friction are
 * snapshotted only if a term covers them), the three switches go back, the state is freed; seed and env_offset are kept.
 * TREX_E_INVALID, the previous terms intact: more than 16 terms, an unknown kind, lo > hi or a bound that is not finite, a mask
 * bit beyond the model's bodies (MASS) or joints (KP, KD, MAX_FORCE), two terms of one kind whose masks overlap (two FRICTION
 * terms, two COMMAND terms of one component), more than 4 PUSH terms or two on one body, a body or command index out of range,
 * interval < 1 or duration < 1 on a PUSH term, interval < 0 on a COMMAND term, a probability outside [0, 1], KP or KD while
 * stiffness actions are on (the step launches write those columns), env_offset + N beyond 2^32. */
int trex_batch_set_randomization(TrexBatch *batch, const TrexRandomTerm *terms_host, int num_terms, uint64_t seed, uint32_t env_offset);
/* ONE launch for all N envs, once per step behind the step call and once per reset: done_dev[e * done_stride] is the env's done
 * flag (the done column of the rows, or any f32 array). command_dev: [N, 3], nullable without COMMAND terms. Writes the batch's
 * mass scale, friction, gains and wrench as defined above, command_dev and the batch's own state, and nothing else. CALLING IT
 * TWICE FOR ONE ROW ADVANCES k TWICE. TREX_E_INVALID, nothing launched: no terms set, command_dev missing and a COMMAND term set,
 * done_dev NULL, done_stride < 1, host memory or another device's, a short buffer. */
int trex_batch_apply_randomization(TrexBatch *batch, const float *done_dev, int done_stride, float *command_dev, void *stream);
/* Mark the envs with mask_dev[e] != 0 (u8 [N]; NULL: all): their next applied row is the first of an episode. One launch. */
int trex_batch_randomization_reset(TrexBatch *batch, const uint8_t *mask_dev, void *stream);
/* What is set: num_terms (nullable) and stream-ordered device copies, each nullable, each needing terms (push buffers: PUSH terms):
 * values_dev [N, num_terms, 32]: the draws of each env's current episode by body or joint element - a shared term repeats its one
 *   value, a COMMAND term holds its current value at element 0, PUSH terms and elements outside the mask read 0;
 * push_force_dev [N, num_push_terms, 3]: the force in effect, zeros while push_left is 0 (push terms in the order they were set);
 * push_left_dev [N, num_push_terms]: the steps the push still acts on. */
int trex_batch_randomization_info(const TrexBatch *batch, int *num_terms, float *values_dev, float *push_force_dev, int32_t *push_left_dev,
                                  void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_RANDOMIZE_H */
