/*
 * trex_planner.h - C-ABI of a sampling-based planner on the device: MPPI, or predictive sampling when only the best sample is
 * kept, over any open-loop rollout engine - trex_batch_step_many (include/trex_batch.h) is one. K21.
 *
 * Not part of the physics boundary and not tied to it: the planner reads and writes plain device buffers - an action block
 * [S, N, A] it fills, reward and done columns it reads in place. A caller with a rollout engine of its own needs this header alone.
 *
 * Conventions as in trex_batch.h and trex_policy.h: 0 / negative TREX_E_* codes (TREX_OK 0, TREX_E_INVALID -1, TREX_E_HIP -5),
 * trex_last_error(), caller-owned device buffers that are validated once per allocation, stream-ordered asynchronous launches
 * (void* = hipStream_t), capturable from the second call with the same buffers on. On TREX_E_INVALID nothing is launched and
 * nothing is changed.
 *
 * Semantics (ONE definition). Every product and every sum below is rounded to f32, no fma, unless it says "host" or "f64".
 *
 * Sizes. G groups (one per robot that plans), K samples per group, N = G K sample envs, env e = g K + k; S steps of horizon, P
 *   knots, A action columns. 1 <= K <= 4096, 1 <= S <= 256, 1 <= P <= min(S, 32), 1 <= A <= 64, G >= 1, S N A < 2^31.
 *
 * State. The nominal knots nominal [G, P, A] (zeros at create), the knots of the last samples knots [N, P, A] (zeros), the sample
 *   count `it` (u32, on the device, 0), the noise (sigma = 0, lo = -inf, hi = +inf until trex_planner_set_noise).
 *   clip(v, lo, hi) = lo where v < lo, else hi where v > hi, else v: a NaN passes, values are not validated.
 *
 * Knot times and taps. Knot p sits at step t_p = p (S - 1) / (P - 1); with P == 1 the one knot is a constant. A time tau in
 *   [0, S - 1] is the knot coordinate u = tau (P - 1) / (S - 1) = num / den, formed in INTEGERS: for step s, num = s (P - 1),
 *   den = S - 1. It has four taps - knot indices i0..i3 and f32 weights w0..w3 - and the spline's value there is
 *       value = ((w0 k[i0] + w1 k[i1]) + w2 k[i2]) + w3 k[i3]
 *   P == 1, or S == 1:  i = (0, 0, 0, 0), w = (1, 0, 0, 0).
 *   TREX_PLAN_HOLD:     the knot at or before tau: j = min(num / den, P - 1) (integer division), i = (j, j, j, j), w = (1, 0, 0, 0).
 *   TREX_PLAN_LINEAR:   j = min(num / den, P - 2), t = (num - j den) / den in f64; i = (j, j + 1, j + 1, j + 1),
 *                       W = (1 - t, t, 0, 0).
 *   TREX_PLAN_CUBIC:    Catmull-Rom with the end knots repeated: j and t as for LINEAR; i = (max(j - 1, 0), j, j + 1,
 *                       min(j + 2, P - 1)), W = ((-t^3 + 2 t^2 - t) / 2, (3 t^3 - 5 t^2 + 2) / 2, (-3 t^3 + 4 t^2 + t) / 2,
 *                       (t^3 - t^2) / 2), evaluated in f64 as written.
 *   The weights: built on the host in f64 and rounded once, w = (float)W - but for the LAST tap whose W is not 0, which is the
 *   f32 complement of the taps before it: w_last = 1 - (the f32 sum, in tap order, of the w before it; 1 - 0 where it is the
 *   first). So ((w0 + w1) + w2) + w3 == 1 in f32 exactly, and a constant that is a power of two is reproduced bit for bit. All
 *   three kinds are one 4-tap evaluation; the table is the kind.
 *
 * Noise (trex_planner_set_noise). Sample k == 0 of every group is the nominal: knot[e, p, a] = clip(nominal[g, p, a], lo[a],
 *   hi[a]); no draw is consumed for it. For k > 0: knot = clip(nominal[g, p, a] + sigma[a] * z, lo[a], hi[a]); sigma[a] == 0 adds
 *   nothing, the knot is bitwise the clipped nominal. z is the Gaussian of include/trex_sensing.h - Box-Muller pairs, the precise
 *   logf, sinf, cosf, sqrtf - of Philox4x32-10 with key = (low half of seed, high half of seed) and
 *       counter = (env_offset + e, it, (TREX_PLAN_STREAM << 16) | (a >> 2), p),    output a & 3
 *   stream 8 beside the 0..7 of the sensor model, the episode randomisation and the start states. There is no generator state: a
 *   run sharded over groups (env_offset = the first group's g K) draws what the whole run draws; a graph replay advances `it` on
 *   the device.
 *
 * Sample (trex_planner_sample). Writes knots [N, P, A] as above, then actions[s, e, a] = clip(value of the env's knots at step s,
 *   lo[a], hi[a]) for every step, then it += 1.
 *
 * Update (trex_planner_update). g_s = (float)pow((double)gamma, s), a host table, s = 0 .. S.
 *   Return: R_e = 0; for s = 0, 1, ..: R_e = R_e + g_s * reward[s step_stride + e env_stride]; the loop ends behind the first
 *   step whose done[s step_stride + e env_stride] != 0 (that step's reward counts). If no step was done and terminal_dev is given:
 *   R_e = R_e + g_S * terminal[e]. An R_e that is not finite - NaN, or an infinity of either sign - counts as -inf from here on,
 *   in returns_out too.
 *   Per group: R_max = the largest R[g, k]; best = the smallest k with R[g, k] == R_max. A group with no finite return keeps its
 *   nominal, best = -1, its weights are 0 and its stats (-inf, 0, 0, -inf).
 *   temperature == 0 (predictive sampling): w_k = 1 for k == best, else 0; the nominal becomes knots[g K + best] bit for bit.
 *   temperature > 0 (MPPI): w_k = expf((R_k - R_max) / temperature), the precise expf and an IEEE division; expf(-inf) = 0;
 *   nominal[g, p, a] = (sum_k w_k * knots[g K + k, p, a]) / (sum_k w_k), both sums sequential in k = 0, 1, .. from 0.
 *   stats[g] = (R_max, (sum_k R_k over the finite ones, sequential in k) / (float)their number, (sum_k w_k)^2 / (sum_k w_k * w_k)
 *   - the effective sample size, sequential sums again -, R[g, 0]).
 *   The definition fixes the order of every sum, not the launch shape: results are bitwise repeatable and do not depend on how
 *   the work is cut into workgroups. There are no float atomics.
 *
 * Shift (trex_planner_shift). Receding horizon: new nominal knot p = the value of the old nominal's spline at
 *   tau = min(t_p + steps, S - 1), i.e. num = min(p (S - 1) + steps (P - 1), (P - 1) (S - 1)), den = S - 1: the same four taps,
 *   unclipped. steps beyond S - 1 act as S - 1.
 *
 * Action (trex_planner_action). actions[g, a] = clip(value at `step` of the knots clip(nominal[g, p, a], lo[a], hi[a]), lo[a],
 *   hi[a]): what sample 0 of the group plays at that step.
 */
#ifndef TREX_PLANNER_H
#define TREX_PLANNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define TREX_PLAN_HOLD        0
#define TREX_PLAN_LINEAR      1
#define TREX_PLAN_CUBIC       2
#define TREX_PLAN_KINDS       3
#define TREX_PLAN_STREAM      8
#define TREX_PLAN_MAXSAMPLES  4096
#define TREX_PLAN_MAXHORIZON  256
#define TREX_PLAN_MAXKNOTS    32
#define TREX_PLAN_MAXACT      64

typedef struct TrexPlanner TrexPlanner;

/* Owns the nominal, the samples' knots, `it` and the tables. TREX_E_INVALID: a size outside the limits above, an unknown
 * interpolation, a device that does not exist. */
int trex_planner_create(int groups, int samples, int horizon, int knots, int act_dim, int interpolation, int device, TrexPlanner **out);
void trex_planner_destroy(TrexPlanner *planner);
/* The sizes and the kind (each nullable) and, where it_host is given, the sample count `it` copied out: that synchronises the stream. */
int trex_planner_info(const TrexPlanner *planner, int *groups, int *samples, int *horizon, int *knots, int *act_dim, int *interpolation,
                      uint32_t *it_host, void *stream);

/* nominal[g] = knots_dev[g] for the groups with mask_dev[g] != 0 (u8 [G]; NULL: all). One launch. */
int trex_planner_set_nominal(TrexPlanner *planner, const float *knots_dev, const uint8_t *mask_dev, void *stream);
/* Stream-ordered device copies of the nominal [G, P, A] and of the last samples' knots [N, P, A]. */
int trex_planner_get_nominal(const TrexPlanner *planner, float *knots_dev, void *stream);
int trex_planner_get_samples(const TrexPlanner *planner, float *knots_dev, void *stream);

/* sigma, lo, hi: A host values each, copied; seed: the Philox key; env_offset: the global index of this planner's env 0.
 * Synchronises the device and starts the sample count afresh: it = 0. TREX_E_INVALID, the previous noise intact: a NULL array, a
 * sigma that is negative or not finite, a lo or hi that is NaN, lo > hi, env_offset + N beyond 2^32. */
int trex_planner_set_noise(TrexPlanner *planner, const float *sigma_host, const float *lo_host, const float *hi_host, uint64_t seed,
                           uint32_t env_offset);

/* ONE launch: the samples' knots, then actions_dev [S, N, A] - the layout trex_batch_step_many reads -, then it += 1.
 * TREX_E_INVALID: before trex_planner_set_noise, actions_dev NULL, host memory or another device's, a short buffer. */
int trex_planner_sample(TrexPlanner *planner, float *actions_dev, void *stream);

/* The returns of the N rollouts and the new nominal: three launches. reward_dev, done_dev (nullable): element (s, e) at
 * s step_stride + e env_stride FLOATS, so that the reward and done columns of a row block [S, N, row_stride] are read in place
 * (reward_dev = rows + 3J, done_dev = rows + 3J + 1, step_stride = N row_stride, env_stride = row_stride); done is read as f32,
 * non-zero = done. terminal_dev [N] nullable. Outputs, each nullable: returns_out [N], weights_out [N], best_out [G] i32,
 * stats_out [G, 4]. The discount table of a gamma is built and kept on the first call with it: capturable from the second call
 * with the same gamma on. TREX_E_INVALID: before trex_planner_set_noise, reward_dev NULL, a stride below 1, gamma or temperature
 * negative or not finite, host memory or another device's, a buffer shorter than its strides reach. */
int trex_planner_update(TrexPlanner *planner, const float *reward_dev, int64_t step_stride, int64_t env_stride, const float *done_dev,
                        const float *terminal_dev, float gamma, float temperature, float *returns_out, float *weights_out,
                        int32_t *best_out, float *stats_out, void *stream);

/* One launch. The tap table of a `steps` is built and kept on the first call with it (that call synchronises nothing but
 * allocates: capturable from the second call with the same `steps` on). TREX_E_INVALID: steps < 0. */
int trex_planner_shift(TrexPlanner *planner, int steps, void *stream);

/* One launch: actions_dev [G, A]. TREX_E_INVALID: step outside [0, S), the usual buffer checks. */
int trex_planner_action(TrexPlanner *planner, int step, float *actions_dev, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_PLANNER_H */
