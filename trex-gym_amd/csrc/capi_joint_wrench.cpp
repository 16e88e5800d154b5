// C-ABI of include/trex_joint_wrench.h: the joint force/torque sensor and the generalised velocity with its backward difference -
// the batch, the buffers and the launches of joint_wrench.hip. Both calls read the batch's state and write caller buffers only.
#include <cmath>

#include "batch.hpp"
#include "joint_wrench.h"

extern "C" {

int trex_batch_joint_wrench(TrexBatch *b, const float *accel_dev, const float *wrench_a_dev, const float *wrench_b_dev, int axes,
                            float *out_dev, float *base_out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "trex_batch_joint_wrench: out is null");
  if (axes != TREX_AXES_WORLD && axes != TREX_AXES_LINK)
    return fail(TREX_E_INVALID, "trex_batch_joint_wrench: axes " + std::to_string(axes) + " is neither TREX_AXES_WORLD nor TREX_AXES_LINK");
  if (b->nj < 1) return fail(TREX_E_INVALID, "trex_batch_joint_wrench: the model has no joint");
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n, body_bytes = n * b->nb * 6 * sizeof(float);
  BUF_TRY(b, accel_dev, n * (6 + b->nj) * sizeof(float), "trex_batch_joint_wrench: accel");
  BUF_TRY(b, wrench_a_dev, body_bytes, "trex_batch_joint_wrench: wrench_a");
  BUF_TRY(b, wrench_b_dev, body_bytes, "trex_batch_joint_wrench: wrench_b");
  BUF_TRY(b, out_dev, n * b->nj * 6 * sizeof(float), "trex_batch_joint_wrench: out");
  BUF_TRY(b, base_out_dev, n * 6 * sizeof(float), "trex_batch_joint_wrench: base_out");
  TrexJwArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q; a.qd = b->arr.qd;
  a.mass_scale = b->arr.domain ? b->arr.mass_scale : nullptr;
  a.n_envs = b->n; a.nb = b->nb;
  a.accel = accel_dev; a.wrench_a = wrench_a_dev; a.wrench_b = wrench_b_dev;
  a.out = out_dev; a.base_out = base_out_dev;
  a.link_axes = axes == TREX_AXES_LINK;
  HIP_TRY(trex_launch_joint_wrench(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_generalized_velocity(TrexBatch *b, float *vel_dev, const float *prev_dev, float inv_dt, const float *done_dev,
                                    int done_stride, float *accel_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_generalized_velocity: ";
  if (!vel_dev && !prev_dev) return fail(TREX_E_INVALID, me + "vel and prev are both null");
  if (prev_dev && !accel_dev) return fail(TREX_E_INVALID, me + "prev is given and accel is null");
  if (!prev_dev && accel_dev) return fail(TREX_E_INVALID, me + "accel is given and prev is null");
  if (prev_dev && !std::isfinite(inv_dt)) return fail(TREX_E_INVALID, me + "inv_dt is not finite");
  if (done_dev && done_stride < 1) return fail(TREX_E_INVALID, me + "done_stride " + std::to_string(done_stride) + " < 1");
  const size_t n = (size_t)b->n, bytes = n * (6 + b->nj) * sizeof(float);
  if (vel_dev && prev_dev && vel_dev != prev_dev && trex::ranges_overlap(vel_dev, bytes, prev_dev, bytes))
    return fail(TREX_E_INVALID, me + "vel overlaps prev without being prev");
  if (accel_dev && ((vel_dev && trex::ranges_overlap(accel_dev, bytes, vel_dev, bytes)) || trex::ranges_overlap(accel_dev, bytes, prev_dev, bytes)))
    return fail(TREX_E_INVALID, me + "accel overlaps vel or prev");
  DeviceGuard guard(b->device);
  BUF_TRY(b, vel_dev, bytes, "trex_batch_generalized_velocity: vel");
  BUF_TRY(b, prev_dev, bytes, "trex_batch_generalized_velocity: prev");
  BUF_TRY(b, accel_dev, bytes, "trex_batch_generalized_velocity: accel");
  if (done_dev) BUF_TRY(b, done_dev, trex::row_block_bytes(n, done_stride, 1), "trex_batch_generalized_velocity: done");
  TrexGenVelArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.qd = b->arr.qd;
  a.n_envs = b->n;
  a.vel = vel_dev; a.prev = prev_dev; a.accel = accel_dev;
  a.done = done_dev; a.done_stride = done_dev ? done_stride : 0;
  a.inv_dt = inv_dt;
  HIP_TRY(trex_launch_generalized_velocity(a, (hipStream_t)stream));
  return TREX_OK;
}

}  // extern "C"
