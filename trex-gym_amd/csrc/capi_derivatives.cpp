// C-ABI of include/trex_dynamics_derivatives.h: the derivatives of the inverse dynamics along the configuration tangent and the
// generalised velocity - the batch, the buffers and the launch of dynamics_derivatives.hip. The call reads the batch's state and
// writes caller buffers only.
#include "batch.hpp"
#include "dynamics_derivatives.h"

extern "C" {

int trex_batch_inverse_dynamics_derivatives(TrexBatch *b, const float *accel_dev, float *dfdq_dev, float *dfdv_dev, uint32_t flags,
                                            void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_inverse_dynamics_derivatives: ";
  if (!dfdq_dev && !dfdv_dev) return fail(TREX_E_INVALID, me + "dfdq and dfdv are both null");
  if (flags & ~TREX_DERIV_BY_DIRECTION) return fail(TREX_E_INVALID, me + "unknown flag bits " + std::to_string(flags & ~TREX_DERIV_BY_DIRECTION));
  if (b->nj < 1) return fail(TREX_E_INVALID, me + "the model has no joint");
  const size_t n = (size_t)b->n, D = 6 + (size_t)b->nj;
  const size_t row_bytes = n * D * sizeof(float), out_bytes = n * D * D * sizeof(float);
  if (accel_dev && ((dfdq_dev && trex::ranges_overlap(dfdq_dev, out_bytes, accel_dev, row_bytes)) ||
                    (dfdv_dev && trex::ranges_overlap(dfdv_dev, out_bytes, accel_dev, row_bytes))))
    return fail(TREX_E_INVALID, me + "an output overlaps accel");
  if (dfdq_dev && dfdv_dev && trex::ranges_overlap(dfdq_dev, out_bytes, dfdv_dev, out_bytes))
    return fail(TREX_E_INVALID, me + "dfdq overlaps dfdv");
  DeviceGuard guard(b->device);
  BUF_TRY(b, accel_dev, row_bytes, "trex_batch_inverse_dynamics_derivatives: accel");
  BUF_TRY(b, dfdq_dev, out_bytes, "trex_batch_inverse_dynamics_derivatives: dfdq");
  BUF_TRY(b, dfdv_dev, out_bytes, "trex_batch_inverse_dynamics_derivatives: dfdv");
  TrexDdArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q; a.qd = b->arr.qd;
  a.mass_scale = b->arr.domain ? b->arr.mass_scale : nullptr;
  a.n_envs = b->n; a.nb = b->nb;
  a.accel = accel_dev; a.dfdq = dfdq_dev; a.dfdv = dfdv_dev;
  a.by_direction = (flags & TREX_DERIV_BY_DIRECTION) != 0;
  HIP_TRY(trex_launch_dynamics_derivatives(a, (hipStream_t)stream));
  return TREX_OK;
}

}  // extern "C"
