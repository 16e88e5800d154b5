// Derivatives of the inverse dynamics (trex_batch_inverse_dynamics_derivatives; include/trex_dynamics_derivatives.h): launch
// arguments shared by capi_derivatives.cpp and dynamics_derivatives.hip. The step kernels do not see any of this; the query only
// reads the batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

#define TREX_DD_WAVES 4          /* envs per workgroup: one per wavefront, one body per lane of either half */
#define TREX_DD_NOMINAL 21       /* LDS floats per body of the nominal pass, [component][body] */
#define TREX_DD_TANGENT 9        /* LDS floats per body and direction of a tangent pass: force, moment, lever tangent */

struct TrexDdArgs {
  const TrexDeviceModel *model;
  const float *base, *q, *qd;     /* the batch's state (read only) */
  const float *mass_scale;        /* [N][32] per-env mass scale, NULL = 1 (no domain set) */
  int n_envs, nb;                 /* nb = moving bodies; J = nb - 1 joints, D = 6 + J generalised velocities */
  const float *accel;             /* [N, D], NULL = zeros */
  float *dfdq, *dfdv;             /* [N, D, D] each, NULL = not asked for (no passes) */
  int by_direction;               /* != 0: out[n][j][i], one row per direction j; else out[n][i][j] */
};

/* the dynamic LDS bytes of a workgroup: per env the nominal records and the tangent records of the two directions of a pass,
 * then the staged D x D block of every output asked for (two: 31 KB of 51 KB at D = 31) */
constexpr int trex_dd_lds_bytes(int nb, int outputs) {
  return TREX_DD_WAVES * (TREX_TL * (TREX_DD_NOMINAL + 2 * TREX_DD_TANGENT) + outputs * (5 + nb) * (5 + nb)) * (int)sizeof(float);
}

extern "C" hipError_t trex_launch_dynamics_derivatives(const TrexDdArgs &args, hipStream_t stream);   /* dynamics_derivatives.hip */
