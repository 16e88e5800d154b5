// Joint force/torque sensor (trex_batch_joint_wrench, trex_batch_generalized_velocity; include/trex_joint_wrench.h): launch
// arguments shared by capi_joint_wrench.cpp and joint_wrench.hip. The step kernels do not see any of this; the queries only read the
// batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

#define TREX_JW_WAVES 4          /* envs per workgroup: one per wavefront, one body per lane */
#define TREX_JW_BODY_FLOATS 512  /* LDS floats per env for the per-body records of the inward pass (16 per body) */

struct TrexJwArgs {
  const TrexDeviceModel *model;
  const float *base, *q, *qd;     /* the batch's state (read only) */
  const float *mass_scale;        /* [N][32] per-env mass scale, NULL = 1 (no domain set) */
  int n_envs, nb;                 /* nb = moving bodies; J = nb - 1 joints, D = 6 + J generalised velocities */
  const float *accel;             /* [N, D], NULL = zeros */
  const float *wrench_a, *wrench_b;   /* [N, nb, 6] each, NULL = none: world axes, force at the COM, torque about it */
  float *out;                     /* [N, J, 6] */
  float *base_out;                /* [N, 6], NULL = not asked for */
  int link_axes;                  /* != 0: every row in its child body's axes */
};

struct TrexGenVelArgs {
  const TrexDeviceModel *model;
  const float *base, *qd;
  int n_envs;
  float *vel;                     /* [N, D], NULL = not asked for; may be `prev` itself */
  const float *prev;              /* [N, D], NULL = no difference */
  float *accel;                   /* [N, D] = (current - prev) * inv_dt; with prev only */
  const float *done;              /* done[e * done_stride] != 0: a zero accel row; NULL = none */
  int done_stride;
  float inv_dt;
};

/* the dynamic LDS bytes of a workgroup: the body records of the four envs, then their joint rows and their base rows, each block
 * back to back as it lies in HBM (multiples of 16 bytes) */
constexpr int trex_jw_lds_bytes(int nb) {
  return TREX_JW_WAVES * (TREX_JW_BODY_FLOATS + 6 * (nb - 1) + 6) * (int)sizeof(float);
}

extern "C" hipError_t trex_launch_joint_wrench(const TrexJwArgs &args, hipStream_t stream);              /* joint_wrench.hip */
extern "C" hipError_t trex_launch_generalized_velocity(const TrexGenVelArgs &args, hipStream_t stream);  /* joint_wrench.hip */
