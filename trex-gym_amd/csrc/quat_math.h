// Rotation matrix -> quaternion for the query kernels (link_state.hip, inverse_kinematics.hip). Kept apart from device_math.h:
// that header is hashed into the step kernels' build id.
#pragma once
#include <hip/hip_runtime.h>

// rotation matrix -> quaternion xyzw (w >= 0): the conversion of trex_link_transforms_kernel (batch_util.hip), operation for
// operation
__device__ __forceinline__ void mat_to_quat(const float *R, float *q) {
  float qx, qy, qz, qw;
  const float tr = R[0] + R[4] + R[8];
  if (tr > 0.f) {
    const float s = sqrtf(tr + 1.f) * 2.f;
    qw = 0.25f * s; qx = (R[7] - R[5]) / s; qy = (R[2] - R[6]) / s; qz = (R[3] - R[1]) / s;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    const float s = sqrtf(1.f + R[0] - R[4] - R[8]) * 2.f;
    qw = (R[7] - R[5]) / s; qx = 0.25f * s; qy = (R[1] + R[3]) / s; qz = (R[2] + R[6]) / s;
  } else if (R[4] >= R[8]) {
    const float s = sqrtf(1.f + R[4] - R[0] - R[8]) * 2.f;
    qw = (R[2] - R[6]) / s; qx = (R[1] + R[3]) / s; qy = 0.25f * s; qz = (R[5] + R[7]) / s;
  } else {
    const float s = sqrtf(1.f + R[8] - R[0] - R[4]) * 2.f;
    qw = (R[3] - R[1]) / s; qx = (R[2] + R[6]) / s; qy = (R[5] + R[7]) / s; qz = 0.25f * s;
  }
  const float sg = qw < 0.f ? -1.f : 1.f;
  q[0] = sg * qx; q[1] = sg * qy; q[2] = sg * qz; q[3] = sg * qw;
}
