// The utility kernels of a batch and their launchers (called by capi.cpp): pack / unpack state, head position, link transforms,
// per-env scalars, fills and the layout copies of the per-env buffers. None of them shares code with the step kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_walk.h"
#include "device_math.h"
#include "device_model.h"
#include "step_launch.h"

namespace {
constexpr int TL = TREX_TL, ACT_ROWS = TREX_ACT_ROWS, SENS_ROWS = TREX_SENS_ROWS;
}  // namespace

__global__ void trex_pack_state_kernel(const TrexDeviceModel *M, TrexBatchArrays arr, int n, float *out, int pack) {
  // pack=1: internal -> [N, 13+2J]; pack=0: [N, 13+2J] -> internal
  const int env = blockIdx.x * (blockDim.x / TL) + threadIdx.x / TL;
  const int lane = threadIdx.x & (TL - 1);
  if (env >= n) return;
  const int nj = M->nb - 1, width = 13 + 2 * nj;
  float *row = out + (size_t)env * width;
  float *b = arr.base + env * 16;
  if (pack) {
    if (lane < 13) row[lane] = b[lane];
    if (lane >= 1 && lane < M->nb) {
      const int s = M->obs_slot[lane];
      row[13 + s] = arr.q[env * TL + lane];
      row[13 + nj + s] = arr.qd[env * TL + lane];
    }
  } else {
    if (lane < 13) b[lane] = row[lane];
    float qv = 0.f, qdv = 0.f;
    if (lane >= 1 && lane < M->nb) {
      const int s = M->obs_slot[lane];
      qv = row[13 + s]; qdv = row[13 + nj + s];
    }
    arr.q[env * TL + lane] = qv;
    arr.qd[env * TL + lane] = qdv;
  }
}

// world position of the head point: one env per thread, which walks the head body's chain from the base
__global__ void trex_head_kernel(const TrexDeviceModel *M, TrexBatchArrays arr, int n, float *out) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  const float *b = arr.base + env * 16;
  Walk k;
  walk_chain<false, false>(M, arr.base, arr.q, nullptr, nullptr, env, M->head_body, 0, k);
  const float hp[3] = {M->head_point[0], M->head_point[1], M->head_point[2]};
  float o[3];
  matvec3(k.R, hp, o);
  for (int c = 0; c < 3; c++) out[env * 3 + c] = b[c] + k.r[c] + o[c];
}

// Rollout export: world pose of every URDF link. One 64-thread block per env: lanes < nb walk their
// body's chain from the base (<= 6 hinges) and park R, p in LDS; then the block strides over the links.
__global__ __launch_bounds__(64) void trex_link_transforms_kernel(const TrexDeviceModel *M, TrexBatchArrays arr, float *out, int L,
                                                                  const int *frame_body, const float *frame_tf) {
  __shared__ float bodyR[TL][9], bodyP[TL][3];
  const int env = blockIdx.x;
  const int t = threadIdx.x;
  if (t < M->nb) {
    const float *b = arr.base + env * 16;
    Walk k;
    walk_chain<false, false>(M, arr.base, arr.q, nullptr, nullptr, env, t, 0, k);
    for (int c = 0; c < 9; c++) bodyR[t][c] = k.R[c];
    for (int c = 0; c < 3; c++) bodyP[t][c] = b[c] + k.r[c];
  }
  __syncthreads();
  // the frames to export: the URDF link frames (trex_batch_link_transforms) or the <visual> meshes
  // (trex_batch_visual_transforms), each given by its body and its transform in that body's frame
  for (int l = t; l < L; l += blockDim.x) {
    const int body = frame_body[l];
    const float *tf = frame_tf + 12 * l;
    float R[9], o[3];
    matmul3(bodyR[body], tf, R);
    matvec3(bodyR[body], tf + 9, o);
    float *w = out + ((size_t)env * L + l) * 7;
    for (int c = 0; c < 3; c++) w[c] = bodyP[body][c] + o[c];
    // rotation matrix -> quaternion xyzw (w >= 0)
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
    w[3] = sg * qx; w[4] = sg * qy; w[5] = sg * qz; w[6] = sg * qw;
  }
}

// the per-env scalars of the base row (device_model.h): read out / set by the C-ABI's accessors
__global__ void trex_scalars_get_kernel(const float *base, int n, int32_t *count, float *impulse, int32_t *steps) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float *b = base + (size_t)e * 16;
  if (count) count[e] = __float_as_int(b[TREX_BASE_FLAGS]) & 255;
  if (impulse) impulse[e] = b[TREX_BASE_IMPULSE];
  if (steps) steps[e] = __float_as_int(b[TREX_BASE_STEPS]);
}
__global__ void trex_scalars_set_kernel(float *base, int n, const int32_t *steps, int set_steps, int motors) {
  // set_steps: word 15 <- steps[e] (or 0 if steps == null); motors >= 0: the motors flag <- motors
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float *b = base + (size_t)e * 16;
  if (set_steps) b[TREX_BASE_STEPS] = __int_as_float(steps ? steps[e] : 0);
  if (motors >= 0) {
    const int f = __float_as_int(b[TREX_BASE_FLAGS]);
    b[TREX_BASE_FLAGS] = __int_as_float(motors ? (f | TREX_MOTORS_BIT) : (f & ~TREX_MOTORS_BIT));
  }
}

__global__ void trex_fill_kernel(float *p, float v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ void trex_fill_u8_kernel(uint8_t *p, uint8_t v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ void trex_copy_mass_scale_kernel(const float *src, float *dst, int n, int nb) {
  // [N, nb] -> [N, 32]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * TL) return;
  const int e = i / TL, l = i % TL;
  dst[i] = l < nb ? src[e * nb + l] : 1.0f;
}
__global__ void trex_copy_wrench_kernel(const float *src, float *dst, int n, int nb) {
  // [N, nb, 6] -> [N, 6, 32] (component-major: the step's body lanes load one coalesced row per component)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 6 * TL) return;
  const int e = i / (6 * TL), c = (i / TL) % 6, l = i % TL;
  dst[i] = l < nb ? src[((size_t)e * nb + l) * 6 + c] : 0.0f;
}
__global__ void trex_copy_gains_kernel(const TrexDeviceModel *M, const float *kp, const float *kd, const float *max_force, float *dst, int n) {
  // three [N, J] arrays in observation order, each nullable = the model parameter -> the first four of [N, ACT_ROWS, 32] (row per gain: the
  // step's body lanes load one coalesced row per gain); a negative value is clamped to 0, a non-finite one is kept (the step
  // contains that env); max_force also as the largest impulse of a substep, the product the model's motor_max_impulse is
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * TL) return;
  const int e = i / TL, l = i % TL, nj = M->nb - 1;
  float v[ACT_ROWS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (l >= 1 && l < M->nb) {
    const size_t at = (size_t)e * nj + M->obs_slot[l];
    const float p = kp ? kp[at] : M->prm[TP_MOTOR_KP], d = kd ? kd[at] : M->prm[TP_MOTOR_KD];
    const float f = max_force ? max_force[at] : M->prm[TP_MOTOR_MAX_FORCE];
    v[0] = p < 0.f ? 0.f : p; v[1] = d < 0.f ? 0.f : d; v[3] = f < 0.f ? 0.f : f;
    v[2] = v[3] * M->prm[TP_DT];
  }
#pragma unroll
  for (int c = 0; c < ACT_ROWS; c++) dst[((size_t)e * ACT_ROWS + c) * TL + l] = v[c];
}
__global__ void trex_contact_wrench_kernel(const float *src, float *dst, int n, int nb) {
  // the sensor's rows 0..5 [N, SENS_ROWS, 32] -> [N, nb, 6]
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * nb * 6) return;
  const int e = i / (nb * 6), l = (i / 6) % nb, c = i % 6;
  dst[i] = src[(size_t)e * (SENS_ROWS * TL) + c * TL + l];
}

// ---------------------------------------------------------------- host launchers (called by capi.cpp)
extern "C" {

hipError_t trex_launch_pack_state(const TrexDeviceModel *model, TrexBatchArrays arr, int n, float *state, int pack,
                                  hipStream_t stream) {
  hipLaunchKernelGGL(trex_pack_state_kernel, dim3((n + 7) / 8), dim3(256), 0, stream, model, arr, n, state, pack);
  return hipGetLastError();
}

hipError_t trex_launch_head(const TrexDeviceModel *model, TrexBatchArrays arr, int n, float *out, hipStream_t stream) {
  hipLaunchKernelGGL(trex_head_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, model, arr, n, out);
  return hipGetLastError();
}

hipError_t trex_launch_link_transforms(const TrexDeviceModel *model, TrexBatchArrays arr, int n, float *out, hipStream_t stream,
                                       int visuals) {
  if (visuals) hipLaunchKernelGGL(trex_link_transforms_kernel, dim3(n), dim3(64), 0, stream, model, arr, out, arr.num_visuals, arr.visual_body, arr.visual_tf);
  else hipLaunchKernelGGL(trex_link_transforms_kernel, dim3(n), dim3(64), 0, stream, model, arr, out, arr.num_links, arr.link_body, arr.link_tf);
  return hipGetLastError();
}

hipError_t trex_launch_scalars_get(TrexBatchArrays arr, int n, int32_t *count, float *impulse, int32_t *steps, hipStream_t stream) {
  hipLaunchKernelGGL(trex_scalars_get_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, arr.base, n, count, impulse, steps);
  return hipGetLastError();
}
hipError_t trex_launch_scalars_set(TrexBatchArrays arr, int n, const int32_t *steps, int set_steps, int motors, hipStream_t stream) {
  hipLaunchKernelGGL(trex_scalars_set_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, arr.base, n, steps, set_steps, motors);
  return hipGetLastError();
}

hipError_t trex_launch_fill(float *p, float v, int n, hipStream_t stream) {
  hipLaunchKernelGGL(trex_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, v, n);
  return hipGetLastError();
}
hipError_t trex_launch_fill_u8(uint8_t *p, uint8_t v, int n, hipStream_t stream) {
  hipLaunchKernelGGL(trex_fill_u8_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, v, n);
  return hipGetLastError();
}
hipError_t trex_launch_copy_mass_scale(const float *src, float *dst, int n, int nb, hipStream_t stream) {
  hipLaunchKernelGGL(trex_copy_mass_scale_kernel, dim3((n * TL + 255) / 256), dim3(256), 0, stream, src, dst, n, nb);
  return hipGetLastError();
}
hipError_t trex_launch_contact_wrench(const float *src, float *dst, int n, int nb, hipStream_t stream) {
  hipLaunchKernelGGL(trex_contact_wrench_kernel, dim3((n * nb * 6 + 255) / 256), dim3(256), 0, stream, src, dst, n, nb);
  return hipGetLastError();
}
hipError_t trex_launch_copy_gains(const TrexDeviceModel *model, const float *kp, const float *kd, const float *max_force, float *dst,
                                  int n, hipStream_t stream) {
  hipLaunchKernelGGL(trex_copy_gains_kernel, dim3((n * TL + 255) / 256), dim3(256), 0, stream, model, kp, kd, max_force, dst, n);
  return hipGetLastError();
}
hipError_t trex_launch_copy_wrench(const float *src, float *dst, int n, int nb, hipStream_t stream) {
  hipLaunchKernelGGL(trex_copy_wrench_kernel, dim3((n * 6 * TL + 255) / 256), dim3(256), 0, stream, src, dst, n, nb);
  return hipGetLastError();
}

}  // extern "C"
