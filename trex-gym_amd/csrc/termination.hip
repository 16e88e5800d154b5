// Kernel K8: per-body floor clearance (trex_batch_body_clearance) and the fall-termination predicate of the step sequence
// (trex_batch_set_termination), include/trex_batch.h. One env per wavefront, one wavefront per workgroup. The query reads the batch
// state and writes only its outputs; the predicate also writes the batch-owned mask / reason / values / terminal observation and,
// for an env that terminates, the done flags and the reward the step launch wrote.
//
// Phases 1 to 3 are body_clearance of clearance_sweep.h, which start_state.hip shares.
// Phase 1: lane b walks body b's chain once (chain_walk.h) and parks its pose in LDS, relative to the env's base origin. Phase 2:
// the lanes stride over the env's collision points - TrexDeviceModel::hull: hull vertices, or sphere centres / capsule ends with
// their radius, one code path - and take (z row of the body's rotation) . point + origin z - radius: three FMAs per point. A lane
// keeps the minimum of the body it is in and hands it to LDS when its points move on to the next body, with a 64-bit atomic min on
// (order-preserving bits of the height << 32 | point index): ties go to the earlier point, whatever the order of arrival. Phase 3:
// lane b adds (base z - floor z) and writes body b's clearance, on request the lowest point. No bounding volume is consulted:
// every point is evaluated.
//
// The predicate path is the same kernel with PRED set: the three values, the comparison and the writes follow phase 3.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/trex_batch.h"
#include "clearance_sweep.h"
#include "device_math.h"
#include "termination.h"

namespace {

constexpr int BLOCK = TREX_TERM_BLOCK;
constexpr int TL = TREX_TL;
constexpr int POSE = CLR_POSE;   // LDS floats per body: R 9 (row-major) | origin 3, relative to the base origin
constexpr uint32_t NO_POINT = CLR_NO_POINT;

}  // namespace

template <bool PRED>
__global__ __launch_bounds__(64) void trex_termination_kernel(TrexTermArgs a) {
  __shared__ __attribute__((aligned(16))) float sPose[TL * POSE];
  __shared__ int sStart[TL + 1];
  __shared__ unsigned long long sBest[TL];

  const TrexDeviceModel *M = a.model;
  const int t = threadIdx.x, env = blockIdx.x, nb = M->nb;
  const float *base = a.base + (size_t)env * 16;
  uint32_t low;
  float head_z;
  const float clr = body_clearance<PRED>(a, env, t, PRED ? a.watch_any != 0 : true, sPose, sStart, sBest, low, head_z);

  if (!PRED) {
    if (t >= nb) return;
    const size_t g = (size_t)env * nb + t;
    a.clearance[g] = clr;
    if (a.lowest) {
      float *w = a.lowest + 3 * g;
      if (low == NO_POINT) {
        w[0] = w[1] = w[2] = NAN;
      } else {
        const float *P = sPose + t * POSE;
        const float4 p = a.hull[low];
        const float v[3] = {p.x, p.y, p.z};
        float o[3];
        matvec3(P, v, o);
        w[0] = base[0] + (P[9] + o[0]);
        w[1] = base[1] + (P[10] + o[1]);
        w[2] = (base[2] + (P[11] + o[2])) - p.w;
      }
    }
    return;
  }

  // ---- the predicate: the three values, wave-uniform
  const float cm = a.clear_min[t & (TL - 1)];
  float d = (a.watch_any && t < nb && cm == cm) ? clr - cm : INFINITY;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) d = fminf(d, __shfl_xor(d, off));
  const float v0 = __shfl(head_z, M->head_body) - M->prm[TP_FLOOR_Z];
  const float qb[4] = {base[3], base[4], base[5], base[6]}, qs[4] = {M->base_quat0[0], M->base_quat0[1], M->base_quat0[2], M->base_quat0[3]};
  float Rb[9], Rs[9];
  quat_to_mat(qb, Rb);
  quat_to_mat(qs, Rs);
  const float v1 = Rb[6] * Rs[6] + Rb[7] * Rs[7] + Rb[8] * Rs[8];   // z of R_base R_start^-1 e_z
  // an env whose done the step launch already set - time limit, containment - is on its new episode's state: not judged
  const bool ended = a.done ? a.done[env] != 0 : a.done_f[(size_t)env * a.scal_stride] != 0.f;
  int reason = 0;
  if (!ended) {   // strict <; a NaN threshold compares false: off
    if (v0 < a.head_min) reason |= TREX_TERM_BIT_HEAD;
    if (v1 < a.cos_tilt) reason |= TREX_TERM_BIT_TILT;
    if (d < 0.f) reason |= TREX_TERM_BIT_CLEARANCE;
  }
  if (reason && a.obs) {
    const float *src = a.obs + (size_t)env * a.obs_stride;
    float *dst = a.terminal_obs + (size_t)env * a.obs_cols;
    for (int c = t; c < a.obs_cols; c += BLOCK) dst[c] = src[c];
  }
  if (t == 0) {
    a.reason[env] = reason;
    a.mask[env] = reason ? 1 : 0;
    float *v = a.values + 3 * (size_t)env;
    v[0] = v0; v[1] = v1; v[2] = d;
    if (reason) {
      if (a.done) a.done[env] = 1;
      if (a.done_f) a.done_f[(size_t)env * a.scal_stride] = 1.f;
      if (a.reward) a.reward[(size_t)env * a.scal_stride] -= a.penalty;
    }
  }
}

extern "C" hipError_t trex_launch_termination(const TrexTermArgs &args, int predicate, hipStream_t stream) {
  const dim3 grid((unsigned)args.n_envs), block(BLOCK);
  if (predicate) hipLaunchKernelGGL(trex_termination_kernel<true>, grid, block, 0, stream, args);
  else hipLaunchKernelGGL(trex_termination_kernel<false>, grid, block, 0, stream, args);
  return hipGetLastError();
}
