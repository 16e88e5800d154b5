// Joint force/torque sensor: the 6-D wrench every joint transmits (pybullet's jointReactionForces), and the generalised velocity
// with its backward difference, which gives the sensor its acceleration. Read-only: nothing here writes the state. gfx950, the
// shape of dynamics.hip: one env per 64-lane wavefront, one body per lane, four envs per workgroup so that their rows lie back to
// back and leave the chip as 16-byte stores.
//
// Row k of the output is the wrench the parent exerts on the child body of joint k through the joint: what the subtree of that body
// needs for its motion less what the world already applies to it,
//   f_i = sum_{b in S(i)} (m_b a_c,b - F_b),   n_i = sum_{b in S(i)} [Ic_b al_b + w_b x Ic_b w_b - T_b + (c_b - r_i) x (m_b a_c,b - F_b)],
// a_c the classical COM acceleration plus g z, (F_b, T_b) the world's wrench on body b at its COM, r_i the joint origin. This is
// RNEA's inward pass with the subtree force and moment kept instead of projected on the joint axis. As in dynamics.hip everything
// is in world axes relative to the base origin, forces at the COM, moments about the body's own joint origin, shifted to the parent
// by the short lever between the two origins.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "joint_wrench.h"

namespace {

constexpr int TL = TREX_TL;
constexpr int MAXCH = TREX_MAXCH;
constexpr int WAVES = TREX_JW_WAVES;
constexpr int BLOCK = 64 * WAVES;

// `count` floats of the workgroup's envs from LDS, as 16-byte stores where the caller's buffer allows it (four envs are a multiple
// of 16 bytes whatever J is: only the base address can be odd)
__device__ __forceinline__ void block_store(float *dst, const float *src, int count) {
  const int t = threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const int n4 = count >> 2;
    for (int i = t; i < n4; i += BLOCK) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
    for (int i = (n4 << 2) + t; i < count; i += BLOCK) dst[i] = src[i];
  } else {
    for (int i = t; i < count; i += BLOCK) dst[i] = src[i];
  }
}

// WRENCH: one of the two wrench inputs is given (else none is loaded); LINK: the rows in their child body's axes
template <bool WRENCH, bool LINK>
__global__ __launch_bounds__(BLOCK) void trex_joint_wrench_kernel(TrexJwArgs A) {
  extern __shared__ float4 lds4[];
  float *lds = reinterpret_cast<float *>(lds4);
  const TrexDeviceModel *M = A.model;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int env0 = blockIdx.x * WAVES, env = env0 + wave;
  const int nb = A.nb, J = nb - 1, D = 6 + J;
  const bool live = env < A.n_envs;                      // (a wave past the batch's end still meets the barriers)
  const bool is_body = live && lane < nb;
  const int b = is_body ? lane : 0;
  const int e = live ? env : 0;
  float *rec = lds + wave * TREX_JW_BODY_FLOATS;          // [32][16] this env's per-body records
  float *rows = lds + WAVES * TREX_JW_BODY_FLOATS;        // [4][J][6] the joint rows, then [4][6] the base rows
  float *stage = rows + wave * 6 * J;
  float *stage_base = rows + WAVES * 6 * J + wave * 6;
  const int depth = is_body ? M->depth[b] : -1;
  const int maxdepth = M->maxdepth;

  // ---- outward (in registers): classical velocity and acceleration of the body frame; its mass, COM offset and inertia
  Walk k;
  walk_chain<true, true>(M, A.base, A.q, A.qd, A.accel, e, b, D, k);
  const float sc = A.mass_scale ? A.mass_scale[(size_t)e * TL + b] : 1.0f;
  const float m = M->mass[b] * sc;
  float cb[3], Ic[6];
  {
    const float comb[3] = {M->com[0][b], M->com[1][b], M->com[2][b]};
    matvec3(k.R, comb, cb);
    float in[6], t[9];
#pragma unroll
    for (int c = 0; c < 6; c++) in[c] = M->inertia[c][b];
    const float Ib[9] = {in[0], in[1], in[2], in[1], in[3], in[4], in[2], in[4], in[5]};
    matmul3(k.R, Ib, t);
    const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int c = 0; c < 6; c++)
      Ic[c] = sc * (t[3 * ia[c]] * k.R[3 * ib[c]] + t[3 * ia[c] + 1] * k.R[3 * ib[c] + 1] + t[3 * ia[c] + 2] * k.R[3 * ib[c] + 2]);
  }
  // what the world applies to this body: the two inputs added first, so that a + b and their sum passed as one are the same bits
  float W[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if constexpr (WRENCH) {
    const size_t at = ((size_t)e * nb + b) * 6;
    if (A.wrench_a && A.wrench_b) {
#pragma unroll
      for (int c = 0; c < 6; c++) W[c] = A.wrench_a[at + c] + A.wrench_b[at + c];
    } else {
      const float *w = A.wrench_a ? A.wrench_a : A.wrench_b;
#pragma unroll
      for (int c = 0; c < 6; c++) W[c] = w[at + c];
    }
  }
  // the force at the COM and the moment about the body's joint origin that this motion needs from the joint
  float F[3], N[3];
  {
    float t0[3], t1[3], ac[3], Iw[3], Ial[3], wIw[3], cxf[3];
    cross3(k.al, cb, t0);
    cross3(k.w, cb, t1); cross3(k.w, t1, t1);
#pragma unroll
    for (int c = 0; c < 3; c++) ac[c] = k.ao[c] + t0[c] + t1[c];
#pragma unroll
    for (int c = 0; c < 3; c++) F[c] = WRENCH ? m * ac[c] - W[c] : m * ac[c];
    sym3_mul(Ic, k.w, Iw); sym3_mul(Ic, k.al, Ial);
    cross3(k.w, Iw, wIw); cross3(cb, F, cxf);     // (the lever of the body wrench rides in F)
#pragma unroll
    for (int c = 0; c < 3; c++) N[c] = WRENCH ? Ial[c] + wIw[c] - W[3 + c] + cxf[c] : Ial[c] + wIw[c] + cxf[c];
  }
  // ---- inward, level by level: a body adds its children's force, and their moment shifted by the lever child -> body
  if (is_body) {
    float *o = rec + 16 * b;
#pragma unroll
    for (int c = 0; c < 3; c++) { o[c] = F[c]; o[3 + c] = N[c]; o[6 + c] = k.r[c]; }
  }
  __syncthreads();
  for (int d = maxdepth - 1; d >= 0; d--) {
    if (depth == d) {
      bool any = false;
      for (int kc = 0; kc < MAXCH; kc++) {
        const int ch = M->child[kc][b];
        if (ch < 0) break;
        const float *o = rec + 16 * ch;
        const float Fc[3] = {o[0], o[1], o[2]}, lever[3] = {o[6] - k.r[0], o[7] - k.r[1], o[8] - k.r[2]};
        float lxf[3];
        cross3(lever, Fc, lxf);
#pragma unroll
        for (int c = 0; c < 3; c++) { F[c] += Fc[c]; N[c] += o[3 + c] + lxf[c]; }
        any = true;
      }
      if (any) {
        float *o = rec + 16 * b;
#pragma unroll
        for (int c = 0; c < 3; c++) { o[c] = F[c]; o[3 + c] = N[c]; }
      }
    }
    __syncthreads();
  }
  if (is_body) {
    if (b == 0) {
#pragma unroll
      for (int c = 0; c < 3; c++) { stage_base[c] = F[c]; stage_base[3 + c] = N[c]; }
    } else {
      float *o = stage + 6 * M->obs_slot[b];
      if constexpr (LINK) {   // world -> body: R^T
#pragma unroll
        for (int c = 0; c < 3; c++) {
          o[c] = k.R[c] * F[0] + k.R[3 + c] * F[1] + k.R[6 + c] * F[2];
          o[3 + c] = k.R[c] * N[0] + k.R[3 + c] * N[1] + k.R[6 + c] * N[2];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; c++) { o[c] = F[c]; o[3 + c] = N[c]; }
      }
    }
  }
  __syncthreads();
  const int envs_here = min(WAVES, A.n_envs - env0);
  block_store(A.out + (size_t)env0 * 6 * J, rows, envs_here * 6 * J);
  if (A.base_out) block_store(A.base_out + (size_t)env0 * 6, rows + WAVES * 6 * J, envs_here * 6);
}

// One env per 32-lane team: lane b >= 1 carries the velocity of its joint, lanes 0 .. 5 also the base's six. Every element is read
// (prev) and written (vel) by the same thread, so vel may be prev itself.
__global__ void trex_generalized_velocity_kernel(TrexGenVelArgs A) {
  const int env = blockIdx.x * (blockDim.x / TL) + threadIdx.x / TL;
  const int lane = threadIdx.x & (TL - 1);
  if (env >= A.n_envs) return;
  const TrexDeviceModel *M = A.model;
  const int nb = M->nb, D = 6 + nb - 1;
  const bool zero = A.done && A.done[(size_t)env * A.done_stride] != 0.f;
  const size_t row = (size_t)env * D;
#pragma unroll
  for (int part = 0; part < 2; part++) {
    int idx;
    float cur;
    if (part == 0) {
      if (lane >= 6) continue;
      idx = lane; cur = A.base[(size_t)env * 16 + 7 + lane];
    } else {
      if (lane < 1 || lane >= nb) continue;
      idx = 6 + M->obs_slot[lane]; cur = A.qd[(size_t)env * TL + lane];
    }
    if (A.prev) {
      const float diff = cur - A.prev[row + idx];
      A.accel[row + idx] = zero ? 0.f : diff * A.inv_dt;
    }
    if (A.vel) A.vel[row + idx] = cur;
  }
}

}  // namespace

extern "C" hipError_t trex_launch_joint_wrench(const TrexJwArgs &args, hipStream_t stream) {
  if (args.n_envs <= 0 || args.nb < 2 || args.nb > TL || !args.out) return hipErrorInvalidValue;
  const dim3 grid((args.n_envs + WAVES - 1) / WAVES), block(BLOCK);
  const size_t lds = (size_t)trex_jw_lds_bytes(args.nb);
  const bool wrench = args.wrench_a || args.wrench_b, link = args.link_axes != 0;
  if (wrench && link) hipLaunchKernelGGL((trex_joint_wrench_kernel<true, true>), grid, block, lds, stream, args);
  else if (wrench) hipLaunchKernelGGL((trex_joint_wrench_kernel<true, false>), grid, block, lds, stream, args);
  else if (link) hipLaunchKernelGGL((trex_joint_wrench_kernel<false, true>), grid, block, lds, stream, args);
  else hipLaunchKernelGGL((trex_joint_wrench_kernel<false, false>), grid, block, lds, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_generalized_velocity(const TrexGenVelArgs &args, hipStream_t stream) {
  if (args.n_envs <= 0 || (args.prev && !args.accel)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trex_generalized_velocity_kernel, dim3((args.n_envs + 7) / 8), dim3(256), 0, stream, args);
  return hipGetLastError();
}
