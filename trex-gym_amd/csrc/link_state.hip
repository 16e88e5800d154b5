// Batched link kinematics (trex_batch_link_state, include/trex_batch.h): pose, velocity and classical acceleration of points
// fixed in URDF links - the probes of a set - at the batch's current state. One lane per probe; a workgroup of 256 lanes serves up
// to 8 whole envs (few probes per env) or one 256-probe chunk of one env (many): trex_link_shape. Reads only: the kernel writes
// nothing but the outputs.
//
// Phase 1: lane (slot, body) walks its body's chain once (chain_walk.h) and parks the body's record in LDS. Phase 2: lane
// (slot, probe) composes its body's record with the probe's body <- link transform and its point. Three instantiations - pose,
// pose + velocity, all three - so that a pose query neither loads qd nor carries the velocity recursion.
#include <hip/hip_runtime.h>

#include "../../include/trex_batch.h"
#include "chain_walk.h"
#include "device_math.h"
#include "link_state.h"
#include "quat_math.h"

namespace {

constexpr int BLOCK = TREX_LINK_BLOCK;
constexpr int MAXENV = TREX_LINK_MAXENV;
constexpr int REC = TREX_LINK_REC;
constexpr int SLOT = TREX_LINK_SLOT;

// o = m^T v: a world vector in the axes whose world rotation is m
__device__ __forceinline__ void tmatvec3(const float *m, const float *v, float *o) {
  const float x = m[0] * v[0] + m[3] * v[1] + m[6] * v[2];
  const float y = m[1] * v[0] + m[4] * v[1] + m[7] * v[2];
  const float z = m[2] * v[0] + m[5] * v[1] + m[8] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}

}  // namespace

// LEVEL 0: pose; 1: + velocity; 2: + acceleration. Every output stays nullable within its instantiation.
template <int LEVEL>
__global__ __launch_bounds__(256) void trex_link_state_kernel(TrexLinkArgs a) {
  constexpr bool VEL = LEVEL >= 1, ACC = LEVEL >= 2;
  // per env slot and body: R (row-major) | origin, relative to the base origin | w | vo | al | ao (+ g z)
  __shared__ __attribute__((aligned(16))) float sRec[MAXENV * SLOT];

  const TrexDeviceModel *M = a.model;
  const int t = threadIdx.x;
  const int K = a.num_probes, epw = a.epw;
  const int group = blockIdx.x / a.cpe, chunk = blockIdx.x - group * a.cpe;
  const int env0 = group * epw;

  // ---- phase 1: lane t walks the chain of body t & 31 of env slot t >> 5
  {
    const int s = t >> 5, bd = t & 31, env = env0 + s;
    if (s < epw && env < a.n_envs && bd < M->nb) {
      Walk k;
      walk_chain<VEL, ACC>(M, a.base, a.q, a.qd, a.accel, env, bd, a.D, k);
      float *o = sRec + s * SLOT + bd * REC;
#pragma unroll
      for (int c = 0; c < 9; c++) o[c] = k.R[c];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        o[9 + c] = k.r[c];
        if (VEL) { o[12 + c] = k.w[c]; o[15 + c] = k.vo[c]; }
        if (ACC) { o[18 + c] = k.al[c]; o[21 + c] = k.ao[c]; }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: this lane's probe. (Lanes past the batch's or the set's end have met the barrier and write nothing.)
  int s, probe;
  if (epw == 1) {
    s = 0; probe = chunk * BLOCK + t;
  } else {
    s = t / K; probe = t - s * K;
  }
  const int env = env0 + s;
  if (!(s < epw && env < a.n_envs && probe < K)) return;
  const size_t g = (size_t)env * K + probe;
  const float *P = sRec + s * SLOT + a.probe_body[probe] * REC;
  const float *tf = a.probe_tf + 12 * (size_t)probe;
  float Rl[9], d[3];
  matmul3(P, tf, Rl);       // world <- link
  matvec3(P, tf + 9, d);    // body origin -> the point, world axes

  // the axes the vectors are expressed in: world <- axes rotation A (WORLD: none)
  const int axes = a.axes;
  float A[9], e0[3] = {0.f, 0.f, 0.f};
  if (axes == TREX_AXES_BASE) {   // URDF link 0's frame, from its body's record of this env
    const float *P0 = sRec + s * SLOT + a.base_body * REC;
    matmul3(P0, a.base_tf, A);
    matvec3(P0, a.base_tf + 9, e0);
#pragma unroll
    for (int c = 0; c < 3; c++) e0[c] += P0[9 + c];   // its origin, relative to the base origin
  } else {
#pragma unroll
    for (int c = 0; c < 9; c++) A[c] = Rl[c];
  }

  if (a.pose) {
    float *w = a.pose + g * 7;
    if (axes == TREX_AXES_BASE) {
      float e[3], p[3], Rr[9];
#pragma unroll
      for (int c = 0; c < 3; c++) e[c] = (P[9 + c] - e0[c]) + d[c];
      tmatvec3(A, e, p);
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rr[3 * i + j] = A[i] * Rl[j] + A[3 + i] * Rl[3 + j] + A[6 + i] * Rl[6 + j];
#pragma unroll
      for (int c = 0; c < 3; c++) w[c] = p[c];
      mat_to_quat(Rr, w + 3);
    } else {
      const float *b = a.base + (size_t)env * 16;
#pragma unroll
      for (int c = 0; c < 3; c++) w[c] = (b[c] + P[9 + c]) + d[c];
      mat_to_quat(Rl, w + 3);
    }
  }
  if (VEL) {
    const float *wv = P + 12;
    float lin[3], ang[3] = {wv[0], wv[1], wv[2]};
    cross3(wv, d, lin);
#pragma unroll
    for (int c = 0; c < 3; c++) lin[c] += P[15 + c];
    if (a.vel) {
      float *w = a.vel + g * 6;
      float ol[3] = {lin[0], lin[1], lin[2]}, oa[3] = {ang[0], ang[1], ang[2]};
      if (axes != TREX_AXES_WORLD) { tmatvec3(A, lin, ol); tmatvec3(A, ang, oa); }
#pragma unroll
      for (int c = 0; c < 3; c++) { w[c] = ol[c]; w[3 + c] = oa[c]; }
    }
    if (ACC && a.acc) {
      // a_p = ao + al x d + w x (w x d); ao carries + g z from the walk: the specific force, taken out again unless `proper`
      const float *alv = P + 18;
      float wxd[3], wwd[3], axd[3], la[3], aa[3] = {alv[0], alv[1], alv[2]};
      cross3(wv, d, wxd);
      cross3(wv, wxd, wwd);
      cross3(alv, d, axd);
#pragma unroll
      for (int c = 0; c < 3; c++) la[c] = P[21 + c] + axd[c] + wwd[c];
      if (!a.proper) la[2] -= M->prm[TP_GRAVITY];
      float *w = a.acc + g * 6;
      float ol[3] = {la[0], la[1], la[2]}, oa[3] = {aa[0], aa[1], aa[2]};
      if (axes != TREX_AXES_WORLD) { tmatvec3(A, la, ol); tmatvec3(A, aa, oa); }
#pragma unroll
      for (int c = 0; c < 3; c++) { w[c] = ol[c]; w[3 + c] = oa[c]; }
    }
  }
}

extern "C" hipError_t trex_launch_link_state(const TrexLinkArgs &args, hipStream_t stream) {
  TrexLinkArgs a = args;
  trex_link_shape(a.num_probes, &a.epw, &a.cpe);
  const int groups = (a.n_envs + a.epw - 1) / a.epw;
  const dim3 grid((unsigned)groups * (unsigned)a.cpe), block(BLOCK);
  if (a.acc) {
    hipLaunchKernelGGL(trex_link_state_kernel<2>, grid, block, 0, stream, a);
  } else if (a.vel) {
    a.accel = nullptr;
    hipLaunchKernelGGL(trex_link_state_kernel<1>, grid, block, 0, stream, a);
  } else {
    a.accel = nullptr; a.qd = nullptr;
    hipLaunchKernelGGL(trex_link_state_kernel<0>, grid, block, 0, stream, a);
  }
  return hipGetLastError();
}
