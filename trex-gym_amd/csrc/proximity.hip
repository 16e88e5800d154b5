// Batched closest-point queries between bodies (trex_batch_proximity, include/trex_batch.h): for every env and every body pair of
// the batch's proximity table the closest capsule of A and capsule of B at the env's current state - signed distance, the two
// surface points, the normal from B to A and the winning capsules. One workgroup of 256 lanes per env. Reads only: the kernel
// writes nothing but the outputs.
//
// Phase 1: lane b walks body b's chain once (chain_walk.h) and parks its pose in LDS. Phase 2: lane c carries capsule c to world
// axes, relative to the env's base origin (differences of nearby points then keep their f32 digits wherever the env stands).
// Phase 3: the lanes stride over the host-built list of capsule-pair tests - sorted by (pair, capsule of A, capsule of B) - and
// reduce per pair with a 64-bit LDS atomic min on (order-preserving bits of the distance << 32 | test index): ties go to the
// earlier test, and the result does not depend on the order of arrival. The lanes of a wave that share a pair are reduced in
// registers first (a segmented scan over the sorted list), so one lane per pair and wave goes to LDS. Phase 4: lane p recomputes
// the winner of pair p and writes its row.
#include <hip/hip_runtime.h>

#include "../../include/trex_batch.h"
#include "chain_walk.h"
#include "device_math.h"
#include "proximity.h"

namespace {

constexpr int BLOCK = TREX_PROX_BLOCK;
constexpr int POSE = 12;   // LDS floats per body: R 9 (row-major) | origin 3, relative to the base origin

// float -> u32 whose unsigned order is the float order (NaNs at either end), and back
__device__ __forceinline__ uint32_t ordered_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ float ordered_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // (a NaN gives 0)

// Closest points of the segments p1 + s d1 and p2 + t d2, s and t in [0, 1] (a zero d: a point); i1, i2 = 1 / |d|^2, 0 for a point.
// s starts at the closest point of the two LINES, through n = d1 x d2: s = n . (d2 x r) / |n|^2, the same number as
// (b f - c e) / (a e - b^2) without the cancellation that leaves no digit of a e - b^2 below 1e-3 rad between the axes (a 1-ulp
// reciprocal will do: s is only where the two projections start); then t is the best answer to s and s the best answer to t,
// each clamped. -> diff = (p1 + s d1) - (p2 + t d2) and the two parameters.
__device__ __forceinline__ void segment_closest(const float *p1, const float *d1, float i1, const float *p2, const float *d2, float i2,
                                                float *diff, float &s, float &t) {
  const float r[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  const float b = dot3(d1, d2), c = dot3(d1, r), f = dot3(d2, r);
  float n[3], m[3];
  cross3(d1, d2, n);
  cross3(d2, r, m);
  const float nn = dot3(n, n);
  s = nn > 0.f ? clamp01(dot3(n, m) * __builtin_amdgcn_rcpf(nn)) : 0.f;
  t = clamp01((b * s + f) * i2);
  s = clamp01((b * t - c) * i1);
#pragma unroll
  for (int k = 0; k < 3; k++) diff[k] = (r[k] + s * d1[k]) - t * d2[k];
}

}  // namespace

__global__ __launch_bounds__(256) void trex_proximity_kernel(TrexProxArgs a) {
  __shared__ __attribute__((aligned(16))) float sPose[TREX_TL * POSE];
  // per capsule: p0 xyz, radius | d = p1 - p0 xyz, 1 / |d|^2 (a sphere: 0) - world axes, relative to the base origin
  __shared__ __attribute__((aligned(16))) float sCap[TREX_PROX_MAXCAPS * 8];
  __shared__ unsigned long long sBest[TREX_PROX_MAXPAIRS];

  const TrexDeviceModel *M = a.model;
  const int t = threadIdx.x, env = blockIdx.x;
  const int C = a.num_capsules, P = a.num_pairs, T = a.num_tests;

  // ---- phase 1: lane b < nb walks the chain of body b. Every pair starts at its own first test with the largest key: whatever
  // wins - a NaN included - is a test of this pair
  if (t < M->nb) {
    const float *const none = nullptr;
    Walk k;
    walk_chain<false, false>(M, a.base, a.q, none, none, env, t, 0, k);
    float *o = sPose + t * POSE;
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = k.R[c];
#pragma unroll
    for (int c = 0; c < 3; c++) o[9 + c] = k.r[c];
  }
  for (int p = t; p < P; p += BLOCK) sBest[p] = (0xFFFFFFFFull << 32) | (uint32_t)a.pair_first[p];
  __syncthreads();

  // ---- phase 2: capsule c to world axes
  for (int c = t; c < C; c += BLOCK) {
    const float *B = sPose + a.cap_body[c] * POSE;
    const float *src = a.cap + 8 * (size_t)c;
    float w0[3], w1[3];
    matvec3(B, src, w0);
    matvec3(B, src + 4, w1);
    float *o = sCap + 8 * c;
    float dd = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float x0 = w0[k] + B[9 + k], x1 = w1[k] + B[9 + k], d = x1 - x0;   // (a sphere: p1 = p0 in the table, so exactly 0)
      o[k] = x0;
      o[4 + k] = d;
      dd += d * d;
    }
    o[3] = src[3];
    o[7] = dd > 0.f ? 1.f / dd : 0.f;
  }
  __syncthreads();

  // ---- phase 3: every test once; the trip count is the same for all lanes (the scan below shuffles across the wave)
  const int lane = t & 63;
  for (int i0 = 0; i0 < T; i0 += BLOCK) {
    const int i = i0 + t;
    int pair = -1;                           // (past the end: a segment of its own kind, never sent to LDS)
    unsigned long long key = ~0ull;
    if (i < T) {
      const uint32_t w = a.test[i];
      pair = (int)(w >> 16);
      const float *A = sCap + 8 * ((w >> 8) & 255u), *B = sCap + 8 * (w & 255u);
      float diff[3], s, u;
      segment_closest(A, A + 4, A[7], B, B + 4, B[7], diff, s, u);
      const float d = __builtin_amdgcn_sqrtf(dot3(diff, diff)) - A[3] - B[3];   // (1 ulp: what the pairs are ranked by, and reported)
      key = ((unsigned long long)ordered_bits(d) << 32) | (uint32_t)i;
    }
    // segmented min towards the first lane of each run of equal pairs: `run` = the lanes behind this one in its run. (Measured
    // against every lane going to LDS by itself, 4 096 envs: 35 against 34 us on the T-rex table, 995 against 1 274 us where
    // 16 384 tests share a pair - profiles/r18_proximity.txt.)
    const int before = __shfl_up(pair, 1);
    const bool head = lane == 0 || before != pair;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run = above ? __ffsll((long long)above) - 1 : 63 - lane;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long ok = __shfl_down(key, off);
      if (off <= run && ok < key) key = ok;
    }
    if (i < T && head) atomicMin(&sBest[pair], key);
  }
  __syncthreads();

  // ---- phase 4: lane p writes pair p's row
  const float *base = a.base + (size_t)env * 16;
  for (int p = t; p < P; p += BLOCK) {
    const unsigned long long best = sBest[p];
    const uint32_t w = a.test[(uint32_t)best];
    const int ca = (int)((w >> 8) & 255u), cb = (int)(w & 255u);
    const size_t g = (size_t)env * P + p;
    a.distance[g] = ordered_float((uint32_t)(best >> 32));
    if (a.capsule) { a.capsule[2 * g] = ca; a.capsule[2 * g + 1] = cb; }
    if (a.point_a || a.point_b || a.normal) {
      const float *A = sCap + 8 * ca, *B = sCap + 8 * cb;
      float diff[3], s, u;
      segment_closest(A, A + 4, A[7], B, B + 4, B[7], diff, s, u);
      const float len = sqrtf(dot3(diff, diff));
      float n[3] = {0.f, 0.f, 1.f};
      if (!(len < TREX_PROX_EPS)) {
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = diff[k] / len;
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (a.normal) a.normal[3 * g + k] = n[k];
        if (a.point_a) a.point_a[3 * g + k] = (base[k] + (A[k] + s * A[4 + k])) - A[3] * n[k];
        if (a.point_b) a.point_b[3 * g + k] = (base[k] + (B[k] + u * B[4 + k])) + B[3] * n[k];
      }
    }
  }
}

extern "C" hipError_t trex_launch_proximity(const TrexProxArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(trex_proximity_kernel, dim3((unsigned)args.n_envs), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}
