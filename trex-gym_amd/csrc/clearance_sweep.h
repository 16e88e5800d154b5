// The chain walk into LDS and the sweep over an env's collision points: phases 1 to 3 of the floor-clearance kernel
// (termination.hip, which describes them), shared with the floor placement of start_state.hip. One env per wavefront of
// TREX_TERM_BLOCK lanes. Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

#include "chain_walk.h"
#include "device_math.h"
#include "termination.h"

constexpr int CLR_POSE = 12;   // LDS floats per body: R 9 (row-major) | origin 3, relative to the base origin

// float -> u32 whose unsigned order is the float order, and back (as proximity.hip)
__device__ __forceinline__ uint32_t clr_ordered_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ float clr_ordered_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
constexpr uint32_t CLR_NO_POINT = 0xFFFFFFFFu;
constexpr unsigned long long CLR_EMPTY = (0xFF800000ull << 32) | CLR_NO_POINT;   // +inf, no point: a body without collision points

// Phases 1 to 3 for body lane t of env: -> the body's clearance (+inf: no collision points) and the index of its lowest point.
// `sweep` false skips phase 2 (a predicate launch that watches no body). HEAD: lane head_body also returns the world z of the
// head point, with the arithmetic of trex_head_kernel (batch_util.hip). Every lane of the wave calls it. Of `a` it reads model,
// base, q and hull. sPose [TREX_TL * CLR_POSE], sStart [TREX_TL + 1], sBest [TREX_TL]: LDS; behind the call sBest[b] holds body
// b's (order-preserving bits of the lowest height relative to the base origin << 32 | point index), CLR_EMPTY for a body without
// points.
template <bool HEAD>
__device__ __forceinline__ float body_clearance(const TrexTermArgs &a, int env, int t, bool sweep, float *sPose, int *sStart,
                                                unsigned long long *sBest, uint32_t &lowest, float &head_z) {
  constexpr int BLOCK = TREX_TERM_BLOCK, TL = TREX_TL, POSE = CLR_POSE;
  const TrexDeviceModel *M = a.model;
  const int nb = M->nb;
  const float *base = a.base + (size_t)env * 16;
  head_z = 0.f;
  if (t < TL) sBest[t] = CLR_EMPTY;
  if (t <= TL) sStart[t] = M->hull_start[t];
  if (t < nb) {
    const float *const none = nullptr;
    Walk k;
    walk_chain<false, false>(M, a.base, a.q, none, none, env, t, 0, k);
    float *o = sPose + t * POSE;
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = k.R[c];
#pragma unroll
    for (int c = 0; c < 3; c++) o[9 + c] = k.r[c];
    if (HEAD && t == M->head_body) {
      const float hp[3] = {M->head_point[0], M->head_point[1], M->head_point[2]};
      float w[3];
      matvec3(k.R, hp, w);
      head_z = base[2] + k.r[2] + w[2];
    }
  }
  __syncthreads();

  if (sweep) {
    const int nv = sStart[nb];
    int b = 0, cur = -1;
    unsigned long long key = ~0ull;
    for (int v = t; v < nv; v += BLOCK) {
      while (v >= sStart[b + 1]) b++;   // (v < nv = sStart[nb]: ends at a body < nb)
      if (b != cur) {
        if (cur >= 0) atomicMin(&sBest[cur], key);
        cur = b;
        key = ~0ull;
      }
      const float *P = sPose + b * POSE;
      const float4 p = a.hull[v];
      const float h = ((P[6] * p.x + P[7] * p.y + P[8] * p.z) + P[11]) - p.w;
      const unsigned long long kv = ((unsigned long long)clr_ordered_bits(h) << 32) | (uint32_t)v;
      key = kv < key ? kv : key;
    }
    if (cur >= 0) atomicMin(&sBest[cur], key);
  }
  __syncthreads();

  float clr = INFINITY;
  lowest = CLR_NO_POINT;
  if (t < nb) {
    const unsigned long long best = sBest[t];
    lowest = (uint32_t)best;
    if (lowest != CLR_NO_POINT) clr = clr_ordered_float((uint32_t)(best >> 32)) + (base[2] - M->prm[TP_FLOOR_Z]);
  }
  return clr;
}
