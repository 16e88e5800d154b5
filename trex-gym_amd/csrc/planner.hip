// The planner's kernels (include/trex_planner.h, which states the semantics and the random numbers): K21. Sampling - knots and
// the interpolated action block in one launch -, the update - returns, the groups' weights, the new nominal: three launches -,
// the receding-horizon shift and the nominal's action.
//
// Sample launch: a workgroup owns `tile` consecutive envs (16, fewer where P A is large) and keeps their knots [tile][P][A] in LDS
// (32 KB at most). Phase 1: an item is (env, knot, four actions) - ONE Philox evaluation serves the four - written to LDS and
// to the planner's knots. Phase 2: a lane owns one (env, action) column of the tile and walks the S steps; the tap set of a step
// is wave-uniform (scalar loads), the store of a step is `tile * A` consecutive floats of the [S, N, A] block. The sample count
// is read by every workgroup's lane 0 before the workgroup counts itself in (an integer atomic); the last one in moves it on.
//
// Update: (1) one lane per env walks its S rewards - a strided read, accepted - without a branch on done, so that the loads
// pipeline; (2) one workgroup per group: R_max and the smallest k at it by a tree (max is exact, so the tree changes no bit), the
// weights lane-parallel, then the three sequential sums of the header by three lanes of three waves out of LDS; (3) a workgroup
// per 64 (p, a) elements of a group - G ceil(P A / 64) workgroups, so that G = 1, K = 4096 is spread over ceil(P A / 64) CUs -
// whose four waves load tiles of samples, coalesced along (p, a), while its wave 0 sums w_k knot_k over k in the header's order,
// one lane per element.
// No scratch, no float atomics; every "rounded, no fma" product passes through product() of philox.h.
#include "planner.h"

#include "philox.h"

namespace {

constexpr int BLOCK = TREX_PLAN_BLOCK;
constexpr int SUM_BLOCK = TREX_PLAN_SUM_BLOCK;
constexpr int SUM_TILE = TREX_PLAN_SUM_TILE;
constexpr float TWO_PI = 6.2831855f;
constexpr float NEG_INF = -__builtin_huge_valf();

__device__ __forceinline__ float clip(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// output j of a block's four standard normals (include/trex_sensing.h)
__device__ __forceinline__ float normal(const uint32_t (&r)[4], int j) {
  const int p = j & 2;
  const float R = sqrtf(__fmul_rn(-2.f, logf(u_open_closed(r[p])))), ang = __fmul_rn(TWO_PI, u_half_open(r[p + 1]));
  return __fmul_rn(R, (j & 1) ? sinf(ang) : cosf(ang));
}

// ((w0 k0 + w1 k1) + w2 k2) + w3 k3 of the knots `stride` floats apart
__device__ __forceinline__ float taps4(const TrexPlanTap &t, const float *knot, int stride) {
  float v = product(t.w[0], knot[t.i[0] * stride]);
  v = v + product(t.w[1], knot[t.i[1] * stride]);
  v = v + product(t.w[2], knot[t.i[2] * stride]);
  return v + product(t.w[3], knot[t.i[3] * stride]);
}

__global__ __launch_bounds__(BLOCK) void trex_plan_sample_kernel(TrexPlanSampleArgs a) {
  __shared__ float s_knot[TREX_PLAN_TILE_FLOATS];
  __shared__ uint32_t s_it;
  const TrexPlanState &st = a.st;
  const int P = st.P, A = st.A, PA = P * A, A4 = (A + 3) >> 2;
  const int e0 = blockIdx.x * a.tile, ne = min(a.tile, st.N - e0);
  if (threadIdx.x == 0) s_it = st.it[0];
  __syncthreads();
  const uint32_t it = s_it;
  const TrexPlanNoise *nz = st.noise;
  const int items = ne * P * A4;
  for (int i = threadIdx.x; i < items; i += BLOCK) {
    const int a4 = i % A4, p = (i / A4) % P, el = i / (A4 * P);
    const int e = e0 + el, g = e / st.K, k = e - g * st.K, c0 = a4 * 4;
    const float *nom = st.nominal + ((size_t)g * P + p) * A;
    float v[4], sg[4];
    bool draw = false;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = c0 + j;
      v[j] = c < A ? nom[c] : 0.f;
      sg[j] = c < A ? nz->sigma[c] : 0.f;
      draw |= sg[j] > 0.f;
    }
    uint32_t r[4] = {0u, 0u, 0u, 0u};
    if (k > 0 && draw) philox(a.env_offset + (uint32_t)e, it, ((uint32_t)TREX_PLAN_STREAM << 16) | (uint32_t)a4, (uint32_t)p, a.key0, a.key1, r);
    float *out = st.knots + (size_t)e * PA + p * A;
    float *lds = s_knot + el * PA + p * A;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = c0 + j;
      if (c < A) {
        float y = v[j];
        if (k > 0 && sg[j] > 0.f) y = y + product(sg[j], normal(r, j));   // (a sigma of 0 adds nothing)
        y = clip(y, nz->lo[c], nz->hi[c]);
        lds[c] = y;
        out[c] = y;
      }
    }
  }
  __syncthreads();   // the tile's knots are in LDS; every lane of the workgroup holds `it`
  if (threadIdx.x == 0) {
    const uint32_t before = atomicAdd(&st.it[1], 1u);
    if (before == gridDim.x - 1) {   // every workgroup has read the count: it moves on, the arrivals start afresh
      st.it[1] = 0u;
      st.it[0] = it + 1u;
    }
  }
  const size_t plane = (size_t)st.N * A;
  float *out = a.actions + (size_t)e0 * A;
  for (int i = threadIdx.x; i < ne * A; i += BLOCK) {
    const int el = i / A, c = i - el * A;
    const float lo = nz->lo[c], hi = nz->hi[c];
    const float *knot = s_knot + el * PA + c;
    for (int s = 0; s < st.S; s++) out[(size_t)s * plane + i] = clip(taps4(st.taps[s], knot, A), lo, hi);
  }
}

__global__ __launch_bounds__(BLOCK) void trex_plan_return_kernel(TrexPlanUpdateArgs a) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= a.st.N) return;
  const float *r = a.reward + (size_t)e * a.env_stride, *d = a.done ? a.done + (size_t)e * a.env_stride : nullptr;
  float R = 0.f;
  bool live = true;
  // (no branch on done: the loads of the steps behind it are in bounds, and four steps' loads are in flight together)
  for (int s0 = 0; s0 < a.st.S; s0 += 4) {
    float rew[4], dn[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int s = min(s0 + j, a.st.S - 1);
      rew[j] = r[(size_t)s * a.step_stride];
      dn[j] = d ? d[(size_t)s * a.step_stride] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int s = s0 + j;
      const float next = R + product(a.discount[min(s, a.st.S)], rew[j]);
      R = live && s < a.st.S ? next : R;
      live = live && dn[j] == 0.f;
    }
  }
  if (live && a.terminal) R = R + product(a.discount[a.st.S], a.terminal[e]);
  if (!(fabsf(R) < __builtin_huge_valf())) R = NEG_INF;     // NaN and both infinities
  a.returns[e] = R;
  if (a.returns_out) a.returns_out[e] = R;
}

// One sequential sum over n values in LDS (n a multiple of 32, the array 16-byte aligned), 32 of them read ahead of their adds.
// ROLE 0: sum x; 1: sum x x; 2: sum and count the x above -inf.
template <int ROLE> __device__ __forceinline__ void chain(const float *values, int n, float &sum, int &count) {
  const float4 *src = reinterpret_cast<const float4 *>(values);
  for (int k4 = 0; k4 < n / 4; k4 += 8) {
    float4 v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = src[k4 + j];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        if (ROLE == 0) sum = sum + x[c];
        if (ROLE == 1) sum = sum + product(x[c], x[c]);
        if (ROLE == 2) {
          const bool finite = x[c] > NEG_INF;
          const float next = sum + (finite ? x[c] : 0.f);
          sum = finite ? next : sum;
          count += finite ? 1 : 0;
        }
      }
    }
  }
}

__global__ __launch_bounds__(BLOCK) void trex_plan_group_kernel(TrexPlanUpdateArgs a) {
  __shared__ __align__(16) float s_R[TREX_PLAN_MAXSAMPLES], s_w[TREX_PLAN_MAXSAMPLES];
  __shared__ float s_m[BLOCK];
  __shared__ int s_k[BLOCK];
  __shared__ float s_sum[4];
  const int g = blockIdx.x, K = a.st.K, tid = threadIdx.x;
  const size_t e0 = (size_t)g * K;
  float m = NEG_INF;
  int mk = 0x7fffffff;
  for (int k = tid; k < K; k += BLOCK) {
    const float R = a.returns[e0 + k];
    s_R[k] = R;
    if (R > m) { m = R; mk = k; }      // (k rises: the first k at a lane's maximum stays)
  }
  s_m[tid] = m; s_k[tid] = mk;
  __syncthreads();
  for (int half = BLOCK / 2; half > 0; half >>= 1) {
    if (tid < half) {
      const float m2 = s_m[tid + half];
      const int k2 = s_k[tid + half];
      if (m2 > s_m[tid] || (m2 == s_m[tid] && k2 < s_k[tid])) { s_m[tid] = m2; s_k[tid] = k2; }
    }
    __syncthreads();
  }
  const float R_max = s_m[0];
  const int best = R_max > NEG_INF ? s_k[0] : -1;
  for (int k = tid; k < K; k += BLOCK) {
    float w = 0.f;
    if (best >= 0) w = a.temperature > 0.f ? expf((s_R[k] - R_max) / a.temperature) : (k == best ? 1.f : 0.f);
    s_w[k] = w;
    a.weights[e0 + k] = w;
    if (a.weights_out) a.weights_out[e0 + k] = w;
  }
  // (behind K, up to the next multiple of 32: weights of 0 and returns of -inf, which change no bit of a sum below)
  const int Kpad = (K + 31) & ~31;
  for (int k = K + tid; k < Kpad; k += BLOCK) { s_w[k] = 0.f; s_R[k] = NEG_INF; }
  __syncthreads();
  // the header's sequential sums: lane 0 of three waves, one chain each, 32 values read from LDS ahead of their adds
  const int role = __builtin_amdgcn_readfirstlane(tid / 64);      // the wave: 0 sums w, 1 sums w w, 2 the finite returns
  if ((tid & 63) == 0 && role < 3) {      // (one straight-line loop per role: no branch between two adds)
    float sum = 0.f;
    int count = 0;
    if (role == 0) chain<0>(s_w, Kpad, sum, count);
    else if (role == 1) chain<1>(s_w, Kpad, sum, count);
    else chain<2>(s_R, Kpad, sum, count);
    if (role == 0) s_sum[0] = sum;
    else if (role == 1) s_sum[1] = sum;
    else { s_sum[2] = sum; s_sum[3] = (float)count; }
  }
  __syncthreads();
  if (tid == 0) {
    const float sw = s_sum[0], sw2 = s_sum[1], count = s_sum[3];
    a.sums[(size_t)g * 4] = sw;
    a.best[g] = best;
    if (a.best_out) a.best_out[g] = best;
    if (a.stats_out) {
      float *st = a.stats_out + (size_t)g * 4;
      st[0] = R_max;
      st[1] = count > 0.f ? s_sum[2] / count : 0.f;
      st[2] = sw2 > 0.f ? product(sw, sw) / sw2 : 0.f;
      st[3] = s_R[0];
    }
  }
}

// A workgroup owns 64 (p, a) elements of one group. Its four waves LOAD together - a tile of SUM_TILE samples x 64 elements, 28
// loads of 256 contiguous bytes in flight per lane - and wave 0 alone ADDS, in the header's order, out of LDS: the tile behind
// the one in flight (two LDS buffers, one barrier per tile). A sample beyond K enters as 0 * 0, which changes no bit of the sum.
__global__ __launch_bounds__(BLOCK) void trex_plan_nominal_kernel(TrexPlanUpdateArgs a) {
  constexpr int ROWS = BLOCK / SUM_BLOCK, PER = SUM_TILE / ROWS;      // 4 waves, 28 samples of a tile each
  __shared__ float s_x[2][SUM_TILE][SUM_BLOCK];
  __shared__ float s_wt[2][SUM_TILE];
  const int PA = a.st.P * a.st.A, per = (PA + SUM_BLOCK - 1) / SUM_BLOCK, K = a.st.K;
  const int g = blockIdx.x / per, lane = threadIdx.x % SUM_BLOCK, row = threadIdx.x / SUM_BLOCK;
  const int i = (blockIdx.x - g * per) * SUM_BLOCK + lane;
  const bool in = i < PA;
  const int best = a.best[g];
  if (best < 0) return;                  // (a group with no finite return keeps its nominal; the whole workgroup leaves)
  const float *knot = a.st.knots + (size_t)g * K * PA + (in ? i : 0);
  float *nom = a.st.nominal + (size_t)g * PA + i;
  if (!(a.temperature > 0.f)) {
    if (row == 0 && in) *nom = knot[(size_t)best * PA];
    return;
  }
  const float *w = a.weights + (size_t)g * K;
  const int tiles = (K + SUM_TILE - 1) / SUM_TILE;
  float x[PER], wt = 0.f;
  auto load = [&](int t) {
#pragma unroll
    for (int j = 0; j < PER; j++) {
      const int k = t * SUM_TILE + j * ROWS + row;
      x[j] = k < K ? knot[(size_t)k * PA] : 0.f;
    }
    const int k = t * SUM_TILE + (int)threadIdx.x;
    wt = threadIdx.x < SUM_TILE && k < K ? w[k] : 0.f;
  };
  auto store = [&](int b) {
#pragma unroll
    for (int j = 0; j < PER; j++) s_x[b][j * ROWS + row][lane] = x[j];
    if (threadIdx.x < SUM_TILE) s_wt[b][threadIdx.x] = wt;
  };
  load(0);
  store(0);
  __syncthreads();
  float acc = 0.f;
  for (int t = 0; t < tiles; t++) {
    const int b = t & 1;
    if (t + 1 < tiles) load(t + 1);      // in flight while wave 0 adds
    if (row == 0) {
      for (int k0 = 0; k0 < SUM_TILE; k0 += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) acc = acc + product(s_wt[b][k0 + j], s_x[b][k0 + j][lane]);
      }
    }
    if (t + 1 < tiles) store(b ^ 1);     // (wave 0 read that buffer in the round before, ahead of its barrier)
    __syncthreads();
  }
  if (row == 0 && in) *nom = acc / a.sums[(size_t)g * 4];
}

__global__ __launch_bounds__(BLOCK) void trex_plan_shift_kernel(TrexPlanState st, const TrexPlanTap *shift) {
  __shared__ float s_old[TREX_PLAN_MAXKNOTS * TREX_PLAN_MAXACT];
  const int PA = st.P * st.A;
  float *nom = st.nominal + (size_t)blockIdx.x * PA;
  for (int i = threadIdx.x; i < PA; i += BLOCK) s_old[i] = nom[i];
  __syncthreads();
  for (int i = threadIdx.x; i < PA; i += BLOCK) {
    const int p = i / st.A, c = i - p * st.A;
    nom[i] = taps4(shift[p], s_old + c, st.A);
  }
}

__global__ __launch_bounds__(BLOCK) void trex_plan_action_kernel(TrexPlanState st, int step, float *actions) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= st.G * st.A) return;
  const int g = i / st.A, c = i - g * st.A;
  const float lo = st.noise->lo[c], hi = st.noise->hi[c];
  const TrexPlanTap t = st.taps[step];
  const float *knot = st.nominal + (size_t)g * st.P * st.A + c;
  float v = product(t.w[0], clip(knot[t.i[0] * st.A], lo, hi));
  v = v + product(t.w[1], clip(knot[t.i[1] * st.A], lo, hi));
  v = v + product(t.w[2], clip(knot[t.i[2] * st.A], lo, hi));
  v = v + product(t.w[3], clip(knot[t.i[3] * st.A], lo, hi));
  actions[i] = clip(v, lo, hi);
}

__global__ __launch_bounds__(BLOCK) void trex_plan_set_nominal_kernel(TrexPlanState st, const float *knots, const uint8_t *mask) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x, PA = (size_t)st.P * st.A;
  if (i >= (size_t)st.G * PA || (mask && !mask[i / PA])) return;
  st.nominal[i] = knots[i];
}

unsigned blocks_of(size_t items, int block) { return (unsigned)((items + block - 1) / block); }

}  // namespace

extern "C" hipError_t trex_launch_plan_sample(const TrexPlanSampleArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(trex_plan_sample_kernel, dim3(blocks_of((size_t)args.st.N, args.tile)), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_plan_update(const TrexPlanUpdateArgs &args, hipStream_t stream) {
  const TrexPlanState &st = args.st;
  hipLaunchKernelGGL(trex_plan_return_kernel, dim3(blocks_of((size_t)st.N, BLOCK)), dim3(BLOCK), 0, stream, args);
  hipLaunchKernelGGL(trex_plan_group_kernel, dim3((unsigned)st.G), dim3(BLOCK), 0, stream, args);
  const size_t per = ((size_t)st.P * st.A + SUM_BLOCK - 1) / SUM_BLOCK;
  hipLaunchKernelGGL(trex_plan_nominal_kernel, dim3((unsigned)(per * st.G)), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_plan_shift(const TrexPlanState &st, const TrexPlanTap *shift, hipStream_t stream) {
  hipLaunchKernelGGL(trex_plan_shift_kernel, dim3((unsigned)st.G), dim3(BLOCK), 0, stream, st, shift);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_plan_action(const TrexPlanState &st, int step, float *actions, hipStream_t stream) {
  hipLaunchKernelGGL(trex_plan_action_kernel, dim3(blocks_of((size_t)st.G * st.A, BLOCK)), dim3(BLOCK), 0, stream, st, step, actions);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_plan_set_nominal(const TrexPlanState &st, const float *knots, const uint8_t *mask, hipStream_t stream) {
  hipLaunchKernelGGL(trex_plan_set_nominal_kernel, dim3(blocks_of((size_t)st.G * st.P * st.A, BLOCK)), dim3(BLOCK), 0, stream, st, knots, mask);
  return hipGetLastError();
}
