// Sensor model (trex_batch_apply_sensing / _sensing_reset / _delay_actions, include/trex_sensing.h, which states the semantics
// and the random numbers): K13. One launch rewrites the covered observation columns of every env's row - delay, bias, white
// noise, resolution -, one more delays the action rows.
//
// Shape of the apply launch: an env's row is `lanes` consecutive lanes of a 256-thread workgroup (a power of two, 8 to 256), lane
// b owning the four columns of Philox block b - ONE Philox evaluation per stream serves them - read and written as dwords (a row
// is not 16-byte aligned: 308 bytes plain). The history [slot][env][delayed column] is walked by the same lanes in the same
// order. An env's counters are read by all its lanes before the workgroup's barrier and written by its lane 0 behind it; every
// lane reads a column before it writes it, so out == rows is safe. No scratch, no atomics.
#include "sensing.h"

#include "../../include/trex_sensing.h"
#include "philox.h"

namespace {

constexpr int BLOCK = TREX_SENSE_BLOCK;
constexpr float TWO_PI = 6.2831855f;

// (philox, u_half_open, u_open_closed, draw_int: philox.h)
__device__ __forceinline__ float symmetric(uint32_t r) { return __fsub_rn(__fmul_rn(2.f, u_half_open(r)), 1.f); }       // 2u - 1, exact

// column j of a block's four standard normals
__device__ __forceinline__ float normal(const uint32_t (&r)[4], int j) {
  const int p = j & 2;
  const float R = sqrtf(__fmul_rn(-2.f, logf(u_open_closed(r[p])))), ang = __fmul_rn(TWO_PI, u_half_open(r[p + 1]));
  return __fmul_rn(R, (j & 1) ? sinf(ang) : cosf(ang));
}

__global__ __launch_bounds__(BLOCK) void trex_sensing_kernel(TrexSenseArgs a) {
  __shared__ int32_t s_delay[(BLOCK / 8) * TREX_SENSE_MAXGROUPS];
  const int lanes = a.lanes, slot = threadIdx.x / lanes, lane = threadIdx.x % lanes;
  const int env = blockIdx.x * (BLOCK / lanes) + slot, G = a.num_groups, D = a.obs_dim;
  const bool live = env < a.n_envs;
  const uint32_t eid = a.env_offset + (uint32_t)env;
  const float *row = a.rows + (size_t)(live ? env : 0) * a.row_stride;
  uint32_t ep = 0, k = 0;
  if (live) {
    const bool first = row[D + 1] != 0.f || a.started[env] == 0u;
    ep = a.ep[env] + (first ? 1u : 0u);
    k = first ? 0u : a.k[env] + 1u;
    for (int g = lane; g < G; g += lanes) {
      int d;
      if (first) {
        const int lo = a.group[g].delay_min, hi = a.group[g].delay_max;
        d = lo;
        if (hi > lo) {
          uint32_t r[4];
          philox(eid, 0u, ((uint32_t)TREX_SENSE_STREAM_DELAY << 16) | (uint32_t)g, ep, a.key0, a.key1, r);
          d = draw_int(r[0], lo, hi);
        }
        a.delay[(size_t)env * G + g] = d;
      } else {
        d = a.delay[(size_t)env * G + g];
      }
      s_delay[slot * TREX_SENSE_MAXGROUPS + g] = d;
    }
  }
  __syncthreads();   // every lane of the env has read its counters; its delays are in LDS
  if (!live) return;
  if (lane == 0) { a.ep[env] = ep; a.k[env] = k; a.started[env] = 1u; }
  const int width = D + a.tail, c0 = lane * 4;
  if (c0 >= width) return;
  float *out = a.out + (size_t)env * a.out_stride;
  float v[4];
  int grp[4];
  bool need_white = false, need_bias = false;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = c0 + j;
    v[j] = c < width ? row[c] : 0.f;
    grp[j] = c < D ? (int)a.col_group[c] : -1;
    if (grp[j] >= 0) {
      need_white |= a.group[grp[j]].noise > 0.f;
      need_bias |= a.group[grp[j]].bias > 0.f;
    }
  }
  uint32_t white[4] = {0u, 0u, 0u, 0u}, held[4] = {0u, 0u, 0u, 0u};
  if (need_white) philox(eid, k, ((uint32_t)TREX_SENSE_STREAM_WHITE << 16) | (uint32_t)lane, ep, a.key0, a.key1, white);
  if (need_bias) philox(eid, 0u, ((uint32_t)TREX_SENSE_STREAM_BIAS << 16) | (uint32_t)lane, ep, a.key0, a.key1, held);
  const size_t plane = (size_t)a.n_envs * a.delayed;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = c0 + j;
    if (c >= width) break;
    float y = v[j];
    if (grp[j] >= 0) {
      const TrexSenseGrp gr = a.group[grp[j]];
      const int hc = a.col_hist[c];
      if (hc >= 0) {   // the group can be late: row k into slot k % 9, the reading from row max(k - d, 0)
        float *h = a.hist + (size_t)env * a.delayed + hc;
        h[(size_t)(k % TREX_SENSE_SLOTS) * plane] = v[j];
        const uint32_t d = (uint32_t)s_delay[slot * TREX_SENSE_MAXGROUPS + grp[j]];
        const uint32_t src = k > d ? k - d : 0u;
        if (src != k) y = h[(size_t)(src % TREX_SENSE_SLOTS) * plane];
      }
      // (a magnitude of 0 adds nothing, not a zero: -0 stays -0 and an empty-effect group leaves the row bit for bit)
      if (gr.bias > 0.f) y = __fadd_rn(y, __fmul_rn(gr.bias, symmetric(held[j])));
      if (gr.noise > 0.f) y = __fadd_rn(y, __fmul_rn(gr.noise, gr.kind == TREX_SENSE_UNIFORM ? symmetric(white[j]) : normal(white, j)));
      if (gr.quantum > 0.f) y = __fmul_rn(gr.quantum, rintf(__fmul_rn(y, gr.inv_quantum)));
    }
    out[c] = y;
  }
}

__global__ void trex_sensing_reset_kernel(const uint8_t *mask, int n_envs, uint32_t *started, uint32_t *act_started) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  if (started) started[env] = 0u;
  if (act_started) act_started[env] = 0u;
}

// an env's action row is 64 consecutive lanes (A <= 62), four envs to a workgroup
constexpr int ACT_LANES = 64;
__global__ __launch_bounds__(BLOCK) void trex_delay_actions_kernel(TrexActDelayArgs a) {
  const int slot = threadIdx.x / ACT_LANES, lane = threadIdx.x % ACT_LANES;
  const int env = blockIdx.x * (BLOCK / ACT_LANES) + slot;
  const bool live = env < a.n_envs;
  uint32_t ep = 0, k = 0;
  int d = 0;
  if (live) {
    const bool first = (a.done_prev && a.done_prev[env]) || a.started[env] == 0u;
    ep = a.ep[env] + (first ? 1u : 0u);
    k = first ? 0u : a.k[env] + 1u;
    if (first) {
      d = a.delay_min;
      if (a.delay_max > a.delay_min) {
        uint32_t r[4];
        philox(a.env_offset + (uint32_t)env, 0u, (uint32_t)TREX_SENSE_STREAM_ACTION << 16, ep, a.key0, a.key1, r);
        d = draw_int(r[0], a.delay_min, a.delay_max);
      }
    } else {
      d = a.delay[env];
    }
  }
  __syncthreads();   // every lane of the env has read its counters
  if (!live) return;
  if (lane == 0) { a.ep[env] = ep; a.k[env] = k; a.started[env] = 1u; a.delay[env] = d; }
  if (lane >= a.cols) return;
  const size_t plane = (size_t)a.n_envs * a.cols, at = (size_t)env * a.cols + lane;
  const float v = a.actions[at];
  a.hist[(size_t)(k % TREX_SENSE_SLOTS) * plane + at] = v;
  const uint32_t src = k > (uint32_t)d ? k - (uint32_t)d : 0u;
  a.out[at] = src != k ? a.hist[(size_t)(src % TREX_SENSE_SLOTS) * plane + at] : v;
}

}  // namespace

extern "C" hipError_t trex_launch_sensing(const TrexSenseArgs &args, hipStream_t stream) {
  const int per = BLOCK / args.lanes;
  const dim3 grid((unsigned)((args.n_envs + per - 1) / per)), block(BLOCK);
  hipLaunchKernelGGL(trex_sensing_kernel, grid, block, 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_sensing_reset(const uint8_t *mask, int n_envs, uint32_t *started, uint32_t *act_started,
                                                hipStream_t stream) {
  const dim3 grid((unsigned)((n_envs + 255) / 256)), block(256);
  hipLaunchKernelGGL(trex_sensing_reset_kernel, grid, block, 0, stream, mask, n_envs, started, act_started);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_delay_actions(const TrexActDelayArgs &args, hipStream_t stream) {
  const int per = BLOCK / ACT_LANES;
  const dim3 grid((unsigned)((args.n_envs + per - 1) / per)), block(BLOCK);
  hipLaunchKernelGGL(trex_delay_actions_kernel, grid, block, 0, stream, args);
  return hipGetLastError();
}
