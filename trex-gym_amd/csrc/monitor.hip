// Episode monitor (trex_batch_monitor_apply / _monitor_reset / _monitor_summary, include/trex_monitor.h, which states the
// semantics): K15. Returns, lengths, end reasons and column sums of every finished episode, a ring of the last W records.
//
// An apply is TWO launches, no workgroup ever waiting for another:
//  accumulate: an env is a team of `team` lanes, the smallest power of two that holds its C columns (1 .. 64: a team never spans
//    wavefronts), TREX_MON_BLOCK / team envs to a workgroup. Lane c owns column c, so that the f64 read-modify-write of col and the
//    f32 store of the last record's columns coalesce; lane 0 owns the scalars as well. A finished env leaves its record in its
//    own per-env slots (the "last record") and a flag; the workgroup leaves its count of finished envs.
//  commit: ONE workgroup. It sums the counts - all 0: t += 1 and out -, then walks the envs in ascending order, 1024 at a time,
//    ranks the finished ones by wavefront ballots and a scan of the 16 wavefront counts, and copies the records of rank
//    >= count - W from the per-env slots to ring slot (total + rank) % W: ascending env order, each slot written once, whether
//    one call finishes more episodes than the window holds or fewer.
// No float atomics anywhere: every f64 sum has a fixed order (the summary's: a strided partial per lane, then a tree in LDS). The
// integer counts of the reasons are LDS integer adds, which commute.
#include "monitor.h"

namespace {

constexpr int BLOCK = TREX_MON_BLOCK, CBLOCK = TREX_MON_COMMIT_BLOCK, SBLOCK = TREX_MON_SUMMARY_BLOCK, WAVE = 64;

__global__ __launch_bounds__(BLOCK) void trex_monitor_accumulate_kernel(TrexMonArgs a) {
  const int team = a.team, shift = __builtin_ctz(team), lane = threadIdx.x & (team - 1);   // (team: a power of two)
  const int env = blockIdx.x * (BLOCK >> shift) + (threadIdx.x >> shift);
  const TrexMonState &s = a.st;
  const bool live = env < a.n_envs;
  bool fin = false;
  if (live) {
    fin = a.done[(size_t)env * a.done_stride] != 0.f;
    const int C = a.cols_n;
    if (lane < C) {
      const float x = lane < a.cols_a_n ? a.cols_a[(size_t)env * a.stride_a + lane] : a.cols_b[(size_t)env * a.stride_b + (lane - a.cols_a_n)];
      const size_t at = (size_t)env * C + lane;
      const double c = s.col[at] + (double)x;
      if (fin) s.last_cols[at] = (float)c;
      s.col[at] = fin ? 0.0 : c;
    }
    if (lane == 0) {
      const double r = s.ret[env] + (double)a.reward[(size_t)env * a.reward_stride];
      const int32_t l = s.len[env] + 1;
      if (fin) {
        s.last_return[env] = (float)r;
        s.last_length[env] = l;
        s.last_reason[env] = a.reason ? a.reason[env] : 0;
        s.last_t[env] = *s.t;
        s.episodes[env] += 1u;
      }
      s.ret[env] = fin ? 0.0 : r;
      s.len[env] = fin ? 0 : l;
      s.fin[env] = fin ? 1u : 0u;
    }
  }
  const int count = __syncthreads_count(live && fin && lane == 0);
  if (threadIdx.x == 0) s.counts[blockIdx.x] = (uint32_t)count;
}

// bucket b of by_reason: reason 0, or bit b - 1 of the reason
__device__ __forceinline__ bool in_bucket(int32_t reason, int b) { return b == 0 ? reason == 0 : ((reason >> (b - 1)) & 1) != 0; }

__global__ __launch_bounds__(CBLOCK) void trex_monitor_commit_kernel(TrexMonArgs a) {
  __shared__ unsigned int part[CBLOCK / WAVE];
  __shared__ unsigned int bucket[4];
  __shared__ unsigned int sum;
  const TrexMonState &s = a.st;
  const int tid = threadIdx.x, wave = tid / WAVE, wl = tid % WAVE;
  if (tid == 0) sum = 0u;
  if (tid < 4) bucket[tid] = 0u;
  __syncthreads();
  unsigned int mine = 0u;
  for (int g = tid; g < a.groups; g += CBLOCK) mine += s.counts[g];
  if (mine) atomicAdd(&sum, mine);
  __syncthreads();
  const unsigned int count = sum;
  if (count == 0u) {
    if (tid == 0) *s.t += 1u;
    return;
  }
  const unsigned long long total = *s.total;
  const unsigned int W = (unsigned int)a.window, first = count > W ? count - W : 0u;   // ranks below `first` are overwritten in this very call
  const int C = a.cols_n;
  unsigned int before = 0u;   // finished envs below this chunk
  for (int base = 0; base < a.n_envs; base += CBLOCK) {
    const int env = base + tid;
    const bool fin = env < a.n_envs && s.fin[env] != 0u;
    const int32_t reason = fin ? s.last_reason[env] : 0;
    const unsigned long long votes = __ballot(fin);
    if (wl == 0) part[wave] = (unsigned int)__popcll(votes);
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const unsigned long long in = __ballot(fin && in_bucket(reason, b));
      if (wl == 0 && in) atomicAdd(&bucket[b], (unsigned int)__popcll(in));
    }
    __syncthreads();
    unsigned int lower = 0u, chunk = 0u;
    for (int w = 0; w < CBLOCK / WAVE; w++) {
      const unsigned int p = part[w];
      lower += w < wave ? p : 0u;
      chunk += p;
    }
    if (fin) {
      const unsigned int rank = before + lower + (unsigned int)__popcll(votes & ((1ull << wl) - 1ull));
      if (rank >= first) {
        const unsigned int slot = (unsigned int)((total + rank) % W);
        s.ring_return[slot] = s.last_return[env];
        s.ring_length[slot] = s.last_length[env];
        s.ring_reason[slot] = reason;
        s.ring_env[slot] = a.env_offset + (uint32_t)env;
        s.ring_t[slot] = s.last_t[env];
        for (int c = 0; c < C; c++) s.ring_cols[(size_t)slot * C + c] = s.last_cols[(size_t)env * C + c];
      }
    }
    before += chunk;
    __syncthreads();   // (part is rewritten by the next chunk)
  }
  if (tid < 4) s.by_reason[tid] += bucket[tid];
  if (tid == 0) { *s.total = total + count; *s.t += 1u; }
}

__global__ void trex_monitor_reset_kernel(TrexMonState s, const uint8_t *mask, int n_envs, int cols) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = cols + 1;
  if (i >= (long long)n_envs * per) return;
  const int env = (int)(i / per), k = (int)(i % per);
  if (mask && !mask[env]) return;
  if (k == 0) { s.ret[env] = 0.0; s.len[env] = 0; }
  else s.col[(size_t)env * cols + (k - 1)] = 0.0;
}

// a block's sum / minimum / maximum of one f64 per lane: a tree in LDS, the same order every time
__device__ double block_sum(double x, double *lds) {
  __syncthreads();
  lds[threadIdx.x] = x;
  __syncthreads();
  for (int h = SBLOCK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
    __syncthreads();
  }
  return lds[0];
}
__device__ double block_extreme(double x, double *lds, bool largest) {
  __syncthreads();
  lds[threadIdx.x] = x;
  __syncthreads();
  for (int h = SBLOCK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      const double p = lds[threadIdx.x], q = lds[threadIdx.x + h];
      // a NaN return stays: (q < p) is false for a NaN p, and a NaN q is taken by the second test
      lds[threadIdx.x] = largest ? ((q > p || q != q) ? q : p) : ((q < p || q != q) ? q : p);
    }
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(SBLOCK) void trex_monitor_summary_kernel(TrexMonState s, int window, int cols, double *out) {
  __shared__ double lds[SBLOCK];
  const int tid = threadIdx.x;
  const unsigned long long total = *s.total;
  const int n = total < (unsigned long long)window ? (int)total : window;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  double rs = 0.0, rlo = inf, rhi = -inf, ls = 0.0, llo = inf, lhi = -inf, rc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += SBLOCK) {
    const double r = (double)s.ring_return[i], l = (double)s.ring_length[i];
    const int32_t reason = s.ring_reason[i];
    rs += r; ls += l;
    rlo = (r < rlo || r != r) ? r : rlo; rhi = (r > rhi || r != r) ? r : rhi;
    llo = l < llo ? l : llo; lhi = l > lhi ? l : lhi;
#pragma unroll
    for (int b = 0; b < 4; b++) rc[b] += in_bucket(reason, b) ? 1.0 : 0.0;
  }
  double v[TREX_MON_SUMMARY];
  v[TREX_MON_N] = (double)n;
  v[TREX_MON_RET_MEAN] = block_sum(rs, lds) / (double)n;
  v[TREX_MON_RET_MIN] = block_extreme(rlo, lds, false);
  v[TREX_MON_RET_MAX] = block_extreme(rhi, lds, true);
  v[TREX_MON_LEN_MEAN] = block_sum(ls, lds) / (double)n;
  v[TREX_MON_LEN_MIN] = block_extreme(llo, lds, false);
  v[TREX_MON_LEN_MAX] = block_extreme(lhi, lds, true);
#pragma unroll
  for (int b = 0; b < 4; b++) v[TREX_MON_WIN_REASON + b] = block_sum(rc[b], lds);
  v[TREX_MON_TOTAL] = (double)total;
#pragma unroll
  for (int b = 0; b < 4; b++) v[TREX_MON_BY_REASON + b] = (double)s.by_reason[b];
  v[TREX_MON_T] = (double)*s.t;
  if (n == 0) {
#pragma unroll
    for (int k = TREX_MON_RET_MEAN; k <= TREX_MON_LEN_MAX; k++) v[k] = nan;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < TREX_MON_SUMMARY; k++) out[k] = v[k];
  }
  for (int c = 0; c < cols; c++) {
    double cs = 0.0;
    for (int i = tid; i < n; i += SBLOCK) cs += (double)s.ring_cols[(size_t)i * cols + c];
    const double mean = block_sum(cs, lds) / (double)n;
    if (tid == 0) out[TREX_MON_SUMMARY + c] = n == 0 ? nan : mean;
  }
}

}  // namespace

extern "C" hipError_t trex_launch_monitor(const TrexMonArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(trex_monitor_accumulate_kernel, dim3((unsigned)args.groups), dim3(BLOCK), 0, stream, args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(trex_monitor_commit_kernel, dim3(1), dim3(CBLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_monitor_reset(const TrexMonState &st, const uint8_t *mask, int n_envs, int cols, hipStream_t stream) {
  const long long lanes = (long long)n_envs * (cols + 1);
  hipLaunchKernelGGL(trex_monitor_reset_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, st, mask, n_envs, cols);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_monitor_summary(const TrexMonState &st, int window, int cols, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(trex_monitor_summary_kernel, dim3(1), dim3(SBLOCK), 0, stream, st, window, cols, out);
  return hipGetLastError();
}
