// The mirror kernels (include/trex_symmetry.h, which states the semantics): K22. Pure data movement plus a sign bit - the rows travel
// as 32-bit words, so no float instruction ever sees them and the results are defined bit for bit.
//
// Shape of a row launch. A workgroup of TREX_MIRROR_BLOCK lanes takes a tile of R = TREX_MIRROR_TILE_FLOATS / width whole rows
// (symmetry_limits.h). It reads the table once and the tile's rows into LDS, lane i taking word i, i + 256, .. of the tile: with
// packed rows that is one contiguous stretch of global memory, with a larger stride one stretch per row. Behind the barrier it
// stores word i of the out tile from rows[row(i)][src[col(i)]]: the gather happens in LDS, the global stores are as contiguous as
// the loads. Every row of the tile is in LDS before any is stored and no other workgroup touches these rows: that is what makes
// in == out correct. (row, col) of a lane's words are kept by adding 256 / width and 256 % width per word: one division per lane.
// The launch shape depends on n and width alone. No scratch, 16 KB + 2 KB of LDS: eight workgroups to a CU.
#include "symmetry.h"

namespace {

__device__ __forceinline__ void mirror_tile(const TrexMirrorBlock &b, int tile, uint32_t *tab, uint32_t *rows) {
  const int t = threadIdx.x, W = b.width;
  const int R = TREX_MIRROR_TILE_FLOATS / W;
  const int r0 = tile * R;
  const int nr = min(R, b.n - r0);
  const int count = nr * W;
  for (int c = t; c < W; c += TREX_MIRROR_BLOCK) tab[c] = b.table[c];
  const uint32_t *in = (const uint32_t *)b.in + (size_t)r0 * b.in_stride;
  uint32_t *out = (uint32_t *)b.out + (size_t)r0 * b.out_stride;
  const int dq = TREX_MIRROR_BLOCK / W, dr = TREX_MIRROR_BLOCK % W;
  int r = t / W, c = t - r * W;
#pragma unroll 4
  for (int i = t; i < count; i += TREX_MIRROR_BLOCK) {
    rows[i] = in[(size_t)r * b.in_stride + c];
    r += dq; c += dr;
    if (c >= W) { c -= W; r++; }
  }
  __syncthreads();
  r = t / W; c = t - r * W;
#pragma unroll 4
  for (int i = t; i < count; i += TREX_MIRROR_BLOCK) {
    const uint32_t w = tab[c];
    out[(size_t)r * b.out_stride + c] = rows[i - c + (int)(w & ~TREX_MIRROR_NEG)] ^ (w & TREX_MIRROR_NEG);
    r += dq; c += dr;
    if (c >= W) { c -= W; r++; }
  }
}

__global__ __launch_bounds__(TREX_MIRROR_BLOCK) void mirror_rows_kernel(TrexMirrorBlock b) {
  __shared__ uint32_t tab[TREX_MIRROR_MAXWIDTH + 3];
  __shared__ uint32_t rows[TREX_MIRROR_TILE_FLOATS];
  mirror_tile(b, blockIdx.x, tab, rows);
}

// workgroups [0, obs tiles) | [.., + act tiles) | [.., + obs_v tiles) | 4 x copy_groups of the columns: a workgroup's job is uniform
__global__ __launch_bounds__(TREX_MIRROR_BLOCK) void mirror_augment_kernel(TrexMirrorAugmentArgs a) {
  __shared__ uint32_t tab[TREX_MIRROR_MAXWIDTH + 3];
  __shared__ uint32_t rows[TREX_MIRROR_TILE_FLOATS];
  int g = blockIdx.x;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (g < a.block[k].tiles) {
      mirror_tile(a.block[k], g, tab, rows);
      return;
    }
    g -= a.block[k].tiles;
  }
  const int col = g / a.copy_groups, part = g - col * a.copy_groups;
  uint32_t *p = (uint32_t *)(col == 0 ? a.column[0] : col == 1 ? a.column[1] : col == 2 ? a.column[2] : a.column[3]);
  const long long first = (long long)part * TREX_MIRROR_COPY_ELEMS;
  const long long end = min(first + TREX_MIRROR_COPY_ELEMS, a.n);
#pragma unroll 4
  for (long long i = first + threadIdx.x; i < end; i += TREX_MIRROR_BLOCK) p[a.n + i] = p[i];
}

// A value that the compiler must have as a rounded f64 before it goes on: the library is built with -ffp-contract=fast, under which
// a product - the halving included - that feeds a sum becomes an fma whatever pragma stands there (seen in the ISA; philox.h has
// the f32 twin). An empty asm statement: no instruction.
__device__ __forceinline__ double rounded(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

// the order of include/trex_symmetry.h, every operation an f64 operation of its own
__global__ __launch_bounds__(TREX_MIRROR_BLOCK) void mirror_moments_kernel(const uint32_t *table, double *stats, int D) {
  const int t = threadIdx.x;
  double m = 0.0, a = 0.0, v = 0.0, vp = 0.0;
  if (t < D) {
    const uint32_t w = table[t];
    const int cp = (int)(w & ~TREX_MIRROR_NEG);
    m = stats[t];
    a = stats[cp];
    if (w & TREX_MIRROR_NEG) a = -a;
    v = stats[D + t];
    vp = stats[D + cp];
  }
  __syncthreads();   // every old value is in a register before any new one is stored
  if (t < D) {
    const double h = (m - a) / 2.0;
    stats[t] = (m + a) / 2.0;            // (the halving is exact: fused or not, it rounds once, in the sum)
    stats[D + t] = rounded((v + vp) / 2.0) + rounded(h * h);
  }
}

}  // namespace

extern "C" hipError_t trex_launch_mirror_rows(const TrexMirrorBlock &block, hipStream_t stream) {
  hipLaunchKernelGGL(mirror_rows_kernel, dim3(block.tiles), dim3(TREX_MIRROR_BLOCK), 0, stream, block);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_mirror_augment(const TrexMirrorAugmentArgs &args, hipStream_t stream) {
  const int groups = args.block[0].tiles + args.block[1].tiles + args.block[2].tiles + 4 * args.copy_groups;
  hipLaunchKernelGGL(mirror_augment_kernel, dim3(groups), dim3(TREX_MIRROR_BLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_mirror_moments(const uint32_t *table, double *stats, int D, hipStream_t stream) {
  hipLaunchKernelGGL(mirror_moments_kernel, dim3(1), dim3(TREX_MIRROR_BLOCK), 0, stream, table, stats, D);
  return hipGetLastError();
}
