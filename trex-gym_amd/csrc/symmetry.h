// The mirror maps (include/trex_symmetry.h): launch arguments shared by capi_symmetry.cpp, capi_policy.cpp and symmetry.hip; the
// table words are built by host_tables.cpp. The row kernels know neither a batch nor a policy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "symmetry_limits.h"

// one block of rows through one table: out[e * out_stride + c] = sign[c] * in[e * in_stride + src[c]], e < n, c < width
struct TrexMirrorBlock {
  const uint32_t *table;           /* [width] words of symmetry_limits.h */
  const float *in;
  float *out;
  int in_stride, out_stride, n, width;
  int tiles;                       /* workgroups: ceil(n / trex_mirror_tile_rows(width)); 0: the block is not there */
};

struct TrexMirrorAugmentArgs {
  TrexMirrorBlock block[3];        /* obs, act, obs_v: in = the buffer, out = the buffer + n * width, packed rows */
  float *column[4];                /* logp, val, adv, ret: [2 n] each */
  long long n;                     /* num_samples */
  int copy_groups;                 /* workgroups per column: ceil(n / TREX_MIRROR_COPY_ELEMS) */
};

extern "C" hipError_t trex_launch_mirror_rows(const TrexMirrorBlock &block, hipStream_t stream);
extern "C" hipError_t trex_launch_mirror_augment(const TrexMirrorAugmentArgs &args, hipStream_t stream);
// mean [D] | var [D] at the head of `stats` (f64) -> those of the augmented stream, in place; one workgroup
extern "C" hipError_t trex_launch_mirror_moments(const uint32_t *table, double *stats, int D, hipStream_t stream);
