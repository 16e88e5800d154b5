// Batched closest-point queries between bodies (trex_batch_set_proximity_shapes / trex_batch_proximity): launch arguments and the
// table layout shared by capi_queries.cpp and proximity.hip; the table itself is built by host_tables.cpp, which shares the limits of
// proximity_limits.h. The step kernels do not see any of this; the query only reads the batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"
#include "proximity_limits.h"      /* TREX_PROX_MAXCAPS / _MAXPAIRS / _MAXTESTS, TREX_PROX_TEST */

#define TREX_PROX_BLOCK 256        /* lanes per workgroup: one env per workgroup */
#define TREX_PROX_EPS 1e-6f        /* axis distance below which the normal is (0, 0, 1) */

struct TrexProxArgs {
  const TrexDeviceModel *model;
  const float *base, *q;          /* the batch's state (read only) */
  const float *cap;               /* [C][8] p0 xyz, radius | p1 xyz, 0; body frame */
  const int32_t *cap_body;        /* [C] */
  const uint32_t *test;           /* [T] TREX_PROX_TEST words */
  const int32_t *pair_first;      /* [P] index of each pair's first test */
  float *distance;                /* [N, P] */
  float *point_a, *point_b, *normal;   /* [N, P, 3], each nullable */
  int32_t *capsule;               /* [N, P, 2] nullable */
  int n_envs, num_capsules, num_pairs, num_tests;
};

/* proximity.hip: one launch, one workgroup per env */
extern "C" hipError_t trex_launch_proximity(const TrexProxArgs &args, hipStream_t stream);
