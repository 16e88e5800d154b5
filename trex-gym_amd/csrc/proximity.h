// Batched closest-point queries between bodies (trex_batch_set_proximity_shapes / trex_batch_proximity): launch arguments and the
// table layout shared by capi.cpp and proximity.hip. The step kernels do not see any of this; the query only reads the batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

#define TREX_PROX_BLOCK 256        /* lanes per workgroup: one env per workgroup */
#define TREX_PROX_MAXCAPS 256      /* capsules per table */
#define TREX_PROX_MAXPAIRS 1024    /* body pairs per table */
#define TREX_PROX_MAXTESTS 65536   /* capsule-pair tests per table: the sum over pairs of capsules(A) x capsules(B) */
#define TREX_PROX_EPS 1e-6f        /* axis distance below which the normal is (0, 0, 1) */

/* One capsule-pair test, host-built, sorted by (pair, capsule of A, capsule of B): pair << 16 | capsule of A << 8 | capsule of B
 * (capsule = index into the table). The index of a test in the list is its rank in the tie rule. */
#define TREX_PROX_TEST(pair, ca, cb) (((uint32_t)(pair) << 16) | ((uint32_t)(ca) << 8) | (uint32_t)(cb))

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
