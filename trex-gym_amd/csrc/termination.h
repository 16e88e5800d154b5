// Per-body floor clearance and the fall-termination predicate (trex_batch_body_clearance / trex_batch_set_termination): launch
// arguments shared by capi.cpp and termination.hip. The step kernels do not see any of this. (The launcher's prototype lives here
// and not in step_launch.h: that header is hashed into the step kernels' build id.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

#define TREX_TERM_BLOCK 64      /* lanes per workgroup: one env per wavefront, one wavefront per workgroup */

/* reason bits of the predicate (include/trex_batch.h: TREX_TERM_*) */
#define TREX_TERM_BIT_HEAD 1
#define TREX_TERM_BIT_TILT 2
#define TREX_TERM_BIT_CLEARANCE 4

struct TrexTermArgs {
  const TrexDeviceModel *model;
  const float *base, *q;          /* the batch's state (read only) */
  const float4 *hull;             /* [nv] body-frame collision points: xyz + support radius */
  int n_envs;
  /* ---- the query (trex_batch_body_clearance); both null in a predicate launch */
  float *clearance;               /* [N, nb] */
  float *lowest;                  /* [N, nb, 3] nullable */
  /* ---- the predicate (a step of a batch with termination on) */
  int watch_any;                  /* some body is watched: else the sweep over the collision points is skipped, values[2] = +inf */
  float head_min, cos_tilt, penalty;   /* thresholds (a NaN: that criterion is off) and what a terminated env's reward loses */
  uint8_t *mask;                  /* [N] batch-owned: the reset mask of the RESET launch that follows */
  int32_t *reason;                /* [N] batch-owned */
  float *values;                  /* [N, 3] batch-owned */
  float *terminal_obs;            /* [N, 3J] batch-owned: the observation row of an env that terminates */
  /* where the step launch wrote its outputs, each nullable: observation rows, reward and done (as 0.0 / 1.0) with their strides,
   * done as bytes. One of done and done_f is non-null: how the launch tells an env that the step launch already ended */
  const float *obs;
  float *reward, *done_f;
  uint8_t *done;
  int obs_stride, scal_stride, obs_cols;
  float clear_min[TREX_TL];       /* per body: the clearance it has to keep, NaN = not watched (by value: nothing to upload) */
};

/* termination.hip: one launch, one wavefront per env; predicate != 0: the predicate path */
extern "C" hipError_t trex_launch_termination(const TrexTermArgs &args, int predicate, hipStream_t stream);
