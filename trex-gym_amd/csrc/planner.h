// The planner (include/trex_planner.h): launch arguments shared by capi_planner.cpp and planner.hip; the tap, shift and discount
// tables and the noise are built by host_tables.cpp. Nothing here knows a batch: the kernels read and write plain device buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "planner_limits.h"

// the sizes of include/trex_planner.h and the planner's own device memory
struct TrexPlanState {
  float *nominal;                  /* [G][P][A] */
  float *knots;                    /* [N][P][A]: the last samples' */
  uint32_t *it;                    /* [2]: the sample count, and the workgroups of a sample launch that have read it */
  const TrexPlanTap *taps;         /* [S] */
  const TrexPlanNoise *noise;
  int G, K, S, P, A, N;
};

struct TrexPlanSampleArgs {
  TrexPlanState st;
  float *actions;                  /* [S][N][A] */
  int tile;                        /* envs to a workgroup */
  uint32_t key0, key1, env_offset;
};

struct TrexPlanUpdateArgs {
  TrexPlanState st;
  const float *reward, *done;      /* element (s, e) at s * step_stride + e * env_stride; done nullable */
  const float *terminal;           /* [N] or NULL */
  const float *discount;           /* [S + 1] */
  long long step_stride, env_stride;
  float temperature;
  float *returns, *weights;        /* [N] each: the planner's own */
  int32_t *best;                   /* [G]: the planner's own */
  float *sums;                     /* [G][4]: sum w, R_max, unused, unused - the planner's own */
  float *returns_out, *weights_out, *stats_out;   /* the caller's, each nullable */
  int32_t *best_out;
};

// knots, actions, it += 1
extern "C" hipError_t trex_launch_plan_sample(const TrexPlanSampleArgs &args, hipStream_t stream);
// the three launches of an update: returns, the groups' weights, the nominal
extern "C" hipError_t trex_launch_plan_update(const TrexPlanUpdateArgs &args, hipStream_t stream);
// nominal <- the taps of a shift table [P]
extern "C" hipError_t trex_launch_plan_shift(const TrexPlanState &st, const TrexPlanTap *shift, hipStream_t stream);
// actions [G][A] <- the nominal at the tap set of `step`
extern "C" hipError_t trex_launch_plan_action(const TrexPlanState &st, int step, float *actions, hipStream_t stream);
// nominal[g] <- knots[g] where mask[g] (NULL: all)
extern "C" hipError_t trex_launch_plan_set_nominal(const TrexPlanState &st, const float *knots, const uint8_t *mask, hipStream_t stream);
