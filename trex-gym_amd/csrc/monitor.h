// Episode monitor (trex_batch_set_monitor / _monitor_apply / _monitor_reset / _monitor_summary / _monitor_info,
// include/trex_monitor.h): launch arguments shared by capi_monitor.cpp and monitor.hip; the shape and the layout of the state are
// worked out by host_tables.cpp (trex::monitor_layout). The step kernels do not see any of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/trex_monitor.h"

#define TREX_MON_BLOCK 256          /* the accumulate launch: TREX_MON_BLOCK / team envs to a workgroup */
#define TREX_MON_COMMIT_BLOCK 1024  /* the commit launch: ONE workgroup */
#define TREX_MON_SUMMARY_BLOCK 256  /* the summary launch: ONE workgroup */

// the batch's state, ONE allocation zeroed by every set, laid out as trex::MonitorLayout says
struct TrexMonState {
  double *ret, *col;                            /* [N], [N][C]: the running episode */
  unsigned long long *total, *by_reason;        /* [1], [4] */
  int32_t *len;                                 /* [N] */
  uint32_t *episodes, *fin;                     /* [N] each; fin: the env finished an episode in the last apply */
  float *last_return;                           /* [N]: the env's last finished record ... */
  int32_t *last_length, *last_reason;
  uint32_t *last_t;
  float *last_cols;                             /* ... [N][C] */
  uint32_t *t;                                  /* [1] */
  float *ring_return;                           /* [W]: the ring ... */
  int32_t *ring_length, *ring_reason;
  uint32_t *ring_env, *ring_t;
  float *ring_cols;                             /* ... [W][C] */
  uint32_t *counts;                             /* [groups]: finished envs per workgroup of the accumulate launch */
};

struct TrexMonArgs {
  TrexMonState st;
  const float *reward, *done;       /* element e at [e * stride] */
  const int32_t *reason;            /* [N] or NULL: zeros */
  const float *cols_a, *cols_b;     /* column c of env e at [e * stride + c]; NULL where the width is 0 */
  int reward_stride, done_stride, stride_a, stride_b;
  int n_envs, window, cols_a_n, cols_n, team, groups;
  uint32_t env_offset;
};

// the two launches of an apply: accumulate (every env; a count of finished envs per workgroup), then commit (one workgroup: the
// ring in ascending env order, total, by_reason, t)
extern "C" hipError_t trex_launch_monitor(const TrexMonArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_monitor_reset(const TrexMonState &st, const uint8_t *mask, int n_envs, int cols, hipStream_t stream);
extern "C" hipError_t trex_launch_monitor_summary(const TrexMonState &st, int window, int cols, double *out, hipStream_t stream);
