// Sensor model (trex_batch_set_sensing / _apply_sensing / _sensing_reset / _set_action_delay / _delay_actions,
// include/trex_sensing.h): launch arguments shared by capi_sensing.cpp and sensing.hip; the group table is built by
// host_tables.cpp. The step kernels do not see any of this. The apply launch writes the caller's out rows, the counters, the
// drawn delays and the history; the delay launch the caller's out actions and the action history.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sensing_limits.h"

#define TREX_SENSE_BLOCK 256

struct TrexSenseArgs {
  const TrexSenseGrp *group;      /* [G] */
  const int16_t *col_group;       /* [D] */
  const int16_t *col_hist;        /* [D] */
  const float *rows;              /* [N][row_stride] */
  float *out;                     /* [N][out_stride]; may be `rows` itself */
  uint32_t *ep, *k, *started;     /* [N] each: episode count, row count, 0 = the next row is a first one */
  int32_t *delay;                 /* [N][G]: the delays of the current episode */
  float *hist;                    /* [TREX_SENSE_SLOTS][N][delayed] or NULL */
  int n_envs, obs_dim, tail, num_groups, delayed, row_stride, out_stride;
  int lanes;                      /* lanes of an env: a power of two in [8, 256], >= ceil((obs_dim + tail) / 4) */
  uint32_t key0, key1, env_offset;
};

struct TrexActDelayArgs {
  const float *actions;           /* [N][A] */
  const uint8_t *done_prev;       /* [N] or NULL */
  float *out;                     /* [N][A]; may be `actions` itself */
  uint32_t *ep, *k, *started;     /* [N] each */
  int32_t *delay;                 /* [N] */
  float *hist;                    /* [TREX_SENSE_SLOTS][N][A] */
  int n_envs, cols, delay_min, delay_max;
  uint32_t key0, key1, env_offset;
};

extern "C" hipError_t trex_launch_sensing(const TrexSenseArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_sensing_reset(const uint8_t *mask, int n_envs, uint32_t *started, uint32_t *act_started,
                                                hipStream_t stream);
extern "C" hipError_t trex_launch_delay_actions(const TrexActDelayArgs &args, hipStream_t stream);
