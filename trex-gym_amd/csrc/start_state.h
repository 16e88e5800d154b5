// Start-state randomisation (trex_batch_set_start_state / _apply_start_state / _start_state_reset / _start_state_info,
// include/trex_start_state.h): launch arguments shared by capi_start_state.cpp and start_state.hip; the term table is built by
// host_tables.cpp. The step kernels do not see any of this: the apply launch writes the state they read anyway.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"
#include "start_state_limits.h"

// the batch's state, ONE allocation, T terms
struct TrexStartState {
  uint32_t *ep, *started;         /* [N] each: episode count, 0 = the next row is a first one */
  float *shift;                   /* [N]: the z shift of the floor placement */
  int32_t *lowest;                /* [N]: the collision point that decided it, -1: none */
  float *values;                  /* [N][T][TREX_TL] */
};

struct TrexStartArgs {
  const TrexStartTable *table;
  const TrexDeviceModel *model;
  TrexStartState st;
  const float *done;              /* element e at done[e * done_stride] */
  float *base, *q, *qd;           /* the batch's state */
  const float4 *hull;             /* [nv] body-frame collision points: xyz + support radius */
  float *warm;                    /* [N][TREX_WARM_WORDS] or NULL */
  float *rows;                    /* nullable: row e at rows + e * row_stride */
  int n_envs, nj, done_stride, row_stride;
  uint32_t key0, key1, env_offset;
};

extern "C" hipError_t trex_launch_start_state(const TrexStartArgs &args, hipStream_t stream);
// started[e] = 0 for the marked envs (mask NULL: all)
extern "C" hipError_t trex_launch_start_state_reset(const uint8_t *mask, int n_envs, uint32_t *started, hipStream_t stream);
