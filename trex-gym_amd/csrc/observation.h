// Observation channels (trex_batch_set_observation / trex_batch_compose_rows): launch arguments shared by capi_queries.cpp and
// observation.hip; the channel table is built by host_tables.cpp. The step kernels do not see any of this; the launch only reads the
// batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"
#include "observation_limits.h"

#define TREX_OBS_BLOCK 256        /* lanes per workgroup: 8 env slots x 32 lanes - one lane per body in phase 1, 32 columns a pass in phase 2 */
#define TREX_OBS_MAXENV 8         /* envs per workgroup */
/* LDS floats per body: R 9 | origin 3 | w 3 | vo 3, + 1: an odd stride, so that the 32 body lanes of a slot write 32 banks */
#define TREX_OBS_REC 19
#define TREX_OBS_SLOT (TREX_TL * TREX_OBS_REC + 4)
/* LDS floats per env slot for URDF link 0's frame: A = world <- base axes 9 | its origin, relative to the base body's 3 | the
 * origin's velocity 3 | the angular velocity 3, both already in base axes */
#define TREX_OBS_FRAME 20

struct TrexObsArgs {
  const TrexDeviceModel *model;
  const float *base, *q, *qd;     /* the batch's state (read only) */
  const TrexObsChan *chan;        /* [C] */
  const uint8_t *col_chan;        /* [E] channel of every extra column */
  const float *rows;              /* [N] rows of row_stride floats: 3J observation columns | tail */
  const float *actions;           /* [N, act_cols], NULL = zeros */
  const float *ext;               /* [N] rows of ext_stride floats (EXTERNAL channels), else NULL */
  const float *sens;              /* the batch's contact sensor [N][TREX_SENS_ROWS][TREX_TL] (CONTACT_FORCE channels), else NULL */
  float *out;                     /* [N] rows of out_stride floats: 3J | E | tail */
  int n_envs, D;                  /* D = 6 + J: the width walk_chain takes for its accelerations (none here) */
  int nobs, extra, tail;          /* 3J, E, 2 or 5 */
  int row_stride, out_stride, ext_stride, act_cols;
  unsigned body_mask;             /* bit b: phase 1 walks body b (the channels' bodies and URDF link 0's) */
  int base_body;                  /* body of URDF link 0 ... */
  float base_tf[12];              /* ... and its body <- link transform ("link_tf") */
};

extern "C" hipError_t trex_launch_observation(const TrexObsArgs &args, hipStream_t stream);
