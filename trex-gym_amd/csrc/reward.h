// Reward terms (trex_batch_set_reward / trex_batch_compose_reward / trex_batch_reward_reset): launch arguments shared by
// capi_queries.cpp and reward.hip; the term table is built by host_tables.cpp. The step kernels do not see any of this; the launch
// reads the batch state and writes the reward column of the caller's rows, the breakdown and the batch's reward history.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"
#include "observation.h"
#include "reward_limits.h"

/* The launch shape and the LDS records are K10's (observation.h): 256 lanes = 8 env slots x 32, per body R | origin | w | vo at an
 * odd stride, per slot URDF link 0's frame. */
#define TREX_REW_BLOCK TREX_OBS_BLOCK
#define TREX_REW_MAXENV TREX_OBS_MAXENV

struct TrexRewArgs {
  const TrexDeviceModel *model;
  const float *base, *q, *qd;     /* the batch's state (read only) */
  const TrexRewTerm *term;        /* [T] */
  const int32_t *joint_body;      /* [32] body lane of joint j, observation order */
  float *rows;                    /* [N] rows of row_stride floats: 3J observation columns | reward | done ...; column 3J is rewritten */
  const float *actions;           /* [N, act_cols], NULL without ACTION_RATE */
  const float *command;           /* [N, 3], NULL without a tracking term */
  const float *sens;              /* the batch's contact sensor [N][TREX_SENS_ROWS][TREX_TL], NULL without a contact kind */
  float *terms_out;               /* [N, T] or NULL */
  /* history, the batch's: */
  float *prev_act;                /* [N, act_cols] */
  float *prev_qd;                 /* [N, J] */
  float *timer, *held;            /* [N, T] each */
  int32_t *valid;                 /* [N] */
  int n_envs, D;                  /* D = 6 + J: the width walk_chain takes for its accelerations (none here) */
  int nj, num_terms, row_stride, act_cols;
  float Ts;                       /* dt * substeps */
  unsigned body_mask;             /* bit b: phase 1 walks body b (the terms' bodies and URDF link 0's) */
  int base_body;                  /* body of URDF link 0 ... */
  float base_tf[12];              /* ... and its body <- link transform ("link_tf") */
};

extern "C" hipError_t trex_launch_reward(const TrexRewArgs &args, hipStream_t stream);
/* invalidate the history of the envs with mask != 0 (NULL: all): flag 0, timers 0, held values 0 */
extern "C" hipError_t trex_launch_reward_reset(const uint8_t *mask, int n_envs, int num_terms, float *timer, float *held, int32_t *valid,
                                               hipStream_t stream);
