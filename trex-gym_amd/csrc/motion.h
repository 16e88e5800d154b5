// Motion clip (trex_batch_set_motion / _motion_sample / _set_motion_reward / _compose_motion_reward / _motion_reset,
// include/trex_motion.h): launch arguments shared by capi_motion.cpp and motion.hip; the clip table is built by host_tables.cpp.
// The step kernels do not see any of this. The sample launch only reads; the compose launch writes the reward column of the
// caller's rows, the breakdown, the clocks and the held values; the reset launch writes the state of the masked envs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"
#include "motion_limits.h"

#define TREX_MOT_BLOCK 256
#define TREX_MOT_MAXENV 8          /* env slots of a workgroup: 32 lanes each */
#define TREX_MOT_REF 80            /* floats of a slot's reference state in LDS: 13 + 2J <= 75 */
#define TREX_MOT_REC 13            /* floats of a chain record in LDS: R (9) | origin (3), an odd stride */
#define TREX_MOT_ROLES 18          /* chain records per slot: probe k at the state [k], at the reference [8 + k]; URDF link 0's body [16], [17] */

struct TrexMotArgs {
  const TrexDeviceModel *model;
  const float *table;             /* the clip: [frames][stride] */
  float *base, *q, *qd;           /* the batch's state: read by compose, written by reset */
  const float *time;              /* [N] or NULL: sample - NULL = the clocks; reset - NULL = 0 */
  const uint8_t *mask;            /* reset: [N] or NULL = all */
  float *t0;                      /* the clocks: start time [N] ... */
  int32_t *k;                     /* ... and step count [N] */
  float *held;                    /* [N, T], NULL while no terms are set */
  float *rows;                    /* compose: rewritten in column 3J; reset: columns [0, 3J), or NULL */
  float *terms_out;               /* compose: [N, T] or NULL */
  float *state_out, *points_out, *phase_out;   /* sample */
  float *warm;                    /* reset: the warm-start records [N][TREX_WARM_WORDS] or NULL */
  const int32_t *probe_body;      /* [K] */
  const float *probe_tf;          /* [K][12] body <- link rotation | the point in the body frame */
  TrexMotTerm term[TREX_MOT_MAXTERMS];
  int n_envs, nj, frames, stride, loop, num_terms, num_probes, row_stride;
  float frame_dt, inv_dt, duration, inv_duration, disp[2], Ts, step_weight;
  int base_body;                  /* body of URDF link 0 ... */
  float base_tf[12];              /* ... and its body <- link transform */
};

extern "C" hipError_t trex_launch_motion_sample(const TrexMotArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_motion_compose(const TrexMotArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_motion_reset(const TrexMotArgs &args, hipStream_t stream);
