// Episode randomisation (trex_batch_set_randomization / _apply_randomization / _randomization_reset / _randomization_info,
// include/trex_randomize.h): launch arguments shared by capi_randomize.cpp, capi.cpp (the push base of
// trex_batch_set_external_wrench) and randomize.hip; the term table is built by host_tables.cpp. The step kernels do not see any
// of this: the apply launch writes the buffers they read anyway.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/trex_randomize.h"
#include "device_model.h"

#define TREX_RAND_BLOCK 256

// the device table: the terms as host_tables.cpp checked them, the index of each among the PUSH terms (-1: another kind), the body
// of every PUSH term
struct TrexRandTable {
  TrexRandomTerm term[TREX_RAND_MAXTERMS];
  int32_t push_slot[TREX_RAND_MAXTERMS];
  int32_t push_body[TREX_RAND_MAXPUSHES];
};

// the batch's state, ONE allocation, T terms of which P are pushes
struct TrexRandState {
  uint32_t *ep, *k, *started;     /* [N] each: episode count, row count, 0 = the next row is a first one */
  int32_t *off;                   /* [N][P]: the phase of the episode */
  int32_t *push_left;             /* [N][P] */
  float *push_force;              /* [N][P][3]: the force in effect, zeros while push_left is 0 */
  float *push_base;               /* [N][P][6]: the caller's wrench on the push bodies */
  float *values;                  /* [N][T][TREX_TL] */
};

struct TrexRandArgs {
  const TrexRandTable *table;
  const TrexDeviceModel *model;
  TrexRandState st;
  const float *done;              /* element e at done[e * done_stride] */
  float *command;                 /* [N][3] or NULL */
  float *mass_scale;              /* [N][TREX_TL] */
  float *friction;                /* [N] */
  float *gains;                   /* [N][TREX_ACT_ROWS][TREX_TL] or NULL */
  const float *nominal;           /* the same, as snapshotted at the set */
  float *wrench;                  /* [N][6][TREX_TL] or NULL */
  int n_envs, num_terms, num_pushes, done_stride;
  uint32_t key0, key1, env_offset;
};

extern "C" hipError_t trex_launch_randomize(const TrexRandArgs &args, hipStream_t stream);
extern "C" hipError_t trex_launch_randomize_reset(const uint8_t *mask, int n_envs, uint32_t *started, hipStream_t stream);
// the push bodies' columns after trex_batch_set_external_wrench copied the caller's wrench `src` ([N, nb, 6]; NULL: zeros): base =
// src, wrench = base + the force in effect; restore 1: wrench = the base as kept, no force (what a clear leaves
// behind); restore 2: base = the wrench as found (what a set starts from)
extern "C" hipError_t trex_launch_randomize_rebase(const TrexRandTable *table, TrexRandState st, const float *src, float *wrench, int n_envs,
                                                   int nb, int num_pushes, int restore, hipStream_t stream);
