// The boundary between capi.cpp and the kernels of trex_step.hip / trex_step_act.hip (the step launches) and batch_util.hip (the
// utility kernels): the step launch's argument struct, the one way to ask for a step launch, and the prototype of every launcher -
// written here once, for the definition and the call alike.
// Shared by the translation units of libtrex_hip.so (not installed, not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

// ACT rows of an env, per body lane: the joint's motor kp, kd, largest impulse of a substep (max_force * dt) and max_force - the
// gains as set -, then the kp and kd of the CURRENT env-step under stiffness actions (written by the step's action decode, read by
// its row set-ups on the same lane: the decode has the registers for the action's address and the square root, the set-up has not)
#define TREX_ACT_GAINS 4
#define TREX_ACT_ROWS 6
#define TREX_ACT_FLOATS (TREX_ACT_ROWS * TREX_TL)     /* per env: the batch's motor-gain buffer */
// SENS rows of an env: 0..5 the floor-contact wrench of every body (fx fy fz tx ty tz, world axes, at / about its COM), 6..8 the
// body's COM of the current substep relative to the base origin (written by the tree phases, read by the env's results pass)
#define TREX_SENS_ROWS 9
#define TREX_SENS_FLOATS (TREX_SENS_ROWS * TREX_TL)   /* per env: the batch's contact-sensor buffer */

// The kernel argument of every step launch, by value. (The field order is the kernels' kernarg layout.)
struct TrexStepArgs {
  const TrexDeviceModel *model;
  TrexBatchArrays arr;
  int n_envs;
  const float *actions;   // [N, J]
  float *obs;             // [N, 3J] nullable; row e starts at obs + e * obs_stride
  float *reward;          // [N] nullable; element e at reward[e * scal_stride]
  uint8_t *done;          // [N] nullable
  float *done_f;          // done as 0.0 / 1.0 at done_f[e * scal_stride] (row-block output), nullable
  int obs_stride, scal_stride;
  float *penalties;       // [N, 3] nullable
  const uint8_t *reset_mask;  // RESET only, nullable = all
  int32_t *bal;               // rank lists of the wave balance (step launches), nullable = workgroup k runs env k
  float w_distance, w_energy, w_drift;
  float *debug;           // diagnostics of env 0's last substep (tests), nullable
  // MULTI launches (trex_batch_step_many): n_steps env-steps per launch; step s reads actions + s * N * J and writes the
  // row block at + s * step_rows floats (obs, reward, done_f alike), done bytes at + s * N, penalties at + s * 3 N
  int n_steps;
  long long step_rows;
  int pen_in_rows;        // row-block launches of a batch with trex_batch_set_penalties_in_rows: the three penalties follow done in the row
  float *warm;            // WARM launches: the per-env warm-start records [N][TREX_WARM_WORDS] (device_model.h); last, so that
                          // every other argument keeps its offset
  const float *ext;       // EXT launches: the per-env external wrench [N][6][TREX_TL] (fx fy fz tx ty tz, world axes, at / about the
                          // body's COM; trex_batch_set_external_wrench); after warm for the same reason
  float *sens;            // SENS launches: the per-env contact sensor [N][TREX_SENS_ROWS][TREX_TL] (trex_batch_set_contact_sensor)
  // ACT launches (the actuator model): the per-env motor gains [N][TREX_ACT_ROWS][TREX_TL], which body lanes' joints are VELOCITY /
  // TORQUE controlled (bit b = body lane b; wave- and batch-uniform: scalar registers), the width of an action row - J, or 2J with
  // stiffness actions - and the upper clip of an action's stiffness; last, so that every other argument keeps its offset
  float *act;             // (not const: with stiffness actions the action decode writes the env-step's kp, kd into rows 4, 5)
  unsigned act_vel, act_tor;
  int act_cols;
  float act_kp_max;
};

// What a launch is for. The feature variant of its kernel is read off the arguments: a non-null warm / ext / sens / act pointer IS
// that feature switched on.
enum TrexStepKind {
  TREX_KIND_STEP,         // one env-step; the pair form where trex_step_launch_shape says so
  TREX_KIND_STEP_MANY,    // args.n_steps env-steps per launch
  TREX_KIND_RESET,
  TREX_KIND_STEP_DEBUG    // one env-step with the diagnostics dump (args.debug): env k in workgroup k, whatever args.bal says
};
enum : unsigned { TREX_FEAT_WARM = 1u, TREX_FEAT_EXT = 2u, TREX_FEAT_SENS = 4u, TREX_FEAT_ACT = 8u, TREX_FEAT_COUNT = 16u };
inline unsigned trex_step_features(const TrexStepArgs &a) {
  return (a.warm ? TREX_FEAT_WARM : 0u) | (a.ext ? TREX_FEAT_EXT : 0u) | (a.sens ? TREX_FEAT_SENS : 0u) | (a.act ? TREX_FEAT_ACT : 0u);
}
// launch shape of a launch of this kind for n envs with these features: what it is launched with, and what trex_batch_launch_info
// reports of the step launch
struct TrexStepShape { int envs_per_workgroup, grid, block, lds_bytes; };
// a step kernel as the variant table (trex_step_body.h) hands it out
typedef void (*TrexStepKernel)(TrexStepArgs);

extern "C" {
TrexStepShape trex_step_launch_shape(TrexStepKind kind, int n, unsigned features);
hipError_t trex_launch_step(const TrexStepArgs *args, TrexStepKind kind, hipStream_t stream);
TrexStepKernel trex_step_act_variant(int form, unsigned features);   // trex_step_act.hip's half of the variant table
hipError_t trex_launch_pack_state(const TrexDeviceModel *model, TrexBatchArrays arr, int n, float *state, int pack, hipStream_t stream);
hipError_t trex_launch_head(const TrexDeviceModel *model, TrexBatchArrays arr, int n, float *out, hipStream_t stream);
hipError_t trex_launch_link_transforms(const TrexDeviceModel *model, TrexBatchArrays arr, int n, float *out, hipStream_t stream,
                                       int visuals);
hipError_t trex_launch_scalars_get(TrexBatchArrays arr, int n, int32_t *count, float *impulse, int32_t *steps, hipStream_t stream);
hipError_t trex_launch_scalars_set(TrexBatchArrays arr, int n, const int32_t *steps, int set_steps, int motors, hipStream_t stream);
hipError_t trex_launch_fill(float *p, float v, int n, hipStream_t stream);
hipError_t trex_launch_fill_u8(uint8_t *p, uint8_t v, int n, hipStream_t stream);
hipError_t trex_launch_copy_mass_scale(const float *src, float *dst, int n, int nb, hipStream_t stream);
hipError_t trex_launch_copy_wrench(const float *src, float *dst, int n, int nb, hipStream_t stream);
hipError_t trex_launch_copy_gains(const TrexDeviceModel *model, const float *kp, const float *kd, const float *max_force, float *dst,
                                  int n, hipStream_t stream);
hipError_t trex_launch_contact_wrench(const float *src, float *dst, int n, int nb, hipStream_t stream);
}
