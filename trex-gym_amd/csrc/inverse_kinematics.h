// Batched inverse kinematics (trex_batch_inverse_kinematics): launch arguments shared by capi_queries.cpp and inverse_kinematics.hip;
// the per-probe task values are built by host_tables.cpp. The step kernels do not see any of this; the query only reads the batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/trex_batch.h"
#include "device_model.h"

#define TREX_IK_WAVES 4           /* envs per workgroup: one 64-lane wavefront each */
/* LDS floats per env (= per wave), all of it private to the wave: */
#define TREX_IK_REC 16            /* per body: R 9 | origin 3 | joint axis 3 | pad */
#define TREX_IK_ASTRIDE 33        /* A [24][32 body lanes], rows one bank apart */
#define TREX_IK_GSTRIDE 25        /* Gram matrix / Cholesky factor [24][24], lower triangle, rows one bank apart */
#define TREX_IK_OFF_Q 0                                                        /* the iterate, by body lane        32 */
#define TREX_IK_OFF_REC (TREX_IK_OFF_Q + TREX_TL)                              /* body records                    512 */
#define TREX_IK_OFF_P (TREX_IK_OFF_REC + TREX_TL * TREX_IK_REC)                /* the probes' points [8][4]        32 */
#define TREX_IK_OFF_X (TREX_IK_OFF_P + TREX_IK_MAXPROBES * 4)                  /* the solve's x [24]               32 */
#define TREX_IK_OFF_A (TREX_IK_OFF_X + 32)                                     /* A                               792 */
#define TREX_IK_OFF_G (TREX_IK_OFF_A + TREX_IK_MAXROWS * TREX_IK_ASTRIDE)      /* G                               600 */
#define TREX_IK_ENV_FLOATS (TREX_IK_OFF_G + TREX_IK_MAXROWS * TREX_IK_GSTRIDE) /* 2000 floats = 8000 B per env        */

struct TrexIkArgs {
  const TrexDeviceModel *model;
  const float *base, *q;          /* the batch's state (read only) */
  const float *probe_tf;          /* [K][12] body <- link rotation, row-major (9) | the point in the BODY frame (3) */
  const float *target;            /* [N, K, 7] */
  const float *q_init;            /* [N, J] observation order; NULL: the batch's q */
  float *q_out, *info;            /* [N, J]; [N, 4] nullable */
  int n_envs, nb, K, M;
  int frame;                      /* TREX_AXES_WORLD / TREX_AXES_BASE */
  float base_tf[12];              /* TREX_AXES_BASE: URDF link 0's frame in the base body ("link_tf") */
  uint32_t move_mask;             /* bit b: the joint of body lane b may move */
  /* per probe, host values: its body, its mode, its first task row, and the bodies whose joints carry it (bit b: body b is
   * the probe's body or an ancestor of it, the base excluded) - from the model's tree */
  uint8_t body[TREX_IK_MAXPROBES], mode[TREX_IK_MAXPROBES], row0[TREX_IK_MAXPROBES];
  uint32_t chain[TREX_IK_MAXPROBES];
  int iterations;
  float damping2, gain, max_step, tol_pos, tol_ori;
};

extern "C" hipError_t trex_launch_inverse_kinematics(const TrexIkArgs &args, hipStream_t stream);
