// Batched link kinematics (trex_batch_set_link_probes / trex_batch_link_state): launch arguments shared by capi_queries.cpp and
// link_state.hip; the probe table is built by host_tables.cpp. The step kernels do not see any of this; the query only reads the batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

#define TREX_LINK_BLOCK 256       /* lanes per workgroup = probes per workgroup at most: 4 waves, one probe per lane */
#define TREX_LINK_MAXENV 8        /* envs whose body records one workgroup holds in LDS: 8 x 32 body lanes = one pass of the 256 lanes */
#define TREX_LINK_SETS 8          /* probe sets per batch */
#define TREX_LINK_MAXPROBES 1024  /* probes per set */
/* LDS floats per body: R 9 | origin 3 | w 3 | vo 3 | al 3 | ao 3 - six 16-byte reads */
#define TREX_LINK_REC 24
/* LDS floats per env slot: TREX_TL records, + 4 so that the slots of one wave's lanes start 4 banks apart (a 16-byte read of the
 * same body by lanes of different envs then touches disjoint banks), as TREX_RAY_SLOT */
#define TREX_LINK_SLOT (TREX_TL * TREX_LINK_REC + 4)

struct TrexLinkArgs {
  const TrexDeviceModel *model;
  const float *base, *q, *qd;     /* the batch's state (read only; qd with velocity or acceleration only) */
  const float *accel;             /* [N, D], NULL = zeros (read with acceleration only) */
  const int32_t *probe_body;      /* [K] body of each probe's link */
  const float *probe_tf;          /* [K][12] body <- link rotation, row-major (9) | the point in the BODY frame (3) */
  float *pose, *vel, *acc;        /* [N, K, 7], [N, K, 6], [N, K, 6], each nullable */
  int n_envs, num_probes, D;
  int axes, proper;               /* TREX_AXES_*; proper: + g z on the linear acceleration */
  int base_body;                  /* TREX_AXES_BASE: body of URDF link 0 ... */
  float base_tf[12];              /* ... and its body <- link transform ("link_tf") */
  int epw, cpe;                   /* envs per workgroup; workgroups (chunks of 256 probes) per env group: trex_link_shape */
};

/* How a call of N envs x K probes is cut into workgroups: K >= 256: one env per workgroup, ceil(K / 256) workgroups per env;
 * below: min(8, 256 / K) whole envs per workgroup, lane = slot * K + probe. */
static inline void trex_link_shape(int num_probes, int *epw, int *cpe) {
  if (num_probes >= TREX_LINK_BLOCK) {
    *epw = 1;
    *cpe = (num_probes + TREX_LINK_BLOCK - 1) / TREX_LINK_BLOCK;
  } else {
    const int e = TREX_LINK_BLOCK / num_probes;
    *epw = e < TREX_LINK_MAXENV ? e : TREX_LINK_MAXENV;
    *cpe = 1;
  }
}

/* link_state.hip: the instantiation is chosen by the outputs given - pose only, pose + velocity, all three */
extern "C" hipError_t trex_launch_link_state(const TrexLinkArgs &args, hipStream_t stream);
