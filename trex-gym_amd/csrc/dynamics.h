// Dynamics queries (trex_batch_inverse_dynamics / _mass_matrix / _jacobian / _centroidal / _forward_dynamics / _solve_mass):
// launch arguments shared by capi.cpp and dynamics.hip. The step kernels do not see any of this; the queries only read the batch state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

#define TREX_DYN_WAVES 4          /* envs per workgroup: one per wavefront, one body per lane */
#define TREX_DYN_BODY_FLOATS 512  /* LDS floats per env for the per-body records of the tree passes (16 per body) */
#define TREX_DYN_CENT_FLOATS 16   /* floats per env of trex_batch_centroidal */
/* forward dynamics and solve_mass (ABA): 37 floats per body - articulated inertia 21, origin 3, one wrench / acceleration slot
 * of 6 for each of the two right-hand sides a wave carries in its lane halves, 1 pad: an odd stride, so that the 32 bodies of an
 * env read one field from 32 different LDS banks */
#define TREX_DYN_ABA_STRIDE 37
#define TREX_DYN_ABA_FLOATS (32 * TREX_DYN_ABA_STRIDE)
#define TREX_DYN_MAX_RHS 64       /* right-hand sides per env of trex_batch_solve_mass: 4 x (1184 + 64 x 31) floats = 50.7 KB of LDS */

enum TrexDynQuery {
  TREX_DYN_INVERSE_DYNAMICS, TREX_DYN_MASS_MATRIX, TREX_DYN_JACOBIAN, TREX_DYN_CENTROIDAL, TREX_DYN_FORWARD_DYNAMICS, TREX_DYN_SOLVE_MASS,
  TREX_DYN_COUNT
};

struct TrexDynArgs {
  const TrexDeviceModel *model;
  const float *base, *q, *qd;     /* the batch's state (read only) */
  const float *mass_scale;        /* [N][32] per-env mass scale, NULL = 1 (no domain set) */
  int n_envs, nb;                 /* nb = moving bodies; D = 6 + nb - 1 generalised velocities */
  const float *accel;             /* inverse dynamics: [N, D], NULL = zeros */
  float *out;                     /* [N, D] | [N, D, D] | [N, 6, D] | [N, 16] | [N, D] | [N, K, D] */
  int jac_body;                   /* Jacobian: the body that carries the point ... */
  float jac_point[3];             /* ... and the point in that body's frame (link frame composed on the host) */
  const float *rhs;               /* forward dynamics: force [N, D], NULL = zeros; solve_mass: [N, K, D], NULL = the identity (K = D) */
  int num_rhs;                    /* solve_mass: K, 1 .. TREX_DYN_MAX_RHS (forward dynamics: 1) */
};

/* floats each env writes, and the dynamic LDS bytes of a workgroup, for query q of a model with D velocities (K right-hand
 * sides: solve_mass only) */
constexpr int trex_dyn_out_floats(int q, int D, int K = 1) {
  return q == TREX_DYN_INVERSE_DYNAMICS || q == TREX_DYN_FORWARD_DYNAMICS ? D
         : q == TREX_DYN_MASS_MATRIX  ? D * D
         : q == TREX_DYN_JACOBIAN     ? 6 * D
         : q == TREX_DYN_SOLVE_MASS   ? K * D
                                      : TREX_DYN_CENT_FLOATS;
}
constexpr int trex_dyn_body_floats(int q) {
  return q == TREX_DYN_FORWARD_DYNAMICS || q == TREX_DYN_SOLVE_MASS ? TREX_DYN_ABA_FLOATS : TREX_DYN_BODY_FLOATS;
}
constexpr int trex_dyn_lds_bytes(int q, int D, int K = 1) {
  /* the body records of the four envs, then their outputs back to back as they lie in HBM (a multiple of 16 bytes) */
  return TREX_DYN_WAVES * (trex_dyn_body_floats(q) + trex_dyn_out_floats(q, D, K)) * (int)sizeof(float);
}

extern "C" hipError_t trex_launch_dynamics(const TrexDynArgs &args, int query, hipStream_t stream);   /* dynamics.hip */
