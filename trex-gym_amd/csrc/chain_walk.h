// The base-to-body chain walk: the pose of one body from the env's base pose and joint angles, and on request the classical
// velocity and acceleration of its frame. One place for every kernel that needs forward kinematics outside the step body
// (dynamics.hip, batch_util.hip); the step body shares parents' results between lanes instead (forward_kinematics).
#pragma once
#include "device_math.h"
#include "device_model.h"

// What a lane knows of its body after walking the chain base -> body (at most MAXD hinges): pose, joint axis, and - VEL, ACC -
// the classical velocity and acceleration of the body frame. All in world axes, positions relative to the base origin.
struct Walk {
  float R[9];    // world <- body
  float r[3];    // body (= joint) origin
  float a[3];    // joint axis
  float w[3];    // angular velocity
  float vo[3];   // velocity of the body origin
  float al[3];   // angular acceleration
  float ao[3];   // classical acceleration of the body origin, PLUS g z: gravity as the base's upward acceleration
};

// Level by level over depth: at level d every lane of depth >= d advances over its ancestor at that depth (itself at its
// own). The lanes of one chain repeat their common ancestors' arithmetic in registers instead of waiting for them in LDS.
// base_rows, q, qd: the batch's state arrays ([N][16], [N][TREX_TL]; qd read with VEL only), env: the env; accel: with ACC the
// [N, D] rows of generalised accelerations (base linear, base angular, joints in observation order), null = zeros; b: the body.
// (The arrays by reference: a kernel-argument field is then loaded where the walk first uses it, as it was before the walk was
// shared, and the dynamics kernels keep their instruction streams.)
template <bool VEL, bool ACC>
__device__ __forceinline__ void walk_chain(const TrexDeviceModel *M, const float *const &base_rows, const float *const &q, const float *const &qd,
                                           const float *const &accel, int env, int b, int D, Walk &k) {
  const float *base = base_rows + (size_t)env * 16;
  const float quat[4] = {base[3], base[4], base[5], base[6]};
  quat_to_mat(quat, k.R);
  const float *acc = ACC && accel ? accel + (size_t)env * D : nullptr;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    k.r[c] = 0.f; k.a[c] = 0.f;
    k.vo[c] = VEL ? base[7 + c] : 0.f; k.w[c] = VEL ? base[10 + c] : 0.f;
    k.ao[c] = acc ? acc[c] : 0.f; k.al[c] = acc ? acc[3 + c] : 0.f;
  }
  if (ACC) k.ao[2] += M->prm[TP_GRAVITY];
  const int maxdepth = M->maxdepth;
  for (int d = 1; d <= maxdepth; d++) {
    const int i = M->anc[d - 1][b];
    if (i < 0) continue;
    const float ax[3] = {M->axis[0][i], M->axis[1][i], M->axis[2][i]}, jp[3] = {M->jpos[0][i], M->jpos[1][i], M->jpos[2][i]};
    float jr[9], rq[9], t[9], dw[3];
#pragma unroll
    for (int c = 0; c < 9; c++) jr[c] = M->jrot[c][i];
    matvec3(k.R, jp, dw);   // parent origin -> this origin, a point of the PARENT body
    if (VEL) {
      float wxd[3];
      cross3(k.w, dw, wxd);
      if (ACC) {
        float axd[3], wwd[3];
        cross3(k.al, dw, axd); cross3(k.w, wxd, wwd);
#pragma unroll
        for (int c = 0; c < 3; c++) k.ao[c] += axd[c] + wwd[c];
      }
#pragma unroll
      for (int c = 0; c < 3; c++) k.vo[c] += wxd[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) k.r[c] += dw[c];
    const float qi = q[(size_t)env * TREX_TL + i];
    hinge_rot(nullptr, ax, cosf(qi), sinf(qi), rq);
    matmul3(k.R, jr, t);
    matmul3(t, rq, k.R);
    matvec3(k.R, ax, k.a);
    if (VEL) {
      const float qdi = qd[(size_t)env * TREX_TL + i];
      if (ACC) {
        // d/dt (a qd) = a qdd + (w_parent x a) qd
        const float qdd = acc ? acc[6 + M->obs_slot[i]] : 0.f;
        float wxa[3];
        cross3(k.w, k.a, wxa);
#pragma unroll
        for (int c = 0; c < 3; c++) k.al[c] += k.a[c] * qdd + wxa[c] * qdi;
      }
#pragma unroll
      for (int c = 0; c < 3; c++) k.w[c] += k.a[c] * qdi;
    }
  }
}
