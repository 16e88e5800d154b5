// The pose pass of the ray kernels (render.hip, raycast.hip): the world pose of ONE body of an env from the env's base row and
// joint angles, one lane per body, every lane composing the hinges of its own chain in registers (anc: ancestor per depth).
// Unlike walk_chain (chain_walk.h) the origin is the world's, not the base's, and nothing but the pose is kept.
#pragma once
#include "device_math.h"
#include "device_model.h"

// Declares `float R[9], p[3]` in the caller's scope: world <- body rotation (row-major) and origin of body `t` (< M->nb) of
// env `env`. M: the device model, b: the env's base row ([16]: position, quaternion xyzw, ...), q: the batch's joint angles
// [N][TREX_TL].
// (A macro, not an inline function: as a function - by value, by reference or into arrays of the caller - the compiler commutes
// operands and reorders the multiply-adds of trex_render_kernel, whose instruction stream is to stay what it was when
// render.hip held this loop itself. Textual inclusion keeps it byte for byte.)
#define TREX_BODY_WORLD_POSE(M, b, q, env, t, R, p)                                                                                \
  float R[9], p[3] = {(b)[0], (b)[1], (b)[2]};                                                                                     \
  {                                                                                                                                \
    const float quat[4] = {(b)[3], (b)[4], (b)[5], (b)[6]};                                                                        \
    quat_to_mat(quat, R);                                                                                                          \
    const int dep = (M)->depth[t];                                                                                                 \
    for (int d = 1; d <= dep; d++) {                                                                                               \
      const int i = (M)->anc[d - 1][t];                                                                                            \
      const float ax[3] = {(M)->axis[0][i], (M)->axis[1][i], (M)->axis[2][i]},                                                     \
                  jp[3] = {(M)->jpos[0][i], (M)->jpos[1][i], (M)->jpos[2][i]};                                                     \
      float jr[9], rq[9], tmp[9];                                                                                                  \
      for (int c = 0; c < 9; c++) jr[c] = (M)->jrot[c][i];                                                                         \
      const float qi = (q)[(size_t)(env) * TREX_TL + i];                                                                           \
      const float c = cosf(qi), s = sinf(qi), tt = 1.f - c;                                                                        \
      rq[0] = tt * ax[0] * ax[0] + c;         rq[1] = tt * ax[0] * ax[1] - s * ax[2]; rq[2] = tt * ax[0] * ax[2] + s * ax[1];      \
      rq[3] = tt * ax[0] * ax[1] + s * ax[2]; rq[4] = tt * ax[1] * ax[1] + c;         rq[5] = tt * ax[1] * ax[2] - s * ax[0];      \
      rq[6] = tt * ax[0] * ax[2] - s * ax[1]; rq[7] = tt * ax[1] * ax[2] + s * ax[0]; rq[8] = tt * ax[2] * ax[2] + c;              \
      for (int r = 0; r < 3; r++) p[r] += R[3 * r] * jp[0] + R[3 * r + 1] * jp[1] + R[3 * r + 2] * jp[2];                          \
      for (int r = 0; r < 3; r++)                                                                                                  \
        for (int k = 0; k < 3; k++) tmp[3 * r + k] = R[3 * r] * jr[k] + R[3 * r + 1] * jr[3 + k] + R[3 * r + 2] * jr[6 + k];       \
      for (int r = 0; r < 3; r++)                                                                                                  \
        for (int k = 0; k < 3; k++) R[3 * r + k] = tmp[3 * r] * rq[k] + tmp[3 * r + 1] * rq[3 + k] + tmp[3 * r + 2] * rq[6 + k];   \
    }                                                                                                                              \
  }
