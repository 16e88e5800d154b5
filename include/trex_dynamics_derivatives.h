/*
 * trex_dynamics_derivatives.h - C-ABI of the first-order derivatives of the rigid-body dynamics of a TrexBatch
 * (include/trex_batch.h, whose conventions hold here: return codes, pointer validation - TREX_E_INVALID with nothing launched and
 * nothing changed -, streams, capturable from the second call with the same buffers on). trex_batch.h includes this header at its
 * end; including either one declares both.
 */
#ifndef TREX_DYNAMICS_DERIVATIVES_H
#define TREX_DYNAMICS_DERIVATIVES_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* out[n][j][i], one contiguous row per direction j - the rhs layout of trex_batch_solve_mass - instead of out[n][i][j] */
#define TREX_DERIV_BY_DIRECTION 1u

/* ---- derivatives of the inverse dynamics: with f = ID(q, v, a) = M(q) a + h(q, v) exactly as trex_batch_inverse_dynamics defines
 * it - D = 6 + J, classical accelerations, base torque about the base origin, joints in observation order, the env's mass scale,
 * gravity from the model parameter, RIGID-BODY terms only -, two [N, D, D] matrices per env at the env's current state:
 *
 * dfdq_dev[n][i][j] = d f_i / d xi_j, xi the configuration tangent, ordered like the generalised velocity: xi_0..2 move the base
 *   origin along the world axes; xi_3..5 turn the base by a WORLD-axis rotation vector, R <- exp([xi]x) R; xi_6.. are the joint
 *   angles in observation order. The NUMBERS of the velocity and of the acceleration are held fixed while the configuration moves:
 *   the world-axis base velocities v and w, qd, and the classical accelerations.
 * dfdv_dev[n][i][j] = d f_i / d v_j, v the generalised velocity (base linear, base angular, world axes; qd).
 * d f / d a is the mass matrix (trex_batch_mass_matrix).
 * accel_dev [N, D], nullable: the accelerations a the derivatives are taken at (NULL: zeros - the derivatives of the bias force).
 *
 * Exact zeros (== 0, not small numbers): columns 0..2 of dfdq (uniform gravity: no dependence on the position), columns 0..2 of
 *   dfdv (Galilean invariance of the classical form), and every joint-row / joint-column pair whose two joints lie on different
 *   branches of the tree, neither an ancestor of the other.
 * flags: 0, or TREX_DERIV_BY_DIRECTION: both outputs transposed, out[n][j][i] - a direction's D forces in one contiguous row, ready
 *   to be the K = D right-hand sides of trex_batch_solve_mass (d a / d x = -M^-1 d f / d x at a = forward dynamics).
 * Either output may be NULL; an output that is NULL costs no passes, and the other's bits do not depend on it. The results are
 *   bitwise repeatable.
 * The kinematic block of a state-space matrix is the caller's: for this rotation tangent d eps / dt = d w + w x eps.
 * Like the dynamics queries: asynchronous on `stream`, nothing allocated or waited for, only the outputs written, from the second
 * call with known buffers ONE plain kernel launch, usable inside a single-stream capture; a non-finite env affects its own block
 * only. TREX_E_INVALID, nothing launched: both outputs NULL, unknown flag bits, an output that overlaps accel_dev or the other
 * output, a buffer shorter than stated, host memory or another device's. */
int trex_batch_inverse_dynamics_derivatives(TrexBatch *batch, const float *accel_dev, float *dfdq_dev, float *dfdv_dev, uint32_t flags,
                                            void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_DYNAMICS_DERIVATIVES_H */
