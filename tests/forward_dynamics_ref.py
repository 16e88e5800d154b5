"""numpy f64 reference of the two inverse queries (include/trex_batch.h: trex_batch_forward_dynamics, trex_batch_solve_mass),
built on tests/dynamics_ref.py by dense linear algebra - no articulated-body recursion, which both the kernel and the oracle use:

    forward_dynamics = solve(M, force - h)      M from per-body Jacobians, h from RNEA with zero accelerations
    minv             = inv(M)

tests/test_forward_dynamics_ref.py ties it to the oracle's ABA (oracle_forward_dynamics, oracle_minv). Conventions as in
dynamics_ref: generalised velocity [v(3), w(3), qd in observation order], forces its duals."""
import numpy as np

import dynamics_ref as R


def forward_dynamics(model, state, force=None, mass_scale=None, gravity=9.81, velocity_terms=True):
    """[D] accelerations M^-1 (force - h); force None = zeros. velocity_terms False: h of the same pose at rest (gravity
    alone) - the WRONG answer a tolerance has to tell from the right one."""
    state = np.asarray(state, np.float64)
    if not velocity_terms:
        nj = (len(state) - 13) // 2
        state = state.copy()
        state[7:13] = 0.0
        state[13 + nj:] = 0.0
    M = R.mass_matrix(model, state, mass_scale)
    h = R.inverse_dynamics(model, state, None, mass_scale, gravity)
    f = np.zeros(len(h)) if force is None else np.asarray(force, np.float64)
    return np.linalg.solve(M, f - h)


def minv(model, state, mass_scale=None):
    return np.linalg.inv(R.mass_matrix(model, state, mass_scale))


def solve_mass(model, state, rhs, mass_scale=None):
    """rows of rhs [K, D] -> rows of x [K, D] = (M^-1 rhs^T)^T"""
    return np.linalg.solve(R.mass_matrix(model, state, mass_scale), np.asarray(rhs, np.float64).T).T


def accel_dev(got, want):
    """fd_accel: |a - a_ref| per block (base linear, base angular, joints) over the block's largest |a_ref|, floored at
    1 m/s^2, 1 rad/s^2, 1 rad/s^2"""
    d = np.abs(np.asarray(got, np.float64) - want)
    return max(d[sl].max() / max(np.abs(want[sl]).max(), 1.0) for sl in (slice(0, 3), slice(3, 6), slice(6, None)))


def minv_dev(M, Minv_got):
    """minv: (M / sqrt(M_ii M_jj)) @ (Minv_got * sqrt(M_ii M_jj)) - I, over ||N^-1||_1 of the exact inverse in that scaling
    (the normalisation of the `minv` figure of tests/test_gpu_dynamics.py), and the largest asymmetry of Minv_got in the same
    scaling and over the same norm"""
    dg = np.sqrt(np.diag(M))
    Ni = np.linalg.inv(M) * np.outer(dg, dg)
    G = np.asarray(Minv_got, np.float64) * np.outer(dg, dg)
    norm = np.abs(Ni).sum(0).max()
    E = (M / np.outer(dg, dg)) @ G - np.eye(len(dg))
    return np.abs(E).max() / norm, np.abs(G - G.T).max() / norm
