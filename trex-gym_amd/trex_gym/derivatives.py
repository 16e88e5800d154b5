"""First-order derivatives of the rigid-body dynamics of a TrexVecEnv (include/trex_dynamics_derivatives.h): how the generalised
force of inverse_dynamics(), and the acceleration of forward_dynamics(), change with the configuration and the velocity - what
iLQR / DDP, linearised MPC, LQR around a pose, sensitivity-based identification and analytic policy gradients ask of a model.

    inverse_dynamics_derivatives(env, accel=None, wrt=("q", "v"), ...)   (dfdq, dfdv) [n, D, D], one launch
    forward_dynamics_derivatives(env, force=None, tau=None, out=None)    (accel, dadq, dadv, minv), no host round trip
    gravity_stiffness(env)                                               [n, J, J] the joint block of dfdq at zero acceleration

Every function takes a TrexVecEnv or a TrexBulletEnv (its one env: n = 1) and returns device tensors.

D = 6 + J and the conventions are those of the dynamics queries: classical accelerations, base torque about the base origin, the
env's mass scale, rigid-body terms only. out[e, i, j] = d f_i / d x_j. The configuration tangent is ordered like the generalised
velocity: columns 0..2 move the base origin along the world axes (exact zeros), columns 3..5 turn the base by a WORLD-axis rotation
vector (R <- exp([xi]x) R), columns 6.. are the joint angles in observation order; the numbers of the world-axis velocities and of
the accelerations are held fixed while the configuration moves. d f / d a is mass_matrix().

Not here: derivatives of the STEP (contacts, limits, motors, damping), second derivatives, and the kinematic block of a state-space
A matrix - for this rotation tangent d eps / dt = d w + w x eps, left to the caller."""
import torch

from . import derivatives_capi as DC
from ._capi import _shaped


def _vec(env):
    return getattr(env, "_vec", env)


def _api(v):
    return DC.BatchDerivatives(v.batch)


def inverse_dynamics_derivatives(env, accel=None, wrt=("q", "v"), by_direction=False, out_q=None, out_v=None):
    """-> (dfdq, dfdv), each [n, D, D] or None where `wrt` leaves it out (an output left out costs nothing, and the other's bits do
    not depend on it): the derivatives of inverse_dynamics(accel) at the current state; accel [n, D] or None (zeros: the derivatives
    of the bias force). by_direction: both transposed, out[e, j, i] - one contiguous row per direction, the rhs layout of
    solve_mass. out_q, out_v: tensors to fill instead of new ones (they must not overlap accel)."""
    v = _vec(env)
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    if not wrt or any(x not in ("q", "v") for x in wrt):
        raise ValueError("wrt: expected 'q', 'v' or both, got %r" % (wrt,))
    if accel is not None:
        accel = v._dev(torch.as_tensor(accel))
    want = lambda key, out: (True if out is None else out) if key in wrt else None
    return _api(v).inverse_dynamics_derivatives(accel, want("q", out_q), want("v", out_v), DC.BY_DIRECTION if by_direction else 0)


def forward_dynamics_derivatives(env, force=None, tau=None, out=None):
    """-> (accel [n, D], dadq, dadv, minv [n, D, D]): accel = forward_dynamics(force, tau), its derivatives along the configuration
    tangent and the generalised velocity at a fixed force, d a / d x = -M^-1 (d f / d x at that accel), in Jacobian layout
    out[e, i, j], and minv = d a / d force = inverse_mass_matrix(). out: four tensors of these shapes to fill instead of new ones.
    Five launches and two negated transposes, no host round trip and no buffer besides the four: with `out` the call allocates
    nothing, and from the second call with the same tensors on it is capturable."""
    v = _vec(env)
    n, D = v.num_envs, 6 + v.J
    if out is None:
        new = lambda *shape: torch.empty(n, *shape, dtype=torch.float32, device=v.device)
        out = [new(D), new(D, D), new(D, D), new(D, D)]
    accel, dadq, dadv, minv = out
    for k, t in enumerate(out):
        _shaped(t, (n, D) if k == 0 else (n, D, D), "out[%d]" % k)
    v.forward_dynamics(force, tau, out=accel)
    # the derivatives BY DIRECTION - one row per direction, K = D right-hand sides - into the two buffers that are free yet
    _api(v).inverse_dynamics_derivatives(accel, dadv, minv, DC.BY_DIRECTION)
    v.solve_mass(dadv, dadv)                               # (in place)
    torch.neg(dadv.transpose(1, 2), out=dadq)
    v.solve_mass(minv, minv)
    torch.neg(minv.transpose(1, 2), out=dadv)
    v.inverse_mass_matrix(minv)
    return accel, dadq, dadv, minv


def gravity_stiffness(env):
    """-> [n, J, J]: the joint block of dfdq at zero acceleration, d tau_i / d q_j of the torques that hold the state - the
    stiffness a gravity-compensating PD loop sees (at rest: gravity alone; in motion the velocity-product terms are in it)."""
    dfdq, _ = inverse_dynamics_derivatives(env, None, "q")
    return dfdq[:, 6:, 6:].contiguous()
