"""Shared by the GPU parity tests: the committed golden rollout, the one-step comparison with the f64 oracle at the tolerances stated
at the top of tests/test_gpu_parity.py, for any joint count and motor limit, and the per-body contact wrench of one env-step restated
on the oracle."""
import os

import numpy as np

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_rollout.npz"))


def assert_step_close(g_obs, o_obs, g_rew=None, o_rew=None, what="", q_atol=1e-4, loosen=1.0, J=25, max_force=3.0e5,
                      tau_floor=1.0, tau_extra=0.0):
    """tau_floor / tau_extra: the absolute part of the torque tolerance - the T-rex's +1 N m; for a model whose torques are
    themselves a few N m, 0 and 3 x the deviation of the oracle's own f32 build on the same state."""
    assert np.isfinite(g_obs).all(), what
    np.testing.assert_allclose(g_obs[:J], o_obs[:J], atol=q_atol, rtol=0, err_msg=what + " q")
    np.testing.assert_allclose(g_obs[J:2 * J], o_obs[J:2 * J], atol=loosen * 3e-3 * max(1.0, np.abs(o_obs[J:2 * J]).max()),
                               rtol=0, err_msg=what + " qd")
    # motor torque: a joint saturated in the oracle (3e5 N m, trex_robot.py:260) must be saturated with the same sign;
    # the others are compared on the scale of the largest UNsaturated torque (a saturated neighbour must not hide
    # an error of hundreds of N m)
    gt, ot = g_obs[2 * J:], o_obs[2 * J:]
    sat = np.abs(ot) >= 0.999 * max_force
    assert np.all(np.abs(gt[sat]) >= 0.999 * max_force) and np.all(np.sign(gt[sat]) == np.sign(ot[sat])), what + " saturated tau"
    if (~sat).any():
        tscale = np.abs(ot[~sat]).max()
        np.testing.assert_allclose(gt[~sat], ot[~sat], atol=3e-3 * tscale + tau_floor + tau_extra, rtol=0, err_msg=what + " tau")
    if g_rew is not None:
        # reward = -lift - drift - w_e sum|qd tau| (trex_env.py:186-192): 2e-3 relative on the whole, plus what the
        # stated qd / tau tolerances allow in the energy term (w_e = 0.005, the default of every test here)
        qd_tol = 3e-3 * max(1.0, np.abs(o_obs[J:2 * J]).max())
        tau_tol = np.where(sat, 1e-3 * max_force, 3e-3 * (np.abs(ot[~sat]).max() if (~sat).any() else 0.0) + tau_floor + tau_extra)
        energy_tol = 0.005 * np.sum(np.abs(o_obs[J:2 * J]) * tau_tol + np.abs(ot) * qd_tol)
        assert abs(g_rew - o_rew) <= 2e-3 * abs(o_rew) + 1e-3 + 0.1 * energy_tol, (what, g_rew, o_rew)


def oracle_wrench(orc, model, state, action, mass_scale=None, friction=None, oracle_state=None, counts=None):
    """One env-step restated on the oracle: the clipped action as the joint targets, motors on, `substeps` substeps; per
    substep the contact points (body, lambda = (normal, x, y) - the oracle's row order - and world point) with the body COMs
    of the pose the rows were built at (body_poses BEFORE the substep + R com). Returns the mean wrench [nb, 6] and the touched
    bodies. oracle_state: step THAT oracle state on, in place (state, mass_scale and friction are then not used).
    counts: a list that receives the number of contact points of every substep."""
    oo, nb = model["obs_order"], model["nb"]
    s = oracle_state
    if s is None:
        s = orc.new_state()
        orc.set_state(s, np.asarray(state, np.float64))
        if mass_scale is not None or friction is not None:
            orc.set_domain(s, None if mass_scale is None else mass_scale.astype(np.float64), friction)
    orc.set_motors_on(s, 1)
    target = np.clip(np.asarray(action, np.float64), model["q_lower"][oo], model["q_upper"][oo])
    n_sub, dt = int(orc.params["substeps"]), orc.params["dt"]
    W = np.zeros((nb, 6))
    touched = set()
    for _ in range(n_sub):
        pos, rot = orc.body_poses(s)
        com = pos + np.einsum("bij,bj->bi", rot, model["com"])
        orc.substep(s, target)
        body, lam, pt, _ = orc.contacts(s)
        if counts is not None:
            counts.append(len(body))
        for b, l, p in zip(body, lam, pt):
            f = np.array([l[1], l[2], l[0]])
            W[b, :3] += f
            W[b, 3:] += np.cross(p - com[b], f)
            touched.add(int(b))
    return W / (n_sub * dt), touched
