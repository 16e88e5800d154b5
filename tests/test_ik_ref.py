"""Pins tests/ik_ref.py - the f64 restatement the GPU inverse kinematics are compared with - without a GPU: its kinematics are
link_state_ref.link_state's and its matrix A the joint columns of dynamics_ref.jacobian; -A is the derivative of the error with
respect to the joint angles (central differences); the BASE-frame solve is the WORLD-frame solve of the transformed targets;
joints outside the mask never move; results respect the joint limits. On the T-rex and on the depth-6 / oblique-axis generated
models. It also checks that the library and the Python surface carry the query at all.

Central differences: h = 1e-6 rad, tolerance 1e-6 x max(1, the largest entry of A) - truncation h^2 x third derivative / 6 ~ 1e-12,
round-off ~ 1e-16 / h = 1e-10. The position rows hold at any target. The orientation error 2 sign(w) vec(q_target o q_link^-1) is
the rotation vector to first order only, so its derivative is -a_j exactly where the error vanishes: the orientation targets of
this check are the links' orientations at the point of differentiation (the position targets are arbitrary)."""
import numpy as np
import pytest

import dynamics_ref as R
import ik_cases as C
import ik_ref as IK
import link_state_ref as L
import synthetic_models as sm

H = 1e-6
FD_TOL = 1e-6


@pytest.fixture(scope="module")
def suites(model, tmp_path_factory):
    """name -> (model dict, [state f64]): T-rex, deep_chain, bushy, at airborne states with joint angles inside the limits"""
    out = dict(trex=(model, R.random_states(model, 3)[0]))
    for n in ("deep_chain", "bushy"):
        _, _, om = sm.compile_both(n, tmp_path_factory.mktemp(n))
        out[n] = (om, R.random_states(om, 3, seed=31)[0])
    assert out["deep_chain"][0]["depth"].max() == 6 and out["bushy"][0]["depth"].max() == 6
    return out


def full_form(om):
    """head, two toes (or two other branches) and the deepest link, every one with position and orientation: M = 24"""
    p = C.pick(om)
    links = [p["head"], p["toe_a"], p["toe_b"], p["deepest"]]
    return links, [(0.0, 0.0, 0.0), C.OFFSET, (0.0, 0.0, 0.0), C.OFFSET], [3, 3, 3, 3]


@pytest.mark.parametrize("name", ["trex", "deep_chain", "bushy"])
def test_kinematics_are_link_state_and_jacobian(name, suites):
    om, states = suites[name]
    links, pts, modes = full_form(om)
    for s in states:
        k, p, Rl, body = IK.kinematics(om, s, links, pts)
        r = L.link_state(om, s, links, pts)
        assert np.array_equal(p, r["position"]) and np.array_equal(Rl, r["rotation"])
        pT, qT = r["position"] + 0.1, r["orientation"]
        _, A, _, _ = IK.error(om, s, links, pts, modes, pT, qT)
        want = np.concatenate([R.jacobian(om, s, l, x)[:, 6:] for l, x in zip(links, pts)])
        assert A.shape == (24, om["nb"] - 1) and np.abs(A - want).max() <= 1e-14 * max(1.0, np.abs(want).max())
        assert np.array_equal(A == 0, want == 0)


@pytest.mark.parametrize("name", ["trex", "deep_chain", "bushy"])
def test_minus_a_is_the_derivative_of_the_error(name, suites):
    om, states = suites[name]
    links, pts, modes = full_form(om)
    J = om["nb"] - 1
    rng = np.random.default_rng(11)
    for s in states:
        r = L.link_state(om, s, links, pts)
        pT, qT = r["position"] + rng.uniform(-0.5, 0.5, (4, 3)), r["orientation"]
        q = s[13:13 + J]
        _, A, _, _ = IK.error(om, s, links, pts, modes, pT, qT)
        fd = np.zeros_like(A)
        for j in range(J):
            dq = np.zeros(J)
            dq[j] = H
            ep = IK.error(om, IK.with_q(om, s, q + dq), links, pts, modes, pT, qT, jacobian=False)[0]
            em = IK.error(om, IK.with_q(om, s, q - dq), links, pts, modes, pT, qT, jacobian=False)[0]
            fd[:, j] = (ep - em) / (2 * H)
        assert np.abs(A).max() > 0.1
        assert np.abs(fd + A).max() <= FD_TOL * max(1.0, np.abs(A).max()), (name, np.abs(fd + A).max())


@pytest.mark.parametrize("name", ["trex", "bushy"])
def test_base_frame_solve_is_the_world_frame_solve_of_the_transformed_targets(name, suites):
    om, states = suites[name]
    links, pts, modes = full_form(om)
    J = om["nb"] - 1
    lo, hi = IK.limits(om)
    rng = np.random.default_rng(12)
    for s in states:
        s = s.copy()
        s[3:7] /= np.linalg.norm(s[3:7])     # (an f32-rounded quaternion is a unit one to 1e-7 only, and so far R0 R0^T is the identity)
        q_star = np.clip(s[13:13 + J] + 0.2 * rng.uniform(-1, 1, J), lo, hi)
        sq = IK.with_q(om, s, q_star)
        tw = L.pose_array(L.link_state(om, sq, links, pts))
        tb = L.pose_array(L.link_state(om, sq, links, pts, axes="base"))
        a = IK.solve(om, s, links, pts, modes, tw, "world", iterations=5)
        b = IK.solve(om, s, links, pts, modes, tb, "base", iterations=5)
        assert np.abs(a["q"] - b["q"]).max() < 1e-9 and abs(a["initial_error"] - b["initial_error"]) < 1e-9
        assert a["norms"][-1] < 0.5 * a["norms"][0]


def test_masked_joints_never_move_and_limits_hold(model):
    lo, hi = IK.limits(model)
    for form in C.forms(model):
        for c in C.reachable(model, form, 3):
            start = c.q_start + np.where(np.arange(len(lo)) % 5 == 0, 10.0, 0.0)       # every fifth joint starts far outside
            r = IK.solve(model, c.state, form.links, form.points, form.modes, c.targets["world"], q_init=start,
                         joints=form.joints, iterations=6)
            move = IK.joint_mask(model, form.joints)
            assert np.array_equal(r["q"][~move], start[~move])
            assert (r["q"][move] >= lo[move]).all() and (r["q"][move] <= hi[move]).all()
            assert r["iterations"] == 6 and len(r["norms"]) == 7


def test_rank_deficient_task_and_early_stop(model):
    form = [f for f in C.forms(model) if f.name == "same_body"][0]
    c = C.reachable(model, form, 1)[0]
    # a pivot that is not positive becomes lambda2: a Gram matrix of rank 5 with a pivot rounded below zero still solves
    G = np.ones((3, 3))
    G[2, 2] = 0.999                            # its pivot: 0.999 - 1 / 1.0001 - ... < 0
    x = IK.cholesky_solve(G + np.diag([1e-4, 1e-4, 0.0]), np.ones(3), 1e-4)
    assert np.isfinite(x).all()
    r = IK.solve(model, c.state, form.links, form.points, form.modes, c.targets["world"], iterations=30, tol=(1e-3, 1e-3))
    assert r["iterations"] < 30 and r["position_error"] <= 1e-3


def test_library_and_python_surface_carry_the_query():
    from trex_gym import _capi, trex_env, vec_env
    assert "trex_batch_inverse_kinematics" in _capi.SYMBOLS and hasattr(_capi.lib, "trex_batch_inverse_kinematics")
    assert callable(_capi.Batch.inverse_kinematics)
    assert callable(vec_env.TrexVecEnv.inverse_kinematics) and callable(vec_env.TrexVecEnv.joint_targets_to_actions)
    assert callable(trex_env.TrexBulletEnv.calculateInverseKinematics) and callable(trex_env.TrexBulletEnv.calculateInverseKinematics2)
    assert vec_env.IkInfo._fields == ("position_error", "orientation_error", "iterations", "initial_error")
