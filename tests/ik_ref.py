"""numpy f64 restatement of the inverse kinematics query (include/trex_batch.h, "inverse kinematics"), one env at a time: damped
least squares on the stacked position / orientation errors of a few task points, exactly the algorithm the header fixes.

Built on dynamics_ref.Kin: the task points and link orientations are those of link_state_ref.link_state, the matrix A the joint
columns of dynamics_ref.jacobian - one Kin per iteration serves all of them, and tests/test_ik_ref.py pins that this is the same
as calling the two functions (and that -A is the derivative of the error). The GPU tests compare trex_batch_inverse_kinematics
against a single iteration of this element by element, and judge its convergence with link_state_ref alone.

Conventions: the state vector [pos 3, quat xyzw 4, v 3, w 3, q J, qd J]; q, masks and results in observation order; a target row is
xyz + quaternion xyzw; modes 1 = position, 2 = orientation, 3 = both; task rows in probe order, a probe's position rows first."""
import numpy as np

import dynamics_ref as R
import link_state_ref as L

DEFAULTS = dict(iterations=20, damping=0.01, gain=0.1, max_step=0.2, tol=(0.0, 0.0))


def quat_mul(a, b):
    """a o b, xyzw"""
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def with_q(model, state, q):
    """the state with the joint angles q (observation order) in place of its own"""
    J = model["nb"] - 1
    s = np.asarray(state, np.float64).copy()
    s[13:13 + J] = q
    return s


def limits(model):
    oo = model["obs_order"]
    return np.asarray(model["q_lower"], np.float64)[oo], np.asarray(model["q_upper"], np.float64)[oo]


def base_frame(model, state):
    """(R0, p0): URDF link 0's frame in the world; it belongs to the base body, so the joint angles do not move it"""
    assert int(model["link_body"][0]) == 0
    b0 = L.link_state(model, state, [0])
    return b0["rotation"][0], b0["position"][0]


def world_targets(model, state, targets, frame="world"):
    """targets [K, 7] in `frame` -> (p [K, 3], quat [K, 4]) in the world, the quaternions normalised"""
    t = np.asarray(targets, np.float64).reshape(-1, 7)
    with np.errstate(invalid="ignore"):
        qn = t[:, 3:] / np.linalg.norm(t[:, 3:], axis=1, keepdims=True)
    if frame == "world":
        return t[:, :3].copy(), qn
    assert frame == "base"
    R0, p0 = base_frame(model, state)
    rot = np.stack([R0 @ R.quat_to_mat(q) for q in qn])
    with np.errstate(invalid="ignore"):
        return p0 + t[:, :3] @ R0.T, L.mats_to_quats(rot)


def task_rows(modes):
    return int(sum(3 * (int(m) & 1) + 3 * (int(m) >> 1 & 1) for m in modes))


def kinematics(model, state, links, points):
    """(Kin, p [K, 3] the task points, Rl [K, 3, 3] the link orientations, body [K]) at `state`: link_state_ref.link_state's"""
    links = np.asarray(links, int).reshape(-1)
    K = len(links)
    pts = np.zeros((K, 3)) if points is None else np.asarray(points, np.float64).reshape(K, 3)
    k = R.Kin(model, state)
    body = np.asarray(model["link_body"], int)[links]
    tf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)[links]
    tfR = tf[:, :9].reshape(K, 3, 3)
    Rb = k.R[body]
    p = k.p[body] + np.einsum("kij,kj->ki", Rb, np.einsum("kij,kj->ki", tfR, pts) + tf[:, 9:12])
    return k, p, Rb @ tfR, body


def error(model, state, links, points, modes, pT, qT, move=None, jacobian=True):
    """At `state`: e [M], A [M, J] (None unless `jacobian`; the columns of joints outside `move` zeroed), the residuals
    (largest |p_target - p|, largest orientation angle 2 asin(min(1, |vec|)))"""
    J = model["nb"] - 1
    k, p, Rl, body = kinematics(model, state, links, points)
    ql = L.mats_to_quats(Rl)
    e, rows, rp, ro = [], [], 0.0, 0.0
    for i, m in enumerate(modes):
        Jm = k.point_jacobian(body[i], p[i])[:, 6:] if jacobian else None
        if int(m) & 1:
            d = pT[i] - p[i]
            e.append(d)
            rp = max(rp, np.linalg.norm(d)) if np.isfinite(d).all() else np.nan
            if jacobian:
                rows.append(Jm[0:3])
        if int(m) & 2:
            qe = quat_mul(qT[i], ql[i] * [-1, -1, -1, 1])
            e.append(2.0 * (-1.0 if qe[3] < 0 else 1.0) * qe[:3])
            vn = np.linalg.norm(qe[:3])
            ro = max(ro, 2.0 * np.arcsin(min(1.0, vn))) if np.isfinite(vn) else np.nan
            if jacobian:
                rows.append(Jm[3:6])
    e = np.concatenate(e)
    A = None
    if jacobian:
        A = np.concatenate(rows)
        if move is not None:
            A = A * np.asarray(move, bool)[None, :]
    return e, A, rp, ro


def cholesky_solve(G, rhs, lambda2):
    """x with G x = rhs, G = L L^T column by column; a pivot that is not positive is replaced by lambda2"""
    n = len(rhs)
    Lm = np.zeros((n, n))
    for k in range(n):
        s = G[k:, k] - Lm[k:, :k] @ Lm[k, :k]
        piv = s[0] if s[0] > 0 else lambda2
        d = np.sqrt(piv)
        Lm[k, k] = d
        Lm[k + 1:, k] = s[1:] / d
    y = np.zeros(n)
    for k in range(n):
        y[k] = (rhs[k] - Lm[k, :k] @ y[:k]) / Lm[k, k]
    x = np.zeros(n)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - Lm[k + 1:, k] @ x[k + 1:]) / Lm[k, k]
    return x


def step(e, A, q, move, lo, hi, damping=0.01, gain=0.1, max_step=0.2):
    """one update of the iterate q from the error e and the matrix A at q"""
    lambda2 = damping * damping + gain * (e @ e)
    x = cholesky_solve(A @ A.T + lambda2 * np.eye(len(e)), e, lambda2)
    dq = np.where(move, A.T @ x, 0.0)
    big = np.abs(dq).max()
    if big > max_step:
        dq = dq * (max_step / big)
    return np.where(move, np.clip(q + dq, lo, hi), q)


def joint_mask(model, joints):
    """bool [J]: `joints` = None (all), or observation indices"""
    J = model["nb"] - 1
    move = np.ones(J, bool) if joints is None else np.zeros(J, bool)
    if joints is not None:
        move[np.asarray(joints, int)] = True
    return move


def solve(model, state, links, points, modes, targets, frame="world", q_init=None, joints=None, iterations=20, damping=0.01,
          gain=0.1, max_step=0.2, tol=(0.0, 0.0)):
    """The whole query for one env: dict(q [J], position_error, orientation_error, iterations, initial_error, norms: |e| at the
    iterate of every pass of kinematics, the last one at q). The base pose is the state's."""
    J = model["nb"] - 1
    state = np.asarray(state, np.float64)
    lo, hi = limits(model)
    move = joint_mask(model, joints)
    q = np.array(state[13:13 + J] if q_init is None else q_init, np.float64)
    q = np.where(move, np.clip(q, lo, hi), q)
    pT, qT = world_targets(model, state, targets, frame)
    it, norms = 0, []
    while True:
        last = it >= iterations
        e, A, rp, ro = error(model, with_q(model, state, q), links, points, modes, pT, qT, move, jacobian=not last)
        norms.append(float(np.sqrt(e @ e)))
        if last or ((tol[0] > 0 or tol[1] > 0) and rp <= tol[0] and ro <= tol[1]):
            break
        q = step(e, A, q, move, lo, hi, damping, gain, max_step)
        it += 1
    return dict(q=q, position_error=rp, orientation_error=ro, iterations=it, initial_error=norms[0], norms=np.array(norms))


def residuals(model, state, q, links, points, modes, targets, frame="world"):
    """(largest position error, largest orientation error, |e|) of the joint angles q, by forward kinematics alone"""
    pT, qT = world_targets(model, state, targets, frame)
    e, _, rp, ro = error(model, with_q(model, state, q), links, points, modes, pT, qT, jacobian=False)
    return rp, ro, float(np.sqrt(e @ e))
