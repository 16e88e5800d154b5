"""numpy f64 restatement of the dynamics queries (include/trex_batch.h, "dynamics queries"), built from the compiled model
arrays of oracle/trex_model.py: dense mass matrix, inverse dynamics / bias force by RNEA, point Jacobian, centroidal sums.

The GPU tests compare against this element by element; tests/test_dynamics_ref.py ties it to the oracle (M^-1, forward
dynamics, energy, body poses). Written from the textbook definitions and not from the kernel: the mass matrix is summed from
per-body Jacobians (M = sum m Jv^T Jv + Jw^T Ic Jw), which neither the kernel (composite bodies) nor the oracle (ABA) does.

Every function takes dtype (default float64). dtype=np.float32 is the f32 run: the same textbook formulas with every array and
every intermediate in float32 - no care over cancellation, world positions kept as they are -, whose deviation from the f64 run
is what tests/dynamics_model_cases.py sets its bounds from. The f64 results do not depend on the argument's existence.

Generalised velocity, D = 6 + J: base linear v(3) and angular w(3), world axes, then qd in observation order - the velocity
part of the state vector [pos 3, quat xyzw 4, v 3, w 3, q J, qd J]. Forces are the duals (base torque about the base origin).
"""
import numpy as np


def quat_to_mat(q, dtype=np.float64):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype)


def axis_angle_mat(a, q, dtype=np.float64):
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype)
    return np.cos(q) * np.eye(3, dtype=dtype) + np.sin(q) * K + (1 - np.cos(q)) * np.outer(a, a)


def perm_to_oracle(model):
    """index array p with x_oracle = x[p]: the oracle orders [w, v, joints in body order 1..nb-1]."""
    slot = np.empty(model["nb"], int)
    slot[model["obs_order"]] = np.arange(model["nb"] - 1)
    return np.concatenate([[3, 4, 5, 0, 1, 2], 6 + slot[1:]])


class Kin:
    """pose of every body for one state: R[b] world <- body, p[b] body origin in the world, a[b] joint axis (world), and the
    joint values in body order. dtype: the type of every array and every intermediate (module docstring)."""

    def __init__(self, model, state, mass_scale=None, dtype=np.float64):
        nb = model["nb"]
        J = nb - 1
        dt = self.dtype = np.dtype(dtype).type
        state = np.asarray(state, dt)
        fm = {key: np.asarray(model[key], dt) for key in ("joint_rot", "joint_axis", "joint_pos", "mass", "com", "inertia")}
        self.model, self.nb, self.D = model, nb, 6 + J
        self.slot = np.full(nb, -1)
        self.slot[model["obs_order"]] = np.arange(J)
        self.pos, self.quat, self.v, self.w = state[0:3], state[3:7], state[7:10], state[10:13]
        self.q, self.qd = np.zeros(nb, dt), np.zeros(nb, dt)
        self.q[model["obs_order"]] = state[13:13 + J]
        self.qd[model["obs_order"]] = state[13 + J:13 + 2 * J]
        self.R, self.p, self.a = np.zeros((nb, 3, 3), dt), np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)
        self.R[0], self.p[0] = quat_to_mat(self.quat, dt), self.pos
        for i in range(1, nb):
            pa = model["parent"][i]
            assert pa < i
            self.R[i] = self.R[pa] @ fm["joint_rot"][i].reshape(3, 3) @ axis_angle_mat(fm["joint_axis"][i], self.q[i], dt)
            self.p[i] = self.p[pa] + self.R[pa] @ fm["joint_pos"][i]
            self.a[i] = self.R[i] @ fm["joint_axis"][i]
        ms = np.ones(nb, dt) if mass_scale is None else np.asarray(mass_scale, dt)
        self.mass = fm["mass"] * ms
        self.c = self.p + np.einsum("bij,bj->bi", self.R, fm["com"])
        ib = fm["inertia"]
        Ib = np.stack([np.array([[x[0], x[1], x[2]], [x[1], x[3], x[4]], [x[2], x[4], x[5]]], dt) for x in ib])
        self.Ic = ms[:, None, None] * np.einsum("bij,bjk,blk->bil", self.R, Ib, self.R)

    def chain(self, b):
        out = []
        while b > 0:
            out.append(b)
            b = self.model["parent"][b]
        return out

    def point_jacobian(self, body, point_world):
        """[6, D]: linear velocity of the world point carried by `body`, angular velocity of `body`."""
        Jm = np.zeros((6, self.D), self.dtype)
        Jm[0:3, 0:3] = np.eye(3, dtype=self.dtype)
        Jm[3:6, 3:6] = np.eye(3, dtype=self.dtype)
        for l in range(3):
            Jm[0:3, 3 + l] = np.cross(np.eye(3, dtype=self.dtype)[l], point_world - self.pos)
        for i in self.chain(body):
            Jm[0:3, 6 + self.slot[i]] = np.cross(self.a[i], point_world - self.p[i])
            Jm[3:6, 6 + self.slot[i]] = self.a[i]
        return Jm


def mass_matrix(model, state, mass_scale=None, dtype=np.float64):
    k = Kin(model, state, mass_scale, dtype)
    M = np.zeros((k.D, k.D), k.dtype)
    for b in range(k.nb):
        Jb = k.point_jacobian(b, k.c[b])
        M += k.mass[b] * Jb[0:3].T @ Jb[0:3] + Jb[3:6].T @ k.Ic[b] @ Jb[3:6]
    return M


def inverse_dynamics(model, state, accel=None, mass_scale=None, gravity=9.81, dtype=np.float64):
    """M a + h by the recursive Newton-Euler algorithm in classical (point) accelerations; accel None = zeros: h."""
    k = Kin(model, state, mass_scale, dtype)
    dt = k.dtype
    nb, par = k.nb, model["parent"]
    acc = np.zeros(k.D, dt) if accel is None else np.asarray(accel, dt)
    w, al = np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)
    vo, ao = np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)
    w[0], vo[0], ao[0], al[0] = k.w, k.v, acc[0:3] + np.array([0, 0, gravity], dt), acc[3:6]
    for i in range(1, nb):
        pa = par[i]
        d = k.p[i] - k.p[pa]
        qdd = acc[6 + k.slot[i]]
        w[i] = w[pa] + k.a[i] * k.qd[i]
        al[i] = al[pa] + k.a[i] * qdd + np.cross(w[pa], k.a[i]) * k.qd[i]
        vo[i] = vo[pa] + np.cross(w[pa], d)
        ao[i] = ao[pa] + np.cross(al[pa], d) + np.cross(w[pa], np.cross(w[pa], d))
    F, N = np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)  # subtree force, subtree moment about the WORLD origin
    for b in range(nb):
        cb = k.c[b] - k.p[b]
        ac = ao[b] + np.cross(al[b], cb) + np.cross(w[b], np.cross(w[b], cb))
        F[b] = k.mass[b] * ac
        N[b] = k.Ic[b] @ al[b] + np.cross(w[b], k.Ic[b] @ w[b]) + np.cross(k.c[b], F[b])
    out = np.zeros(k.D, dt)
    for b in range(nb - 1, 0, -1):
        out[6 + k.slot[b]] = k.a[b] @ (N[b] - np.cross(k.p[b], F[b]))
        F[par[b]] += F[b]
        N[par[b]] += N[b]
    out[0:3] = F[0]
    out[3:6] = N[0] - np.cross(k.pos, F[0])
    return out


def jacobian(model, state, link, local_xyz=(0.0, 0.0, 0.0), dtype=np.float64, kin=None):
    """[6, D] for the point local_xyz of URDF link `link` (link frame = body frame o link_tf). kin: a Kin of this model, state and
    dtype made before (many links at one state)."""
    k = Kin(model, state, None, dtype) if kin is None else kin
    body = int(model["link_body"][link])
    tf = np.asarray(model["link_tf"][link], k.dtype)
    pt = tf[:9].reshape(3, 3) @ np.asarray(local_xyz, k.dtype) + tf[9:12]
    return k.point_jacobian(body, k.p[body] + k.R[body] @ pt)


def point_velocity(model, state, link, local_xyz=(0.0, 0.0, 0.0), dtype=np.float64, kin=None):
    """[3] world linear velocity of the point local_xyz of URDF link `link`, by the outward recursion over the bodies (not through
    the Jacobian): v_origin(child) = v_origin(parent) + w(parent) x (p_child - p_parent), w(child) = w(parent) + a qd. kin: as
    for jacobian (the recursion is then run once per Kin)."""
    k = Kin(model, state, None, dtype) if kin is None else kin
    if not hasattr(k, "body_vel"):
        par = model["parent"]
        w, vo = np.zeros((k.nb, 3), k.dtype), np.zeros((k.nb, 3), k.dtype)
        w[0], vo[0] = k.w, k.v
        for i in range(1, k.nb):
            w[i] = w[par[i]] + k.a[i] * k.qd[i]
            vo[i] = vo[par[i]] + np.cross(w[par[i]], k.p[i] - k.p[par[i]])
        k.body_vel = (w, vo)
    w, vo = k.body_vel
    body = int(model["link_body"][link])
    tf = np.asarray(model["link_tf"][link], k.dtype)
    pt = tf[:9].reshape(3, 3) @ np.asarray(local_xyz, k.dtype) + tf[9:12]
    return vo[body] + np.cross(w[body], k.R[body] @ pt)


def centroidal(model, state, mass_scale=None, gravity=9.81, dtype=np.float64):
    """the 16 values of trex_batch_centroidal"""
    k = Kin(model, state, mass_scale, dtype)
    gv = np.concatenate([k.v, k.w, k.qd[model["obs_order"]]])
    mt = k.mass.sum()
    com = (k.mass[:, None] * k.c).sum(0) / mt
    p, L, ke = np.zeros(3, k.dtype), np.zeros(3, k.dtype), 0.0
    for b in range(k.nb):
        Jb = k.point_jacobian(b, k.c[b])
        vc, wb = Jb[0:3] @ gv, Jb[3:6] @ gv
        p += k.mass[b] * vc
        L += k.Ic[b] @ wb + k.mass[b] * np.cross(k.c[b] - com, vc)
        ke += 0.5 * k.mass[b] * vc @ vc + 0.5 * wb @ k.Ic[b] @ wb
    pe = gravity * (k.mass * k.c[:, 2]).sum()
    return np.concatenate([com, p / mt, p, L, np.array([ke, pe, mt, 0.0], k.dtype)])


def random_tau(model, state, mass_scale, rng, alpha=10.0, gravity=9.81, with_accel=False):
    """random joint torques that move EVERY joint gently: joint accelerations qdd drawn uniformly in [-alpha, alpha] rad/s^2, the
    base acceleration that a free-floating base then takes (zero base force: a_b = -M_bb^-1 (M_bj qdd + h_b)), and tau the joint
    rows of M a + h. Forward dynamics of tau returns exactly these accelerations, so no light link - toes, tail tip - is thrown
    at 1e3 .. 1e5 rad/s^2, as it is when torques are drawn joint by joint without regard to the coupling.
    with_accel: also the accelerations [base linear, base angular, qdd]."""
    h = inverse_dynamics(model, state, None, mass_scale, gravity)
    M = mass_matrix(model, state, mass_scale)
    qdd = rng.uniform(-alpha, alpha, len(h) - 6)
    ab = -np.linalg.solve(M[:6, :6], M[:6, 6:] @ qdd + h[:6])
    tau = M[6:, :6] @ ab + M[6:, 6:] @ qdd + h[6:]
    return (tau, np.concatenate([ab, qdd])) if with_accel else tau


def block_dev(got, want, base_scale, joint_scale):
    """largest deviation of a generalised force, the base rows (N, N m about the base origin) over base_scale and the joint rows
    (N m) over joint_scale: the two blocks carry different units and sizes"""
    d = np.abs(np.asarray(got, np.float64) - want)
    return max(d[:6].max() / base_scale, d[6:].max() / joint_scale)


def random_states(model, count, seed=7):
    """airborne states: joint angles inside the limits, a random base orientation, non-zero base and joint velocities; the last
    two carry a per-body mass scale in [0.5, 2] (None for the others)."""
    rng = np.random.default_rng(seed)
    oo = model["obs_order"]
    lo, hi = model["q_lower"][oo], model["q_upper"][oo]
    states, scales = [], []
    for i in range(count):
        quat = rng.normal(size=4)
        quat /= np.linalg.norm(quat)
        s = np.concatenate([rng.uniform(-1, 1, 2), [rng.uniform(4, 6)], quat, rng.normal(size=3), 1.5 * rng.normal(size=3),
                            rng.uniform(lo, hi), 2.0 * rng.normal(size=len(oo))])
        states.append(s.astype(np.float32).astype(np.float64))     # exactly representable: the GPU gets the same state
        scales.append(rng.uniform(0.5, 2.0, model["nb"]).astype(np.float32).astype(np.float64) if i >= count - 2 else None)
    return states, scales
