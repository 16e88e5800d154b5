"""numpy f64 restatement of the link kinematics query (include/trex_batch.h, "link kinematics"): pose, velocity and classical
acceleration of points fixed in URDF links, the axes they are expressed in, and the accelerometer's specific force.

Built on dynamics_ref.Kin and on the recursion of dynamics_ref.inverse_dynamics (classical point accelerations, parent to child);
tests/test_link_state_ref.py pins it - the velocity to dynamics_ref.jacobian, the acceleration to central differences of its own
velocity. The GPU tests compare trex_batch_link_state against it element by element.

Conventions of the dynamics queries: generalised velocity / acceleration [D = 6 + J] = base linear (of the base origin), base
angular, world axes, then the joints in observation order; the state vector [pos 3, quat xyzw 4, v 3, w 3, q J, qd J]."""
import numpy as np

import dynamics_ref as R

AXES = ("world", "link", "base")


def mat_to_quat(m):
    """rotation matrix -> quaternion xyzw, w >= 0"""
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    elif m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
        s = np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2
        q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
    elif m[1, 1] >= m[2, 2]:
        s = np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2
        q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
    else:
        s = np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2
        q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
    q = np.array(q)
    return -q if q[3] < 0 else q


def mats_to_quats(m):
    """mat_to_quat over [K, 3, 3] at once: the four branches computed for every matrix, the valid one taken"""
    m = np.asarray(m, np.float64)
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        s0, s1 = np.sqrt(m00 + m11 + m22 + 1.0) * 2, np.sqrt(1.0 + m00 - m11 - m22) * 2
        s2, s3 = np.sqrt(1.0 + m11 - m00 - m22) * 2, np.sqrt(1.0 + m22 - m00 - m11) * 2
        c0 = np.stack([(m[:, 2, 1] - m[:, 1, 2]) / s0, (m[:, 0, 2] - m[:, 2, 0]) / s0, (m[:, 1, 0] - m[:, 0, 1]) / s0, 0.25 * s0], 1)
        c1 = np.stack([0.25 * s1, (m[:, 0, 1] + m[:, 1, 0]) / s1, (m[:, 0, 2] + m[:, 2, 0]) / s1, (m[:, 2, 1] - m[:, 1, 2]) / s1], 1)
        c2 = np.stack([(m[:, 0, 1] + m[:, 1, 0]) / s2, 0.25 * s2, (m[:, 1, 2] + m[:, 2, 1]) / s2, (m[:, 0, 2] - m[:, 2, 0]) / s2], 1)
        c3 = np.stack([(m[:, 0, 2] + m[:, 2, 0]) / s3, (m[:, 1, 2] + m[:, 2, 1]) / s3, 0.25 * s3, (m[:, 1, 0] - m[:, 0, 1]) / s3], 1)
    b0 = m00 + m11 + m22 > 0
    b1 = ~b0 & (m00 >= m11) & (m00 >= m22)
    b2 = ~b0 & ~b1 & (m11 >= m22)
    q = np.where(b0[:, None], c0, np.where(b1[:, None], c1, np.where(b2[:, None], c2, c3)))
    return np.where(q[:, 3:] < 0, -q, q)


class BodyMotion:
    """per body of one state: pose (Kin), angular velocity w, velocity vo of the body origin, and - at the generalised
    accelerations accel [D] (None: zeros) - angular acceleration al and classical acceleration ao of the origin (NO gravity term)"""

    def __init__(self, model, state, accel=None):
        k = self.k = R.Kin(model, state)
        nb, par = k.nb, model["parent"]
        acc = np.zeros(k.D) if accel is None else np.asarray(accel, np.float64)
        self.w, self.al = np.zeros((nb, 3)), np.zeros((nb, 3))
        self.vo, self.ao = np.zeros((nb, 3)), np.zeros((nb, 3))
        w, al, vo, ao = self.w, self.al, self.vo, self.ao
        w[0], vo[0], ao[0], al[0] = k.w, k.v, acc[0:3], acc[3:6]
        for i in range(1, nb):
            pa = par[i]
            d = k.p[i] - k.p[pa]
            qdd = acc[6 + k.slot[i]]
            w[i] = w[pa] + k.a[i] * k.qd[i]
            al[i] = al[pa] + k.a[i] * qdd + np.cross(w[pa], k.a[i]) * k.qd[i]
            vo[i] = vo[pa] + np.cross(w[pa], d)
            ao[i] = ao[pa] + np.cross(al[pa], d) + np.cross(w[pa], np.cross(w[pa], d))


def link_state(model, state, links, points=None, accel=None, axes="world", proper=False, gravity=9.81):
    """The probes (links[k], points[k] in the link frame; None: the link origins) at one state -> dict of arrays over the K probes:
    position [K, 3], rotation [K, 3, 3] (world <- link; with axes "base": base <- link, the position in the base frame too),
    orientation [K, 4] (its quaternion xyzw, w >= 0), linear_velocity, angular_velocity, linear_acceleration,
    angular_acceleration [K, 3]: world quantities expressed in `axes`; proper: + g z (world) on the linear acceleration."""
    assert axes in AXES
    links = np.asarray(links, int).reshape(-1)
    K = len(links)
    pts = np.zeros((K, 3)) if points is None else np.asarray(points, np.float64).reshape(K, 3)
    bm = BodyMotion(model, state, accel)
    k = bm.k
    body = np.asarray(model["link_body"], int)[links]
    tf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)[links]
    tfR = tf[:, :9].reshape(K, 3, 3)
    Rb = k.R[body]
    Rl = Rb @ tfR
    d = np.einsum("kij,kj->ki", Rb, np.einsum("kij,kj->ki", tfR, pts) + tf[:, 9:12])    # body origin -> point, world axes
    pos = k.p[body] + d
    w, al = bm.w[body], bm.al[body]
    lv = bm.vo[body] + np.cross(w, d)
    la = bm.ao[body] + np.cross(al, d) + np.cross(w, np.cross(w, d))
    if proper:
        la = la + np.array([0.0, 0.0, gravity])
    rot = Rl
    if axes == "world":
        A = np.broadcast_to(np.eye(3), (K, 3, 3))
    elif axes == "link":
        A = Rl
    else:
        b0 = int(model["link_body"][0])
        tf0 = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)[0]
        R0 = k.R[b0] @ tf0[:9].reshape(3, 3)
        p0 = k.p[b0] + k.R[b0] @ tf0[9:12]
        A = np.broadcast_to(R0, (K, 3, 3))
        pos = (pos - p0) @ R0          # rows: R0^T (p - p0)
        rot = R0.T @ Rl
    ex = lambda v: np.einsum("kji,kj->ki", A, v)     # A^T v
    return dict(position=pos, rotation=rot, orientation=mats_to_quats(rot),
                linear_velocity=ex(lv), angular_velocity=ex(w), linear_acceleration=ex(la), angular_acceleration=ex(al))


def pose_array(r):
    """[K, 7] as trex_batch_link_state writes it"""
    return np.concatenate([r["position"], r["orientation"]], 1)


def velocity_array(r):
    return np.concatenate([r["linear_velocity"], r["angular_velocity"]], 1)


def acceleration_array(r):
    return np.concatenate([r["linear_acceleration"], r["angular_acceleration"]], 1)


def advance(model, state, accel, h):
    """the state a time h later (h may be negative) under constant generalised accelerations, as the central difference of the
    tests needs it: position by v h, base orientation by the exponential map of w h (world axes), joints by qd h, velocities
    by h a"""
    s = np.asarray(state, np.float64).copy()
    J = model["nb"] - 1
    a = np.zeros(6 + J) if accel is None else np.asarray(accel, np.float64)
    s[0:3] += s[7:10] * h
    rv = s[10:13] * h
    th = np.linalg.norm(rv)
    dq = np.concatenate([rv * (0.5 if th < 1e-12 else np.sin(0.5 * th) / th), [np.cos(0.5 * th)]])
    x1, y1, z1, w1 = dq
    x2, y2, z2, w2 = s[3:7]
    s[3:7] = [w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
              w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]      # dq o q
    s[13:13 + J] += s[13 + J:13 + 2 * J] * h
    s[7:13] += h * a[:6]
    s[13 + J:13 + 2 * J] += h * a[6:]
    return s
