"""numpy f64 restatement of the joint force/torque sensor (include/trex_joint_wrench.h: trex_batch_joint_wrench), written from the
header's definition and not from the kernel: per-body Newton-Euler wrenches from dynamics_ref.Kin, summed over EXPLICIT subtree
sets with every moment referred directly to the joint origin - no inward recursion, no lever between a child and its parent, which
is how the kernel (and RNEA) gets there.

    f_i = sum_{b in S(i)} (m_b a_c,b - F_b)
    n_i = sum_{b in S(i)} [Ic_b al_b + w_b x Ic_b w_b - T_b + (c_b - r_i) x (m_b a_c,b - F_b)]

a_c the classical COM acceleration plus g z, (F_b, T_b) the world's wrench on body b at its COM (world axes), r_i the origin of
joint i = of body i's frame. World positions are kept as they are (z = 4 .. 6 m), also in the float32 run, whose deviation from
the f64 run sets the bounds of tests/joint_wrench_cases.py. tests/test_joint_wrench_ref.py ties it to dynamics_ref.inverse_dynamics
and to the closed form at rest, and qualifies it against the four MISTAKES below."""
import numpy as np

import dynamics_ref as R

# deliberate mistakes a bound has to tell from the right answer (tests/test_joint_wrench_ref.py)
MISTAKES = ("moment_about_com",     # every moment about the COM of body i instead of the joint origin r_i
            "wrench_lever_dropped",  # the body wrench's force enters f_i, its lever (c_b - r_i) x F_b does not enter n_i
            "wrench_sign",           # the world's wrench added instead of subtracted
            "child_not_shifted")     # a child's moment added to its parent's as it is, about the child's own origin


def subtree_sets(parent):
    """[nb] lists: the bodies of the subtree of body i, i itself included; from the parent array alone, no recursion"""
    nb = len(parent)
    sets = [[] for _ in range(nb)]
    for b in range(nb):
        a = b
        while True:
            sets[a].append(b)
            if a == 0:
                break
            a = int(parent[a])
    return sets


def body_motion(k, accel, gravity):
    """(w, al, a_c) [nb, 3] each: angular velocity and acceleration of every body, classical acceleration of its COM plus g z;
    outward over the bodies in index order (a parent comes before its children)"""
    dt, nb, par = k.dtype, k.nb, k.model["parent"]
    acc = np.zeros(k.D, dt) if accel is None else np.asarray(accel, dt)
    w, al, ao = np.zeros((nb, 3), dt), np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)
    w[0], al[0], ao[0] = k.w, acc[3:6], acc[0:3] + np.array([0, 0, gravity], dt)
    for i in range(1, nb):
        pa = int(par[i])
        d = k.p[i] - k.p[pa]
        w[i] = w[pa] + k.a[i] * k.qd[i]
        al[i] = al[pa] + k.a[i] * acc[6 + k.slot[i]] + np.cross(w[pa], k.a[i]) * k.qd[i]
        ao[i] = ao[pa] + np.cross(al[pa], d) + np.cross(w[pa], np.cross(w[pa], d))
    cb = k.c - k.p
    ac = ao + np.cross(al, cb) + np.cross(w, np.cross(w, cb))
    return w, al, ac


def joint_wrench(model, state, accel=None, wrench=None, mass_scale=None, gravity=9.81, axes="world", dtype=np.float64, mistake=None):
    """-> (rows [J, 6] in observation order, base [6]): force and moment about the joint origin of every joint, in world axes or -
    axes "link" - in the child body's; the whole tree's sums about the base origin, world axes. wrench [nb, 6] or None: the
    world's force at each body's COM and torque about it."""
    assert axes in ("world", "link") and (mistake is None or mistake in MISTAKES)
    k = R.Kin(model, state, mass_scale, dtype)
    dt, nb = k.dtype, k.nb
    w, al, ac = body_motion(k, accel, gravity)
    Wr = np.zeros((nb, 6), dt) if wrench is None else np.asarray(wrench, dt)
    sign = dt(1) if mistake == "wrench_sign" else dt(-1)
    inertial = k.mass[:, None] * ac                                            # m a_c
    fb = inertial + sign * Wr[:, 0:3]                                          # what body b needs through its joint: force ...
    nc = np.einsum("bij,bj->bi", k.Ic, al) + np.cross(w, np.einsum("bij,bj->bi", k.Ic, w)) + sign * Wr[:, 3:6]   # ... moment about its COM
    sets = subtree_sets(model["parent"])
    f, n = np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)
    for i in range(nb):
        ref = k.c[i] if mistake == "moment_about_com" else k.p[i]
        S = sets[i]
        f[i] = fb[S].sum(0)
        if mistake == "child_not_shifted":
            n[i] = (nc[S] + np.cross(k.c[S] - k.p[S], fb[S])).sum(0)
        elif mistake == "wrench_lever_dropped":
            n[i] = (nc[S] + np.cross(k.c[S] - ref, inertial[S])).sum(0)
        else:
            n[i] = (nc[S] + np.cross(k.c[S] - ref, fb[S])).sum(0)
    rows = np.zeros((nb - 1, 6), dt)
    for i in range(1, nb):
        Rt = k.R[i].T if axes == "link" else np.eye(3, dtype=dt)
        rows[k.slot[i]] = np.concatenate([Rt @ f[i], Rt @ n[i]])
    return rows, np.concatenate([f[0], n[0]])


def axis_component(model, state, rows_world):
    """[J] the component of every row's moment along its joint axis (rows in WORLD axes), in f64"""
    k = R.Kin(model, state)
    out = np.zeros(k.nb - 1)
    for i in range(1, k.nb):
        out[k.slot[i]] = k.a[i] @ np.asarray(rows_world[k.slot[i]][3:6], np.float64)
    return out
