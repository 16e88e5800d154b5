"""numpy restatement of the derivatives of the inverse dynamics (include/trex_dynamics_derivatives.h), written from the textbook
recursion of dynamics_ref.inverse_dynamics - world positions, subtree moments about the WORLD origin, projected afterwards - by
differentiating every line of it, and not from the kernel (own-point moments relative to the base origin, levers between origins).

Every quantity of the recursion gets a tangent with a trailing direction axis; all 2 D directions go through at once:

    directions 0 .. D-1      the configuration tangent xi, ordered like the generalised velocity: the base origin along the world
                             axes, the base turned by a WORLD-axis rotation vector (R <- exp([xi]x) R), the joint angles in
                             observation order; the NUMBERS of the velocity (world-axis v, w; qd) and of the classical accelerations
                             are held fixed
    directions D .. 2D-1     the generalised velocity

A rotation's tangent is the vector dphi with dR = [dphi]x R. dtype as in dynamics_ref: float32 is the careless f32 run - every
array and every intermediate in float32, world positions kept as they are -, whose deviation from the f64 run sets the bounds of
tests/derivatives_cases.py. tests/test_derivatives_ref.py ties the f64 run to central differences of dynamics_ref.inverse_dynamics
and qualifies the bounds against the MISTAKES below."""
import numpy as np

import dynamics_ref as R

# deliberate mistakes a bound has to tell from the right answer (tests/test_derivatives_ref.py)
MISTAKES = ("axis_tangent_dropped",       # the joint axis does not turn with its body: d a = 0
            "inertia_rotation_dropped",   # the inertia does not turn: no [dphi]x Ic - Ic [dphi]x
            "lever_tangent_dropped",      # the lever parent origin -> child origin does not turn
            "com_offset_tangent_dropped", # the COM moves with the body origin only: its offset does not turn
            "wxa_dqd_dropped")            # the (w_parent x a) d qd term of the angular acceleration


def X(a, b):
    """cross product along axis 0 of [3] or [3, K] arrays (a [3] broadcasts over the directions)"""
    a = a[:, None] if a.ndim == 1 and b.ndim == 2 else a
    b = b[:, None] if b.ndim == 1 and a.ndim == 2 else b
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def inverse_dynamics_derivatives(model, state, accel=None, mass_scale=None, gravity=9.81, dtype=np.float64, mistake=None):
    """-> (f [D], dfdq [D, D], dfdv [D, D]), d f_i / d x_j at [i][j]; f is dynamics_ref.inverse_dynamics, computed alongside"""
    assert mistake is None or mistake in MISTAKES
    k = R.Kin(model, state, mass_scale, dtype)
    dt, nb, par, D = k.dtype, k.nb, model["parent"], k.D
    K = 2 * D
    acc = np.zeros(D, dt) if accel is None else np.asarray(accel, dt)
    z3 = lambda: np.zeros((nb, 3, K), dt)
    eye = np.eye(3, dtype=dt)
    # ---- the seeds: what each direction moves
    dq, dqd = np.zeros((nb, K), dt), np.zeros((nb, K), dt)
    for i in range(1, nb):
        dq[i, 6 + k.slot[i]] = 1
        dqd[i, D + 6 + k.slot[i]] = 1
    dphi, dp, dw, dal, dao = z3(), z3(), z3(), z3(), z3()
    dp[0][:, 0:3] = eye
    dphi[0][:, 3:6] = eye
    dw[0][:, D + 3:D + 6] = eye
    # ---- outward: the nominal recursion of dynamics_ref.inverse_dynamics and, line by line, its tangent
    w, al, ao = np.zeros((nb, 3), dt), np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)
    w[0], ao[0], al[0] = k.w, acc[0:3] + np.array([0, 0, gravity], dt), acc[3:6]
    da = z3()
    for i in range(1, nb):
        pa = int(par[i])
        a, d, qd, qdd = k.a[i], k.p[i] - k.p[pa], k.qd[i], acc[6 + k.slot[i]]
        dd = X(dphi[pa], d)
        if mistake == "lever_tangent_dropped":
            dd = np.zeros_like(dd)
        dp[i] = dp[pa] + dd
        dphi[i] = dphi[pa] + a[:, None] * dq[i]
        if mistake != "axis_tangent_dropped":
            da[i] = X(dphi[i], a)
        wxa = np.cross(w[pa], a)
        w[i] = w[pa] + a * qd
        dw[i] = dw[pa] + da[i] * qd + a[:, None] * dqd[i]
        al[i] = al[pa] + a * qdd + wxa * qd
        dal[i] = dal[pa] + da[i] * qdd + (X(dw[pa], a) + X(w[pa], da[i])) * qd
        if mistake != "wxa_dqd_dropped":
            dal[i] = dal[i] + wxa[:, None] * dqd[i]
        wxd = np.cross(w[pa], d)
        ao[i] = ao[pa] + np.cross(al[pa], d) + np.cross(w[pa], wxd)
        dao[i] = dao[pa] + X(dal[pa], d) + X(al[pa], dd) + X(dw[pa], wxd) + X(w[pa], X(dw[pa], d) + X(w[pa], dd))
    # ---- every body: force, and moment about the WORLD origin
    F, N = np.zeros((nb, 3), dt), np.zeros((nb, 3), dt)
    dF, dN = z3(), z3()
    for b in range(nb):
        Ic, cb = k.Ic[b], k.c[b] - k.p[b]
        dcb = X(dphi[b], cb)
        if mistake == "com_offset_tangent_dropped":
            dcb = np.zeros_like(dcb)
        dc = dp[b] + dcb
        wxc = np.cross(w[b], cb)
        ac = ao[b] + np.cross(al[b], cb) + np.cross(w[b], wxc)
        dac = dao[b] + X(dal[b], cb) + X(al[b], dcb) + X(dw[b], wxc) + X(w[b], X(dw[b], cb) + X(w[b], dcb))
        F[b], dF[b] = k.mass[b] * ac, k.mass[b] * dac
        Iw, Ial = Ic @ w[b], Ic @ al[b]
        dIw, dIal = Ic @ dw[b], Ic @ dal[b]
        if mistake != "inertia_rotation_dropped":       # d Ic x = dphi x (Ic x) - Ic (dphi x x)
            dIw = dIw + X(dphi[b], Iw) - Ic @ X(dphi[b], w[b])
            dIal = dIal + X(dphi[b], Ial) - Ic @ X(dphi[b], al[b])
        N[b] = Ial + np.cross(w[b], Iw) + np.cross(k.c[b], F[b])
        dN[b] = dIal + X(dw[b], Iw) + X(w[b], dIw) + X(dc, F[b]) + X(k.c[b], dF[b])
    # ---- inward: subtree sums, then the projection on the joint axis with the moment referred to the joint origin
    f, df = np.zeros(D, dt), np.zeros((D, K), dt)
    for b in range(nb - 1, 0, -1):
        n_own = N[b] - np.cross(k.p[b], F[b])
        dn_own = dN[b] - X(dp[b], F[b]) - X(k.p[b], dF[b])
        f[6 + k.slot[b]] = k.a[b] @ n_own
        df[6 + k.slot[b]] = (da[b] * n_own[:, None]).sum(0) + (k.a[b][:, None] * dn_own).sum(0)
        pa = int(par[b])
        F[pa] += F[b]
        N[pa] += N[b]
        dF[pa] += dF[b]
        dN[pa] += dN[b]
    f[0:3], df[0:3] = F[0], dF[0]
    f[3:6] = N[0] - np.cross(k.pos, F[0])
    df[3:6] = dN[0] - X(dp[0], F[0]) - X(k.pos, dF[0])
    assert df.dtype == np.dtype(dt)
    return f, df[:, :D].copy(), df[:, D:].copy()


def branch_zero_mask(model):
    """[D, D] bool: the joint-row / joint-column pairs whose two joints lie on different branches (neither an ancestor of the other)"""
    nb = model["nb"]
    slot = np.full(nb, -1)
    slot[model["obs_order"]] = np.arange(nb - 1)
    chains = []
    for b in range(nb):
        c, a = set(), b
        while a > 0:
            c.add(a)
            a = int(model["parent"][a])
        chains.append(c)
    mask = np.zeros((5 + nb, 5 + nb), bool)
    for i in range(1, nb):
        for j in range(1, nb):
            if i not in chains[j] and j not in chains[i]:
                mask[6 + slot[i], 6 + slot[j]] = True
    return mask
