"""numpy f64 restatement of the motion clip (include/trex_motion.h): the table trex_batch_set_motion builds (normalised
quaternions in one hemisphere, derived velocities, the loop's displacement), the map from a time to a segment, the interpolated
reference state, the clock rules, the five tracking terms, the composed column and the state RSI writes - and the tolerance each
is compared within. Built on link_state_ref for the kinematics, as reward_ref is. tests/test_motion_ref.py pins it; the GPU tests
compare the three launches against it, tests/test_motion_tables_host.py the host builder.

A specification here is a list of (kind, mask, weight, scale, aux) - what motion_capi.BatchMotion.set_reward takes.

What both sides share as f32 values, and the reference therefore takes as f32: the table as uploaded, the row (q, qd, reward,
done), the state, the parameters of a term, Ts = f32(dt * substeps), and the TIME ARITHMETIC - t, frame_dt, T, their reciprocals
and u are f32 on the device, and which segment a time falls into is decided by them, so map_time repeats the kernel's f32
operations one by one (an fma as an f64 product and sum rounded once). Everything behind u - the interpolation, the forward
kinematics, the terms - is f64 here."""
import numpy as np

import link_state_ref as L
from tolerances import LINK_TOL

POSE, VELOCITY, END_EFFECTOR, ROOT_POSE, ROOT_VELOCITY = range(5)
KINDS = 5
MAX_TERMS, MAX_FRAMES, MAX_PROBES = 8, 4096, 8
NLERP_DOT = 0.9995
U = 2.0 ** -24              # unit roundoff of f32
TINY = 2.0 ** -126          # the smallest normal f32
f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
F32 = np.float32


def step_seconds(dt=1.0 / 240.0, substeps=5):
    """Ts as the kernel holds it: f32(dt * substeps)"""
    return float(np.float32(dt * substeps))


def joints_of(mask, J):
    return [j for j in range(J) if (mask >> j) & 1] if mask else list(range(J))


# ---------------------------------------------------------------- the builder
def quat_mul(a, b):
    """a o b, xyzw: the rotation b, then a"""
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def rotation_vector(q):
    """the rotation vector of the unit quaternion q, the shorter way round"""
    q = -q if q[3] < 0 else q
    s = np.linalg.norm(q[:3])
    return np.zeros(3) if s == 0 else q[:3] * (2.0 * np.arctan2(s, q[3]) / s)


def refusal(model, frames, velocities, frame_dt):
    """why trex_batch_set_motion refuses these host values, or None"""
    frames = np.asarray(frames, np.float64)
    F = len(frames)
    J = model["nb"] - 1
    if F < 2 or F > MAX_FRAMES:
        return "num_frames"
    if not np.isfinite(frame_dt) or not frame_dt > 0:
        return "frame_dt"
    if not np.isfinite(frames).all() or (velocities is not None and not np.isfinite(velocities).all()):
        return "not finite"
    if (np.linalg.norm(frames[:, 3:7], axis=1) == 0).any():
        return "norm 0"
    oo = model["obs_order"]
    if (frames[:, 7:] < model["q_lower"][oo] - 1e-6).any() or (frames[:, 7:] > model["q_upper"][oo] + 1e-6).any():
        return "outside its limits"
    return None


def build_table(model, frames, velocities, frame_dt, loop):
    """What build_motion_table (csrc/host_tables.cpp) makes of the host values: dict of rows [F, 13 + 2J] (f64, to be rounded to
    f32 by the comparison; the device rows are padded to a multiple of 4 floats), the f32 constants frame_dt, inv_dt, duration,
    inv_duration, disp [2] as f64 numbers, loop, frames."""
    frames = np.asarray(frames, np.float64)
    F, J = len(frames), model["nb"] - 1
    assert refusal(model, frames, velocities, frame_dt) is None
    quat = frames[:, 3:7] / np.linalg.norm(frames[:, 3:7], axis=1, keepdims=True)
    for k in range(1, F):
        if quat[k] @ quat[k - 1] < 0:
            quat[k] = -quat[k]
    pos, q = frames[:, :3], frames[:, 7:]
    disp = np.array([pos[-1, 0] - pos[0, 0], pos[-1, 1] - pos[0, 1], 0.0])
    rows = np.zeros((F, 13 + 2 * J))
    rows[:, 0:3], rows[:, 3:7], rows[:, 13:13 + J] = pos, quat, q
    if velocities is not None:
        vel = np.asarray(velocities, np.float64)
        rows[:, 7:13], rows[:, 13 + J:] = vel[:, :6], vel[:, 6:]
    else:
        for k in range(F):
            km, kp, om, op = max(k - 1, 0), min(k + 1, F - 1), 0.0, 0.0
            if loop and k == 0:
                km, om = F - 2, -1.0
            if loop and k == F - 1:
                kp, op = 1, 1.0
            span = (2 if loop else kp - km) * frame_dt
            rows[k, 7:10] = ((pos[kp] + op * disp) - (pos[km] + om * disp)) / span
            rows[k, 10:13] = rotation_vector(quat_mul(quat[kp], quat[km] * np.array([-1, -1, -1, 1.0]))) / span
            rows[k, 13 + J:] = (q[kp] - q[km]) / span
    dt = float(F32(frame_dt))
    T = float(F32((F - 1) * dt))
    return dict(rows=rows, frames=F, loop=bool(loop), frame_dt=dt, inv_dt=float(F32(1.0 / dt)), duration=T,
                inv_duration=float(F32(1.0 / T)), disp=f32(disp[:2]))


def device_table(tab):
    """the table with its rows as the f32 values of the upload: what the interpolation below reads"""
    return dict(tab, rows=f32(tab["rows"]))


# ---------------------------------------------------------------- time -> segment, in the kernel's f32 operations
def _fma(a, b, c):
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def map_time(tab, t):
    """-> (k, u, cycles, phase) of the time t (an f32 value), as map_time of csrc/motion.hip computes them"""
    T, invT, inv_dt = F32(tab["duration"]), F32(tab["inv_duration"]), F32(tab["inv_dt"])
    t = F32(t)
    if not t > 0:
        t = F32(0)
    t = min(t, F32(1.0e30))
    cycles, tw = F32(0), t
    if tab["loop"]:
        cycles = np.floor(F32(t * invT))
        tw = _fma(-cycles, T, t)
        if tw < 0:
            tw, cycles = F32(tw + T), F32(cycles - 1)
        if tw >= T:
            tw, cycles = F32(tw - T), F32(cycles + 1)
    tw = min(max(tw, F32(0)), T)
    s = F32(tw * inv_dt)
    k = max(0, min(int(s), tab["frames"] - 2))
    u = min(max(F32(s - F32(k)), F32(0)), F32(1))
    return k, float(u), float(cycles), float(min(F32(tw * invT), F32(1)))


def clock_time(clock, Ts):
    """the env's reference time t0 + k Ts, one fma in f32"""
    return float(_fma(F32(clock["k"]), F32(Ts), F32(clock["t0"])))


def slerp(a, b, u):
    d = float(a @ b)
    if d < 0:
        b, d = -b, -d
    if d > NLERP_DOT:
        q = (1 - u) * a + u * b
        return q / np.linalg.norm(q)
    th = np.arccos(d)
    return (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th)


def sample(tab, t):
    """the reference state [13 + 2J] at time t (tab: device_table) and its phase"""
    k, u, cycles, phase = map_time(tab, t)
    a, b = tab["rows"][k], tab["rows"][k + 1]
    s = (1 - u) * a + u * b
    s[0:2] += cycles * tab["disp"]
    s[3:7] = slerp(a[3:7], b[3:7], u)
    return s, phase


def sample_bound(tab, t):
    """[13 + 2J]: how far the f32 interpolation may lie from sample(). A lerp column is fl(u b + fl(fl(1 - u) a)): three
    roundings, each at most U times the larger end, and a fourth of the result where the cycles' displacement is added by an
    fma. A quaternion component: the dot product (4 fmas on values <= 1: 4 U), acosf and three sinf (2 ulp each on values <=
    pi/2: the angle's error enters the two weights only through d/dth sin(u th)/sin(th), at most th/3 < 0.53), a division, two
    products and an fma per weight pair - under 16 U on a component of magnitude <= 1; the same count covers the normalised
    lerp (sum of squares, sqrt, reciprocal, product)."""
    k, u, cycles, _ = map_time(tab, t)
    a, b = np.abs(tab["rows"][k]), np.abs(tab["rows"][k + 1])
    mag = np.maximum(a, b)
    mag[0:2] = np.maximum(mag[0:2], np.abs(cycles * tab["disp"]) + mag[0:2])
    out = 4 * U * mag + TINY
    out[3:7] = 16 * U
    return out


# ---------------------------------------------------------------- the terms
def new_clock():
    return dict(t0=0.0, k=0)


def probe_positions(model, state, links, points, axes):
    return L.link_state(model, state, links, points, axes=axes)["position"]


def quat_angle(a, b):
    """the angle in [0, pi] of a^-1 o b"""
    r = quat_mul(a * np.array([-1, -1, -1, 1.0]), b)
    return 2.0 * np.arctan2(np.linalg.norm(r[:3]), abs(r[3]))


def evaluate(model, tab, spec, state, row, clock, held, Ts, probes=None):
    """One call of trex_batch_compose_motion_reward for one env. state: get_state()'s [13 + 2J] behind the row; row: the env's row
    [>= 3J + 2]; clock (new_clock) and held [T]: the env's, advanced in place; probes: (links [K], points [K, 3]) of the clip's
    end effectors. -> (v [T] f64, cases [T]): cases[t] is what bound(kind, cases[t]) needs."""
    J = model["nb"] - 1
    row, state = f32(row), f32(state)
    T = len(spec)
    if row[3 * J + 1] != 0:      # the new episode's state is behind the row: the step before, again; then everything restarts
        v = held.copy()
        held[:] = 0.0
        clock.update(t0=0.0, k=0)
        return v, [dict(held=True, value=x) for x in v]
    clock["k"] += 1
    t = clock_time(clock, Ts)
    ref, _ = sample(tab, t)
    rb = sample_bound(tab, t)
    q, qd = row[:J], row[J:2 * J]
    v, cases = np.zeros(T), []
    for i, (kind, mask, weight, scale, aux) in enumerate(spec):
        scale, aux = float(F32(scale)), float(F32(aux))
        js = joints_of(mask, J)
        if kind in (POSE, VELOCITY):
            x, xr, xb = (q, ref[13:13 + J], rb[13:13 + J]) if kind == POSE else (qd, ref[13 + J:], rb[13 + J:])
            d = x[js] - xr[js]
            s = (d ** 2).sum()
            # each difference: the reference's own bound and one rounding; its square and the sum: (n + 2) roundings of the sum
            dd = xb[js] + U * np.abs(d)
            ds = (2 * np.abs(d) * dd + dd ** 2).sum() + (len(js) + 2) * 2 * U * s
        elif kind == END_EFFECTOR:
            links, points = probes
            pa = probe_positions(model, state, links, points, "base")
            pr = probe_positions(model, ref, links, points, "base")
            d = pa - pr
            s = (d ** 2).sum()
            # each position: the link query's own tolerance, and at the reference pose the reference's rounding carried down the
            # chain - a joint angle's bound times the probe's distance from the base, summed over the joints, and the quaternion's
            reach = np.abs(pr).max() + 1.0
            tol = LINK_TOL["pose"] * max(1.0, np.abs(pa).max(), np.abs(pr).max())
            dd = 2 * tol + (rb[13:13 + J].sum() + 2 * rb[3:7].sum()) * reach + U * np.abs(d)
            ds = (2 * np.abs(d) * dd + dd ** 2).sum() + (d.size + 2) * 2 * U * s
        elif kind == ROOT_POSE:
            dp = state[0:3] - ref[0:3]
            th = quat_angle(state[3:7], ref[3:7])
            s = (dp ** 2).sum() + aux * th * th
            # theta = 2 atan2(|vector part|, |w|): the quaternion's bound on each of the 8 products behind either argument,
            # and the roundings of products, root and atan2f - 16 U on the arguments; d theta <= 2 x that (atan2's gradient is
            # at most 1 / hypot, the arguments' hypot is 1)
            dth = 2 * (4 * rb[3:7].max() + 16 * U) + 4 * U * th
            ddp = rb[0:3] + U * np.abs(dp)
            ds = (2 * np.abs(dp) * ddp + ddp ** 2).sum() + aux * (2 * th * dth + dth ** 2) + 8 * 2 * U * s
        elif kind == ROOT_VELOCITY:
            dv, dw = state[7:10] - ref[7:10], state[10:13] - ref[10:13]
            s = (dv ** 2).sum() + aux * (dw ** 2).sum()
            ddv, ddw = rb[7:10] + U * np.abs(dv), rb[10:13] + U * np.abs(dw)
            ds = (2 * np.abs(dv) * ddv + ddv ** 2).sum() + aux * (2 * np.abs(dw) * ddw + ddw ** 2).sum() + 10 * 2 * U * s
        else:
            raise ValueError("unknown kind %r" % (kind,))
        v[i] = np.exp(-scale * s)
        cases.append(dict(held=False, value=v[i], arg=scale * s, darg=scale * ds))
    held[:] = v
    return v, cases


def bound(kind, case):
    """The tolerance of one term's value v = exp(-arg): the argument's own error darg (derived per kind in evaluate, from the
    reference's interpolation bound, the link query's tolerance and the operation counts), then the product with the scale, the
    negation and expf - (4 + 4 arg) roundings of 2 U relative, as reward_ref counts its tracking terms. A held value is a copy:
    it is compared with the value the test recorded from the step before, bitwise - bound 0."""
    if case["held"]:
        return 0.0
    v = abs(case["value"])
    return v * np.expm1(case["darg"]) + (4 + 4 * case["arg"]) * 2 * U * v + TINY


def compose(spec, v, column, step_weight):
    """(weighted terms [T] f32, the reward column f32): the products rounded to f32, added in f32 in term order to the rounded
    product step_weight * column"""
    w = np.array([s[2] for s in spec], np.float32)
    prod = (w * np.asarray(v, np.float32)).astype(np.float32)
    total = np.float32(np.float32(step_weight) * np.float32(column))
    for p in prod:
        total = np.float32(total + p)
    return prod, total


def ordered_sum(first, prod):
    """[n] f32: first + the columns of prod [n, T] f32 in column order, an f32 sum"""
    total = np.asarray(first, np.float32).copy()
    for t in range(prod.shape[1]):
        total = (total + np.asarray(prod[:, t], np.float32)).astype(np.float32)
    return total
