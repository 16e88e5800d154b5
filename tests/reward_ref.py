"""numpy f64 restatement of the reward terms (include/trex_reward.h): the values v_t of one env's terms, its history
rules, the composed column, and the tolerance each kind is compared within. Built on link_state_ref for the kinematics - the base
axes are its axes="base", URDF link 0's frame, as in observation_ref. tests/test_reward_ref.py pins it; the GPU tests compare
trex_batch_compose_reward against it.

A specification here is a list of (kind, link, mask, xyz, weight, p0, p1) - what reward_capi.BatchRewards.set_reward takes: kind a TREX_REW_* value,
link a URDF link index, mask the bits of the joints (0 = all) or, for CONTACT_COUNT, of the bodies.

What both sides share as f32 values, and the reference therefore takes as f32: the row (q, qd, torque, reward, done), the actions,
the command, the sensor's forces, the parameters of a term, the joint limits and start angles the kernel reads from the device
model, and Ts = f32(dt * substeps)."""
import numpy as np

import link_state_ref as L
from tolerances import LINK_TOL

(STEP, ALIVE, TRACK_LIN, TRACK_ANG, LIN_VEL_Z, ANG_VEL_XY, ORIENTATION, BASE_HEIGHT, POINT_HEIGHT, TORQUE, JOINT_VEL, JOINT_ACC,
 ACTION_RATE, JOINT_LIMIT, POWER, JOINT_POSE, CONTACT_COUNT, FOOT_AIR_TIME, FOOT_SLIP) = range(19)
KINDS = 19
MAX_TERMS = 32
JOINT_SUMS = (TORQUE, JOINT_VEL, JOINT_ACC, JOINT_LIMIT, POWER, JOINT_POSE)
CONTACT_KINDS = (CONTACT_COUNT, FOOT_AIR_TIME, FOOT_SLIP)
FLOOR_Z = 0.0005            # oracle.trex_model.default_params()
U = 2.0 ** -24              # unit roundoff of f32
TINY = 2.0 ** -126          # the smallest normal f32
f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)


def step_seconds(dt=1.0 / 240.0, substeps=5):
    """Ts as the kernel holds it: f32(dt * substeps)"""
    return float(np.float32(dt * substeps))


def new_history(T, J, A):
    return dict(valid=0, prev_act=np.zeros(A), prev_qd=np.zeros(J), timer=np.zeros(T), held=np.zeros(T))


def reset_history(h):
    """trex_batch_reward_reset for this env"""
    h["valid"] = 0
    h["timer"][:] = 0.0
    h["held"][:] = 0.0


def joints_of(mask, J):
    return [j for j in range(J) if (mask >> j) & 1] if mask else list(range(J))


def limits(model):
    """(lower, upper, start angles) in observation order, as the f32 values of the device model"""
    oo = model["obs_order"]
    return f32(model["q_lower"][oo]), f32(model["q_upper"][oo]), f32(model["q_start"][oo])


def evaluate(model, spec, state, row, hist, Ts, action=None, command=None, force=None, floor_z=FLOOR_Z):
    """One call of trex_batch_compose_reward for one env. state: get_state()'s [13 + 2J] behind the row; row: the env's row as the
    step wrote it [>= 3J + 2]; hist: the env's history (new_history), advanced in place; action [A], command [3], force
    [num_bodies, 3] (the contact sensor's fx fy fz) where a term needs them. -> (v [T] f64, cases [T]): cases[t] is what
    bound(kind, cases[t]) needs."""
    J = model["nb"] - 1
    row = f32(row)
    q, qd, tau = row[:J], row[J:2 * J], row[2 * J:3 * J]
    done = row[3 * J + 1] != 0
    lo, hi, qs = limits(model)
    lb = np.asarray(model["link_body"], int)
    act = None if action is None else f32(action)
    c = None if command is None else f32(command)
    base_w = base_b = None
    v, cases = np.zeros(len(spec)), []
    timer = hist["timer"].copy()
    for t, (kind, link, mask, xyz, weight, p0, p1) in enumerate(spec):
        xyz, p0, p1 = f32(xyz), float(np.float32(p0)), float(np.float32(p1))
        case = dict(value=0.0)
        new_timer = 0.0
        if kind == STEP:
            v[t] = row[3 * J]
        elif done:
            v[t] = hist["held"][t]
        elif kind == ALIVE:
            v[t] = 1.0
        elif kind in (TRACK_LIN, TRACK_ANG, LIN_VEL_Z, ANG_VEL_XY, ORIENTATION, BASE_HEIGHT):
            if base_b is None:
                base_w = L.link_state(model, state, [0], axes="world")
                base_b = L.link_state(model, state, [0], axes="base")
            lin, ang = base_b["linear_velocity"][0], base_b["angular_velocity"][0]
            g = base_w["rotation"][0].T @ np.array([0.0, 0.0, -1.0])
            tol_lin = LINK_TOL["velocity"] * max(1.0, np.abs(lin).max())
            tol_ang = LINK_TOL["velocity"] * max(1.0, np.abs(ang).max())
            if kind == TRACK_LIN:
                d = np.array([lin[0] - c[0], lin[1] - c[1]])
                arg = (d ** 2).sum() / p0
                v[t] = np.exp(-arg)
                case.update(arg=arg, darg=(2 * np.abs(d).sum() * tol_lin + 2 * tol_lin ** 2) / p0)
            elif kind == TRACK_ANG:
                d = ang[2] - c[2]
                arg = d * d / p0
                v[t] = np.exp(-arg)
                case.update(arg=arg, darg=(2 * abs(d) * tol_ang + tol_ang ** 2) / p0)
            elif kind == LIN_VEL_Z:
                v[t] = lin[2] ** 2
                case.update(first=2 * abs(lin[2]) * tol_lin + tol_lin ** 2)
            elif kind == ANG_VEL_XY:
                v[t] = ang[0] ** 2 + ang[1] ** 2
                case.update(first=2 * (abs(ang[0]) + abs(ang[1])) * tol_ang + 2 * tol_ang ** 2)
            elif kind == ORIENTATION:
                tol = LINK_TOL["pose"] * max(1.0, np.abs(g).max())
                v[t] = g[0] ** 2 + g[1] ** 2
                case.update(first=2 * (abs(g[0]) + abs(g[1])) * tol + 2 * tol ** 2)
            else:
                h = base_w["position"][0][2] - floor_z
                tol = LINK_TOL["pose"] * max(1.0, abs(h))
                v[t] = (h - p0) ** 2
                case.update(first=2 * abs(h - p0) * tol + tol ** 2)
        elif kind == POINT_HEIGHT:
            h = L.link_state(model, state, [link], [xyz], axes="world")["position"][0][2] - floor_z
            tol = LINK_TOL["pose"] * max(1.0, abs(h))
            v[t] = (h - p0) ** 2
            case.update(first=2 * abs(h - p0) * tol + tol ** 2)
        elif kind in JOINT_SUMS:
            js = joints_of(mask, J)
            if kind == TORQUE:
                x = tau[js] ** 2
            elif kind == JOINT_VEL:
                x = qd[js] ** 2
            elif kind == JOINT_ACC:
                x = ((qd[js] - hist["prev_qd"][js]) / Ts) ** 2 if hist["valid"] else np.zeros(len(js))
            elif kind == JOINT_LIMIT:
                m = 0.5 * (1.0 - p0) * (hi[js] - lo[js])
                x = np.maximum(0.0, lo[js] + m - q[js]) + np.maximum(0.0, q[js] - (hi[js] - m))
            elif kind == POWER:
                x = np.abs(tau[js] * qd[js])
            else:
                x = (q[js] - qs[js]) ** 2
            v[t] = x.sum()
            case.update(n=len(js), abs_sum=np.abs(x).sum())
        elif kind == ACTION_RATE:
            x = (act - hist["prev_act"]) ** 2 if hist["valid"] else np.zeros(len(act))
            v[t] = x.sum()
            case.update(n=len(act), abs_sum=np.abs(x).sum())
        elif kind == CONTACT_COUNT:
            f = f32(force)
            norm = np.sqrt((f ** 2).sum(1))
            bodies = [b for b in range(model["nb"]) if (mask >> b) & 1]
            v[t] = sum(1.0 for b in bodies if norm[b] > p0)
            # (a norm within its own f32 rounding of the threshold may fall on either side)
            case.update(ambiguous=sum(1 for b in bodies if abs(norm[b] - p0) <= 4 * U * norm[b]))
        elif kind == FOOT_AIR_TIME:
            contact = f32(force)[lb[link], 2] > p0
            if not contact:
                new_timer = timer[t] + Ts
            elif timer[t] > 0:
                v[t] = timer[t] - p1
            case.update(timer=timer[t], steps=int(round(timer[t] / Ts)))
        elif kind == FOOT_SLIP:
            r = L.link_state(model, state, [link], [xyz], axes="world")
            lv = r["linear_velocity"][0]
            tol = LINK_TOL["velocity"] * max(1.0, np.abs(lv).max())
            contact = f32(force)[lb[link], 2] > p0
            v[t] = lv[0] ** 2 + lv[1] ** 2 if contact else 0.0
            case.update(first=(2 * (abs(lv[0]) + abs(lv[1])) * tol + 2 * tol ** 2) if contact else 0.0)
        else:
            raise ValueError("unknown kind %r" % (kind,))
        case["value"] = v[t]
        case["held"] = bool(done and kind != STEP)
        cases.append(case)
        timer[t] = new_timer
    if done:
        hist["valid"] = 0
        hist["timer"][:] = 0.0
    else:
        hist["timer"][:] = timer
        hist["held"][:] = v
        hist["prev_qd"][:] = qd
        if act is not None:
            hist["prev_act"][:] = act
        hist["valid"] = 1
    return v, cases


def bound(kind, case):
    """The deviation |v_gpu - v_ref| the test allows for a term of `kind`; `case` comes from evaluate().
      - a held value (done row) and STEP, ALIVE: 0 - they are copies;
      - terms of the base or a point: their inputs deviate by tolerances.LINK_TOL['pose' | 'velocity'] x max(1, largest |entry| of
        the input vector), as test_gpu_observations applies it; that propagates through the term's formula to first order (the
        square of the input deviation included, so that the bound also holds at a zero of the formula), plus 4 ulps of the value
        for the formula's own f32 arithmetic;
      - tracking terms: the same propagation gives |d arg|, and exp turns it into v (e^|d arg| - 1); plus 4 ulps of expf and the
        rounding of the argument, |arg| x 4 ulps, both times v; plus the smallest normal f32: expf may flush a subnormal result;
      - joint sums and ACTION_RATE: the inputs are the same f32 values on both sides: (n + 2) 2^-23 sum |summand|;
      - CONTACT_COUNT: 0, plus 1 for every body whose |f| lies within its own rounding of the threshold;
      - FOOT_AIR_TIME: the timer is an f32 sum of `steps` equal addends and one subtraction: (steps + 2) 2^-23 |timer|."""
    if case.get("held") or kind in (STEP, ALIVE):
        return 0.0
    v = abs(case["value"])
    if kind in (TRACK_LIN, TRACK_ANG):
        return v * np.expm1(case["darg"]) + (4 + 4 * case["arg"]) * 2 * U * v + TINY
    if kind in (LIN_VEL_Z, ANG_VEL_XY, ORIENTATION, BASE_HEIGHT, POINT_HEIGHT, FOOT_SLIP):
        return case["first"] + 4 * 2 * U * v
    if kind in JOINT_SUMS or kind == ACTION_RATE:
        return (case["n"] + 2) * 2 * U * case["abs_sum"]
    if kind == CONTACT_COUNT:
        return float(case["ambiguous"])
    if kind == FOOT_AIR_TIME:
        return (case["steps"] + 2) * 2 * U * abs(case["timer"])
    raise ValueError("unknown kind %r" % (kind,))


def compose(spec, v):
    """(weighted terms [T] f32, the reward column f32): the products rounded to f32, summed in f32 in term order from the first"""
    w = np.array([s[4] for s in spec], np.float32)
    prod = (w * np.asarray(v, np.float32)).astype(np.float32)
    total = prod[0]
    for p in prod[1:]:
        total = np.float32(total + p)
    return prod, total


def ordered_sum(prod):
    """[n] f32: the f32 sum of the columns of prod [n, T] f32 in column order, starting from the first"""
    prod = np.asarray(prod, np.float32)
    total = prod[:, 0].copy()
    for t in range(1, prod.shape[1]):
        total = (total + prod[:, t]).astype(np.float32)
    return total


def reward_table(model, spec):
    """What build_reward_table (csrc/host_tables.cpp) makes of the specification: dict of kind, body, mask [T]
    (integers), tf [T, 12], point [T, 3], weight, p0, p1 [T] (f64, to be rounded to f32 by the comparison), joint_body [32],
    body_mask, contact, actions, command."""
    J = model["nb"] - 1
    lb = np.asarray(model["link_body"], int)
    ltf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)
    T = len(spec)
    t = dict(kind=np.zeros(T, int), body=np.zeros(T, int), mask=np.zeros(T, np.int64),
             tf=np.zeros((T, 12)), point=np.zeros((T, 3)), weight=np.zeros(T), p0=np.zeros(T), p1=np.zeros(T),
             joint_body=np.zeros(32, int), body_mask=0, contact=False, actions=False, command=False)
    t["joint_body"][:J] = np.asarray(model["obs_order"], int)
    for k, (kind, link, mask, xyz, weight, p0, p1) in enumerate(spec):
        t["kind"][k], t["weight"][k], t["p0"][k], t["p1"][k] = kind, weight, p0, p1
        t["tf"][k] = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
        if kind in (POINT_HEIGHT, FOOT_AIR_TIME, FOOT_SLIP):
            t["body"][k], t["tf"][k] = lb[link], ltf[link]
            t["point"][k] = ltf[link][:9].reshape(3, 3) @ f32(xyz) + ltf[link][9:]
            if kind != FOOT_AIR_TIME:
                t["body_mask"] |= 1 << int(lb[link])
        if kind in JOINT_SUMS:
            t["mask"][k] = mask if mask else (1 << J) - 1
        if kind == CONTACT_COUNT:
            t["mask"][k] = mask
        t["contact"] |= kind in CONTACT_KINDS
        t["actions"] |= kind == ACTION_RATE
        t["command"] |= kind in (TRACK_LIN, TRACK_ANG)
    return t
