"""Case groups that move the step kernel's engine parameters off their defaults (TP_* in csrc/device_model.h, the same names in
oracle/oracle.py). Everything is generated from seeds and qualified by the oracle alone: tests/test_param_cases_host.py asserts
the conditions below on the CPU, tests/test_gpu_engine_params.py feeds the same arrays to the kernels. A helper, not a conftest.

A group = one parameter set and one batch (one model, one set of control modes); every group but all_moved moves ONE parameter,
given relative to the defaults of oracle/trex_model.py (the GPU test asserts that Model.get_param reports the same defaults).
A case = one env: an f32 state and an f32 action held for 3 env-steps after set_state, compared after env-step 1 and env-step 3.

Candidates are the states of tests/state_sets.py and tests/joint_limit_states.py rolled out again under the group's own f64
oracle (a landing under gravity 3.7 is another trajectory), and seeded airborne states. For a moved floor the rollout is made
over the default floor and translated in z by the same amount (the physics does not know where z = 0 is).

Acceptance (accept): at both compared env-steps the oracle's f32 build passes parity_helpers.assert_step_close against its f64
build at loosen = 1, with the same contact count and the same touched bodies - on the state itself (feature_cases.accept) AND on
PERTURBED copies of it moved by about one f32 ulp (the yardstick of test_gpu_parity.py::test_config4_size_on_one_gpu: "a single
f32 evaluation can be lucky in the component that matters"). Three env-steps through contact amplify rounding; a state on which
the oracle's own f32 build leaves the bound when the state moves by an ulp measures f32, not the kernel (the first GPU run showed
four such cases, profiles/r26_engine_params.txt). A candidate that fails is replaced by the next one; nothing is loosened. The share of examined candidates that failed is a group's `replaced` share (capped by the host test).
Sensitivity (sensitivity): the f64 oracle with the DEFAULT value of the moved parameter, on the same state and action, fails
assert_step_close against the group's oracle, and its rates differ by >= EFFECT x the rate tolerance. pick() takes sensitive
candidates first (at least half of a group), then the others (an airborne state does not feel gravity in its joint rates, but it
belongs to the group all the same).
Branch conditions (a candidate without them is not a candidate of the group; it counts as passed over, not as replaced):
  cerp_*: a contact point with negative distance; erp_*: a joint beyond its stop; iters_*: >= 6 contact points at the first
  compared step; friction_*: a contact point that slides at > SLIDE m/s; vmax_2, base cases: the same world twist on an upright
  base (identity quaternion) is >= EFFECT away (frame_gap).
"""
import os
import zlib

import numpy as np

import feature_cases as fc
import joint_limit_states as jl
import synthetic_models as sm
from state_sets import landing_states

EFFECT = fc.EFFECT              # sensitivity: rate difference in units of the rate tolerance of assert_step_close
QD_TOL = fc.QD_TOL
COMPARED = (0, 2)               # indices of the compared env-steps: after step 1 and after step 3
N_STEPS = 3
N_CASES = 12                    # cases per group (8 .. 16)
SLIDE = 0.05                    # m/s: tangential speed of a contact point that makes friction matter
VMAX = 2.0                      # max_coordinate_velocity of the vmax groups
TILT = 0.5                      # rad: least roll and pitch of the tilted-base cases
VEL_JOINTS = (1, 6, 11, 16, 21)  # observation columns in VELOCITY mode in the group vmax_2_velocity
MODE_VELOCITY = 1
PERTURBED, ULP = 6, 6e-8        # acceptance: the f32 oracle also on that many copies of the state moved by about one f32 ulp


def defaults():
    from oracle import trex_model as tm
    return dict(tm.default_params())


def moved_parameters():
    """group -> the parameters it moves, relative to the defaults"""
    d = defaults()
    g = {
        "dt_half": dict(dt=0.5 * d["dt"]), "dt_double": dict(dt=2.0 * d["dt"]),
        "substeps_1": dict(substeps=1), "substeps_3": dict(substeps=3), "substeps_8": dict(substeps=8),
        "iters_1": dict(iterations=1), "iters_7": dict(iterations=7), "iters_120": dict(iterations=120),
        "gravity_low": dict(gravity=3.7), "gravity_high": dict(gravity=15.0), "gravity_zero": dict(gravity=0.0),
        "friction_low": dict(friction=0.05), "friction_high": dict(friction=1.0),
        "erp_low": dict(erp=0.05), "erp_high": dict(erp=0.8),
        "cerp_low": dict(contact_erp=0.05), "cerp_high": dict(contact_erp=0.8),
        "damping_zero": dict(link_damping=0.0), "damping_high": dict(link_damping=0.5),
        "vmax_2": dict(max_coordinate_velocity=VMAX), "vmax_2_velocity": dict(max_coordinate_velocity=VMAX),
        "floor_up": dict(floor_z=d["floor_z"] + 0.3), "floor_down": dict(floor_z=d["floor_z"] - 0.2),
    }
    # every parameter above at once, the non-extreme value of each
    g["all_moved"] = dict(dt=0.5 * d["dt"], substeps=3, iterations=7, gravity=3.7, friction=1.0, erp=0.8, contact_erp=0.8,
                          link_damping=0.5, max_coordinate_velocity=VMAX, floor_z=d["floor_z"] + 0.3)
    for name in ("erp_low", "erp_high", "all_moved"):
        g[name + "_deep_chain"] = dict(g[name])
    return g


GROUPS = list(moved_parameters())
for _k in moved_parameters()["all_moved"]:
    assert any(set(v) == {_k} for v in moved_parameters().values()), _k       # all_moved moves what the single groups move


# ---------------------------------------------------------------- models
def built(name, moved, directory):
    """the fc.Built (oracle model, both oracle builds, urdf, params) of group `name`"""
    if name.endswith("_deep_chain"):
        d = os.path.join(str(directory), "deep_chain")
        os.makedirs(d, exist_ok=True)
        path, props, om = sm.compile_both("deep_chain", d)
        return fc.Built(om, path, dict(sm.SMALL_PARAMS, **moved), tau_floor=0.0)
    return fc.trex(moved)


def with_defaults(b, keys):
    """b's model with the parameters `keys` back at their defaults: the oracle a kernel that ignores them would agree with"""
    d = defaults()
    return fc.Built(b.om, b.urdf, {k: (d[k] if k in keys else v) for k, v in b.params.items()}, tau_floor=b.tau_floor)


def without_floor(b):
    """(the Built the candidates are rolled out on, the z shift to apply to its states)"""
    d = defaults()
    if "floor_z" not in b.params:
        return b, 0.0
    p = {k: v for k, v in b.params.items() if k != "floor_z"}
    return fc.Built(b.om, b.urdf, p, tau_floor=b.tau_floor), float(b.params["floor_z"]) - d["floor_z"]


# ---------------------------------------------------------------- running a case on an oracle
def limits(om):
    oo = om["obs_order"]
    return om["q_lower"][oo], om["q_upper"][oo]


def env_step(orc, om, s, case):
    """one env-step of the oracle state s, in place. VELOCITY joints (case['vel'], a bool mask over the observation columns): the
    kernel's row kd (vt - nqd) + nqd with vt = clip(command, +- max_coordinate_velocity) is the oracle's position row with the
    target q + dt kd vt / kp, q the joint's angle at the substep - restated substep by substep."""
    a = case["action"].astype(np.float64)
    vel = case.get("vel")
    if vel is None:
        obs, rew, pen = orc.step(s, a)
    else:
        p = orc.params
        lo, hi = limits(om)
        J = om["nb"] - 1
        vt = np.clip(a, -p["max_coordinate_velocity"], p["max_coordinate_velocity"])
        orc.set_motors_on(s, 1)
        for _ in range(int(p["substeps"])):
            q = orc.get_state(s)[13:13 + J]
            orc.substep(s, np.where(vel, q + p["dt"] * p["motor_kd"] * vt / p["motor_kp"], np.clip(a, lo, hi)))
        obs = orc.observe(s)
        rew, pen = orc.reward(s)
    body, _, _, dist = orc.contacts(s)
    return dict(obs=obs, rew=rew, pen=pen, cnt=len(body), touched=frozenset(int(x) for x in body),
                dist_min=float(dist.min()) if len(dist) else np.inf, state=orc.get_state(s))


def run(orc, om, case, steps=N_STEPS):
    s = orc.new_state()
    orc.set_state(s, case["state"].astype(np.float64))
    return [env_step(orc, om, s, case) for _ in range(steps)]


def _agrees(b, got, r64, r32):
    return all(fc.close(b, got[i], r64[i], fc.tau_extra(b, r64[i], r32[i])) and r64[i]["cnt"] == got[i]["cnt"]
               and r64[i]["touched"] == got[i]["touched"] for i in COMPARED)


def accept(b, case, perturbed=None):
    """-> (ok, r64, r32): the acceptance conditions of the module docstring at the compared env-steps - for the f32 build on the
    state itself and on `perturbed` (default PERTURBED) copies of it moved by about one f32 ulp, each against the f64 build on
    the state itself"""
    r64, r32 = run(b.o64, b.om, case), run(b.o32, b.om, case)
    ok = _agrees(b, r32, r64, r32)
    rng = np.random.default_rng(zlib.crc32(case["state"].tobytes()))
    st = case["state"].astype(np.float64)
    for _ in range(PERTURBED if perturbed is None else perturbed):
        if not ok:
            break
        ok = _agrees(b, run(b.o32, b.om, dict(case, state=st * (1.0 + ULP * rng.standard_normal(st.shape)))), r64, r32)
    return ok, r64, r32


def rate_gap(b, got, want):
    """largest rate difference over the compared env-steps, in units of the rate tolerance of assert_step_close"""
    J = b.J
    return max(np.abs(got[i]["obs"][J:2 * J] - want[i]["obs"][J:2 * J]).max() / (QD_TOL * max(1.0, np.abs(want[i]["obs"][J:2 * J]).max()))
               for i in COMPARED)


def sensitivity(b, other, case, r64, r32=None):
    """-> (fails, gap): the f64 oracle `other` (the moved parameter at its default, or another variant of the case's own oracle)
    on the same case FAILS assert_step_close against the group's f64 result at a compared step; gap = rate_gap."""
    ro = run(other.o64, other.om, case)
    fails = any(not fc.close(b, ro[i], r64[i], 0.0 if r32 is None else fc.tau_extra(b, r64[i], r32[i])) for i in COMPARED)
    return fails, rate_gap(b, ro, r64)


# ---------------------------------------------------------------- what a candidate is like
def first_contacts(orc, om, case):
    """(body, world point, distance) of the contact points of the FIRST substep: the points of the state itself"""
    s = orc.new_state()
    orc.set_state(s, case["state"].astype(np.float64))
    orc.set_motors_on(s, 1)
    lo, hi = limits(om)
    orc.substep(s, np.clip(case["action"].astype(np.float64), lo, hi))
    body, _, pos, dist = orc.contacts(s)
    return body, pos, dist


def _advance(state, J, eps):
    """the state's pose moved along its own velocities for eps seconds (world-frame angular velocity: q <- dq (x) q)"""
    out = state.copy()
    out[:3] += eps * state[7:10]
    w = state[10:13]
    x, y, z, c = np.append(0.5 * eps * w, 1.0)
    q = state[3:7]
    o = np.array([c * q[0] + x * q[3] + y * q[2] - z * q[1], c * q[1] - x * q[2] + y * q[3] + z * q[0],
                  c * q[2] + x * q[1] - y * q[0] + z * q[3], c * q[3] - x * q[0] - y * q[1] - z * q[2]])
    out[3:7] = o / np.linalg.norm(o)
    out[13:13 + J] += eps * state[13 + J:]
    return out


def sliding_speed(orc, om, case, eps=1e-6):
    """largest tangential (x, y) speed of the material point under a contact point of the state, by a forward difference of the
    body poses along the state's own velocities (f64, eps = 1 us: 1e-6 m/s for the speeds of these states)"""
    body, pos, _ = first_contacts(orc, om, case)
    if not len(body):
        return 0.0
    st = case["state"].astype(np.float64)
    s0, s1 = orc.new_state(), orc.new_state()
    orc.set_state(s0, st)
    orc.set_state(s1, _advance(st, om["nb"] - 1, eps))
    (p0, r0), (p1, r1) = orc.body_poses(s0), orc.body_poses(s1)
    best = 0.0
    for b, x in zip(body, pos):
        local = r0[b].T @ (x - p0[b])
        v = (p1[b] + r1[b] @ local - x) / eps
        best = max(best, float(np.hypot(v[0], v[1])))
    return best


def beyond_stop(om, state):
    """number of joints beyond a stop"""
    lo, hi = limits(om)
    J = om["nb"] - 1
    q = state[13:13 + J].astype(np.float64)
    return int(((q <= lo) | (q >= hi)).sum())


def unconstrained_update(orc, om, state):
    """(base w, base v, joint rates in observation order) after the oracle's unconstrained velocity update of the FIRST substep,
    before its clamp - without the link damping, which moves these by less than 2 % per substep at the rates used here"""
    J = om["nb"] - 1
    s = orc.new_state()
    orc.set_state(s, state.astype(np.float64))
    qdd, ba = orc.forward_dynamics(s, None, with_damping=True)
    dt = orc.params["dt"]
    st = state.astype(np.float64)
    return st[10:13] + ba[:3] * dt, st[7:10] + ba[3:] * dt, st[13 + J:] + qdd * dt


# ---------------------------------------------------------------- candidates
def _case(state, action, origin, **kw):
    return dict(state=np.asarray(state, np.float32), action=np.asarray(action, np.float32), origin=origin, **kw)


def _spread(n):
    """0 .. n-1 in an order that mixes the early (airborne) and late (standing) states of a rollout"""
    step = 7 if n % 7 else 11
    return [(k * step) % n for k in range(n)]


def landing_candidates(b, lateral=0.0, seed=0, noise_seed=5):
    """the 50 states and actions along the 300-step landing of state_sets.landing_states, rolled out on the group's own f64
    oracle (over the default floor, then translated to the group's). lateral: a base velocity of that size in a seeded horizontal
    direction is added to every state - the whole tree then slides over the floor at that speed. noise_seed: the seed of the
    landing's action noise (5: the landing of the other tests)."""
    g, dz = without_floor(b)
    states, acts = landing_states(g.o64, g.om, every=6, seed=noise_seed)
    rng = np.random.default_rng(1000 + seed)
    out = []
    for k in _spread(len(states)):
        st = states[k].copy()
        st[2] += dz
        if lateral:
            phi = rng.uniform(0, 2 * np.pi)
            st[7:9] += lateral * np.array([np.cos(phi), np.sin(phi)])
        out.append(_case(st, acts[k], "landing %d%s" % (6 * k, "" if noise_seed == 5 else " (noise seed %d)" % noise_seed)))
    return out


def penetrating_candidates(b):
    """cerp_*: the landings of three noise seeds; the states in which a contact point is below the floor at one of the three
    env-steps, deepest first (the row's push-out velocity is the depth x contact_erp / dt)"""
    cands = [c for seed in (5, 6, 7) for c in landing_candidates(b, noise_seed=seed)]
    depth = [min(x["dist_min"] for x in run(b.o64, b.om, c)) for c in cands]
    return [dict(cands[k], depth=float(depth[k])) for k in np.argsort(depth, kind="stable") if depth[k] < 0]


def approach_candidates(b, speed=2.5, seed=0):
    """gravity_zero: nothing falls, so the base is sent down at `speed` m/s from the reset pose; a state every env-step until the
    first contact - all airborne, the last ones touch down within their 3 env-steps"""
    om, orc = b.om, b.o64
    q0 = om["q_start"][om["obs_order"]]
    lo, hi = limits(om)
    rng = np.random.default_rng(2000 + seed)
    s = orc.new_state()
    orc.reset(s)
    st = orc.get_state(s)
    st[9] = -speed
    orc.set_state(s, st)
    out = []
    for t in range(60):
        state = orc.get_state(s)
        orc.step(s, np.clip(q0 + 0.15 * rng.normal(size=b.J), lo, hi))
        if len(orc.contacts(s)[0]):
            break
        out.append(_case(state, np.clip(q0 + 0.15 * rng.normal(size=b.J), lo, hi), "approach at %.1f m/s, step %d" % (speed, t)))
    return out[::-1]          # the ones about to touch down first


def airborne_state(b, rng, lift=3.0, rate=0.0, twist=0.0):
    """the reset pose lifted by `lift` m, joints at mid-range +- 0.3 range, joint rates `rate` N(0, 1), base twist `twist` N(0, 1)"""
    om = b.om
    lo, hi = limits(om)
    st = fc.start_state(om)
    st[2] += lift + (float(b.params["floor_z"]) - defaults()["floor_z"] if "floor_z" in b.params else 0.0)
    st[13:13 + b.J] = 0.5 * (lo + hi) + 0.3 * (hi - lo) * rng.uniform(-1, 1, b.J)
    st[13 + b.J:] = rate * rng.normal(size=b.J)
    st[7:13] = twist * rng.normal(size=6)
    return st


def spinning_candidates(b, n=32, seed=0):
    """damping_*: airborne, joint rates 4 N(0, 1) rad/s, base twist 6 N(0, 1), a uniform random action (motors of the heavy joints
    at their bound: the rates then follow the forces, the link damping among them)"""
    rng = np.random.default_rng(3000 + seed)
    lo, hi = limits(b.om)
    return [_case(airborne_state(b, rng, rate=4.0, twist=6.0), rng.uniform(lo, hi), "spinning %d" % k) for k in range(n)]


def quat_roll_pitch_yaw(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def vmax_candidates(b, seed=0):
    """vmax_2, position mode, two kinds in turn:
    'rates': airborne, every joint rate +- (2.5 .. 4) rad/s - the unconstrained update exceeds the bound on most joints;
    'base': airborne, the base rolled and pitched by +- (TILT .. 0.9) rad, falling at 3 .. 5 m/s with 1 m/s sideways, every
    component of its angular velocity +- (2.5 .. 4) rad/s, joint rates 2 N(0, 1)."""
    rng = np.random.default_rng(4000 + seed)
    lo, hi = limits(b.om)
    out = []
    for k in range(24):
        if k % 2 == 0:
            st = airborne_state(b, rng, twist=0.3)
            st[13 + b.J:] = rng.choice([-1.0, 1.0], b.J) * rng.uniform(2.5, 4.0, b.J)
            out.append(_case(st, np.clip(st[13:13 + b.J] + 0.2 * rng.normal(size=b.J), lo, hi), "rates %d" % k, kind="rates"))
        else:
            st = airborne_state(b, rng, lift=4.0, rate=2.0)
            r, p = rng.choice([-1.0, 1.0], 2) * rng.uniform(TILT, 0.9, 2)
            st[3:7] = quat_roll_pitch_yaw(r, p, rng.uniform(-np.pi, np.pi))
            st[7:10] = [rng.normal(), rng.normal(), -rng.uniform(3.0, 5.0)]
            st[10:13] = rng.choice([-1.0, 1.0], 3) * rng.uniform(2.5, 4.0, 3)
            out.append(_case(st, rng.uniform(lo, hi), "base %d" % k, kind="base", roll=r, pitch=p))
    return out


def velocity_mask(J):
    m = np.zeros(J, bool)
    m[list(VEL_JOINTS)] = True
    return m


def velocity_candidates(b, seed=0):
    """vmax_2_velocity: landing and airborne states; the joints VEL_JOINTS take velocity commands of +- (2.5 .. 6) rad/s - beyond
    the bound of 2 - except one of them per case, whose command stays inside it"""
    rng = np.random.default_rng(5000 + seed)
    vel = velocity_mask(b.J)
    out = []
    for c in landing_candidates(b):
        a = c["action"].copy()
        cmd = rng.choice([-1.0, 1.0], len(VEL_JOINTS)) * rng.uniform(2.5, 6.0, len(VEL_JOINTS))
        cmd[rng.integers(len(VEL_JOINTS))] = rng.uniform(-1.5, 1.5)
        a[list(VEL_JOINTS)] = cmd
        out.append(dict(c, action=a.astype(np.float32), vel=vel, kind="velocity"))
    return out


def stop_candidates(b, seed=0):
    """erp_*: the states of tests/joint_limit_states.py made on the group's own oracle - one joint past one stop (airborne and on
    the floor, every fourth) and several joints past their stops on rollout states (every third)"""
    s1, a1 = jl.one_stop_states(b.om, b.o64)
    s2, a2, _ = jl.several_stop_states(b.om, b.o64)
    one = [_case(s, a, "one stop %d" % k) for k, (s, a) in enumerate(zip(s1, a1))][1::4]
    several = [_case(s, a, "several stops %d" % k) for k, (s, a) in enumerate(zip(s2, a2))][::3]
    out = []
    for x, y in zip(one, several):
        out += [x, y]
    return out


def synthetic_candidates(b, name, stops=0, stir=0.0, seed=0):
    """the state set of a generated model (tests/synthetic_models.py) rolled out under the group's parameters (over the default
    floor, then translated); stops: that many seeded joints put PAST (0.03 rad) a seeded stop in every state; stir: the action is
    the state's pose + stir N(0, 1) rad (the set's own action holds the start angles: the joints then hardly move, and the
    observation shows little of what the engine did)"""
    g, dz = without_floor(b)
    ss = sm.state_set(name, g.om, g.params)
    rng = np.random.default_rng(6000 + seed)
    out = []
    for k in _spread(len(ss["states"])):
        st = ss["states"][k].astype(np.float64)
        st[2] += dz
        for col in rng.choice(b.J, size=stops, replace=False):
            jl.put_on_stop(st, b.om, col, rng.integers(0, 2))
        lo, hi = limits(b.om)
        act = np.clip(st[13:13 + b.J] + stir * rng.normal(size=b.J), lo, hi) if stir else ss["actions"][k]
        out.append(_case(st, act, "%s state %d" % (name, k)))
    return out


def drop_candidates(b, name, steps=480, every=8, stir=0.3, seed=0):
    """all_moved on a generated model: the drops of its scenarios (tests/synthetic_models.py) rolled out on the group's own oracle
    for `steps` env-steps - under a third of the default step time, a third of the gravity and a falling speed bounded at 2 m/s
    the sampling steps of the model's own state set end before the floor is reached - one state every `every` steps. The action
    is the state's pose + stir N(0, 1) rad (holding the start angles the joints hardly move, and the observation shows little)."""
    g, dz = without_floor(b)
    rng = np.random.default_rng(7000 + seed)
    lo, hi = limits(b.om)
    out = []
    for i, (start, _) in enumerate(sm._scenarios(name, g.om)):
        s = g.o64.new_state()
        g.o64.set_state(s, start)
        hold = np.clip(start[13:13 + b.J], lo, hi)
        for t in range(steps):
            if t % every == 0:
                st = g.o64.get_state(s)
                st[2] += dz
                out.append(_case(st, np.clip(st[13:13 + b.J] + stir * rng.normal(size=b.J), lo, hi), "%s drop %d step %d" % (name, i, t)))
            g.o64.step(s, hold)
    return [out[k] for k in _spread(len(out))]


# ---------------------------------------------------------------- picking a group's cases
def pick(b, cands, base, n=N_CASES, condition=None, max_plain=None, moved=None):
    """-> (cases, stats). Candidates in order: without `condition` passed over; failing acceptance replaced; accepted ones are
    sensitive (the oracle `base`, the moved parameter at its default, fails against the group's, gap >= EFFECT) or plain. The
    group: sensitive ones first, at most max_plain (default n // 3) plain ones; the search stops when the group is full."""
    max_plain = n // 3 if max_plain is None else max_plain
    sens, plain = [], []
    examined = replaced = passed_over = 0
    for c in cands:
        if len(sens) + min(len(plain), max_plain) >= n:
            break
        if condition is not None and not condition(c):
            passed_over += 1
            continue
        examined += 1
        ok, r64, r32 = accept(b, c)
        if not ok:
            replaced += 1
            continue
        fails, gap = sensitivity(b, base, c, r64, r32)
        c = dict(c, gap=gap, sensitive=bool(fails and gap >= EFFECT))
        (sens if c["sensitive"] else plain).append(c)
    cases = sens[:n] + plain[:max(0, min(max_plain, n - len(sens)))]
    stats = dict(kept=len(cases), examined=examined, replaced=replaced, passed_over=passed_over, sensitive=len(sens[:n]),
                 share=replaced / max(1, examined), moved=sorted(moved or []))
    return cases, stats


def pick_mixed(b, cands, base, moved, n_contact=2 * N_CASES // 3):
    """landing + airborne: n_contact cases that touch the floor in their first env-step, the rest airborne there"""
    touches = [run(b.o64, b.om, c, steps=1)[0]["cnt"] > 0 for c in cands]
    down, s1 = pick(b, [c for c, t in zip(cands, touches) if t], base, n=n_contact, max_plain=1, moved=moved)
    up, s2 = pick(b, [c for c, t in zip(cands, touches) if not t], base, n=N_CASES - n_contact, max_plain=N_CASES - n_contact, moved=moved)
    return down + up, merged(s1, s2)


def merged(s1, s2):
    out = {k: (s1[k] + s2[k] if isinstance(s1[k], int) else s1[k]) for k in s1}
    out["share"] = out["replaced"] / max(1, out["examined"])
    return out


_CACHE = {}


def group(name, directory):
    """dict(name, built, base (the moved parameters at their defaults), cases, stats, modes (None or the control modes of the
    batch), model ('trex' or 'deep_chain')); generated once per process and name"""
    if name in _CACHE:
        return _CACHE[name]
    moved = moved_parameters()[name]
    b = built(name, moved, directory)
    base = with_defaults(b, set(moved))
    om, o64 = b.om, b.o64
    modes, extra = None, {}
    contact6 = lambda c: run(o64, om, c, steps=1)[0]["cnt"] >= 6
    if name.endswith("_deep_chain"):
        stops = 2 if name.startswith("erp") else 0
        cond = (lambda c: beyond_stop(om, c["state"]) > 0) if stops else None
        if stops:
            cases, stats = pick(b, synthetic_candidates(b, "deep_chain", stops), base, condition=cond, moved=moved)
        else:
            cases, stats = pick_mixed(b, drop_candidates(b, "deep_chain"), base, moved)
    elif name.startswith(("dt_", "substeps_", "floor_", "all_moved")) or name in ("gravity_low", "gravity_high"):
        cases, stats = pick_mixed(b, landing_candidates(b), base, moved)
    elif name == "gravity_zero":
        cands = [c for k in range(4) for c in approach_candidates(b, 2.0 + 0.5 * k, k)[:6]]
        cases, stats = pick(b, cands, base, moved=moved)
    elif name.startswith("iters_"):
        cases, stats = pick(b, landing_candidates(b), base, condition=contact6, moved=moved)
    elif name.startswith("friction_"):
        cases, stats = pick(b, landing_candidates(b, lateral=0.5), base, condition=lambda c: sliding_speed(o64, om, c) > SLIDE, moved=moved)
    elif name.startswith("erp_"):
        cases, stats = pick(b, stop_candidates(b), base, condition=lambda c: beyond_stop(om, c["state"]) > 0, moved=moved)
    elif name.startswith("cerp_"):
        cases, stats = pick(b, penetrating_candidates(b), base, condition=lambda c: c["depth"] < 0, moved=moved)
    elif name.startswith("damping_"):
        cases, stats = pick(b, spinning_candidates(b), base, moved=moved)
    elif name == "vmax_2":
        cands = vmax_candidates(b)
        rates, s1 = pick(b, [c for c in cands if c["kind"] == "rates"], base, n=N_CASES // 2, max_plain=0, moved=moved)
        basec, s2 = pick(b, [c for c in cands if c["kind"] == "base"], base, n=N_CASES // 2, max_plain=0, moved=moved,
                         condition=lambda c: frame_gap(b, c)[0] and frame_gap(b, c)[1] >= EFFECT)
        cases = rates + basec
        stats = merged(s1, s2)
    elif name == "vmax_2_velocity":
        modes = [MODE_VELOCITY if k in VEL_JOINTS else 0 for k in range(b.J)]
        cases, stats = pick(b, velocity_candidates(b), base, moved=moved)
    else:
        raise KeyError(name)
    g = dict(name=name, built=b, base=base, cases=cases, stats=stats, modes=modes, moved=moved,
             model="deep_chain" if name.endswith("_deep_chain") else "trex")
    _CACHE[name] = g
    return g


def expected(g):
    """per case, per env-step: the f64 oracle's step with the torque allowance from the f32 build; computed once"""
    if "expected" not in g:
        b = g["built"]
        exp = []
        for c in g["cases"]:
            r64, r32 = run(b.o64, b.om, c), run(b.o32, b.om, c)
            exp.append([dict(x, tau_extra=fc.tau_extra(b, x, y)) for x, y in zip(r64, r32)])
        g["expected"] = exp
    return g["expected"]


def identity_quaternion(case):
    """the case with the base quaternion replaced by identity and the same world twist: what a clamp in the base's own frame
    would be indistinguishable from"""
    st = case["state"].copy()
    st[3:7] = [0, 0, 0, 1]
    return dict(case, state=st)


def frame_gap(b, case):
    """(fails, gap) of the identity-quaternion variant against the case itself, both on the group's f64 oracle"""
    want, upright = run(b.o64, b.om, case), run(b.o64, b.om, identity_quaternion(case))
    return any(not fc.close(b, upright[i], want[i]) for i in COMPARED), rate_gap(b, upright, want)


def reset_expectation(orc, om, action):
    """on the oracle `orc`: (observation after reset, state after reset, the env-step after it under `action`)"""
    s = orc.new_state()
    obs = orc.reset(s)
    state = orc.get_state(s)
    return obs, state, env_step(orc, om, s, dict(action=action))
