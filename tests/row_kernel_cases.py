"""Cases for the observation, reward and motion kernels on the generated models (tests/synthetic_models.py): specifications that
name every kind, the clip, the states - for an oracle model dict of any joint count - and the mistaken variants of the references
that tests/test_row_kernel_cases_host.py separates from the right ones. numpy and the CPU oracle only, no torch and no device: the
host test and tests/test_gpu_row_kernels_models.py take the same cases from here. A helper, not a conftest.

Specifications are those of the references: observation_ref (kind, link, xyz, scale), reward_ref (kind, link, mask, xyz, weight, p0,
p1), motion_ref (kind, mask, weight, scale, aux)."""
import numpy as np

import motion_ref as MR
import observation_ref as OR
import reward_ref as RR
import state_sets
import synthetic_models as sm

MODELS = ("deep_chain", "bushy", "slab", "mount_first")       # J = 6 | J = 25, six merged links | J = 1 | URDF link 0 in body 2
N = 9                                                         # one full 8-env workgroup and a ragged slot
Z = (0.0, 0.0, 0.0)
DT = 1.0 / 32.0                                               # the clip's frame time: exact in f32, and so is every knot
FRAMES = 7
OTHER_PARAMS = dict(dt=1.0 / 200.0, substeps=3, floor_z=0.05)  # not the defaults: Ts = 0.015 s, the floor 5 cm up
FORCE_MIN = 0.5                                               # N: the contact kinds' threshold on the sensor's force


def params_of(props, other=False):
    return dict(props["params"], **(OTHER_PARAMS if other else {}))


# ---------------------------------------------------------------- links
def links_of(om):
    """dict(deepest=, merged=): the first link of the deepest body; the last link that is not its body's own - one merged into the
    body across a fixed joint - and whose link_tf is turned, or None"""
    lb = np.asarray(om["link_body"], int)
    tf = np.asarray(om["link_tf"], np.float64).reshape(-1, 12)
    names, bodies = list(om["link_names"]), list(om["body_names"])
    deepest = [l for l in range(len(lb)) if lb[l] == int(np.argmax(om["depth"]))][0]
    merged = [l for l in range(len(lb)) if names[l] != bodies[lb[l]] and np.abs(tf[l][:9] - np.eye(3).reshape(-1)).max() > 1e-3]
    merged = [l for l in merged if lb[l] > 0] or merged                     # on a moving body where there is one
    return dict(deepest=deepest, merged=merged[-1] if merged else None)


def link_of_body(om, body):
    """the last URDF link that belongs to `body`"""
    return [l for l, b in enumerate(om["link_body"]) if int(b) == int(body)][-1]


# ---------------------------------------------------------------- states
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def oracle_of(name, om, params):
    from oracle import oracle as O
    return _cached(("orc", name, tuple(sorted(params.items()))), lambda: O.Oracle(om, params=params))


def states(name, om, params, n=N):
    """-> (states [n, 13 + 2J] f32-exact f64, actions [n, J] f32): even entries from synthetic_models.state_set - landing, rest,
    touching: five spread over the set from its end -, odd entries from state_sets.query_states - airborne. The action of a
    state holds its joint angles. Read-only; computed once per model and parameter set."""
    def make():
        J = om["nb"] - 1
        ss = sm.state_set(name, om, params)
        k = (n + 1) // 2
        idx = np.round(np.linspace(len(ss["states"]) - 1, 0, k)).astype(int)
        air = state_sets.query_states(om)
        lo, hi = om["q_lower"][om["obs_order"]], om["q_upper"][om["obs_order"]]
        st, act = [], []
        for e in range(n):
            if e % 2 == 0:
                st.append(ss["states"][idx[e // 2]].astype(np.float64))
                act.append(ss["actions"][idx[e // 2]])
            else:
                st.append(np.asarray(air[e // 2], np.float64))
                act.append(np.clip(air[e // 2][13:13 + J], lo, hi).astype(np.float32))
        st, act = np.array(st), np.array(act, np.float32)
        st.setflags(write=False)
        act.setflags(write=False)
        return st, act
    return _cached(("states", name, n, tuple(sorted(params.items()))), make)


def touching(name, om, params, n=N):
    """per case state, the set of bodies in Oracle.contacts with a positive normal impulse after one env-step under its action"""
    def make():
        orc = oracle_of(name, om, params)
        out = []
        for s, a in zip(*states(name, om, params, n)):
            body, lam, _, _ = sm.oracle_step_contacts(orc, s, a)[2]
            out.append(sorted(set(body[lam[:, 0] > 0].tolist())))
        return out
    return _cached(("touching", name, n, tuple(sorted(params.items()))), make)


WILD_STEPS = 3


def wild_inputs(n, J, step):
    """(actions [n, J] f32 well outside the joint limits, commands [n, 3] f32) of step `step` of the reward test"""
    rng = np.random.default_rng(700 + step)
    return (3.0 * rng.normal(size=(n, J))).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


def touching_wild(name, om, params, n=N):
    """[step][env] the bodies in Oracle.contacts with a positive normal impulse along WILD_STEPS env-steps from the case states
    under wild_inputs: what the reward test runs"""
    def make():
        orc = oracle_of(name, om, params)
        held = []
        for s0 in states(name, om, params, n)[0]:
            s = orc.new_state()
            orc.set_state(s, s0)
            orc.set_motors_on(s, 1)
            held.append(s)
        out = []
        for t in range(WILD_STEPS):
            a = wild_inputs(n, om["nb"] - 1, t)[0].astype(np.float64)
            row = []
            for e, s in enumerate(held):
                orc.step(s, a[e])
                body, lam, _, _ = orc.contacts(s)
                row.append(sorted(set(body[lam[:, 0] > 0].tolist())))
            out.append(row)
        return out
    return _cached(("wild", name, n, tuple(sorted(params.items()))), make)


def touch_link(name, om, params, n=N):
    """the last link of a moving body that touches the floor both in the case states (one step under the holding action: the
    observation test) and along the reward test's wild steps - the body that does so most often"""
    hold, wild = np.zeros(om["nb"], int), np.zeros(om["nb"], int)
    for bodies in touching(name, om, params, n):
        hold[bodies] += 1
    for row in touching_wild(name, om, params, n):
        for bodies in row:
            wild[bodies] += 1
    both = np.minimum(hold, wild)
    body = int(np.argmax(both[1:])) + 1
    assert both[body] > 0, (name, hold, wild)
    return link_of_body(om, body)


# ---------------------------------------------------------------- observation channels
def obs_spec(om, touch):
    """every channel kind: position, velocity and height of a point on URDF link 0, on the deepest link and - where the model has
    one - on a link merged across a fixed joint with a turned link_tf; the contact force of `touch`'s body; scales that are not
    1; two EXTERNAL channels that split the caller's columns"""
    ln = links_of(om)
    p, r = (0.1, -0.2, 0.3), (0.05, 0.0, -0.02)
    spec = [(OR.GRAVITY, 0, Z, 1.5), (OR.EXTERNAL, 3, Z, 1.0), (OR.BASE_LIN, 0, Z, 0.5), (OR.BASE_ANG, 0, Z, -0.25),
            (OR.BASE_HEIGHT, 0, Z, 2.0), (OR.POINT_POS, 0, p, 1.0), (OR.POINT_VEL, 0, p, 2.0), (OR.POINT_HEIGHT, 0, p, -1.0),
            (OR.CONTACT, touch, Z, 0.125), (OR.PREV_ACTION, 0, Z, 1.0), (OR.POINT_POS, ln["deepest"], r, -3.0),
            (OR.POINT_VEL, ln["deepest"], Z, 1.0), (OR.POINT_HEIGHT, ln["deepest"], r, 1.0)]
    if ln["merged"] is not None:
        m = ln["merged"]
        spec += [(OR.POINT_POS, m, r, 0.75), (OR.POINT_VEL, m, p, 1.0), (OR.POINT_HEIGHT, m, p, 1.0)]
    return spec + [(OR.EXTERNAL, 4, Z, 1.0)]


# ---------------------------------------------------------------- reward terms
def rterm(kind, weight=1.0, link=0, mask=0, xyz=Z, p0=0.0, p1=0.0):
    return (kind, link, mask, xyz, weight, p0, p1)


def reward_spec(om, touch):
    """T = 32: the 19 kinds in kind order, weights that are not 1, the point on the merged (or the deepest) link, the contact kinds
    on `touch`'s body; then the six joint sums with the mask of joint 0 alone and of joint J - 1 alone, and CONTACT_COUNT on
    that one body"""
    nb, J = om["nb"], om["nb"] - 1
    ln = links_of(om)
    pt = ln["merged"] if ln["merged"] is not None else ln["deepest"]
    first, last = 1, 1 << (J - 1)
    tb = int(om["link_body"][touch])
    spec = [rterm(RR.STEP, 0.75), rterm(RR.ALIVE, 2.0), rterm(RR.TRACK_LIN, 1.5, p0=0.25), rterm(RR.TRACK_ANG, 0.5, p0=0.5),
            rterm(RR.LIN_VEL_Z, -2.0), rterm(RR.ANG_VEL_XY, -0.05), rterm(RR.ORIENTATION, -1.0), rterm(RR.BASE_HEIGHT, -1.0, p0=0.6),
            rterm(RR.POINT_HEIGHT, 1.5, link=pt, xyz=(0.1, -0.2, 0.3), p0=0.1), rterm(RR.TORQUE, -1e-4), rterm(RR.JOINT_VEL, -1e-3),
            rterm(RR.JOINT_ACC, -2.5e-7), rterm(RR.ACTION_RATE, -0.01), rterm(RR.JOINT_LIMIT, -1.0, p0=0.5), rterm(RR.POWER, -1e-3),
            rterm(RR.JOINT_POSE, -0.1), rterm(RR.CONTACT_COUNT, -1.0, mask=(1 << nb) - 2, p0=FORCE_MIN),
            rterm(RR.FOOT_AIR_TIME, 1.25, link=touch, p0=FORCE_MIN, p1=0.005),
            rterm(RR.FOOT_SLIP, -0.1, link=touch, xyz=(0.05, 0.0, -0.02), p0=FORCE_MIN)]
    for kind, w, p0 in ((RR.TORQUE, -1e-4, 0.0), (RR.JOINT_VEL, -1e-3, 0.0), (RR.JOINT_ACC, -2.5e-7, 0.0), (RR.JOINT_LIMIT, -1.0, 0.3),
                        (RR.POWER, -1e-3, 0.0), (RR.JOINT_POSE, -0.1, 0.0)):
        spec += [rterm(kind, w, mask=first, p0=p0), rterm(kind, w, mask=last, p0=p0)]
    spec.append(rterm(RR.CONTACT_COUNT, 0.5, mask=1 << tb, p0=FORCE_MIN))
    assert len(spec) == RR.MAX_TERMS and [s[0] for s in spec[:RR.KINDS]] == list(range(RR.KINDS))
    return spec


# ---------------------------------------------------------------- the clip and its terms
def clip(om, orc):
    """-> (frames [7, 7 + J], velocities [7, 6 + J]): seven successive states of an oracle rollout of the model - a drop from
    30 cm under actions that swing the joints -, the joint angles clipped into the limits trex_batch_set_motion asks for"""
    J = om["nb"] - 1
    oo = om["obs_order"]
    lo, hi = om["q_lower"][oo], om["q_upper"][oo]
    rng = np.random.default_rng(404)
    q0 = np.zeros(om["nb"])
    q0[1:] = rng.uniform(0.6 * om["q_lower"][1:], 0.6 * om["q_upper"][1:])
    start = sm.flat_state(om, 0.3, q0, quat=(np.sin(0.15), 0.0, 0.0, np.cos(0.15)), v=(0.4, -0.2, 0.0), w=(0.3, 0.6, -0.5))
    start[13 + J:] = rng.normal(size=J)
    s = orc.new_state()
    orc.set_state(s, start)
    orc.set_motors_on(s, 1)
    frames, vel = [], []
    for k in range(FRAMES):
        x = orc.get_state(s)
        frames.append(np.concatenate([x[:7], np.clip(x[13:13 + J], lo, hi)]))
        vel.append(np.concatenate([x[7:13], x[13 + J:]]))
        orc.step(s, rng.uniform(lo, hi))
    return np.array(frames), np.array(vel)


def end_effectors(om, K=8):
    """(links [K], points [K, 3]), K = min(8, links): URDF link 0 itself, a merged link where there is one, the deepest link, then
    the others; points off the link origins"""
    ln = links_of(om)
    nl = len(om["link_names"])
    first = [0] + ([ln["merged"]] if ln["merged"] not in (None, 0) else []) + [ln["deepest"]]
    first = list(dict.fromkeys(first))
    links = (first + [l for l in range(nl) if l not in first])[:min(K, nl)]
    pts = np.random.default_rng(77).uniform(-0.2, 0.2, (len(links), 3))
    return links, pts


def motion_spec(om):
    """every kind, then POSE and VELOCITY with the masks of joint 0 alone and of joint J - 1 alone; scales at which a state a
    radian or a metre off the clip still earns a value well above the smallest f32"""
    J = om["nb"] - 1
    last = 1 << (J - 1)
    return [(MR.POSE, 0, 0.65, 2.0 / J, 0.0), (MR.VELOCITY, 0, 0.1, 0.1 / J, 0.0), (MR.END_EFFECTOR, 0, 0.15, 1.0, 0.0),
            (MR.ROOT_POSE, 0, 0.1, 0.03, 0.5), (MR.ROOT_VELOCITY, 0, -0.25, 0.05, 0.5), (MR.POSE, 1, 1.0, 0.5, 0.0),
            (MR.VELOCITY, last, 2.0, 0.01, 0.0), (MR.POSE, last, 0.3, 1.0, 0.0)]


def time_list(n, T, dt=DT, F=FRAMES):
    """knots (exact in f32), mid-segment times, 0, T, beyond T, negative: env e takes entry e"""
    rng = np.random.default_rng(n)
    base = np.concatenate([[2 * dt, 0.37 * T, 0.0, T, 1.7 * T, -0.3, (F - 2) * dt, T - 1e-6], rng.uniform(0, T, max(n - 8, 0))])
    return base[:n].astype(np.float32)


# ---------------------------------------------------------------- the lift-off and the landing
def air_time_case(name, om, params, window=10):
    """A stretch of the model's tumbling drop in which one moving body stands on the floor, leaves it and lands again within
    `window` env-steps, by Oracle.contacts: dict(state = the state before the first of those steps, action, body, steps = how
    many to run, touch = per step whether the body touches)."""
    def make():
        orc = oracle_of(name, om, params)
        J = om["nb"] - 1
        start = sm._scenarios(name, om)[0][0]
        lo, hi = om["q_lower"][om["obs_order"]], om["q_upper"][om["obs_order"]]
        a = np.clip(start[13:13 + J], lo, hi)
        s = orc.new_state()
        orc.set_state(s, start)
        orc.set_motors_on(s, 1)
        sts, touch = [], []
        for t in range(120):
            sts.append(orc.get_state(s).astype(np.float32).astype(np.float64))
            orc.step(s, a)
            body, lam, _, _ = orc.contacts(s)
            touch.append(set(body[lam[:, 0] > 0].tolist()))
        for t0 in range(len(sts)):
            for b in range(1, om["nb"]):
                if b not in touch[t0] or t0 + 1 >= len(sts) or b in touch[t0 + 1]:
                    continue
                for t1 in range(t0 + 2, min(t0 + window, len(sts))):
                    if b in touch[t1]:
                        return dict(state=sts[t0], action=a.astype(np.float32), body=b, steps=t1 - t0 + 1,
                                    touch=[b in touch[t] for t in range(t0, t1 + 1)])
        raise AssertionError("no body of %s lifts off and lands again within %d steps" % (name, window))
    return _cached(("air", name, window, tuple(sorted(params.items()))), make)


def episode_plan(n, limit=2, steps=5):
    """[steps, n] bool: the done rows of `steps` launches when env e starts with an episode count of e % limit and an episode
    ends with the step that brings its count to `limit`"""
    count = np.arange(n) % limit
    done = np.zeros((steps, n), bool)
    for t in range(steps):
        count = count + 1
        done[t] = count >= limit
        count[done[t]] = 0
    return done


# ---------------------------------------------------------------- the mistaken variants
def rows_of(om, sts, reward=0.25):
    """[n, 3J + 2] rows as a step would leave them for these states: q | qd | torque (a fixed pattern) | reward | done = 0"""
    J = om["nb"] - 1
    sts = np.asarray(sts, np.float64)
    tau = 3.0 * np.sin(1.0 + np.arange(len(sts) * J)).reshape(len(sts), J)
    return np.concatenate([sts[:, 13:13 + J], sts[:, 13 + J:], tau, np.full((len(sts), 1), reward), np.zeros((len(sts), 1))], 1).astype(np.float32)


def root_axes_variant(om):
    """'the base axes are body 0's': the model with one more link in front - the root body's own frame - which the references then
    take for URDF link 0. -> (model, shift): every link index of a specification moves up by `shift` = 1."""
    vm = dict(om)
    vm["link_body"] = np.concatenate([[0], np.asarray(om["link_body"], int)])
    vm["link_tf"] = np.concatenate([np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])[None],
                                    np.asarray(om["link_tf"], np.float64).reshape(-1, 12)])
    vm["link_names"] = ["root_axes"] + list(om["link_names"])
    return vm, 1


def shift_obs(spec, shift):
    return [(k, l + shift if k in (OR.POINT_POS, OR.POINT_VEL, OR.POINT_HEIGHT, OR.CONTACT) else l, x, s) for k, l, x, s in spec]


def shift_rew(spec, shift):
    return [(k, l + shift if k in (RR.POINT_HEIGHT, RR.FOOT_AIR_TIME, RR.FOOT_SLIP) else l, m, x, w, a, b) for k, l, m, x, w, a, b in spec]


def body_order_variant(om):
    """'joint columns in body order': the model whose observation order is the body order"""
    vm = dict(om)
    vm["obs_order"] = np.arange(1, om["nb"], dtype=np.asarray(om["obs_order"]).dtype)
    return vm


def body_order_table(om, tab):
    """the clip's table with its joint columns (angles and rates) moved into body order: what a reference pose scattered without
    obs_slot would be"""
    J = om["nb"] - 1
    oo = np.asarray(om["obs_order"], int)
    slot = np.zeros(om["nb"], int)
    slot[oo] = np.arange(J)
    rows = tab["rows"].copy()
    # column j of the variant holds what the right table holds for the joint of body j + 1
    rows[:, 13:13 + J] = tab["rows"][:, 13 + slot[1:]]
    rows[:, 13 + J:13 + 2 * J] = tab["rows"][:, 13 + J + slot[1:]]
    return dict(tab, rows=rows)
