"""Case groups for the step-by-step comparison of the PGS warm start and the external wrench with the CPU oracle
(oracle/trex_oracle.c restates both; include/trex_batch.h states them). Everything is generated from seeds and qualified by the
oracle alone: tests/test_oracle_features_host.py asserts the conditions below on the CPU, tests/test_gpu_feature_oracle.py feeds
the same arrays to the kernels and asserts every kept case. A helper, not a conftest.

A case = one env: an f32 state, an f32 action held for `steps` env-steps after set_state (empty record), and per group a warm-start
factor, per case an external wrench [nb, 6] and a per-body mass scale. A group = one batch (one model, one parameter set).

Acceptance (accept): at every env-step of the case the oracle's f32 build passes parity_helpers.assert_step_close against its f64
build at loosen = 1, with the same contact count and the same touched bodies. A candidate that fails is replaced by the next
candidate / seed; nothing is loosened.
Wrench magnitude: doubled from START_SHARE of the model's weight until the f64 oracle's rates with and without the wrench differ
by >= EFFECT x the qd tolerance of assert_step_close; a case in which a generalised velocity then reaches VEL_SHARE of
max_coordinate_velocity is replaced.
The groups warm_fallen and wrench_fallen start from the fallen states of tests/episode_cases.py (multi_step: every eighth accepted
case of a 1000-step random-action episode, held for 3 env-steps): the root body and the cranium on the floor, contact sets that
change from solve to solve; wrench_fallen pushes exactly those two bodies.
"""
import os

import numpy as np

import synthetic_models as sm
from conftest import ASSET_URDF
from parity_helpers import assert_step_close, oracle_wrench
from state_sets import landing_states

G = 9.81
WARM = 0.85                     # Bullet's warmstartingFactor
WARM_STEPS = (1, 2, 3)          # every warm case is compared after each of its 3 env-steps
EFFECT = 10.0                   # wrench effect on qd, in units of the qd tolerance
VEL_SHARE = 0.9
START_SHARE = 0.02
START_FLOOR = 0.395             # m: 6 mm above the lowest vertex of the T-rex's start pose (both feet inside the margin)
CONTAINED, CONTAIN_AT = 0, 2    # the env of a containment group that is contained, and the env-step at which
QD_TOL = 3e-3                   # the rate tolerance of assert_step_close, x max(1, |qd|)


# ---------------------------------------------------------------- models
class Built:
    """one model + parameter set: the oracle model dict, both oracle builds, and what TrexVecEnv needs to make the same batch"""

    def __init__(self, om, urdf, params=None, collision="hulls", tau_floor=1.0):
        from oracle import oracle as O
        self.om, self.urdf, self.params, self.collision, self.tau_floor = om, urdf, dict(params or {}), collision, tau_floor
        self.o64, self.o32 = O.Oracle(om, params=self.params), O.Oracle(om, params=self.params, precision="f32")
        self.nb, self.J = om["nb"], om["nb"] - 1
        self.max_force = float(self.o64.params["motor_max_force"])
        self.weight = float(om["mass"].sum()) * G


def trex(params=None, collision="hulls"):
    from oracle import trex_model as tm
    om = tm.compile_model(ASSET_URDF)
    if collision == "primitives":
        om = tm.use_primitive_collision(om, 0.2, 3, 4)
    return Built(om, ASSET_URDF, params, collision)


def synthetic(name, directory):
    directory = os.path.join(str(directory), name)      # one directory per model: their mesh files share names
    os.makedirs(directory, exist_ok=True)
    path, props, om = sm.compile_both(name, directory)
    return Built(om, path, props["params"], tau_floor=0.0)


# ---------------------------------------------------------------- running a case on an oracle
def start(orc, case, warm):
    s = orc.new_state()
    orc.set_warmstart(s, warm)
    if case.get("mass_scale") is not None:
        orc.set_domain(s, case["mass_scale"].astype(np.float64))
    if case.get("wrench") is not None:
        orc.set_external_wrench(s, case["wrench"].astype(np.float64))
    orc.set_state(s, case["state"].astype(np.float64))
    return s


def step(orc, om, s, action):
    """one env-step of state s, in place: dict(obs, rew, cnt, touched, wrench [nb, 6] = the mean contact wrench of the step)"""
    w, touched_any = oracle_wrench(orc, om, None, action.astype(np.float64), oracle_state=s)
    body = orc.contacts(s)[0]
    return dict(obs=orc.observe(s), rew=orc.reward(s)[0], cnt=len(body), touched=frozenset(int(b) for b in body), wrench=w,
                vmax=float(np.abs(np.delete(orc.get_state(s), np.r_[0:7, 13:13 + om["nb"] - 1])).max()))


def start_state(om):
    """the start pose at rest: where failure containment puts an env (include/trex_batch.h)"""
    J = om["nb"] - 1
    s = np.zeros(13 + 2 * J)
    s[:3], s[3:7], s[13:13 + J] = om["base_start_pos"], om["base_start_quat"], om["q_start"][om["obs_order"]]
    return s


def run(orc, om, case, warm, steps=None):
    """the case's env-steps; at step index case['contain_at'] the env is contained instead (start pose, empty record: None)"""
    s = start(orc, case, warm)
    out = []
    for i in range(case["steps"] if steps is None else steps):
        if i == case.get("contain_at", -1):
            orc.set_state(s, start_state(om))
            out.append(None)
        else:
            out.append(step(orc, om, s, case["action"]))
    return out


def tau_extra(b, r64, r32):
    """the absolute torque tolerance of a generated model (tests/test_gpu_synthetic_models.py): 3 x the f32 oracle's deviation"""
    if b.tau_floor > 0:
        return 0.0
    ot = r64["obs"][2 * b.J:]
    unsat = np.abs(ot) < 0.999 * b.max_force
    return 3.0 * np.abs(r32["obs"][2 * b.J:] - ot)[unsat].max() if unsat.any() else 0.0


def close(b, got, want, extra=0.0, what=""):
    """assert_step_close at the project's tolerances, loosen = 1, as a predicate"""
    try:
        assert_step_close(got["obs"], want["obs"], got["rew"], want["rew"], what, J=b.J, max_force=b.max_force,
                          tau_floor=b.tau_floor, tau_extra=extra)
        return True
    except AssertionError:
        return False


def accept(b, case, warm):
    """-> (ok, r64, r32): the acceptance conditions of the module docstring over every env-step of the case"""
    r64, r32 = run(b.o64, b.om, case, warm), run(b.o32, b.om, case, warm)
    ok = all(close(b, y, x, tau_extra(b, x, y)) and x["cnt"] == y["cnt"] and x["touched"] == y["touched"]
             for x, y in zip(r64, r32) if x is not None)
    return ok, r64, r32


def deviation(b, r64, r32):
    """largest f32 - f64 rate deviation over the steps, as a share of the qd tolerance"""
    return max(np.abs(y["obs"][b.J:2 * b.J] - x["obs"][b.J:2 * b.J]).max() / (QD_TOL * max(1.0, np.abs(x["obs"][b.J:2 * b.J]).max()))
               for x, y in zip(r64, r32) if x is not None)


# ---------------------------------------------------------------- candidates
def landing_candidates(b):
    """the 50 states and actions along the 300-step landing of state_sets.landing_states (one every 6 steps), on b's own oracle"""
    states, acts = landing_states(b.o64, b.om, every=6)
    return [dict(state=s, action=a, steps=3, origin="landing %d" % (6 * k)) for k, (s, a) in enumerate(zip(states, acts))]


def synthetic_candidates(b, name):
    ss = sm.state_set(name, b.om, b.params)
    return [dict(state=s, action=a, steps=3, origin="%s state %d" % (name, k)) for k, (s, a) in enumerate(zip(ss["states"], ss["actions"]))]


def discriminates(b, case, warm, r64):
    """the cold f64 oracle FAILS assert_step_close against the warm f64 oracle after the first env-step"""
    cold = run(b.o64, b.om, case, 0.0, steps=1)[0]
    return not close(b, cold, r64[0])


def pick_warm(b, cands, warm, n, n_plain=0, n_air=0):
    """accepted candidates: first those in contact on which warm and cold separate (up to n - n_plain - n_air), then in-contact
    ones on which they do not, then airborne ones; in candidate order within each class"""
    sep, plain, air = [], [], []
    for c in cands:
        ok, r64, r32 = accept(b, c, warm)
        if not ok:
            continue
        c = dict(c, in_contact=r64[0]["cnt"] > 0)
        if not c["in_contact"]:
            air.append(c)
        elif discriminates(b, c, warm, r64):
            sep.append(dict(c, separates=True))
        else:
            plain.append(c)
    out = sep[:n - n_plain - n_air]
    out += plain[:n - n_air - len(out)]
    out += air[:n - len(out)]
    assert len(out) == n, (len(sep), len(plain), len(air), n)
    return out


# ---------------------------------------------------------------- wrench cases
def wrench_effect(b, case, warm=0.0):
    """(effect in units of the qd tolerance, largest generalised velocity) of the case's wrench over its steps, f64 oracle"""
    w = run(b.o64, b.om, case, warm)
    p = run(b.o64, b.om, dict(case, wrench=None), warm)
    eff = max(np.abs(x["obs"][b.J:2 * b.J] - y["obs"][b.J:2 * b.J]).max() / (QD_TOL * max(1.0, np.abs(y["obs"][b.J:2 * b.J]).max()))
              for x, y in zip(w, p))
    return eff, max(x["vmax"] for x in w)


def scaled_wrench(b, base, shape, warm=0.0):
    """shape [nb, 6] of unit size (forces in units of the weight, torques of weight x 1 m): scaled by START_SHARE x 2^k, the
    smallest k at which the effect reaches EFFECT. -> (case, effect) or None where 2^12 is not enough or a velocity runs away"""
    vlim = VEL_SHARE * float(b.o64.params["max_coordinate_velocity"])
    for k in range(13):
        c = dict(base, wrench=(shape * (START_SHARE * 2.0 ** k * b.weight)).astype(np.float32))
        eff, vmax = wrench_effect(b, c, warm)
        if vmax >= vlim:
            return None
        if eff >= EFFECT:
            return c, eff
    return None


def make_wrench_case(b, bases, index, shape_of, seed, warm=0.0, mass=False, steps=1):
    """the first seed (seed, seed + 1000, ...) and base state (cycled from `index`) whose scaled wrench is accepted"""
    for attempt in range(8):
        rng = np.random.default_rng(seed + 1000 * attempt)
        base = dict(bases[(index + attempt) % len(bases)], steps=steps)
        if mass:
            base["mass_scale"] = rng.uniform(0.8, 1.2, b.nb).astype(np.float32)
        got = scaled_wrench(b, base, shape_of(rng), warm)
        if got is None:
            continue
        c, eff = got
        if accept(b, c, warm)[0]:
            return dict(c, effect=eff, attempt=attempt)
    raise AssertionError("no acceptable wrench case for seed %d" % seed)


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def one_hot(nb, body, sl, vec):
    w = np.zeros((nb, 6))
    w[body, sl] = vec
    return w


def random_all(b):
    share = b.om["mass"] / b.om["mass"].sum()

    def shape(rng):
        w = np.zeros((b.nb, 6))
        w[:, :3] = rng.normal(size=(b.nb, 3)) * share[:, None]
        w[:, 3:] = rng.normal(size=(b.nb, 3)) * share[:, None]
        return w
    return shape


def settle_run(orc, om, case):
    """the wrench set, then reset, then one env-step: (observation of the reset, the step)"""
    s = orc.new_state()
    orc.set_external_wrench(s, case["wrench"].astype(np.float64))
    first = orc.reset(s)
    return first, step(orc, om, s, case["action"])


def settle_close(b, got, want):
    return np.abs(got[0] - want[0]).max() <= 1e-5 and close(b, got[1], want[1]) and got[1]["cnt"] == want[1]["cnt"]


# ---------------------------------------------------------------- the groups
_CACHE = {}


def groups(directory):
    """name -> dict(built, warm, cases, kind = 'warm' | 'wrench'); generated once per process (directory: where the generated
    models' URDFs are written)"""
    if _CACHE:
        return _CACHE
    out = {}
    t = trex()
    cands = landing_candidates(t)
    # ---- warm (a): 24 landing states; (e): other factors on four of them
    a = pick_warm(t, cands, WARM, 24, n_plain=4, n_air=2)
    out["warm_trex"] = dict(built=t, warm=WARM, cases=a, kind="warm")
    for f, tag in ((1.0, "warm_factor_1.0"), (0.3, "warm_factor_0.3")):
        four = [c for c in a if c.get("separates") and accept(t, c, f)[0]][:4]
        assert len(four) == 4
        out[tag] = dict(built=t, warm=f, cases=four, kind="warm")
    # ---- warm (b): slab (one body, K = 4: the fourth point) and many_hulls
    for name, n in (("slab", 6), ("many_hulls", 6)):
        b = synthetic(name, directory)
        out["warm_" + name] = dict(built=b, warm=WARM, cases=pick_warm(b, synthetic_candidates(b, name), WARM, n), kind="warm")
    # ---- warm (c): more touching bodies than rows, one point each
    for tag, params in (("warm_max_contacts_4", dict(max_contacts=4)), ("warm_margin_0.5", dict(contact_margin=0.5))):
        b = trex(params)
        many = [c for c in cands if len(run(b.o64, b.om, c, 0.0, steps=1)[0]["touched"]) >= 4]
        out[tag] = dict(built=b, warm=WARM, cases=pick_warm(b, many, WARM, 2), kind="warm")
    # ---- warm (d): primitive collision
    b = trex(collision="primitives")
    out["warm_primitives"] = dict(built=b, warm=WARM, cases=pick_warm(b, landing_candidates(b), WARM, 4), kind="warm")

    # ---- wrench (a) - (c): 12 landing states in contact, cycled
    bases = [c for c in cands if run(t.o64, t.om, c, 0.0, steps=1)[0]["cnt"] >= 4 and accept(t, dict(c, steps=1), 0.0)[0]][:12]
    assert len(bases) == 12
    cases = []
    for body in range(t.nb):
        for k, sl in enumerate((slice(0, 3), slice(3, 6))):
            c = make_wrench_case(t, bases, len(cases), lambda rng, body=body, sl=sl: one_hot(t.nb, body, sl, unit(rng)), 100 + 2 * body + k)
            cases.append(dict(c, what="%s on body %d" % ("force" if k == 0 else "torque", body)))
    for comp in range(6):
        c = make_wrench_case(t, bases, len(cases), lambda rng, comp=comp: one_hot(t.nb, 7, comp, 1.0), 200 + comp)
        cases.append(dict(c, what="component %d of body 7" % comp))
    for k in range(6):
        c = make_wrench_case(t, bases, len(cases), random_all(t), 300 + k, mass=True)
        cases.append(dict(c, what="random wrench %d, mass scale" % k))
    out["wrench_trex"] = dict(built=t, warm=0.0, cases=cases, kind="wrench")
    # ---- wrench (d): other body counts
    for name in ("deep_chain", "bushy"):
        b = synthetic(name, directory)
        sb = [c for c in synthetic_candidates(b, name) if run(b.o64, b.om, c, 0.0, steps=1)[0]["cnt"] > 0]
        cs = [dict(make_wrench_case(b, sb, 3 * k, random_all(b), 400 + k, mass=True), what="%s random wrench %d" % (name, k)) for k in range(6)]
        out["wrench_" + name] = dict(built=b, warm=0.0, cases=cs, kind="wrench")
    # ---- wrench (e): with the warm start as well, 3 steps
    sep = [c for c in a if c.get("separates")]
    cs = [dict(make_wrench_case(t, sep, 2 * k, random_all(t), 500 + k, warm=WARM, steps=3), what="warm + random wrench %d" % k) for k in range(2)]
    out["wrench_warm"] = dict(built=t, warm=WARM, cases=cs, kind="wrench")
    # ---- warm (f), wrench (f): from the fallen states of a 1000-step episode under random actions (tests/episode_cases.py) - the
    # T-rex on its side or back, root body and cranium on the floor, contact sets that change from solve to solve
    import episode_cases as ec
    root, cranium = ec.body(t.om, ec.ROOT), ec.body(t.om, ec.CRANIUM)
    out["warm_fallen"] = dict(built=t, warm=WARM, cases=pick_warm(t, ec.multi_step(WARM)[1], WARM, 48, n_plain=8, n_air=8), kind="warm")

    def root_and_cranium(rng):
        w = one_hot(t.nb, root, slice(0, 3), unit(rng)) + one_hot(t.nb, root, slice(3, 6), 0.3 * unit(rng))
        return w + one_hot(t.nb, cranium, slice(0, 3), 0.3 * unit(rng)) + one_hot(t.nb, cranium, slice(3, 6), 0.1 * unit(rng))
    down = [c for c in ec.multi_step(0.0)[1] if c["in_contact"]]
    cs = [dict(make_wrench_case(t, down, 3 * k, root_and_cranium, 800 + k, steps=3), what="root and cranium wrench %d" % k) for k in range(12)]
    out["wrench_fallen"] = dict(built=t, warm=0.0, cases=cs, kind="wrench")
    # ---- containment through set_state: the f64 oracle's state after one warm step, rounded to f32, set again (which empties
    # every record) with env CONTAINED's state made non-finite by the test: that env continues from the oracle's reset
    after = []
    for c in sep:
        s = start(t.o64, c, WARM)
        step(t.o64, t.om, s, c["action"])
        c1 = dict(c, state=t.o64.get_state(s).astype(np.float32), origin=c["origin"] + " + 1 step")
        if accept(t, c1, WARM)[0]:
            after.append(dict(c1, before=c["state"]))
    assert len(after) >= 6
    out["contained_set_state"] = dict(built=t, warm=WARM, cases=after[:6], kind="contained")
    # ---- containment with a populated record (a non-finite wrench at step CONTAIN_AT): the floor raised to the feet of the
    # start pose, so that the contained env's next solve meets the vertices of its last record
    b = trex(dict(floor_z=START_FLOOR))
    rng = np.random.default_rng(600)
    q0, lo, hi = b.om["q_start"][b.om["obs_order"]], b.om["q_lower"][b.om["obs_order"]], b.om["q_upper"][b.om["obs_order"]]
    cs = []
    while len(cs) < 4:
        st = start_state(b.om)
        st[13:13 + b.J] = np.clip(q0 + 0.02 * rng.normal(size=b.J), lo, hi)
        c = dict(state=st.astype(np.float32), action=np.clip(q0 + 0.1 * rng.normal(size=b.J), lo, hi).astype(np.float32), steps=5,
                 origin="start pose on the raised floor %d" % len(cs))
        if len(cs) == CONTAINED:
            c["contain_at"] = CONTAIN_AT
        if accept(b, c, WARM)[0]:
            cs.append(c)
    out["contained_wrench"] = dict(built=b, warm=WARM, cases=cs, kind="contained")
    # ---- the settle substep under a wrench: reset (which must not feel it), then one forced step
    s = t.o64.new_state()
    t.o64.reset(s)
    q0, lo, hi = t.om["q_start"][t.om["obs_order"]], t.om["q_lower"][t.om["obs_order"]], t.om["q_upper"][t.om["obs_order"]]
    rng = np.random.default_rng(700)
    base = [dict(state=t.o64.get_state(s).astype(np.float32), action=np.clip(q0 + 0.1 * rng.normal(size=t.J), lo, hi).astype(np.float32),
                 steps=1, origin="after reset") for _ in range(4)]
    cs = [make_wrench_case(t, base, k, random_all(t), 700 + k) for k in range(4)]
    assert all(settle_close(t, settle_run(t.o32, t.om, c), settle_run(t.o64, t.om, c)) for c in cs)
    out["settle_wrench"] = dict(built=t, warm=0.0, cases=cs, kind="settle")
    _CACHE.update(out)
    return _CACHE


def expected(group):
    """per case, per env-step: the f64 oracle's step, the f32 oracle's contact wrench and the torque allowance; computed once"""
    if "expected" not in group:
        b = group["built"]
        exp = []
        for c in group["cases"]:
            r64, r32 = run(b.o64, b.om, c, group["warm"]), run(b.o32, b.om, c, group["warm"])
            exp.append([None if x is None else dict(x, wrench32=y["wrench"], tau_extra=tau_extra(b, x, y)) for x, y in zip(r64, r32)])
        group["expected"] = exp
    return group["expected"]
