"""The states of a 1000-step episode under uniform random actions - what bench.py and every training run spend their time in -
as cases for a one-step comparison of the step kernel with the CPU oracle. Generated from seeds and qualified by the oracle alone:
tests/test_episode_cases_host.py asserts on the CPU that the sample is what it claims (the T-rex lies on its side or back, the root
body and the cranium touch, the contact budget is reached, the airborne phase of the thrashing is there),
tests/test_gpu_episode_states.py feeds the same arrays to the kernels. A helper, not a conftest.

Recipe: for episode k of a group, rng = default_rng(100 + k), a fresh f64 oracle state, reset; for t in 0..999 one env-step with
lo + (hi - lo) * rng.random(25) (the joint limits in observation order); after the step, if t >= 160 and t % 20 == 0, the state
rounded to f32 is a case, and its action is one more draw from the same rng, rounded to f32. 42 cases per episode.
Groups: `hulls` (16 episodes), `hulls_domain` (16 episodes; before the reset each draws its body-mass scales U(0.8, 1.2) per body,
then its friction U(0.5, 1.25), from its rng - rounded to f32, and the trajectory runs under that domain: BASELINE config 5),
`primitives` (8 episodes, use_primitive_collision(model, 0.2, 3, 4)).
Acceptance, as in tests/feature_cases.py: on the case's one env-step the oracle's f32 build passes parity_helpers.assert_step_close
against its f64 build at loosen = 1 and the default q_atol, reward included, with the same contact count. A case that fails is
dropped; nothing is loosened.
Set aside (F32_LIMITED): an accepted state on which f32 itself is the limit - the f32 oracle passes on the state as it is and fails
on every fourth or fifth copy moved by one f32 ulp. It is kept in the group's `set_aside`, out of `cases`; test_episode_cases_host.py
proves the claim on the reference alone, and every count asserted there holds without it.
Per case: `up` = the z component of the base's up axis, `touched` = the bodies that touch in any of the step's substeps, `max_cnt` =
the largest contact count of a substep, `rate` = the largest joint rate of the state (rad/s).
multi_step(): every eighth accepted `hulls` case held for 3 env-steps, kept where feature_cases.accept passes at every env-step
(also the same touched bodies) - the candidates of feature_cases' `warm_fallen` and `wrench_fallen` groups."""
import numpy as np

import feature_cases as fc
from parity_helpers import oracle_wrench

EPISODES = dict(hulls=16, hulls_domain=16, primitives=8)
STEPS, FIRST, EVERY = 1000, 160, 20
ROOT, CRANIUM = "link_vertebrae_sacral", "link_cranium"
MULTI_EVERY = 8
# hulls, episode 12, age 401 (a toe under load two substeps before the root body lands with 3.8 kN s): one-ulp copies of the state move
# the f64 oracle's rates by up to 0.6 x the rate tolerance and the f32 oracle's by up to 1.9 x - 40 of 200 copies fail assert_step_close.
# Found by the kernel (2.1 x the tolerance, 5 x the spread of seven f32 evaluations; 0.1 .. 2.1 x over its own seven copies).
F32_LIMITED = {"hulls": ("episode 12 age 401",)}


def body(om, name):
    return om["body_names"].index(name)


def up_axis(state):
    """z component of the base's z axis; state[3:7] = the base quaternion x y z w"""
    x, y = float(state[3]), float(state[4])
    return 1.0 - 2.0 * (x * x + y * y)


def start(orc, case):
    s = orc.new_state()
    if case.get("mass_scale") is not None:
        orc.set_domain(s, case["mass_scale"].astype(np.float64), float(case["friction"]))
    orc.set_state(s, case["state"].astype(np.float64))
    return s


def step(orc, om, case):
    """the case's one env-step on an oracle build: dict(obs, rew, cnt = contact points after the step, wrench [nb, 6] = the mean
    contact wrench, touched = over all substeps, max_cnt)"""
    s = start(orc, case)
    counts = []
    w, touched = oracle_wrench(orc, om, None, case["action"].astype(np.float64), oracle_state=s, counts=counts)
    return dict(obs=orc.observe(s), rew=orc.reward(s)[0], cnt=counts[-1], wrench=w, touched=frozenset(touched), max_cnt=max(counts))


def episode(b, k, domain):
    """the candidates of episode k, in order of age"""
    om, orc = b.om, b.o64
    lo, hi = om["q_lower"][om["obs_order"]], om["q_upper"][om["obs_order"]]
    rng = np.random.default_rng(100 + k)
    s = orc.new_state()
    dom = {}
    if domain:
        dom = dict(mass_scale=rng.uniform(0.8, 1.2, b.nb).astype(np.float32), friction=np.float32(rng.uniform(0.5, 1.25)))
        orc.set_domain(s, dom["mass_scale"].astype(np.float64), float(dom["friction"]))
    orc.reset(s)
    out = []
    for t in range(STEPS):
        orc.step(s, lo + (hi - lo) * rng.random(b.J))
        if t >= FIRST and t % EVERY == 0:
            state = orc.get_state(s).astype(np.float32)
            action = (lo + (hi - lo) * rng.random(b.J)).astype(np.float32)
            out.append(dict(dom, state=state, action=action, steps=1, origin="episode %d age %d" % (k, t + 1),
                            up=up_axis(state), rate=float(np.abs(state[13 + b.J:]).max())))
    return out


def make_group(name):
    b = fc.trex(collision="primitives" if name == "primitives" else "hulls")
    cands = [c for k in range(EPISODES[name]) for c in episode(b, k, name == "hulls_domain")]
    cases, set_aside = [], []
    for c in cands:
        r64, r32 = step(b.o64, b.om, c), step(b.o32, b.om, c)
        if fc.close(b, r32, r64) and r32["cnt"] == r64["cnt"]:
            (set_aside if c["origin"] in F32_LIMITED.get(name, ()) else cases).append(
                dict(c, touched=r64["touched"], max_cnt=r64["max_cnt"], r64=r64, r32=r32))
    return dict(built=b, cases=cases, set_aside=set_aside, candidates=len(cands), root=body(b.om, ROOT), cranium=body(b.om, CRANIUM))


_CACHE = {}


def group(name):
    """dict(built, cases = the accepted ones with r64 / r32 = both oracle builds' step, candidates, root, cranium); once per process"""
    if name not in _CACHE:
        _CACHE[name] = make_group(name)
    return _CACHE[name]


def multi_step(warm, every=MULTI_EVERY):
    """-> (candidates, accepted): every `every`-th accepted hulls case with its action held for 3 env-steps at warm-start factor
    `warm`, accepted by feature_cases.accept over each env-step"""
    key = ("multi", warm, every)
    if key not in _CACHE:
        g = group("hulls")
        b = g["built"]
        cands = [dict(state=c["state"], action=c["action"], steps=3, origin=c["origin"], up=c["up"]) for c in g["cases"][::every]]
        kept = []
        for c in cands:
            ok, r64, _ = fc.accept(b, c, warm)
            if ok:
                kept.append(dict(c, in_contact=r64[0]["cnt"] > 0, touched_any=frozenset().union(*(x["touched"] for x in r64))))
        _CACHE[key] = (cands, kept)
    return _CACHE[key]


def weight(b, case):
    ms = case.get("mass_scale")
    return b.weight if ms is None else float((b.om["mass"] * ms).sum()) * fc.G


def f32_spread(o32, o, state, action, seed, setup=None):
    """the yardstick of tests/test_gpu_parity.py::test_config4_size_on_one_gpu for a state on which f32 itself is the limit: the
    largest |f32 oracle - f64 oracle| per entry of q, qd over SEVEN evaluations of the f32 build - the state as it is and six
    copies with every entry moved by about one f32 ulp. o: the f64 oracle's observation; setup(oracle, state): domain, warm start"""
    prng = np.random.default_rng(seed)
    spread = np.zeros(50)
    for k in range(7):
        s32 = o32.new_state()
        if setup is not None:
            setup(o32, s32)
        o32.set_state(s32, state.astype(np.float64) * (1.0 + (6e-8 * prng.standard_normal(state.shape) if k else 0.0)))
        spread = np.maximum(spread, np.abs(o32.step(s32, action.astype(np.float64))[0][:50] - o[:50]))
    return spread
