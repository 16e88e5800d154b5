"""The cases of the start-state tests and the comparison they share: term lists over five models - the T-rex with hulls and with
primitives, the generated models of 1 and 25 joints, the generated model whose URDF link 0 is welded to a moving body -, batch sizes
1, 2, 3 and 65, and compare(), which holds what a device run (tests/test_gpu_start_state.py) must satisfy against the reference
tests/start_state_ref.py. tests/test_start_state_cases_host.py qualifies the cases on the reference and the oracle alone.
numpy only: no torch, no device. A helper, not a conftest.

The comparison, per output of one apply on a found state:
    values, q, qd, the envs that do not start            bitwise the reference's f32 run (sums of f32 numbers in the header's order)
    base position x, y - and z without a clearance term  bitwise
    base velocities of a case without a BASE_RPY term    bitwise
    quaternion, rotated velocities, shift, base z        within the case's own bound: 4 x the largest deviation of the reference's f32
                                                         run from its f64 run over the case, in that quantity, floored at 2 ulp (f32)
                                                         of the quantity's scale - 1 for the quaternion, the largest |component| of the
                                                         reference for the others (the device's sinf, cosf and forward kinematics are
                                                         not numpy's; the factor and the floor are tests/randomize_cases.py's)
    lowest                                               equal: the qualification keeps the two lowest points further apart than the
                                                         bound of the heights
"""
import collections
import math
import os

import numpy as np

import start_state_ref as SR
from start_state_ref import (BASE_ANGULAR_VELOCITY, BASE_LINEAR_VELOCITY, BASE_POSITION, BASE_RPY, FLOOR_CLEARANCE, JOINT_POSITION,
                             JOINT_VELOCITY)

Case = collections.namedtuple("Case", "name model n terms seed env_offset")
Built = collections.namedtuple("Built", "om path params collision")
MODELS = ("trex", "trex_primitives", "slab", "bushy", "mount_first")
NJ = dict(trex=25, trex_primitives=25, slab=1, bushy=25, mount_first=4)
NB = {k: v + 1 for k, v in NJ.items()}


def bits(*elements):
    return sum(1 << i for i in elements)


def _full(nj):
    """every kind, every joint, every axis: 15 terms"""
    return [(JOINT_POSITION, 0, 0, 0, -0.2, 0.2), (JOINT_VELOCITY, 0, 0, 0, -1.0, 1.0),
            (BASE_RPY, 0, 0, 0, -0.1, 0.1), (BASE_RPY, 0, 1, 0, -0.1, 0.1), (BASE_RPY, 0, 2, 0, -math.pi, math.pi),
            (BASE_LINEAR_VELOCITY, 0, 0, 0, -0.5, 0.5), (BASE_LINEAR_VELOCITY, 0, 1, 0, -0.5, 0.5), (BASE_LINEAR_VELOCITY, 0, 2, 0, -0.2, 0.0),
            (BASE_ANGULAR_VELOCITY, 0, 0, 0, -0.5, 0.5), (BASE_ANGULAR_VELOCITY, 0, 1, 0, -0.5, 0.5), (BASE_ANGULAR_VELOCITY, 0, 2, 0, -0.5, 0.5),
            (BASE_POSITION, 0, 0, 0, -1.0, 1.0), (BASE_POSITION, 0, 1, 0, -1.0, 1.0), (BASE_POSITION, 0, 2, 0, 0.0, 0.3),
            (FLOOR_CLEARANCE, 0, 0, 0, 0.01, 0.05)]


def _plain(nj):
    """no rotation, no placement - everything bitwise: the first joint alone, a shared velocity term, lo == hi, offsets on every
    block of the base row"""
    return [(JOINT_POSITION, bits(0), 0, 0, -0.3, 0.3), (JOINT_VELOCITY, 0, 0, 1, -2.0, 2.0),
            (BASE_LINEAR_VELOCITY, 0, 0, 0, 0.25, 0.25), (BASE_ANGULAR_VELOCITY, 0, 2, 0, -1.0, 1.0),
            (BASE_POSITION, 0, 0, 0, -2.0, 2.0), (BASE_POSITION, 0, 1, 0, 0.5, 0.5), (BASE_POSITION, 0, 2, 0, 0.0, 0.1)]


def _masks(nj, last_slot):
    """the joint of the last body lane alone (wide enough to reach a joint limit), a shared term on some of the others, the first
    joint's velocity alone, yaw alone, a placement with lo == hi"""
    others = [i for i in range(nj) if i != last_slot][:7]
    terms = [(JOINT_POSITION, bits(last_slot), 0, 0, -3.0, 3.0), (JOINT_VELOCITY, bits(0), 0, 0, -1.0, 1.0),
             (BASE_RPY, 0, 2, 0, -1.0, 1.0), (FLOOR_CLEARANCE, 0, 0, 0, 0.02, 0.02)]
    if others:
        terms.insert(1, (JOINT_POSITION, bits(*others), 0, 1, -0.1, 0.1))
    return terms


def last_slot(om):
    """the observation slot of the joint of the last body lane"""
    return int(np.flatnonzero(np.asarray(om["obs_order"]) == om["nb"] - 1)[0])


def cases(built):
    """the cases over the built models {name: Built}"""
    out = []
    for name in MODELS:
        nj, ls = NJ[name], last_slot(built[name].om)
        out.append(Case(name + "_n65_full", name, 65, _full(nj), 31, 0))
        out.append(Case(name + "_n3_masks", name, 3, _masks(nj, ls), 2 ** 40 + 32, 2 ** 32 - 3))
    out += [Case("trex_n1_full", "trex", 1, _full(25), 33, 7), Case("trex_n2_full", "trex", 2, _full(25), 34, 1000),
            Case("trex_n65_plain", "trex", 65, _plain(25), 35, 0), Case("slab_n2_plain", "slab", 2, _plain(1), 36, 5),
            Case("trex_n65_masks", "trex", 65, _masks(25, last_slot(built["trex"].om)), 37, 0)]
    return out


def build(directory):
    """{name: Built} of MODELS, the generated ones written under `directory`"""
    import synthetic_models as sm
    from conftest import ASSET_URDF
    from oracle import trex_model as tm
    om = tm.compile_model(ASSET_URDF)
    out = dict(trex=Built(om, ASSET_URDF, None, "hulls"),
               trex_primitives=Built(tm.use_primitive_collision(om, 0.2, 3, 4), ASSET_URDF, None, "primitives"))
    for name in ("slab", "bushy", "mount_first"):
        d = os.path.join(str(directory), name)
        os.makedirs(d, exist_ok=True)
        path, props, m = sm.compile_both(name, d)
        out[name] = Built(m, path, props["params"], "hulls")
    return out


def oracle_of(b):
    from oracle import oracle as O
    return O.Oracle(b.om, dict(b.params or {}), precision="f64")


def found_state(b):
    """the state a plain reset leaves, on the oracle, rounded to f32: what the qualification perturbs"""
    orc = oracle_of(b)
    s = orc.new_state()
    orc.reset(s)
    return np.asarray(orc.get_state(s), np.float64).astype(np.float32)


def floor_z(b):
    return float(oracle_of(b).params["floor_z"])


def done_flags(case):
    """[n] f32 for the second apply: every third env ends its episode, beginning with env 0"""
    return (np.arange(case.n) % 3 == 0).astype(np.float32)


def reference(case, b, found, f32, second=None):
    """-> (Applied of the first apply on `found` [13 + 2J] for every env, Applied of a second apply with done_flags on the states
    `second` [n, 13 + 2J] - default: the results of the f32 run's first apply)"""
    rows = np.tile(np.asarray(found, np.float32), (case.n, 1))
    r = SR.StartState(b.om, case.n, case.terms, case.seed, case.env_offset, floor_z(b), f32=f32)
    one = r.apply(np.zeros(case.n), rows)
    if second is None:      # (the f32 run's, for either run: both perturb the same found states)
        second = one.state if f32 else SR.StartState(b.om, case.n, case.terms, case.seed, case.env_offset, floor_z(b), f32=True).apply(np.zeros(case.n), rows).state
    two = r.apply(done_flags(case), np.asarray(second, np.float32))
    return one, two


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def has(case, kind):
    return any(t[0] == kind for t in case.terms)


def quantities(case, a):
    """the bounded quantities of an Applied, over the envs that started: {name: array}"""
    f = a.first
    s = np.asarray(a.state, np.float64)[f]
    return dict(quat=s[:, 3:7], v=s[:, 7:10], w=s[:, 10:13], z=s[:, 2], shift=np.asarray(a.shift, np.float64)[f])


def bounds(a32, a64, case):
    """{name: bound} from one apply's f32 and f64 runs"""
    q32, q64 = quantities(case, a32), quantities(case, a64)
    out = {}
    for k in q64:
        scale = 1.0 if k == "quat" else max(1.0, float(np.abs(q64[k]).max(initial=0.0)))
        dev = float(np.abs(q32[k] - q64[k]).max(initial=0.0))
        out[k] = max(4.0 * dev, 2.0 * ulp32(scale))
    return out


def compare(case, a32, a64, found_rows, got_state, got_values, got_shift, got_lowest):
    """One apply against its references. found_rows [n, 13 + 2J] f32: the states the apply found; got_*: what the device left.
    (The episode counts have no accessor: they are the last counter word of every draw, so the values of an env's second episode
    are the reference's only if the count is.)
    -> dict(failures=[text], share={quantity: largest deviation / bound})"""
    fails, share = [], {}
    J, f = NJ[case.model], a32.first
    got_state = np.asarray(got_state, np.float32)
    want32 = a32.state.astype(np.float32)

    def same(x, y):
        return np.asarray(x, np.float32).tobytes() == np.asarray(y, np.float32).tobytes()
    if not same(got_values, a32.values):
        fails.append("values differ")
    if not same(got_state[~f], np.asarray(found_rows, np.float32)[~f]):
        fails.append("an env that did not start was touched")
    if not same(got_state[f][:, 13:], want32[f][:, 13:]):
        fails.append("q or qd differ")
    cols = [0, 1] + ([] if has(case, FLOOR_CLEARANCE) else [2])
    if not same(got_state[f][:, cols], want32[f][:, cols]):
        fails.append("base position differs")
    if not has(case, BASE_RPY) and not same(got_state[f][:, 3:13], want32[f][:, 3:13]):
        fails.append("quaternion or base velocities differ where nothing rotates")
    if not np.array_equal(np.asarray(got_lowest, np.int64), a64.lowest) or not np.array_equal(a32.lowest, a64.lowest):
        fails.append("lowest differs")
    got = quantities(case, SR.Applied(got_state, f, None, None, got_shift, None, None))
    want, bound = quantities(case, a64), bounds(a32, a64, case)
    for k in want:
        err = float(np.abs(got[k] - want[k]).max(initial=0.0))
        share[k] = err / bound[k]
        if err > bound[k]:
            fails.append("%s off by %.3g, bound %.3g" % (k, err, bound[k]))
    n2 = np.sqrt((np.asarray(got_state, np.float64)[:, 3:7] ** 2).sum(1))
    if np.abs(n2 - 1).max() > 4 * ulp32(1.0):
        fails.append("a quaternion is not normalised")
    return dict(failures=fails, share=share)
