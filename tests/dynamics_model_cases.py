"""Cases for the first four dynamics queries (trex_batch_inverse_dynamics / _mass_matrix / _jacobian / _centroidal) on the generated
models of tests/synthetic_models.py: the states, the metrics of tests/test_gpu_dynamics.py, bounds that come from the reference
alone, the structure the outputs must have exactly, identities that tie the queries to each other, and four deliberate model
mistakes that tests/test_dynamics_model_cases_host.py separates from the right model. numpy and the CPU oracle only, no torch and
no device: the host test, tests/test_gpu_dynamics_models.py and scripts/dynamics_bench.py take the same cases from here. A
helper, not a conftest.

Models (MODELS): deep_chain - depth 6, oblique axes that are no unit vectors, D = 12; bushy - 26 bodies, four moving children on
the base and on a body at depth 2, six welded links with moved and turned frames, a scattered observation order, D = 31;
mount_first - URDF link 0 welded into body 2 at depth 2 behind a turned frame, a side branch, D = 10; slab - two bodies, D = 7.

States: dynamics_ref.random_states(om, 12, seed=31) - the states of state_sets.query_states with their mass scales kept; the last
two carry a per-body mass scale. Twelve states are three full workgroups of the kernel.

Outputs: every function here works on a dict of numpy arrays, whoever made them - the f64 reference, its f32 run, a mistaken model
or the device:  id_zero [n, D], id_acc [n, D] (inverse dynamics of the round trip's accelerations), mass [n, D, D],
jac [n, L, 2, 6, D] (every URDF link at the points POINTS), cent [n, 16], vel [n, L, 2, 3] (the world velocity of those points).

Bounds: for model m and metric k, bound = min(CAPS[k], max(TOL[k], 4 x d32[m][k])), d32 the largest deviation of the reference's
f32 run (dynamics_ref, dtype=float32) from its f64 run over the model's 12 states, in the metric itself. The f32 run has the
kernel's arithmetic width and takes no care over cancellation - it keeps world positions at z = 4 .. 6 m where the kernel refers
everything to the base origin -, so a correct kernel sits at or under it; 4 is the project's margin for another summation order;
TOL (what the T-rex needs) is a floor, so that a model on which the f32 run is lucky sets no tighter bound than the T-rex does.
d32 is computed when a test runs, from the reference alone; no table of it is kept, and no figure of the device enters.

Identities (no reference in them; f64 arithmetic on one set of outputs):
  id_mass    ID(a) - ID(0) = M a: the residual as a generalised force, base rows over the largest base entry of ID(0), joint rows
             over the largest joint entry of ID(a) - the scales of the round trip, from the outputs themselves;
  cent_mass  with gv the state's own generalised velocity: M[0:3] gv is the linear momentum, M[3:6] gv the angular momentum about
             the base origin (the query's, about the COM, + (com - base) x p), 0.5 gv M gv the kinetic energy; each over its
             magnitude, the momenta floored at 1 % of mass x 1 m/s (x 1 m), as in cent_dev;
  jac_vel    J(link, p)[0:3] gv is the linear velocity the link-state query gives for that link and point; over max(1, the env's
             largest velocity entry), the scale of tests/test_gpu_link_state.py.
Their bounds follow the same rule: 4 x the residual of the f32 run's own outputs in the identity, floored at the loosest TOL of
the metrics involved and capped at the loosest of their caps (IDENTITY_METRICS; jac_vel also involves the link-state velocity).
"""
import numpy as np

import dynamics_ref as R
from state_sets import oracle_state
from tolerances import DYNAMICS_CAPS, DYNAMICS_TOL, LINK_CAPS, LINK_TOL

MODELS = ("deep_chain", "bushy", "mount_first", "slab")
N = 12
G = 9.81
POINTS = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1))
METRICS = ("id_zero", "id_roundtrip", "mass", "jac", "cent")
IDENTITIES = ("id_mass", "cent_mass", "jac_vel")
IDENTITY_METRICS = dict(id_mass=("id_zero", "id_roundtrip", "mass"), cent_mass=("mass", "cent"), jac_vel=("jac",))


def cent_dev(got, want):
    """largest relative deviation over the centroidal quantities: per quantity over its magnitude, the COM floored at 1 m, the
    momenta (and the COM velocity) at 1 % of mass x 1 m/s (x 1 m for the angular one)"""
    m = want[14]
    parts = [(slice(0, 3), max(np.abs(want[0:3]).max(), 1.0)), (slice(3, 6), max(np.abs(want[3:6]).max(), 0.01)),
             (slice(6, 9), max(np.abs(want[6:9]).max(), 0.01 * m)), (slice(9, 12), max(np.abs(want[9:12]).max(), 0.01 * m)),
             (slice(12, 13), max(abs(want[12]), 0.01 * m)), (slice(13, 14), abs(want[13])), (slice(14, 15), m)]
    return max(np.abs(got[sl] - want[sl]).max() / sc for sl, sc in parts)


# ---------------------------------------------------------------- states and the round trip's accelerations
def states(om, n=N):
    """[(state f32-exact f64, mass scale or None)] x n"""
    return list(zip(*R.random_states(om, n, seed=31)))


def oracle_of(m):
    """the f64 oracle of the built model m = dict(path=, props=, om=), under the engine parameters the model is stepped with"""
    from oracle import oracle as O
    return O.Oracle(m["om"], params=m["props"]["params"])


def round_trip(om, orc, cases):
    """(tau [n, J], accel f32 [n, D], accel f64 [n, D], drawn [n, D]): random joint torques of dynamics_ref.random_tau - every joint
    accelerates within 10 rad/s^2 - and the accelerations the model's own f64 oracle answers them with (forward_dynamics, no
    damping), in the order of the queries, rounded to f32 as the device takes them and as they came; `drawn` are the
    accelerations random_tau drew the torques from"""
    rng = np.random.default_rng(3)
    taus, acc, drawn = [], [], []
    for s, ms in cases:
        tau, a = R.random_tau(om, s, ms, rng, with_accel=True)
        qdd, ba = orc.forward_dynamics(oracle_state(orc, s, ms), tau, with_damping=False)
        taus.append(tau)
        acc.append(np.concatenate([ba[3:6], ba[0:3], qdd]))
        drawn.append(a)
    return np.array(taus), np.array(acc).astype(np.float32), np.array(acc), np.array(drawn)


def gen_velocity(om, s):
    J = om["nb"] - 1
    return np.concatenate([s[7:13], s[13 + J:13 + 2 * J]])


# ---------------------------------------------------------------- outputs of the reference
def reference_outputs(om, cases, acc, dtype=np.float64):
    """the outputs dict (module docstring) of dynamics_ref run in `dtype`; an f32 run is asserted to return float32 throughout"""
    nl = len(om["link_names"])
    out = dict(id_zero=[], id_acc=[], mass=[], jac=[], cent=[], vel=[])
    for (s, ms), a in zip(cases, acc):
        out["id_zero"].append(R.inverse_dynamics(om, s, None, ms, G, dtype))
        out["id_acc"].append(R.inverse_dynamics(om, s, a, ms, G, dtype))
        out["mass"].append(R.mass_matrix(om, s, ms, dtype))
        kin = R.Kin(om, s, None, dtype)                  # (kinematics: shared by the links, no mass scale in it)
        out["jac"].append(np.array([[R.jacobian(om, s, l, p, dtype, kin) for p in POINTS] for l in range(nl)]))
        out["cent"].append(R.centroidal(om, s, ms, G, dtype))
        out["vel"].append(np.array([[R.point_velocity(om, s, l, p, dtype, kin) for p in POINTS] for l in range(nl)]))
    out = {k: np.array(v) for k, v in out.items()}
    assert all(v.dtype == np.dtype(dtype) for v in out.values()), {k: v.dtype for k, v in out.items()}
    return out


# ---------------------------------------------------------------- the metrics
def metric_devs(taus, got, ref, round_trip_of_ref=False):
    """{metric: the largest deviation over the envs} of the outputs `got` from the f64 reference outputs `ref`, in the metrics of
    tests/test_gpu_dynamics.py: id_zero and id_roundtrip per block (dynamics_ref.block_dev), the round trip against [0, tau]
    itself (round_trip_of_ref: against the reference's own answer to the same accelerations - how far a changed model moves it,
    exactly 0 where it does not); mass |dM_ij| / sqrt(M_ii M_jj); jac absolute over the largest entry, every link and both
    points; cent cent_dev"""
    dev = dict.fromkeys(METRICS, 0.0)
    f8 = lambda x: np.asarray(x, np.float64)
    for e in range(len(taus)):
        h = ref["id_zero"][e]
        dev["id_zero"] = max(dev["id_zero"], R.block_dev(got["id_zero"][e], h, np.abs(h[:6]).max(), np.abs(h[6:]).max()))
        want = ref["id_acc"][e] if round_trip_of_ref else np.concatenate([np.zeros(6), taus[e]])
        dev["id_roundtrip"] = max(dev["id_roundtrip"], R.block_dev(got["id_acc"][e], want, np.abs(h[:6]).max(), np.abs(taus[e]).max()))
        dg = np.sqrt(np.diag(ref["mass"][e]))
        dev["mass"] = max(dev["mass"], (np.abs(f8(got["mass"][e]) - ref["mass"][e]) / np.outer(dg, dg)).max())
        Jr = ref["jac"][e]
        scale = np.abs(Jr).max(axis=(2, 3), keepdims=True)
        dev["jac"] = max(dev["jac"], (np.abs(f8(got["jac"][e]) - Jr) / scale).max())
        dev["cent"] = max(dev["cent"], cent_dev(f8(got["cent"][e]), ref["cent"][e]))
    return dev


def bounds(d32):
    return {k: min(DYNAMICS_CAPS[k], max(DYNAMICS_TOL[k], 4 * d32[k])) for k in METRICS}


# ---------------------------------------------------------------- the identities
def identity_devs(om, cases, acc, out):
    """{identity: the largest residual over the envs} of one set of outputs, f64 arithmetic on them (module docstring)"""
    dev = dict.fromkeys(IDENTITIES, 0.0)
    for e, (s, _) in enumerate(cases):
        o = {k: np.asarray(v[e], np.float64) for k, v in out.items()}
        gv, M, c = gen_velocity(om, s), o["mass"], o["cent"]
        r = o["id_acc"] - o["id_zero"] - M @ np.asarray(acc[e], np.float64)
        dev["id_mass"] = max(dev["id_mass"], R.block_dev(r, np.zeros(len(r)), np.abs(o["id_zero"][:6]).max(), np.abs(o["id_acc"][6:]).max()))
        m, p, Lc, ke = c[14], c[6:9], c[9:12], c[12]
        Lb = Lc + np.cross(c[0:3] - s[0:3], p)
        parts = [np.abs(M[0:3] @ gv - p).max() / max(np.abs(p).max(), 0.01 * m),
                 np.abs(M[3:6] @ gv - Lb).max() / max(np.abs(Lb).max(), 0.01 * m), abs(0.5 * gv @ M @ gv - ke) / max(abs(ke), 0.01 * m)]
        dev["cent_mass"] = max(dev["cent_mass"], max(parts))
        v = o["vel"]
        dev["jac_vel"] = max(dev["jac_vel"], np.abs(o["jac"][:, :, 0:3, :] @ gv - v).max() / max(1.0, np.abs(v).max()))
    return dev


def identity_bounds(res32):
    out = {}
    for k, ms in IDENTITY_METRICS.items():
        tols = [DYNAMICS_TOL[m] for m in ms] + ([LINK_TOL["velocity"]] if k == "jac_vel" else [])
        caps = [DYNAMICS_CAPS[m] for m in ms] + ([LINK_CAPS["velocity"]] if k == "jac_vel" else [])
        out[k] = min(max(caps), max(max(tols), 4 * res32[k]))
    return out


# ---------------------------------------------------------------- one model's case, computed once per process
_CASES = {}


def case(name, m):
    """dict(om, cases, taus, acc, acc64, drawn, ref, ref32, d32, bound, res32, id_bound) of the built model `m` named `name`; read-only"""
    if name not in _CASES:
        om = m["om"]
        cases = states(om)
        taus, acc, acc64, drawn = round_trip(om, oracle_of(m), cases)
        ref, ref32 = reference_outputs(om, cases, acc), reference_outputs(om, cases, acc, np.float32)
        for v in list(ref.values()) + list(ref32.values()) + [taus, acc, acc64, drawn]:
            v.setflags(write=False)
        d32 = metric_devs(taus, ref32, ref)
        res32 = identity_devs(om, cases, acc, ref32)
        _CASES[name] = dict(om=om, cases=cases, taus=taus, acc=acc, acc64=acc64, drawn=drawn, ref=ref, ref32=ref32, d32=d32, bound=bounds(d32),
                            res32=res32, id_bound=identity_bounds(res32))
    return _CASES[name]


# ---------------------------------------------------------------- structure, from parent and obs_order (and link_body) alone
def ancestors(parent, b):
    """the moving bodies on the chain of body b, b itself included (body 0, the base, is not a joint)"""
    out = []
    while b > 0:
        out.append(int(b))
        b = int(parent[b])
    return out


def joint_column(om):
    """[nb] the column among the D velocities of each body's joint (entry 0 unused: -1)"""
    col = np.full(om["nb"], -1)
    col[np.asarray(om["obs_order"], int)] = 6 + np.arange(om["nb"] - 1)
    return col


def chain_columns(om):
    """per URDF link, the sorted joint columns on the chain of its body: the only joint columns of its Jacobian that may differ from 0"""
    col = joint_column(om)
    return [sorted(int(col[b]) for b in ancestors(om["parent"], int(lb))) for lb in om["link_body"]]


def related_columns(om):
    """[D, D] bool over the joint columns (rows and columns 0 .. 5, the base, are True: every joint moves with the base): one joint's
    body is an ancestor of the other's, or the same. Elsewhere the mass matrix is 0."""
    col, D = joint_column(om), 6 + om["nb"] - 1
    rel = np.zeros((D, D), bool)
    rel[:6, :] = rel[:, :6] = True
    for b in range(1, om["nb"]):
        for a in ancestors(om["parent"], b):
            rel[col[b], col[a]] = rel[col[a], col[b]] = True
    return rel


def base_block(ex):
    """the base block [6, 6] of a Jacobian, [[1, ex], [0, 1]], for the 3 x 3 block ex = columns 3 .. 5 of the linear rows"""
    out = np.eye(6)
    out[0:3, 3:6] = ex
    return out


def structure_faults(om, out):
    """what is not EXACTLY as the tree demands in the outputs `out`, as a list of strings (empty: all well): Jacobian columns of
    joints off the link's chain == 0; its base block exactly [[1, ex], [0, 1]] with ex antisymmetric; mass-matrix entries of joint
    pairs on different branches == 0; M[:3, :3] exactly mass x 1"""
    bad = []
    D = 6 + om["nb"] - 1
    chains, rel = chain_columns(om), related_columns(om)
    jac, M = np.asarray(out["jac"]), np.asarray(out["mass"])
    for l, cols in enumerate(chains):
        off = [c for c in range(6, D) if c not in cols]
        if np.any(jac[:, l][..., off] != 0.0):
            bad.append("jacobian of link %d: a column off its chain is not 0" % l)
        blk = jac[:, l][..., :6]                                   # [n, 2, 6, 6]
        ex = blk[..., 0:3, 3:6]
        if np.any(ex != -np.swapaxes(ex, -1, -2)):
            bad.append("jacobian of link %d: ex is not antisymmetric" % l)
        want = np.broadcast_to(np.eye(6), blk.shape).copy()
        want[..., 0:3, 3:6] = ex
        if np.any(blk != want):
            bad.append("jacobian of link %d: the base block is not [[1, ex], [0, 1]]" % l)
    if np.any(M[:, ~rel] != 0.0):
        bad.append("mass matrix: an entry of two joints on different branches is not 0")
    if np.any(M[:, :3, :3] != M[:, 0, 0][:, None, None] * np.eye(3)):
        bad.append("mass matrix: M[:3, :3] is not mass x 1")
    return bad


# ---------------------------------------------------------------- four deliberate mistakes
def leaf_mass_dropped(om):
    """the last leaf body weighs nothing (its rotational inertia stays)"""
    vm = dict(om)
    par = [int(p) for p in om["parent"]]
    leaf = max(b for b in range(1, om["nb"]) if b not in par)
    vm["mass"] = np.array(om["mass"], np.float64)
    vm["mass"][leaf] = 0.0
    return vm


def link_tf_ignored(om):
    """every URDF link's frame is its body's frame"""
    vm = dict(om)
    nl = len(om["link_names"])
    vm["link_tf"] = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (nl, 1)).reshape(np.shape(om["link_tf"]))
    return vm


def joint_rotation_ignored(om):
    """the origin of the first joint is not turned against its parent"""
    vm = dict(om)
    vm["joint_rot"] = np.array(om["joint_rot"], np.float64)
    vm["joint_rot"][1] = np.eye(3).reshape(vm["joint_rot"][1].shape)
    return vm


def obs_slots_swapped(om):
    """the first two joints of the observation order trade places (a model of one joint has no other order: unchanged)"""
    vm = dict(om)
    oo = np.array(om["obs_order"])
    if len(oo) >= 2:
        oo[[0, 1]] = oo[[1, 0]]
    vm["obs_order"] = oo
    return vm


MISTAKES = dict(leaf_mass=leaf_mass_dropped, link_tf=link_tf_ignored, joint_rot=joint_rotation_ignored, obs_slots=obs_slots_swapped)


def mistake_devs(c, mistake):
    """{metric: how far the f64 reference of the mistaken model lies from the right one} on the case c of case()"""
    return metric_devs(c["taus"], reference_outputs(MISTAKES[mistake](c["om"]), c["cases"], c["acc"]), c["ref"], round_trip_of_ref=True)
