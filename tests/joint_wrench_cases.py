"""Cases for the joint force/torque sensor (trex_batch_joint_wrench): models, states, inputs, the metric and bounds that come from
the reference alone. numpy and the CPU oracle's model compiler only, no torch and no device: tests/test_joint_wrench_ref.py,
tests/test_gpu_joint_wrench.py and scripts/joint_wrench_bench.py take the same cases from here. A helper, not a conftest.

Models (MODELS): the T-rex, then the four of dynamics_model_cases.MODELS - deep_chain (depth 6), bushy (four children on two
bodies, 26 bodies), mount_first (a welded link 0), slab (J = 1).

States: dynamics_ref.random_states(om, 12, seed=31) with their per-body mass scales (the last two carry one). Accelerations: the
ones dynamics_ref.random_tau draws (joints within 10 rad/s^2, the base as a free-floating base answers), rounded to f32. Wrenches:
two per env, wrench_a and wrench_b, every component uniform within the model's weight (N; N m for the torque part), seeded,
rounded to f32.

Variants (VARIANTS): which of accel / wrench_a / wrench_b are given - none, each alone, all three -, each in world and link axes.

Metric (deviation): per env, the largest deviation of the force parts over the env's force scale and of the moment parts over its
moment scale - the joint rows and the base row together. Force scale: max(largest |force entry| of the env's reference rows, total
mass x g); moment scale: max(largest |moment entry|, total mass x g x 1 m). The mass is the env's, scale included.

Bound: the project's rule, min(CAP, max(DYNAMICS_TOL["id_zero"], 4 x d32)), d32 the deviation of the reference's f32 run
(joint_wrench_ref, dtype=float32) from its f64 run over every variant and env of the model, in the metric itself. It is computed
when a test runs; nothing of the device enters. The cap is a condition, not a limit: tests/test_joint_wrench_ref.py asserts
4 x d32 < CAP for every model. The identities' bounds follow the same rule from the f32 run's own residual in the identity."""
import numpy as np

import dynamics_model_cases as DC
import dynamics_ref as R
import joint_wrench_ref as JR
from tolerances import DYNAMICS_TOL

MODELS = ("trex",) + DC.MODELS
N = 12
G = 9.81
CAP = 1e-4
FLOOR = DYNAMICS_TOL["id_zero"]
# name -> (accel given, wrench_a given, wrench_b given)
VARIANTS = dict(static=(False, False, False), accel=(True, False, False), wrench_a=(False, True, False), wrench_b=(False, False, True),
                all=(True, True, True))
AXES = ("world", "link")


def built(tmp_path_factory, model):
    """{name: dict(path=urdf path or None for the T-rex asset, props=, om=)} of MODELS; `model`: the session's T-rex model dict"""
    from state_sets import built_models
    out = {"trex": dict(path=None, props=dict(params=None), om=model)}
    out.update(built_models(DC.MODELS, tmp_path_factory))
    return out


def inputs(om):
    """dict(cases [(state, mass scale or None)] x N, acc [N, D] f32, wa, wb [N, nb, 6] f32, weight [N])"""
    cases = list(zip(*R.random_states(om, N, seed=31)))
    rng = np.random.default_rng(17)
    acc = np.array([R.random_tau(om, s, ms, rng, with_accel=True)[1] for s, ms in cases]).astype(np.float32)
    nb = om["nb"]
    weight = np.array([float((np.asarray(om["mass"], np.float64) * (1.0 if ms is None else ms)).sum()) * G for _, ms in cases])
    wa = (rng.uniform(-1, 1, (N, nb, 6)) * weight[:, None, None]).astype(np.float32)
    wb = (rng.uniform(-1, 1, (N, nb, 6)) * weight[:, None, None]).astype(np.float32)
    return dict(cases=cases, acc=acc, wa=wa, wb=wb, weight=weight)


def given(inp, variant, e):
    """(accel or None, summed wrench f64 or None) of env e under the variant"""
    ua, uwa, uwb = VARIANTS[variant]
    w = None
    if uwa or uwb:
        w = (inp["wa"][e].astype(np.float64) if uwa else 0.0) + (inp["wb"][e].astype(np.float64) if uwb else 0.0)
    return (inp["acc"][e] if ua else None), w


def reference_outputs(om, inp, dtype=np.float64, mistake=None):
    """{(variant, axes): (rows [N, J, 6], base [N, 6])} of joint_wrench_ref run in `dtype`"""
    out = {}
    for v in VARIANTS:
        for ax in AXES:
            rows, base = [], []
            for e, (s, ms) in enumerate(inp["cases"]):
                a, w = given(inp, v, e)
                if w is not None and dtype == np.float32:
                    w = w.astype(np.float32)       # (the sum of the two inputs, rounded once: what the device adds)
                r, b = JR.joint_wrench(om, s, a, w, ms, G, ax, dtype, mistake)
                rows.append(r)
                base.append(b)
            out[v, ax] = (np.array(rows), np.array(base))
            assert out[v, ax][0].dtype == np.dtype(dtype)
    return out


def deviation(rows, base, ref_rows, ref_base, weight):
    """[N] the metric (module docstring) of one variant's outputs against the f64 reference's"""
    f8 = lambda x: np.asarray(x, np.float64)
    got = np.concatenate([f8(rows), f8(base)[:, None, :]], 1)
    ref = np.concatenate([ref_rows, ref_base[:, None, :]], 1)
    d = np.abs(got - ref)
    fs = np.maximum(np.abs(ref[..., 0:3]).max(axis=(1, 2)), weight)
    ms = np.maximum(np.abs(ref[..., 3:6]).max(axis=(1, 2)), weight * 1.0)
    return np.maximum(d[..., 0:3].max(axis=(1, 2)) / fs, d[..., 3:6].max(axis=(1, 2)) / ms)


def largest_deviation(out, ref, weight):
    """the largest metric over every variant, axes and env of the outputs dict `out` against `ref`"""
    return max(float(deviation(*out[key], *ref[key], weight).max()) for key in ref)


def bound_of(d32):
    return min(CAP, max(FLOOR, 4 * d32))


# ---------------------------------------------------------------- identities: what they are, and the f32 run's residual in them
def axis_torques(om, rows_link):
    """[J] the component of every row's moment along its joint axis, from rows in LINK axes: there the axis is the model's constant
    joint_axis, so the projection needs nothing but the rows themselves"""
    oo, ax = np.asarray(om["obs_order"], int), np.asarray(om["joint_axis"], np.float64)
    return np.einsum("kc,kc->k", ax[oo], np.asarray(rows_link, np.float64)[:, 3:6])


def axis_residual(om, inp, rows_link, base, want):
    """the largest |a_i . n_i - want[6 + i]| and |base - want[:6]| over the envs, each over the env's weight (x 1 m for the moments
    and the joint torques); rows_link [N, J, 6] in link axes, base [N, 6], want [N, D] a generalised force"""
    worst = 0.0
    for e in range(len(rows_link)):
        w = inp["weight"][e]
        wt, b = np.asarray(want[e], np.float64), np.asarray(base[e], np.float64)
        worst = max(worst, np.abs(axis_torques(om, rows_link[e]) - wt[6:]).max() / w, np.abs(b - wt[:6]).max() / w)
    return float(worst)


def round_trip_forces(om, inp):
    """[N, D] f32 generalised forces for the forward-dynamics round trip: the joint torques of the drawn accelerations and a base
    block within a tenth of the weight"""
    rng = np.random.default_rng(23)
    out = []
    for e, (s, ms) in enumerate(inp["cases"]):
        f = R.inverse_dynamics(om, s, inp["acc"][e], ms, G)
        f[:6] = rng.uniform(-0.1, 0.1, 6) * inp["weight"][e]
        out.append(f)
    return np.array(out).astype(np.float32)


def identity_residuals32(om, inp, forces):
    """(id, fd): the residuals of the reference's own f32 run in the two identities - the axis components and the base row against
    its f32 inverse dynamics of the same accelerations; and, with accel = its f32 solve(M, force - h), against the force"""
    f4 = np.float32
    rows, base, want = [], [], []
    rows2, base2 = [], []
    for e, (s, ms) in enumerate(inp["cases"]):
        r, b = JR.joint_wrench(om, s, inp["acc"][e], None, ms, G, "link", f4)
        rows.append(r)
        base.append(b)
        want.append(R.inverse_dynamics(om, s, inp["acc"][e], ms, G, f4))
        M, h = R.mass_matrix(om, s, ms, f4), R.inverse_dynamics(om, s, None, ms, G, f4)
        a = np.linalg.solve(M, forces[e] - h).astype(f4)
        r, b = JR.joint_wrench(om, s, a, None, ms, G, "link", f4)
        rows2.append(r)
        base2.append(b)
    return axis_residual(om, inp, rows, base, want), axis_residual(om, inp, rows2, base2, forces)


# ---------------------------------------------------------------- one model's case, computed once per process
_CASES = {}


def case(name, om):
    """dict(om, inp, ref, ref32, d32, bound, forces, res32 (id, fd), id_bound (id, fd)) of the model `om` named `name`; read-only"""
    if name not in _CASES:
        inp = inputs(om)
        ref, ref32 = reference_outputs(om, inp), reference_outputs(om, inp, np.float32)
        d32 = largest_deviation(ref32, ref, inp["weight"])
        forces = round_trip_forces(om, inp)
        res32 = identity_residuals32(om, inp, forces)
        for arr in [inp["acc"], inp["wa"], inp["wb"], inp["weight"], forces] + [x for pair in list(ref.values()) + list(ref32.values()) for x in pair]:
            arr.setflags(write=False)
        _CASES[name] = dict(om=om, inp=inp, ref=ref, ref32=ref32, d32=d32, bound=bound_of(d32), forces=forces, res32=res32,
                            id_bound=tuple(bound_of(r) for r in res32))
    return _CASES[name]
