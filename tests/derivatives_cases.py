"""Cases for the derivatives of the rigid-body dynamics (trex_batch_inverse_dynamics_derivatives, trex_gym.derivatives): models,
states, accelerations, the metric and the bounds, which come from the reference alone. numpy and the CPU oracle's model compiler
only, no torch and no device: tests/test_derivatives_ref.py, tests/test_gpu_derivatives.py and scripts/derivatives_bench.py take the
same cases from here. A helper, not a conftest.

Models (MODELS): the T-rex, then the four of dynamics_model_cases.MODELS - deep_chain (depth 6), bushy (four children on two
bodies, 26 bodies), mount_first (a welded link 0), slab (J = 1).

States: dynamics_ref.random_states(om, 12, seed=31) with their per-body mass scales (the last two carry one). Accelerations
(VARIANTS): the ones dynamics_ref.random_tau draws from default_rng(17) (joints within 10 rad/s^2, the base as a free-floating base
answers), rounded to f32 - "accel" -, and none - "bias".

Metric, PER ROW of a [D, D] matrix in Jacobian layout (row_deviation): max_j |got[i][j] - ref[i][j]| / max_j |ref[i][j]|; the
largest over rows, envs and both matrices. No row of the reference is zero (asserted when the case is made). A whole-block scale
would hide the light links, whose rows are orders of magnitude below the base's.

Bound: the project's rule, min(CAP, max(DYNAMICS_TOL["id_zero"], 4 x d32)), d32 the deviation of the reference's f32 run
(dynamics_derivatives_ref, dtype=float32) from its f64 run over both variants and every env of the model, in the metric itself. It
is computed when a test runs; nothing of the device enters. The cap is a condition, not a limit: tests/test_derivatives_ref.py
asserts 4 x d32 < CAP for every model.

forward_dynamics_derivatives, dadx = -M^-1 dfdx at a = M^-1 (force - h): the metric is the residual form M_ref (X - X_ref) per row
over the row scale of dfdx_ref, so that the conditioning of M stays out of it; its f32 run is np.linalg.solve in float32 on the f32
reference's outputs, and it gets the same rule and the same CAP.

The identity dfdq(2a) - dfdq(0) = 2 (dfdq(a) - dfdq(0)) (dfdq is affine in the accelerations): its bound follows the same rule from
the f32 run's own residual in the identity (linearity_residual32)."""
import numpy as np

import dynamics_derivatives_ref as DR
import dynamics_model_cases as DC
import dynamics_ref as R
from tolerances import DYNAMICS_TOL

MODELS = ("trex",) + DC.MODELS
N = 12
G = 9.81
CAP = 2e-4
FLOOR = DYNAMICS_TOL["id_zero"]
VARIANTS = ("accel", "bias")


def built(tmp_path_factory, model):
    """{name: dict(path=urdf path or None for the T-rex asset, props=, om=)} of MODELS; `model`: the session's T-rex model dict"""
    from state_sets import built_models
    out = {"trex": dict(path=None, props=dict(params=None), om=model)}
    out.update(built_models(DC.MODELS, tmp_path_factory))
    return out


def inputs(om):
    """dict(cases [(state, mass scale or None)] x N, acc [N, D] f32)"""
    cases = list(zip(*R.random_states(om, N, seed=31)))
    rng = np.random.default_rng(17)
    acc = np.array([R.random_tau(om, s, ms, rng, with_accel=True)[1] for s, ms in cases]).astype(np.float32)
    return dict(cases=cases, acc=acc)


def given(inp, variant, e):
    return inp["acc"][e] if variant == "accel" else None


def reference_outputs(om, inp, dtype=np.float64, mistake=None):
    """{variant: (f [N, D], dfdq [N, D, D], dfdv [N, D, D])} of dynamics_derivatives_ref run in `dtype`, Jacobian layout"""
    out = {}
    for v in VARIANTS:
        rows = [DR.inverse_dynamics_derivatives(om, s, given(inp, v, e), ms, G, dtype, mistake) for e, (s, ms) in enumerate(inp["cases"])]
        out[v] = tuple(np.array(x) for x in zip(*rows))
        assert out[v][1].dtype == np.dtype(dtype)
    return out


def row_deviation(got, ref, scale_of=None):
    """the metric: [..., D, D] matrices in Jacobian layout -> the largest over every leading index and row of
    max_j |got - ref| / max_j |scale_of| (scale_of: ref itself when None)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref if scale_of is None else np.asarray(scale_of, np.float64)).max(axis=-1)
    return float((np.abs(got - ref).max(axis=-1) / scale).max())


def largest_deviation(out, ref):
    """over both variants and both matrices; out, ref: {variant: (f, dfdq, dfdv)}"""
    return max(row_deviation(out[v][m], ref[v][m]) for v in ref for m in (1, 2))


def bound_of(d32):
    return min(CAP, max(FLOOR, 4 * d32))


# ---------------------------------------------------------------- forward dynamics: d a / d x = -M^-1 d f / d x
def forward_reference(om, inp, ref, dtype=np.float64):
    """(M [N, D, D], dadq, dadv [N, D, D]) in `dtype` from the outputs `ref` of the same dtype's "accel" variant: the accelerations
    are those of `inp`, i.e. the force is the inverse dynamics of them"""
    Ms = np.array([R.mass_matrix(om, s, ms, dtype) for s, ms in inp["cases"]])
    dadq = np.array([-np.linalg.solve(M, x) for M, x in zip(Ms, ref["accel"][1])])
    dadv = np.array([-np.linalg.solve(M, x) for M, x in zip(Ms, ref["accel"][2])])
    assert dadq.dtype == np.dtype(dtype)
    return Ms, dadq, dadv


def forward_deviation(got_q, got_v, fwd, ref):
    """the residual metric of dadq, dadv [N, D, D] against the f64 forward reference `fwd` and the f64 outputs `ref`"""
    Ms, dadq, dadv = fwd
    f8 = lambda x: np.asarray(x, np.float64)
    return max(row_deviation(Ms @ f8(got_q), Ms @ dadq, ref["accel"][1]), row_deviation(Ms @ f8(got_v), Ms @ dadv, ref["accel"][2]))


# ---------------------------------------------------------------- the identity: dfdq is affine in the accelerations
def linearity_residual(dq2, dq1, dq0, ref):
    """dfdq(2a) - dfdq(0) - 2 (dfdq(a) - dfdq(0)) of [N, D, D] matrices in Jacobian layout, per row over the row scale of the f64
    dfdq(a) of `ref`"""
    f8 = lambda x: np.asarray(x, np.float64)
    lhs, rhs = f8(dq2) - f8(dq0), 2 * (f8(dq1) - f8(dq0))
    return row_deviation(lhs, rhs, ref["accel"][1])


def linearity_residual32(om, inp, ref32, ref):
    """the residual of the reference's own f32 run in the identity"""
    dq2 = np.array([DR.inverse_dynamics_derivatives(om, s, np.float32(2) * inp["acc"][e], ms, G, np.float32)[1]
                    for e, (s, ms) in enumerate(inp["cases"])])
    return linearity_residual(dq2, ref32["accel"][1], ref32["bias"][1], ref)


# ---------------------------------------------------------------- one model's case, computed once per process
_CASES = {}


def case(name, om):
    """dict(om, inp, ref, ref32, d32, bound, fwd, fwd_d32, fwd_bound, lin32, lin_bound, zero (the [D, D] mask of the
    different-branch pairs)) of the model `om` named `name`; read-only"""
    if name not in _CASES:
        inp = inputs(om)
        ref, ref32 = reference_outputs(om, inp), reference_outputs(om, inp, np.float32)
        assert all(np.abs(ref[v][m]).max(axis=-1).min() > 0 for v in VARIANTS for m in (1, 2)), "a zero row in the reference"
        d32 = largest_deviation(ref32, ref)
        fwd = forward_reference(om, inp, ref)
        fwd32 = forward_reference(om, inp, ref32, np.float32)
        fwd_d32 = forward_deviation(fwd32[1], fwd32[2], fwd, ref)
        for arr in [inp["acc"]] + [x for t in list(ref.values()) + list(ref32.values()) for x in t] + list(fwd):
            arr.setflags(write=False)
        lin32 = linearity_residual32(om, inp, ref32, ref)
        _CASES[name] = dict(om=om, inp=inp, ref=ref, ref32=ref32, d32=d32, bound=bound_of(d32), fwd=fwd, fwd_d32=fwd_d32,
                            fwd_bound=bound_of(fwd_d32), lin32=lin32, lin_bound=bound_of(lin32), zero=DR.branch_zero_mask(om))
    return _CASES[name]
