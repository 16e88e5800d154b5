"""The reference of the dynamics derivatives (tests/dynamics_derivatives_ref.py) tied to what is already trusted - Richardson central
differences of dynamics_ref.inverse_dynamics through the retraction -, its exact zeros, its bounds (tests/derivatives_cases.py)
qualified against five deliberate mistakes, and the host side of the feature: the library exports the symbol of
include/trex_dynamics_derivatives.h, the new modules import, and their public surface is the one recorded in
tests/golden/derivatives_surface.json. Host-only: no device.

A pull request that moves the surface rewrites the record in the same commit:  python tests/test_derivatives_ref.py"""
import inspect
import json
import os
import re

import numpy as np
import pytest

import derivatives_cases as DC
import dynamics_derivatives_ref as DR
import dynamics_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derivatives_surface.json")
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FD_STEP = 1e-3
FD_BOUND = 2e-6


@pytest.fixture(scope="module")
def built(tmp_path_factory, model):
    return DC.built(tmp_path_factory, model)


@pytest.fixture(scope="module")
def cases(built):
    return lambda name: DC.case(name, built[name]["om"])


# ---------------------------------------------------------------- the reference against finite differences of dynamics_ref
def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def retract(state, J, xi, eta):
    """the state moved by the configuration tangent xi [D] and the velocity increment eta [D]: pos += xi_p, quat <- exp(xi_r) * quat
    (a WORLD-axis rotation vector), q += xi_q; v, w, qd += eta"""
    s = np.array(state, np.float64)
    s[0:3] += xi[0:3]
    th = np.linalg.norm(xi[3:6])
    if th > 0:
        s[3:7] = quat_mul(np.concatenate([np.sin(th / 2) * xi[3:6] / th, [np.cos(th / 2)]]), s[3:7])
    s[13:13 + J] += xi[6:]
    s[7:13] += eta[0:6]
    s[13 + J:13 + 2 * J] += eta[6:]
    return s


def central(om, state, accel, ms, h):
    """(dfdq, dfdv) [D, D] by central differences of step h"""
    J = om["nb"] - 1
    D = 6 + J
    f = lambda xi, eta: R.inverse_dynamics(om, retract(state, J, xi, eta), accel, ms, DC.G)
    out = np.zeros((2, D, D))
    zero = np.zeros(D)
    for j in range(D):
        e = np.zeros(D)
        e[j] = h
        out[0][:, j] = (f(e, zero) - f(-e, zero)) / (2 * h)
        out[1][:, j] = (f(zero, e) - f(zero, -e)) / (2 * h)
    return out


@pytest.mark.parametrize("name", DC.MODELS)
def test_reference_is_the_richardson_difference_of_inverse_dynamics(name, cases):
    """steps h = 1e-3 and h / 2 combined as (4 c(h/2) - c(h)) / 3: the f64 reference within 2e-6 per row; three states of the
    twelve (the first, and the last two with their mass scales) with the accelerations given, the first also without. The value
    returned beside the tangent is dynamics_ref.inverse_dynamics."""
    c = cases(name)
    om, inp = c["om"], c["inp"]
    worst = [0.0, 0.0]
    for e, v in ((0, "accel"), (0, "bias"), (DC.N - 2, "accel"), (DC.N - 1, "accel")):
        s, ms = inp["cases"][e]
        a = DC.given(inp, v, e)
        fd = (4 * central(om, s, a, ms, FD_STEP / 2) - central(om, s, a, ms, FD_STEP)) / 3
        f, dq, dv = (x[e] for x in c["ref"][v])
        want = R.inverse_dynamics(om, s, a, ms, DC.G)
        assert np.abs(f - want).max() <= 1e-12 * np.abs(want).max(), (name, e, v)
        worst = [max(worst[0], DC.row_deviation(dq, fd[0])), max(worst[1], DC.row_deviation(dv, fd[1]))]
    print("%s: reference against Richardson differences: dfdq %.3g, dfdv %.3g" % (name, worst[0], worst[1]))
    assert max(worst) <= FD_BOUND, (name, worst)


@pytest.mark.parametrize("name", DC.MODELS)
def test_exact_zeros_in_f64_and_f32(name, cases):
    """columns 0..2 of both matrices and the joint pairs on different branches are == 0 in the reference's f64 and f32 runs; the
    different-branch mask is not empty where the tree branches"""
    c = cases(name)
    for ref in (c["ref"], c["ref32"]):
        for v in DC.VARIANTS:
            for m in (1, 2):
                assert (ref[v][m][:, :, 0:3] == 0).all(), (name, v, m)
                assert (ref[v][m][:, c["zero"]] == 0).all(), (name, v, m)
    if name in ("trex", "bushy"):
        assert c["zero"].sum() > 0
    assert (c["zero"] == c["zero"].T).all() and not c["zero"][:6].any()


# ---------------------------------------------------------------- the bounds: set by the f32 run, and able to tell
@pytest.mark.parametrize("name", DC.MODELS)
def test_the_cap_never_binds(name, cases):
    c = cases(name)
    print("%s: d32 %.3g, bound %.3g; forward dynamics: d32 %.3g, bound %.3g" % (name, c["d32"], c["bound"], c["fwd_d32"], c["fwd_bound"]))
    assert 4 * c["d32"] < DC.CAP and 4 * c["fwd_d32"] < DC.CAP
    assert DC.FLOOR <= c["bound"] < DC.CAP and DC.FLOOR <= c["fwd_bound"] < DC.CAP


@pytest.mark.parametrize("mistake", DR.MISTAKES)
@pytest.mark.parametrize("name", DC.MODELS)
def test_the_bound_tells_a_mistake(name, mistake, cases):
    """each deliberate mistake lies more than 10 x CAP from the right reference"""
    c = cases(name)
    worst = DC.largest_deviation(DC.reference_outputs(c["om"], c["inp"], np.float64, mistake), c["ref"])
    print("%s %s: %.3g against 10 x CAP = %.3g" % (name, mistake, worst, 10 * DC.CAP))
    assert worst > 10 * DC.CAP, (name, mistake, worst)


# ---------------------------------------------------------------- the host side of the feature
def _describe(value):
    if inspect.isclass(value):
        return "class"
    if callable(value):
        return str(inspect.signature(value))
    return "attribute: " + type(value).__name__


def surface():
    from trex_gym import derivatives, derivatives_capi
    out = {}
    for mod in (derivatives, derivatives_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    cls = derivatives_capi.BatchDerivatives
    out["trex_gym.derivatives_capi.BatchDerivatives"] = {a: _describe(getattr(cls, a)) for a in sorted(dir(cls)) if not a.startswith("_")}
    out["trex_gym.derivatives_capi.DERIVATIVES_SYMBOLS"] = list(derivatives_capi.DERIVATIVES_SYMBOLS)
    return out


def test_derivatives_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the derivatives' surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_the_env_class_gained_nothing():
    """the derivatives live in modules of their own"""
    from trex_gym import _capi, vec_env
    assert [a for a in vars(vec_env.TrexVecEnv) if "derivative" in a or "stiffness" in a] == []
    assert [a for a in vars(_capi.Batch) if "derivative" in a] == []


def test_the_symbol_is_the_header_s_and_the_library_exports_it():
    """the function include/trex_dynamics_derivatives.h declares is in the signature table, with as many arguments, and none
    besides; the library exports it; trex_batch.h includes the header and does not declare the function itself"""
    from trex_gym import derivatives_capi as M
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trex_dynamics_derivatives.h")).read(), flags=re.S)
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(trex_batch_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(M.DERIVATIVES_SYMBOLS) == ["trex_batch_inverse_dynamics_derivatives"]
    for name, (_, argtypes) in M._DERIVATIVES_API.items():
        assert len(argtypes) == declared[name], name
        assert hasattr(M.lib, name), name
    batch_h = open(os.path.join(ROOT, "include", "trex_batch.h")).read()
    assert '#include "trex_dynamics_derivatives.h"' in batch_h
    assert "trex_batch_inverse_dynamics_derivatives" not in re.sub(r"/\*.*?\*/", "", batch_h, flags=re.S)
    flag = re.search(r"#define\s+TREX_DERIV_BY_DIRECTION\s+(\d+)u", text)
    assert flag and int(flag.group(1)) == M.BY_DIRECTION


if __name__ == "__main__":
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
