"""The reference of the joint force/torque sensor (tests/joint_wrench_ref.py) tied to what is already trusted, its bounds
(tests/joint_wrench_cases.py) qualified against four deliberate mistakes, and the host side of the feature: the library exports the
two symbols of include/trex_joint_wrench.h, the new modules import, and their public surface is the one recorded in
tests/golden/joint_wrench_surface.json. Host-only: no device.

A pull request that moves the surface rewrites the record in the same commit:  python tests/test_joint_wrench_ref.py"""
import inspect
import json
import os
import re

import numpy as np
import pytest

import dynamics_ref as R
import joint_wrench_cases as JC
import joint_wrench_ref as JR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "joint_wrench_surface.json")
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


@pytest.fixture(scope="module")
def built(tmp_path_factory, model):
    return JC.built(tmp_path_factory, model)


@pytest.fixture(scope="module")
def cases(built):
    return lambda name: JC.case(name, built[name]["om"])


# ---------------------------------------------------------------- the reference against dynamics_ref
@pytest.mark.parametrize("name", JC.MODELS)
def test_axis_component_and_base_row_are_inverse_dynamics(name, cases):
    """with no wrench, a_i . n_i is the joint's entry of dynamics_ref.inverse_dynamics - which sums moments about the WORLD origin
    and projects afterwards - and the base row is its base rows; with and without accelerations, to f64 rounding"""
    c = cases(name)
    om, inp = c["om"], c["inp"]
    for v in ("static", "accel"):
        rows, base = c["ref"][v, "world"]
        for e, (s, ms) in enumerate(inp["cases"]):
            want = R.inverse_dynamics(om, s, JC.given(inp, v, e)[0], ms, JC.G)
            scale = inp["weight"][e]
            assert np.abs(JR.axis_component(om, s, rows[e]) - want[6:]).max() <= 1e-10 * scale, (name, v, e)
            assert np.abs(base[e] - want[:6]).max() <= 1e-10 * scale, (name, v, e)


@pytest.mark.parametrize("name", JC.MODELS)
def test_closed_form_at_rest(name, cases):
    """qd = 0, no base velocity, no accel, no wrench: force = (0, 0, g x subtree mass), moment = (subtree COM - r_i) x force"""
    c = cases(name)
    om = c["om"]
    nj = om["nb"] - 1
    for s, ms in c["inp"]["cases"][-3:]:
        s = s.copy()
        s[7:13] = 0.0
        s[13 + nj:] = 0.0
        rows, base = JR.joint_wrench(om, s, None, None, ms, JC.G)
        k = R.Kin(om, s, ms)
        for i, S in enumerate(JR.subtree_sets(om["parent"])):
            m = k.mass[S].sum()
            com = (k.mass[S, None] * k.c[S]).sum(0) / m
            force = np.array([0.0, 0.0, JC.G * m])
            want = np.concatenate([force, np.cross(com - k.p[i], force)])
            got = base if i == 0 else rows[k.slot[i]]
            assert np.abs(got - want).max() <= 1e-9 * JC.G * k.mass.sum(), (name, i)


@pytest.mark.parametrize("name", JC.MODELS)
def test_linear_in_the_wrench_and_link_axes_are_a_rotation(name, cases):
    """rows(wa + wb) - rows(0) = (rows(wa) - rows(0)) + (rows(wb) - rows(0)); a link-axes row is R_i^T times the world row"""
    c = cases(name)
    ref = c["ref"]
    for e, (s, ms) in enumerate(c["inp"]["cases"]):
        a = c["inp"]["acc"][e]
        wa, wb = c["inp"]["wa"][e].astype(np.float64), c["inp"]["wb"][e].astype(np.float64)
        r0, b0 = JR.joint_wrench(c["om"], s, a, None, ms, JC.G)
        ra, ba = JR.joint_wrench(c["om"], s, a, wa, ms, JC.G)
        rb, bb = JR.joint_wrench(c["om"], s, a, wb, ms, JC.G)
        rall, ball = ref["all", "world"][0][e], ref["all", "world"][1][e]
        scale = max(np.abs(rall).max(), 1.0)
        assert np.abs((rall - r0) - (ra - r0) - (rb - r0)).max() <= 1e-10 * scale, (name, e)
        assert np.abs((ball - b0) - (ba - b0) - (bb - b0)).max() <= 1e-10 * scale, (name, e)
        k = R.Kin(c["om"], s)
        link = ref["all", "link"][0][e]
        for i in range(1, k.nb):
            w = rall[k.slot[i]]
            assert np.abs(link[k.slot[i]] - np.concatenate([k.R[i].T @ w[:3], k.R[i].T @ w[3:]])).max() <= 1e-10 * scale


# ---------------------------------------------------------------- the bounds: set by the f32 run, and able to tell
@pytest.mark.parametrize("name", JC.MODELS)
def test_the_cap_never_binds(name, cases):
    c = cases(name)
    print("%s: d32 %.3g, bound %.3g; identities: f32 residuals %s, bounds %s" % (name, c["d32"], c["bound"], c["res32"], c["id_bound"]))
    assert 4 * c["d32"] < JC.CAP
    assert all(4 * r < JC.CAP for r in c["res32"])
    assert JC.FLOOR <= c["bound"] < JC.CAP


@pytest.mark.parametrize("mistake", JR.MISTAKES)
@pytest.mark.parametrize("name", JC.MODELS)
def test_the_bound_tells_a_mistake(name, mistake, cases):
    """each deliberate mistake lies more than 10 x the bound from the reference on at least one variant"""
    c = cases(name)
    om, inp = c["om"], c["inp"]
    worst = 0.0
    for v in ("accel", "all"):
        rows, base = [], []
        for e, (s, ms) in enumerate(inp["cases"]):
            a, w = JC.given(inp, v, e)
            r, b = JR.joint_wrench(om, s, a, w, ms, JC.G, "world", np.float64, mistake)
            rows.append(r)
            base.append(b)
        worst = max(worst, float(JC.deviation(np.array(rows), np.array(base), *c["ref"][v, "world"], inp["weight"]).max()))
    print("%s %s: %.3g against the bound %.3g" % (name, mistake, worst, c["bound"]))
    assert worst > 10 * c["bound"], (name, mistake, worst, c["bound"])


# ---------------------------------------------------------------- the host side of the feature
def _describe(value):
    if inspect.isclass(value):
        return "class"
    if callable(value):
        return str(inspect.signature(value))
    return "attribute: " + type(value).__name__


def surface():
    from trex_gym import joint_sensor, joint_wrench_capi, trex_robot, vec_env
    out = {}
    for mod in (joint_sensor, joint_wrench_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    cls = joint_wrench_capi.BatchJointWrench
    out["trex_gym.joint_wrench_capi.BatchJointWrench"] = {a: _describe(getattr(cls, a)) for a in sorted(dir(cls)) if not a.startswith("_")}
    out["trex_gym.joint_wrench_capi.JOINT_WRENCH_SYMBOLS"] = list(joint_wrench_capi.JOINT_WRENCH_SYMBOLS)
    out["trex_gym.joint_wrench_capi.AXES"] = dict(joint_wrench_capi.AXES)
    out["trex_gym.trex_robot.TrexRobot joint state"] = {a: _describe(getattr(trex_robot.TrexRobot, a))
                                                        for a in ("_get_joint_state_names", "get_joint_state", "get_joint_states")}
    # what the env carries for the sensor (instance attributes do not show in dir(class))
    src = inspect.getsource(vec_env.TrexVecEnv.__init__)
    out["trex_gym.vec_env.TrexVecEnv instance"] = sorted(a for a in set(re.findall(r"self\.(_?[a-z]\w*)\b(?=[^=\n]*=[^=])", src))
                                                        if "joint" in a)
    return out


def test_joint_wrench_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the joint sensor's surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_the_env_class_gained_nothing():
    """the sensor lives in instance attributes and in modules of its own"""
    from trex_gym import _capi, vec_env
    assert [a for a in vars(vec_env.TrexVecEnv) if "joint" in a] == []
    assert [a for a in vars(_capi.Batch) if "joint_wrench" in a or "generalized" in a] == []


def test_the_symbols_are_the_header_s_and_the_library_exports_them():
    """every function include/trex_joint_wrench.h declares is in the signature table, with as many arguments, and none besides;
    the library exports each; trex_batch.h includes the header at its end and declares none of them itself"""
    from trex_gym import joint_wrench_capi as M
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trex_joint_wrench.h")).read(), flags=re.S)
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(trex_batch_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(M.JOINT_WRENCH_SYMBOLS) == ["trex_batch_generalized_velocity", "trex_batch_joint_wrench"]
    for name, (_, argtypes) in M._JOINT_WRENCH_API.items():
        assert len(argtypes) == declared[name], name
        assert hasattr(M.lib, name), name
    batch_h = open(os.path.join(ROOT, "include", "trex_batch.h")).read()
    assert batch_h.rstrip().endswith('#include "trex_joint_wrench.h"\n\n#endif /* TREX_BATCH_H */')
    own = re.sub(r"/\*.*?\*/", "", batch_h, flags=re.S)
    assert "trex_batch_joint_wrench" not in own and "trex_batch_generalized_velocity" not in own
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+TREX_AXES_(\w+)\s+(\d+)", batch_h)}
    assert (defines["WORLD"], defines["LINK"]) == (M.AXES_WORLD, M.AXES_LINK) and M.AXES == dict(world=0, link=1)


if __name__ == "__main__":
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
