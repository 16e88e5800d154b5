"""The public surface of the planner, recorded like the one tests/test_distill_surface.py keeps for policy distillation: every
public name of trex_gym.planner and trex_gym.planner_capi with its signature, the public methods of PlannerHandle and Planner, the
header's functions and constants - against tests/golden/planner_surface.json. Host-only: nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_planner_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_surface.json")
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _describe(value):
    if inspect.isclass(value):
        return "class"
    if callable(value):
        return str(inspect.signature(value))
    return "attribute: " + type(value).__name__


def _members(cls):
    out = {}
    for a in sorted(dir(cls)):
        if not a.startswith("_") or a == "__init__":
            v = inspect.getattr_static(cls, a)
            out[a] = "property" if isinstance(v, property) else _describe(getattr(cls, a))
    return out


def surface():
    from trex_gym import planner, planner_capi
    out = {}
    for mod in (planner, planner_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.planner_capi.PlannerHandle"] = _members(planner_capi.PlannerHandle)
    out["trex_gym.planner_capi.PLANNER_SYMBOLS"] = list(planner_capi.PLANNER_SYMBOLS)
    out["trex_gym.planner_capi constants"] = dict(HOLD=planner_capi.HOLD, LINEAR=planner_capi.LINEAR, CUBIC=planner_capi.CUBIC,
                                                  KINDS=planner_capi.KINDS, STREAM=planner_capi.STREAM, MAX_SAMPLES=planner_capi.MAX_SAMPLES,
                                                  MAX_HORIZON=planner_capi.MAX_HORIZON, MAX_KNOTS=planner_capi.MAX_KNOTS,
                                                  MAX_ACT=planner_capi.MAX_ACT)
    out["trex_gym.planner.Planner"] = _members(planner.Planner)
    out["trex_gym.planner.ROLLOUTS"] = list(planner.ROLLOUTS)
    return out


def test_planner_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the planner's surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_the_env_and_the_binding_gained_nothing():
    """the binding lives in a module and a class of its own: _capi.py, vec_env.py and trex_env.py name no planner"""
    from trex_gym import _capi, trex_env, vec_env
    for mod in (_capi, vec_env, trex_env):
        assert [a for a in vars(mod) if "plan" in a.lower()] == []
    for cls in (_capi.Batch, _capi.Policy, vec_env.TrexVecEnv, trex_env.TrexBulletEnv):
        assert [a for a in vars(cls) if "plan" in a.lower()] == []


def _header():
    raw = open(os.path.join(ROOT, "include", "trex_planner.h")).read()
    return raw, re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


def test_the_symbols_are_the_header_s():
    """every function include/trex_planner.h declares is in the signature table, with as many arguments, and none besides, and the
    built library exports it; the header stands alone: it includes nothing of the project, and no other header includes it"""
    from trex_gym import planner_capi
    raw, text = _header()
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(?:int|void)\s+(trex_planner_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(planner_capi.PLANNER_SYMBOLS) and len(declared) == 11
    for name, (_, argtypes) in planner_capi._PLANNER_API.items():
        assert len(argtypes) == declared[name], name
        assert hasattr(planner_capi.lib, name), name
    assert re.findall(r'#include\s+"([^"]+)"', raw) == [] and re.findall(r"#include\s+<([^>]+)>", raw) == ["stdint.h"]
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "trex_planner.h":
            assert "trex_planner" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_the_constants_are_the_header_s():
    from trex_gym import planner_capi as pc
    _, text = _header()
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(TREX_PLAN_\w+)\s+(\d+)", text)}
    assert defines == {"TREX_PLAN_HOLD": pc.HOLD, "TREX_PLAN_LINEAR": pc.LINEAR, "TREX_PLAN_CUBIC": pc.CUBIC, "TREX_PLAN_KINDS": len(pc.KINDS),
                       "TREX_PLAN_STREAM": pc.STREAM, "TREX_PLAN_MAXSAMPLES": pc.MAX_SAMPLES, "TREX_PLAN_MAXHORIZON": pc.MAX_HORIZON,
                       "TREX_PLAN_MAXKNOTS": pc.MAX_KNOTS, "TREX_PLAN_MAXACT": pc.MAX_ACT}
    # the stream is the next one behind those in use (include/trex_sensing.h 0..3, trex_randomize.h 4..6, trex_start_state.h 7)
    start = open(os.path.join(ROOT, "include", "trex_start_state.h")).read()
    assert int(re.search(r"#define\s+TREX_START_STREAM\s+(\d+)", start).group(1)) + 1 == pc.STREAM
    import planner_ref
    assert (planner_ref.HOLD, planner_ref.LINEAR, planner_ref.CUBIC, planner_ref.STREAM) == (pc.HOLD, pc.LINEAR, pc.CUBIC, pc.STREAM)
    assert (planner_ref.MAXSAMPLES, planner_ref.MAXHORIZON, planner_ref.MAXKNOTS, planner_ref.MAXACT) == \
        (pc.MAX_SAMPLES, pc.MAX_HORIZON, pc.MAX_KNOTS, pc.MAX_ACT)


def test_train_flags():
    import pytest
    from trex_gym import trex_train
    plain = trex_train.parse_args([])
    assert plain.mpc is None and trex_train.mpc_args(plain) is None and plain.save_clip is None
    a = trex_train.parse_args(["--num_envs", "2", "--mpc", "64", "16", "--mpc_knots", "6", "--mpc_sigma", "0.2", "--mpc_temperature", "0",
                               "--mpc_iterations", "2", "--mpc_steps", "50", "--save_clip", "clip.npz", "--frames", "out", "--graphs"])
    assert trex_train.mpc_args(a) == dict(samples=64, horizon=16, knots=6, sigma=0.2, temperature=0.0, iterations=2, steps=50,
                                          save_clip="clip.npz", frames="out", graphs=True, seed=0)
    assert trex_train.mpc_args(trex_train.parse_args(["--mpc", "8", "4"])) == dict(
        samples=8, horizon=4, knots=None, sigma=0.1, temperature=0.1, iterations=1, steps=100, save_clip=None, frames=None, graphs=False, seed=0)
    for bad in (["--mpc_knots", "4"], ["--mpc_sigma", "0.1"], ["--mpc_temperature", "1"], ["--mpc_iterations", "2"], ["--mpc_steps", "5"],
                ["--save_clip", "c.npz"], ["--mpc", "64"], ["--mpc", "0", "16"], ["--mpc", "64", "257"], ["--mpc", "5000", "16"],
                ["--mpc", "64", "16", "--mpc_knots", "17"], ["--mpc", "64", "40", "--mpc_knots", "33"], ["--mpc", "64", "16", "--mpc_sigma", "-1"],
                ["--mpc", "64", "16", "--mpc_temperature", "nan"], ["--mpc", "64", "16", "--mpc_iterations", "0"],
                ["--mpc", "64", "16", "--mpc_steps", "0"], ["--mpc", "64", "16", "--save", "m.pt"], ["--mpc", "64", "16", "--play"],
                ["--mpc", "64", "16", "--distill", "t.pt"], ["--mpc", "64", "16", "--critic", "clean"],
                ["--mpc", "64", "16", "--noptepochs", "2"]):
        with pytest.raises(SystemExit):
            trex_train.parse_args(bad)


if __name__ == "__main__":
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
