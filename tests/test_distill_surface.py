"""The public surface of policy distillation, recorded like the one tests/test_critic_surface.py keeps for the privileged critic:
every public name of trex_gym.distill and trex_gym.distill_capi with its signature, the public methods of PolicyDistill, Teacher and
Distill, the header's functions - against tests/golden/distill_surface.json. Host-only: nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_distill_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distill_surface.json")
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _describe(value):
    if inspect.isclass(value):
        return "class"
    if callable(value):
        return str(inspect.signature(value))
    return "attribute: " + type(value).__name__


def _members(cls, own_only=False):
    out = {}
    for a in sorted(vars(cls) if own_only else dir(cls)):
        if not a.startswith("_") or a == "__init__":
            v = inspect.getattr_static(cls, a)
            out[a] = "property" if isinstance(v, property) else _describe(getattr(cls, a))
    return out


def surface():
    from trex_gym import distill, distill_capi
    out = {}
    for mod in (distill, distill_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.distill_capi.PolicyDistill"] = _members(distill_capi.PolicyDistill)
    out["trex_gym.distill_capi.DISTILL_SYMBOLS"] = list(distill_capi.DISTILL_SYMBOLS)
    out["trex_gym.distill_capi constants"] = dict(MSE=distill_capi.MSE, KL=distill_capi.KL, KINDS=distill_capi.KINDS,
                                                  LEARNER_MAX_OBS_DIM=distill_capi.LEARNER_MAX_OBS_DIM)
    out["trex_gym.distill.Teacher"] = _members(distill.Teacher)
    out["trex_gym.distill.Distill (own)"] = _members(distill.Distill, own_only=True)     # (the rest is trex_gym.ppo.PPO's)
    out["trex_gym.distill.ROW_CHOICES"] = list(distill.ROW_CHOICES)
    return out


def test_distill_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the distillation surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_the_policy_class_and_the_env_class_gained_nothing():
    """the binding lives in a module and a class of its own: the module-level names of _capi.py and vec_env.py stay the recorded ones"""
    from trex_gym import _capi, vec_env
    assert [a for a in vars(_capi.Policy) if "distill" in a] == []
    assert [a for a in vars(_capi) if "distill" in a.lower()] == []
    assert [a for a in vars(vec_env) if "distill" in a.lower()] == []


def test_the_symbols_are_the_header_s():
    """every function include/trex_policy_distill.h declares is in the signature table, with as many arguments, and none besides,
    and the built library exports it; the two constants are the header's; trex_policy.h includes the header at its end and declares
    none of the functions itself"""
    from trex_gym import distill_capi
    raw = open(os.path.join(ROOT, "include", "trex_policy_distill.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(trex_policy_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(distill_capi.DISTILL_SYMBOLS) and len(declared) == 2
    for name, (_, argtypes) in distill_capi._DISTILL_API.items():
        assert len(argtypes) == declared[name], name
        assert hasattr(distill_capi.lib, name), name
    defines = dict(re.findall(r"#define\s+(TREX_DISTILL_\w+)\s+(\d+)", text))
    assert defines == {"TREX_DISTILL_MSE": str(distill_capi.MSE), "TREX_DISTILL_KL": str(distill_capi.KL)}
    policy_h = open(os.path.join(ROOT, "include", "trex_policy.h")).read()
    tail = policy_h[policy_h.rindex("#pragma GCC visibility pop"):]
    assert '#include "trex_policy_distill.h"' in tail
    assert not any(name + "(" in policy_h.replace(" (", "(") for name in declared)


def test_the_limit_is_the_trainer_s():
    from trex_gym import distill_capi, ppo
    assert distill_capi.LEARNER_MAX_OBS_DIM == ppo.LEARNER_MAX_OBS_DIM == 96


def test_train_flags():
    import pytest
    from trex_gym import trex_train
    assert trex_train.parse_args([]).distill is None and trex_train.distill_args(trex_train.parse_args([])) is None
    a = trex_train.parse_args(["--distill", "t.pt", "--teacher_rows", "critic", "--critic", "privileged", "--sensing", "typical",
                               "--randomize", "typical", "--monitor", "--graphs", "--dagger_beta", "0.5"])
    assert trex_train.distill_args(a) == dict(teacher="t.pt", rows="critic", loss="kl", beta=0.5, decay=0.9)
    assert "distill" in inspect.signature(trex_train.train).parameters
    for bad in (["--teacher_rows", "rows"], ["--distill_loss", "mse"], ["--dagger_beta", "0.5"], ["--distill", "t.pt", "--dagger_beta", "2"],
                ["--distill", "t.pt", "--teacher_rows", "critic"], ["--distill", "t.pt", "--distill_loss", "huber"]):
        with pytest.raises(SystemExit):
            trex_train.parse_args(bad)


if __name__ == "__main__":
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
