"""The public Python surface of the sensor model, recorded like the one tests/test_motion_surface.py keeps for the motion clip:
every public name of trex_gym.sensing and trex_gym.sensing_capi with its signature, the public methods of BatchSensing, the fields
of Group and TrexSenseGroup, and the attributes a TrexVecEnv with sensing attached carries on the instance - against
tests/golden/sensing_surface.json. Host-only: nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_sensing_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensing_surface.json")


def _describe(value):
    if inspect.isclass(value):
        return "class"
    if callable(value):
        return str(inspect.signature(value))
    return "attribute: " + type(value).__name__


def _members(cls):
    out = {}
    for a in sorted(dir(cls)):
        if not a.startswith("_"):
            v = inspect.getattr_static(cls, a)
            out[a] = "property" if isinstance(v, property) else _describe(getattr(cls, a))
    return out


def surface():
    from trex_gym import sensing, sensing_capi, vec_env
    out = {}
    for mod in (sensing, sensing_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.sensing.Group"] = list(sensing.Group._fields)
    out["trex_gym.sensing.PRESETS"] = sorted(sensing.PRESETS)
    out["trex_gym.sensing_capi.BatchSensing"] = _members(sensing_capi.BatchSensing)
    out["trex_gym.sensing_capi.TrexSenseGroup"] = [name for name, _ in sensing_capi.TrexSenseGroup._fields_]
    out["trex_gym.sensing_capi.SENSING_SYMBOLS"] = list(sensing_capi.SENSING_SYMBOLS)
    # what the env carries for the sensor model (instance attributes do not show in dir(class))
    src = inspect.getsource(vec_env.TrexVecEnv.__init__) + inspect.getsource(vec_env.TrexVecEnv._set_sensing)
    out["trex_gym.vec_env.TrexVecEnv instance"] = sorted(a for a in set(re.findall(r"self\.([a-z]\w*)\b(?=[^=\n]*=[^=])", src))
                                                        if a.startswith(("sens", "clean")))
    out["trex_gym.vec_env.TrexVecEnv._set_sensing"] = str(inspect.signature(vec_env.TrexVecEnv._set_sensing))
    return out


def test_sensing_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the sensing surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_attach_takes_what_set_sensing_takes():
    from trex_gym import sensing, vec_env
    a = list(inspect.signature(sensing.attach).parameters.values())[1:]
    b = list(inspect.signature(vec_env.TrexVecEnv._set_sensing).parameters.values())[1:]
    assert [(p.name, p.default) for p in a] == [(p.name, p.default) for p in b]


def test_the_env_class_gained_one_private_method_and_nothing_public():
    from trex_gym import vec_env
    assert [a for a in vars(vec_env.TrexVecEnv) if "sensing" in a or "sense" in a or "clean" in a] == ["_set_sensing"]


if __name__ == "__main__":
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path[:0] = [root, os.path.join(root, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
