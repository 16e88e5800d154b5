"""The public Python surface of the start-state randomisation, recorded like the one tests/test_sensing_surface.py keeps for the
sensor model: every public name of trex_gym.start_state and trex_gym.start_state_capi with its signature, the public methods of
BatchStartState, the fields of Term and TrexStartTerm, and the attributes a TrexVecEnv with start-state terms attached carries on
the instance - against tests/golden/start_state_surface.json. Host-only: nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_start_state_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "start_state_surface.json")


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
    from trex_gym import start_state, start_state_capi, vec_env
    out = {}
    for mod in (start_state, start_state_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.start_state.Term"] = list(start_state.Term._fields)
    out["trex_gym.start_state.PRESETS"] = sorted(start_state.PRESETS)
    out["trex_gym.start_state_capi.BatchStartState"] = _members(start_state_capi.BatchStartState)
    out["trex_gym.start_state_capi.TrexStartTerm"] = [name for name, _ in start_state_capi.TrexStartTerm._fields_]
    out["trex_gym.start_state_capi.START_STATE_SYMBOLS"] = list(start_state_capi.START_STATE_SYMBOLS)
    # what the env carries for the start states (instance attributes do not show in dir(class))
    src = inspect.getsource(vec_env.TrexVecEnv.__init__) + inspect.getsource(vec_env.TrexVecEnv._set_start_state)
    out["trex_gym.vec_env.TrexVecEnv instance"] = sorted(a for a in set(re.findall(r"self\.([a-z]\w*)\b(?=[^=\n]*=[^=])", src))
                                                        if a.startswith("start_"))
    out["trex_gym.vec_env.TrexVecEnv._set_start_state"] = str(inspect.signature(vec_env.TrexVecEnv._set_start_state))
    return out


def test_start_state_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the start-state surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_attach_takes_what_set_start_state_takes():
    from trex_gym import start_state, vec_env
    a = list(inspect.signature(start_state.attach).parameters.values())[1:]
    b = list(inspect.signature(vec_env.TrexVecEnv._set_start_state).parameters.values())[1:]
    assert [(p.name, p.default) for p in a] == [(p.name, p.default) for p in b]


def test_the_env_class_gained_one_private_method_and_nothing_public():
    from trex_gym import vec_env
    assert [a for a in vars(vec_env.TrexVecEnv) if "start_state" in a] == ["_set_start_state"]


def test_the_symbols_are_the_header_s():
    """every function include/trex_start_state.h declares is in the signature table, with as many arguments, and none besides"""
    from trex_gym import start_state_capi
    root = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "trex_start_state.h")).read(), flags=re.S)
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(trex_batch_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(start_state_capi.START_STATE_SYMBOLS)
    for name, (_, argtypes) in start_state_capi._START_STATE_API.items():
        assert len(argtypes) == declared[name], name


if __name__ == "__main__":
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path[:0] = [root, os.path.join(root, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
