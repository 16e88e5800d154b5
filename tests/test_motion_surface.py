"""The public Python surface of the motion clip, recorded like the one tests/test_reward_surface.py keeps for the reward terms:
every public name of trex_gym.motion and trex_gym.motion_capi with its signature, the public methods of Clip and BatchMotion, the
fields of TrexMotionTerm, and the attributes a TrexVecEnv with a clip attached carries on the instance - against
tests/golden/motion_surface.json. Host-only: nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_motion_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_surface.json")


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
    from trex_gym import motion, motion_capi, vec_env
    out = {}
    for mod in (motion, motion_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.motion.KINDS"] = dict(motion.KINDS)
    out["trex_gym.motion.Term"] = list(motion.Term._fields)
    out["trex_gym.motion.Clip"] = _members(motion.Clip)
    out["trex_gym.motion.Clip.__init__"] = str(inspect.signature(motion.Clip.__init__))
    out["trex_gym.motion_capi.BatchMotion"] = _members(motion_capi.BatchMotion)
    out["trex_gym.motion_capi.TrexMotionTerm"] = [name for name, _ in motion_capi.TrexMotionTerm._fields_]
    out["trex_gym.motion_capi.MOTION_SYMBOLS"] = list(motion_capi.MOTION_SYMBOLS)
    # what the env carries for the clip (instance attributes do not show in dir(class))
    src = inspect.getsource(vec_env.TrexVecEnv.__init__) + inspect.getsource(vec_env.TrexVecEnv._set_motion)
    out["trex_gym.vec_env.TrexVecEnv instance"] = sorted(a for a in set(re.findall(r"self\.([a-z]\w*)\b(?=[^=\n]*=[^=])", src))
                                                        if a.startswith("motion"))
    out["trex_gym.vec_env.TrexVecEnv._set_motion"] = str(inspect.signature(vec_env.TrexVecEnv._set_motion))
    return out


def test_motion_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the motion surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_attach_takes_what_set_motion_takes():
    from trex_gym import motion, vec_env
    a = list(inspect.signature(motion.attach).parameters.values())[1:]
    b = list(inspect.signature(vec_env.TrexVecEnv._set_motion).parameters.values())[1:]
    assert [(p.name, p.default) for p in a] == [(p.name, p.default) for p in b]


if __name__ == "__main__":
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path[:0] = [root, os.path.join(root, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
