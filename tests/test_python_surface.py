"""The public Python surface does not move without the commit that moves it saying so: every public attribute of TrexVecEnv,
_capi.Model / Batch / Policy and TrexBulletEnv with its signature (parameter names, order, defaults), and the public
module-level names of trex_gym.vec_env and trex_gym._capi, against tests/golden/python_surface.json. Host-only: classes are
inspected, nothing is constructed.

A pull request that adds API rewrites the record in the same commit:  python tests/test_python_surface.py"""
import inspect
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_surface.json")


def _describe(cls, name):
    raw = inspect.getattr_static(cls, name)
    if isinstance(raw, property):
        return "property" + str(inspect.signature(raw.fget))
    value = getattr(cls, name)
    if callable(value):
        try:
            return str(inspect.signature(value))
        except (TypeError, ValueError):
            return "callable"
    return "attribute: " + type(value).__name__


def surface():
    from trex_gym import _capi, trex_env, vec_env
    classes = {"trex_gym.vec_env.TrexVecEnv": vec_env.TrexVecEnv, "trex_gym._capi.Model": _capi.Model,
               "trex_gym._capi.Batch": _capi.Batch, "trex_gym._capi.Policy": _capi.Policy,
               "trex_gym.trex_env.TrexBulletEnv": trex_env.TrexBulletEnv}
    out = {k: {a: _describe(c, a) for a in sorted(dir(c)) if not a.startswith("_")} for k, c in classes.items()}
    for mod in (vec_env, _capi):
        out[mod.__name__] = sorted(a for a in vars(mod) if not a.startswith("_"))
    return out


def test_public_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = []
    for key in sorted(set(want) | set(got)):
        w, g = want.get(key, {}), got.get(key, {})
        if isinstance(w, list) or isinstance(g, list):
            w, g = {a: "name" for a in w}, {a: "name" for a in g}
        for a in sorted(set(w) | set(g)):
            if w.get(a) != g.get(a):
                diff.append("%s.%s: recorded %s, now %s" % (key, a, w.get(a, "(absent)"), g.get(a, "(absent)")))
    print("\n".join(diff))
    assert not diff, "%d public names moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)
    assert got == want


if __name__ == "__main__":
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path[:0] = [root, os.path.join(root, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
