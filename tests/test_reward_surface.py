"""The public Python surface of the reward terms, recorded like the one tests/test_python_surface.py keeps for the older modules:
every public name of trex_gym.rewards and trex_gym.reward_capi with its signature, the public methods of BatchRewards, the fields
of TrexRewardTerm, and the attributes TrexVecEnv(rewards=...) sets on the instance - against tests/golden/reward_surface.json.
Host-only: nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_reward_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reward_surface.json")


def _describe(value):
    if inspect.isclass(value):
        return "class"
    if callable(value):
        return str(inspect.signature(value))
    return "attribute: " + type(value).__name__


def surface():
    from trex_gym import reward_capi, rewards, vec_env
    out = {}
    for mod in (rewards, reward_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.rewards.KINDS"] = dict(rewards.KINDS)
    out["trex_gym.rewards.Term"] = list(rewards.Term._fields)
    out["trex_gym.reward_capi.BatchRewards"] = {a: _describe(getattr(reward_capi.BatchRewards, a))
                                                for a in sorted(dir(reward_capi.BatchRewards)) if not a.startswith("_")}
    out["trex_gym.reward_capi.TrexRewardTerm"] = [name for name, _ in reward_capi.TrexRewardTerm._fields_]
    out["trex_gym.reward_capi.REWARD_SYMBOLS"] = list(reward_capi.REWARD_SYMBOLS)
    # what the constructor adds to the instance for the reward terms (instance attributes do not show in dir(class))
    src = inspect.getsource(vec_env.TrexVecEnv.__init__) + inspect.getsource(vec_env.TrexVecEnv._set_rewards)
    out["trex_gym.vec_env.TrexVecEnv instance"] = sorted(a for a in set(re.findall(r"self\.([a-z]\w*)\b(?=[^=\n]*=[^=])", src))
                                                        if a.startswith(("reward", "commands")))
    out["trex_gym.vec_env.TrexVecEnv.__init__"] = str(inspect.signature(vec_env.TrexVecEnv.__init__))
    return out


def test_reward_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the reward surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


if __name__ == "__main__":
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path[:0] = [root, os.path.join(root, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
