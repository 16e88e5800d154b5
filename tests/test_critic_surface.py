"""The public Python surface of the privileged critic, recorded like the one tests/test_monitor_surface.py keeps for the episode
monitor: every public name of trex_gym.critic and trex_gym.critic_capi with its signature, the public methods of PolicyCritic, and
the attributes a TrexVecEnv carries for the critic row on the instance - against tests/golden/critic_surface.json. Host-only:
nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_critic_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "critic_surface.json")
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
        if not a.startswith("_"):
            v = inspect.getattr_static(cls, a)
            out[a] = "property" if isinstance(v, property) else _describe(getattr(cls, a))
    return out


def surface():
    from trex_gym import critic, critic_capi, ppo, vec_env
    out = {}
    for mod in (critic, critic_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.critic_capi.PolicyCritic"] = _members(critic_capi.PolicyCritic)
    out["trex_gym.critic_capi.CRITIC_SYMBOLS"] = list(critic_capi.CRITIC_SYMBOLS)
    out["trex_gym.critic_capi limits"] = [critic_capi.MAX_CRITIC_DIM, critic_capi.LEARNER_MAX_CRITIC_DIM, critic.MAX_WIDTH]
    out["trex_gym.critic.PRESETS"] = sorted(critic.PRESETS)
    # what the env carries for the critic row (instance attributes do not show in dir(class))
    src = inspect.getsource(vec_env.TrexVecEnv.__init__)
    out["trex_gym.vec_env.TrexVecEnv instance"] = sorted(a for a in set(re.findall(r"self\.(_?[a-z]\w*)\b(?=[^=\n]*=[^=])", src))
                                                        if "critic" in a)
    out["trex_gym.ppo.PPO.__init__"] = str(inspect.signature(ppo.PPO.__init__))
    return out


def test_critic_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the critic surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_the_env_class_and_the_policy_class_gained_nothing():
    """the critic row lives in instance attributes and in classes of its own modules"""
    from trex_gym import _capi, vec_env
    assert [a for a in vars(vec_env.TrexVecEnv) if "critic" in a] == []
    assert [a for a in vars(_capi.Policy) if "critic" in a] == []
    assert [a for a in vars(_capi) if "critic" in a.lower()] == []


def test_the_symbols_are_the_header_s():
    """every function include/trex_policy_critic.h declares is in the signature table, with as many arguments, and none besides;
    trex_policy.h includes the header at its end and declares none of them itself"""
    from trex_gym import critic_capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trex_policy_critic.h")).read(), flags=re.S)
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(trex_policy_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(critic_capi.CRITIC_SYMBOLS)
    for name, (_, argtypes) in critic_capi._CRITIC_API.items():
        assert len(argtypes) == declared[name], name
        assert hasattr(critic_capi.lib, name), name
    policy_h = open(os.path.join(ROOT, "include", "trex_policy.h")).read()
    assert policy_h.rstrip().endswith('#include "trex_policy_critic.h"\n#endif /* TREX_POLICY_H */')
    assert not any(name + "(" in policy_h.replace(" (", "(") for name in declared)


def test_the_limits_are_the_trainer_s():
    from trex_gym import critic, critic_capi, ppo
    assert critic_capi.MAX_CRITIC_DIM == ppo.POLICY_MAX_OBS_DIM == 126
    assert critic_capi.LEARNER_MAX_CRITIC_DIM == ppo.LEARNER_MAX_OBS_DIM == critic.MAX_WIDTH == 96


def test_train_flag_and_checkpoint_fields():
    from trex_gym import trex_train
    assert trex_train.parse_args([]).critic is None
    assert trex_train.parse_args(["--critic", "privileged", "--sensing", "typical", "--randomize", "typical"]).critic == "privileged"
    assert "critic" in inspect.signature(trex_train.build_environment).parameters
    import pytest
    with pytest.raises(SystemExit):
        trex_train.parse_args(["--critic", "everything"])


if __name__ == "__main__":
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
