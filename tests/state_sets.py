"""State sets shared by the tests and by scripts/*_bench.py - with the links they are probed at and the generated models some of
them live on: numpy and the CPU oracle only, no torch and no device, so that the non-GPU tests take their states from here without
importing a GPU test module. The device side (envs holding these states) is tests/gpu_support.py. A helper, not a conftest: plain
functions, cached per process."""
import numpy as np

import dynamics_ref as R

J = 25

_LANDING = {}


def landing_states(oracle64, model, every=12, seed=5):
    """(states f32 [k, 63], actions f32 [k, 25]) sampled every `every` steps along a 300-step landing under noisy actions around
    the start pose: free fall, impact, standing (contacts, friction, joint stops under load). every=6 gives the 50 states of
    tests/test_gpu_parity.py::test_one_step_parity_in_contact_and_at_rest. The oracle may carry other engine parameters than the
    defaults (tests/param_cases.py): the landing is then that oracle's own; `seed` draws other noise. Rolled out once per oracle,
    `every` and `seed`; the arrays are read-only, so that one caller cannot change another's."""
    key = (id(oracle64), every, seed)
    if key not in _LANDING:
        q0 = model["q_start"][model["obs_order"]]
        lo, hi = model["q_lower"][model["obs_order"]], model["q_upper"][model["obs_order"]]
        rng = np.random.default_rng(seed)
        s = oracle64.new_state()
        oracle64.reset(s)
        states, acts = [], []
        for t in range(300):
            oracle64.step(s, np.clip(q0 + 0.15 * rng.normal(size=25), lo, hi))
            if t % every == 0:
                states.append(oracle64.get_state(s).astype(np.float32))
                acts.append(np.clip(q0 + 0.15 * rng.normal(size=25), lo, hi).astype(np.float32))
        states, acts = np.array(states), np.array(acts)
        states.setflags(write=False)
        acts.setflags(write=False)
        _LANDING[key] = (oracle64, states, acts)       # (the oracle is kept: its id stays its own)
    return _LANDING[key][1:]


_CASES = {}


def base_cases(oracle64, model):
    """the (state, mass scale or None) pairs case_states draws from: the landing states, then 8 random airborne ones, two of them
    with a per-body mass scale. Entries 20, 22 and 24 stand on the floor."""
    if "base" not in _CASES:
        ls, _ = landing_states(oracle64, model)
        rs, sc = R.random_states(model, 8)
        _CASES["base"] = [(s.astype(np.float64), None) for s in ls] + list(zip(rs, sc))
    return _CASES["base"]


def case_states(oracle64, model, n):
    """n distinct (state f32-exact f64 [63], mass scale or None); computed once per n"""
    if n in _CASES:
        return _CASES[n]
    base = base_cases(oracle64, model)
    rng = np.random.default_rng(100 + n)
    oo = model["obs_order"]
    lo, hi = model["q_lower"][oo], model["q_upper"][oo]
    out = []
    for e in range(n):
        s, ms = base[(e * 7) % len(base)] if n < len(base) else base[e % len(base)]
        if e >= len(base):
            s = s.copy()
            s[13:13 + J] = np.clip(s[13:13 + J] + 0.1 * rng.normal(size=J), lo, hi)
            s[7:13] += 0.3 * rng.normal(size=6)
            s[13 + J:] += 0.5 * rng.normal(size=J)
            s = s.astype(np.float32).astype(np.float64)
        out.append((s, ms))
    _CASES[n] = out
    return out


def oracle_state(orc, state, scale):
    """a new state of the oracle `orc` holding `state`, with the per-body mass scale `scale` (None: none)"""
    s = orc.new_state()
    if scale is not None:
        orc.set_domain(s, scale)
    orc.set_state(s, state)
    return s


def probe_links(model):
    """head link, one toe link, the base link: what the dynamics queries are probed at"""
    names = model["link_names"]
    hb = int(model["head_body"])
    assert model["link_body"][0] == 0
    return dict(head=[l for l in range(len(names)) if model["link_body"][l] == hb][0],
                toe=[l for l in range(len(names)) if "toe" in names[l]][0], base=0)


def pick_links(model):
    """head, a toe, the base, the deepest link and the last link merged across a fixed joint with a turned link_tf"""
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    tf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)
    out = [0, [l for l in range(len(names)) if lb[l] == int(model["head_body"])][0],
           [l for l in range(len(names)) if lb[l] == int(np.argmax(model["depth"]))][0]]
    out += [l for l in range(len(names)) if "toe" in names[l]][:1]
    turned = [l for l in range(len(names)) if np.abs(tf[l][:9] - np.eye(3).reshape(-1)).max() > 1e-3]
    moved = [l for l in range(len(names)) if np.abs(tf[l][9:]).max() > 1e-3]
    out += (turned or moved)[-1:]
    return out


def built_models(names, tmp_path_factory):
    """{name: dict(path=urdf path, props=, om=oracle model dict)} of the generated models `names` (tests/synthetic_models.py): the
    body of a module-scoped `built` fixture"""
    import synthetic_models as sm
    out = {}
    for name in names:
        path, props, om = sm.compile_both(name, tmp_path_factory.mktemp(name))
        out[name] = dict(path=path, props=props, om=om)
    return out


def query_states(om, count=12):
    """random airborne states of the model `om` for the kernels outside the step"""
    states, _ = R.random_states(om, count, seed=31)
    return [s for s in states]
