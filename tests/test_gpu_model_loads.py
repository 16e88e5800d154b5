"""The step kernel after the change of where and how it fetches the model constants (packed per-body rows, global loads, one batch
of loads per phase: DESIGN 6, profiles/r39_model_loads.txt). No arithmetic changed, so the rows must be BITWISE those of the
kernels before the change: tests/golden/model_loads_parent_rows.txt holds, for every case below, the inputs and the rows that the
parent build produced for them on an MI355X (its header says how it was recorded; record() below wrote it).

A case = (model, feature): the T-rex, `bushy` (4 children on two bodies, welded links, hull-less leaves) and `deep_chain` (six tree
levels) of tests/synthetic_models.py; plain, with the PGS warm start (factor 0.85), with an external wrench attached. Two envs'
inputs per case, both in contact at the first step; 3 env-steps under the held action. Env 0 starts LIMIT - END_AT env-steps into an
episode of LIMIT: its episode ends with env-step END_AT, inside the launch - reward of the finished step, start pose, the
un-actuated settle substep (which feels no wrench and starts an empty warm-start record), the observation of the new episode - and
env-step 3 continues from there. Launches: 2 envs (pair form), 3 envs (single-env form: env 2 is a second copy of env 0's inputs),
step_many over 2 envs.

Asserted per case: (1) the three launch forms agree bitwise, rows and final state; (2) every row is within the project's tolerances
of the f64 oracle (parity_helpers.assert_step_close at loosen = 1, the torque allowance of a generated model from the oracle's own
f32 build as in tests/test_gpu_synthetic_models.py, the same contact count; the reset observation at the 2e-6 of
tests/test_gpu_engine_params.py::test_episode_end_inside_the_launch); (3) the rows and the final state are bitwise the parent's.
The inputs were chosen at recording time by the oracle alone: the first candidates (tests/feature_cases.py) on which its f32 build
passes (2) against its f64 build over all 3 steps; (2) re-asserts that here as well, so a tolerance is never met by luck."""
import os

import numpy as np
import pytest

import feature_cases as fc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "model_loads_parent_rows.txt")
MODELS = ("trex", "bushy", "deep_chain")
FEATURES = ("plain", "warm", "wrench")
STEPS, LIMIT, END_AT = 3, 40, 2
RESET_ATOL = 2e-6
WRENCH_SHARE = 0.2      # the wrench of a case: random over all bodies (feature_cases.random_all), a fifth of the weight in size

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the fixture file
def write_fixture(path, header, data):
    """data: {(model, feature): {field: f32 or i32 array}}; one line per array: model feature field shape hex-words"""
    with open(path, "w") as f:
        for line in header:
            f.write("# %s\n" % line)
        for (model, feature), fields in data.items():
            for name, a in fields.items():
                a = np.ascontiguousarray(a)
                assert a.dtype in (np.float32, np.int32)
                words = a.view(np.uint32).ravel()
                f.write("%s %s %s %s %s %s\n" % (model, feature, name, "f" if a.dtype == np.float32 else "i",
                                                "x".join(str(d) for d in a.shape), " ".join("%08x" % w for w in words)))


def read_fixture(path=GOLDEN):
    out = {}
    with open(path) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            model, feature, name, kind, shape, *words = line.split()
            a = np.array([int(w, 16) for w in words], np.uint32).view(np.float32 if kind == "f" else np.int32)
            out.setdefault((model, feature), {})[name] = a.reshape([int(d) for d in shape.split("x")])
    return out


# ---------------------------------------------------------------- the oracle's side
_BUILT = {}


def built(model, directory):
    if model not in _BUILT:
        _BUILT[model] = fc.trex() if model == "trex" else fc.synthetic(model, directory)
    return _BUILT[model]


def warm_of(feature):
    return fc.WARM if feature == "warm" else 0.0


def oracle_run(orc, b, case, warm, ends):
    """the case's STEPS env-steps on `orc`; ends: the episode ends with env-step END_AT (obs = the reset's, 'reset' set)"""
    s = fc.start(orc, case, warm)
    out = []
    for t in range(STEPS):
        r = fc.step(orc, b.om, s, case["action"])
        if ends and t + 1 == END_AT:
            r = dict(r, obs=orc.reset(s), reset=True)
        out.append(r)
    return out


def close_to(b, got_obs, got_rew, got_cnt, want, extra, what):
    """(2) of the module docstring for one env-step"""
    if want.get("reset"):
        np.testing.assert_allclose(got_obs, want["obs"], atol=RESET_ATOL, rtol=0, err_msg=what + " reset observation")
        # the reward is the finished step's: its energy term needs that step's rates, which the row no longer shows - bounded as
        # assert_step_close bounds it, from the oracle's own row of the finished step
        fc.assert_step_close(want["done_obs"], want["done_obs"], got_rew, want["rew"], what, J=b.J, max_force=b.max_force,
                             tau_floor=b.tau_floor, tau_extra=extra)
        return
    fc.assert_step_close(got_obs, want["obs"], got_rew, want["rew"], what, J=b.J, max_force=b.max_force, tau_floor=b.tau_floor,
                         tau_extra=extra)
    assert got_cnt == want["cnt"], (what, got_cnt, want["cnt"])


def expected(b, case, warm, ends):
    """per env-step: the f64 oracle's step with the torque allowance from its f32 build; asserts that the f32 build passes (2)"""
    s64, s32 = fc.start(b.o64, case, warm), fc.start(b.o32, case, warm)
    out = []
    for t in range(STEPS):
        x, y = fc.step(b.o64, b.om, s64, case["action"]), fc.step(b.o32, b.om, s32, case["action"])
        extra = fc.tau_extra(b, x, y)
        if ends and t + 1 == END_AT:
            x, y = dict(x, done_obs=x["obs"], obs=b.o64.reset(s64), reset=True), dict(y, obs=b.o32.reset(s32))
        close_to(b, y["obs"], y["rew"], y["cnt"], x, extra, "the oracle's f32 build, step %d" % (t + 1))
        out.append(dict(x, tau_extra=extra))
    return out


def accepted(b, case, warm, ends):
    try:
        return expected(b, case, warm, ends)
    except AssertionError:
        return None


def choose_inputs(model, feature, directory):
    """two candidates in contact at the first step that the oracle accepts: the first as env 0 (its episode ends), the next as env 1"""
    b = built(model, directory)
    cands = fc.landing_candidates(b) if model == "trex" else fc.synthetic_candidates(b, model)
    rng = np.random.default_rng(3900 + 10 * MODELS.index(model) + FEATURES.index(feature))
    picked = []
    for c in cands:
        c = dict(c, steps=STEPS)
        if feature == "wrench":
            c["wrench"] = (fc.random_all(b)(rng) * (WRENCH_SHARE * b.weight)).astype(np.float32)
        e = accepted(b, c, warm_of(feature), ends=not picked)
        if e is not None and e[0]["cnt"] > 0:
            picked.append(c)
        if len(picked) == 2:
            return picked
    raise AssertionError("no two accepted candidates for %s %s" % (model, feature))


# ---------------------------------------------------------------- the kernels' side
def launch(b, feature, inputs, form):
    """-> (rows [STEPS, n, 3J + 2], contact counts [STEPS, n], final state [n, 13 + 2J]) of one launch form"""
    import torch
    import gpu_support
    n = 3 if form == "single" else 2
    idx = np.arange(n) % 2
    params = dict(b.params)
    if feature == "warm":
        params["warmstart"] = fc.WARM
    v = gpu_support.make_vec(n, b.urdf, params=params or None, collision=b.collision, max_episode_steps=LIMIT)
    if form != "many":
        assert v.batch.launch_info()["block"] == (64 if form == "single" else 128)
    v.reset()
    if feature == "wrench":
        v.set_external_wrench(torch.tensor(inputs["wrench"][idx]))
    v.set_state(torch.tensor(inputs["state"][idx]))
    v.set_episode_steps(torch.tensor(np.where(idx == 0, LIMIT - END_AT, 0), dtype=torch.int32))
    acts = torch.tensor(inputs["action"][idx], device=gpu_support.DEV)
    cnt = np.zeros((STEPS, n), np.int64)
    if form == "many":
        rows = v.step_many_tensor(acts.unsqueeze(0).expand(STEPS, -1, -1).contiguous()).cpu().numpy()
    else:
        rows = []
        for t in range(STEPS):
            v.step_tensor(acts)
            rows.append(v.rows.cpu().numpy().copy())
            cnt[t] = gpu_support.contact_counts(v).cpu().numpy()
        rows = np.array(rows)
    state = v.get_state().cpu().numpy()
    v.close()
    return rows, cnt, state


def record(path, header, directory):
    """writes the fixture from the library in use (the parent build's, for the committed file): inputs chosen by the oracle, rows
    and final state of the pair launch"""
    data = {}
    for model in MODELS:
        for feature in FEATURES:
            b = built(model, directory)
            cases = choose_inputs(model, feature, directory)
            inputs = dict(state=np.array([c["state"] for c in cases], np.float32), action=np.array([c["action"] for c in cases], np.float32))
            if feature == "wrench":
                inputs["wrench"] = np.array([c["wrench"] for c in cases], np.float32)
            rows, _, state = launch(b, feature, inputs, "pair")
            data[(model, feature)] = dict(inputs, rows=rows.astype(np.float32), final_state=state.astype(np.float32))
    write_fixture(path, header, data)


# ---------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def golden():
    return read_fixture()


@pytest.fixture(scope="module")
def launches(golden, tmp_path_factory):
    """(model, feature) -> {form: (rows, counts, state)}: every launch runs once, the three tests share it"""
    directory = tmp_path_factory.mktemp("model_loads")
    cache = {}

    def get(model, feature):
        if (model, feature) not in cache:
            b = built(model, directory)
            cache[(model, feature)] = {form: launch(b, feature, golden[(model, feature)], form) for form in ("pair", "single", "many")}
        return built(model, directory), cache[(model, feature)]
    return get


CASES = [(m, f) for m in MODELS for f in FEATURES]


@pytest.mark.parametrize("model,feature", CASES)
def test_launch_forms_agree_bitwise(model, feature, launches):
    _, out = launches(model, feature)
    (pr, pc, ps), (sr, sc, ss), (mr, _, ms) = out["pair"], out["single"], out["many"]
    assert pr.tobytes() == sr[:, :2].tobytes() and ps.tobytes() == ss[:2].tobytes() and (pc == sc[:, :2]).all()
    assert sr[:, 2].tobytes() == sr[:, 0].tobytes() and ss[2].tobytes() == ss[0].tobytes()      # the second copy of env 0's inputs
    assert pr.tobytes() == mr.tobytes() and ps.tobytes() == ms.tobytes()
    done = pr[:, :, -1]
    assert done.tolist() == [[float(t + 1 == END_AT and e == 0) for e in range(2)] for t in range(STEPS)]
    assert not np.array_equal(pr[:, 0], pr[:, 1])


@pytest.mark.parametrize("model,feature", CASES)
def test_rows_match_the_oracle(model, feature, launches, golden):
    b, out = launches(model, feature)
    rows, cnt, _ = out["pair"]
    g = golden[(model, feature)]
    in_contact = 0
    for e in range(2):
        case = dict(state=g["state"][e], action=g["action"][e], steps=STEPS)
        if feature == "wrench":
            case["wrench"] = g["wrench"][e]
        want = expected(b, case, warm_of(feature), ends=e == 0)
        for t in range(STEPS):
            what = "%s %s env %d step %d" % (model, feature, e, t + 1)
            close_to(b, rows[t, e, :3 * b.J].astype(np.float64), float(rows[t, e, 3 * b.J]), cnt[t, e], want[t], want[t]["tau_extra"], what)
            in_contact += want[t]["cnt"] > 0
    assert in_contact >= 2


@pytest.mark.parametrize("model,feature", CASES)
def test_rows_are_bitwise_the_parents(model, feature, launches, golden):
    _, out = launches(model, feature)
    rows, _, state = out["pair"]
    g = golden[(model, feature)]
    assert rows.dtype == np.float32 and rows.shape == g["rows"].shape
    assert rows.tobytes() == g["rows"].tobytes(), (model, feature, np.argwhere(rows.view(np.uint32) != g["rows"].view(np.uint32))[:5])
    assert state.astype(np.float32).tobytes() == g["final_state"].tobytes()
