"""The step kernel under every engine parameter moved off its default, against the f64 oracle built with the same parameters: the
case groups of tests/param_cases.py (generated and qualified on the CPU, tests/test_param_cases_host.py - at least half of every
group's cases fail these very comparisons by >= 10 x on an oracle that keeps the moved parameter at its default).

Per env, after env-step 1 and env-step 3: parity_helpers.assert_step_close at its stated tolerances (loosen = 1; the generated
model's torque floor as in tests/test_gpu_synthetic_models.py), the reward, the contact count. No tolerance is new. Batches of
64 (pair form) and 65 (single-env form) envs, padded with copies of the group's cases. Measured: profiles/r26_engine_params.txt."""
import numpy as np
import pytest
import torch

import feature_cases as fc
import gpu_support
import param_cases as pc
from gpu_support import DEV
from parity_helpers import assert_step_close

pytestmark = pytest.mark.gpu
N_PAIR, N_SINGLE = 64, 65
FORMS_GROUPS = ["all_moved", "vmax_2", "vmax_2_velocity", "friction_high", "cerp_high", "substeps_3", "iters_7"]


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return tmp_path_factory.mktemp("param_models")


def make(g, n, **kw):
    """a batch of n envs with the group's parameters (and control modes); Model.get_param reports what was set"""
    b = g["built"]
    if g["modes"] is not None:
        kw["control_mode"] = list(g["modes"])
    v = gpu_support.make_vec(n, b.urdf, params=dict(b.params), **kw)
    for k, val in b.params.items():
        assert v.model.get_param(k) == pytest.approx(val, rel=1e-6, abs=0.0), k
    return v


def load(g, n, **kw):
    """env e holds case e % len(cases): reset, then the states; -> (env, held actions, case index per env)"""
    cases = g["cases"]
    idx = np.arange(n) % len(cases)
    v = make(g, n, **kw)
    v.reset()
    v.set_state(torch.tensor(np.array([cases[k]["state"] for k in idx])))
    return v, torch.tensor(np.array([cases[k]["action"] for k in idx]), device=DEV), idx


def outputs(v):
    cnt, imp = torch.zeros(v.num_envs, dtype=torch.int32, device=DEV), torch.zeros(v.num_envs, device=DEV)
    v.batch.contact_stats(cnt, imp)
    return [v.rows.clone(), v.get_state().clone(), cnt, imp]


class Worst:
    """largest deviations of a run as shares of their bounds (printed: the numbers of profiles/r26_engine_params.txt)"""

    def __init__(self):
        self.q = self.qd = self.tau = 0.0

    def step(self, b, g, o, extra):
        J = b.J
        self.q = max(self.q, np.abs(g[:J] - o[:J]).max() / 1e-4)
        self.qd = max(self.qd, np.abs(g[J:2 * J] - o[J:2 * J]).max() / (3e-3 * max(1.0, np.abs(o[J:2 * J]).max())))
        unsat = np.abs(o[2 * J:]) < 0.999 * b.max_force
        if unsat.any():
            self.tau = max(self.tau, np.abs(g[2 * J:] - o[2 * J:])[unsat].max() / (3e-3 * np.abs(o[2 * J:][unsat]).max() + b.tau_floor + extra + 1e-30))


def check(b, what, g_obs, g_rew, g_cnt, want, worst):
    worst.step(b, g_obs, want["obs"], want["tau_extra"])
    assert_step_close(g_obs, want["obs"], g_rew, want["rew"], what, J=b.J, max_force=b.max_force, tau_floor=b.tau_floor,
                      tau_extra=want["tau_extra"])
    assert g_cnt == want["cnt"], (what, g_cnt, want["cnt"])


def against_the_oracle(g, n, block):
    """the group's batch of n envs stepped 3 times; every env after env-step 1 and 3 against the group's f64 oracle"""
    b, cases, exp = g["built"], g["cases"], pc.expected(g)
    v, acts, idx = load(g, n)
    if block is not None:
        assert v.batch.launch_info()["block"] == block
    worst, in_contact = Worst(), 0
    for t in range(pc.N_STEPS):
        obs, rew, done = v.step_tensor(acts)
        assert not bool(done.any())
        if t not in pc.COMPARED:
            continue
        obs, rew, cnt = obs.cpu().numpy(), rew.cpu().numpy(), gpu_support.contact_counts(v).cpu().numpy()
        for e, k in enumerate(idx):
            what = "%s case %d (%s) env %d step %d" % (g["name"], k, cases[k]["origin"], e, t + 1)
            check(b, what, obs[e], rew[e], cnt[e], exp[k][t], worst)
            in_contact += e < len(cases) and exp[k][t]["cnt"] > 0
    v.close()
    print("ENGINE-PARAMS %-22s %s form, %d envs: largest deviation / bound: q %.3f qd %.3f tau %.3f; %d case-steps in contact"
          % (g["name"], {64: "single", 128: "pair", None: "actuator"}[block], n, worst.q, worst.qd, worst.tau, in_contact))
    return worst


def test_the_defaults_are_the_oracles():
    """the groups are stated relative to oracle/trex_model.default_params(): a model nobody touched reports the same values"""
    v = gpu_support.make_vec(2)
    d = pc.defaults()
    for k in sorted({k for m in pc.moved_parameters().values() for k in m}):
        assert v.model.get_param(k) == pytest.approx(d[k], rel=1e-6), k
    v.close()


# ---------------------------------------------------------------- 1. parity with the oracle, step by step
@pytest.mark.parametrize("name", pc.GROUPS)
def test_group_matches_the_oracle(name, directory):
    g = pc.group(name, directory)
    against_the_oracle(g, N_SINGLE, 64)


# ---------------------------------------------------------------- 2. the launch forms agree bitwise under moved parameters
@pytest.mark.parametrize("name", FORMS_GROUPS)
def test_launch_forms_agree_bitwise(name, directory):
    """pair form (64 envs) = single-env form (65 envs, the first 64) = step_many over 3 steps: rows, state, contact count and
    impulse - the pair form's own reads of friction, floor_z and contact_margin and its own copy of the velocity clamp"""
    g = pc.group(name, directory)
    a, acts, _ = load(g, N_PAIR)
    b, acts65, _ = load(g, N_SINGLE)
    if g["modes"] is None:
        assert a.batch.launch_info()["block"] == 128
    assert b.batch.launch_info()["block"] == 64
    per_step = []
    for t in range(pc.N_STEPS):
        a.step_tensor(acts)
        b.step_tensor(acts65)
        per_step.append(a.rows.clone())
        for x, y in zip(outputs(a), outputs(b)):
            assert torch.equal(x, y[:N_PAIR]), (name, t)
    c, _, _ = load(g, N_PAIR)
    rows = c.step_many_tensor(acts.unsqueeze(0).expand(pc.N_STEPS, -1, -1).contiguous())
    for t in range(pc.N_STEPS):
        assert torch.equal(rows[t], per_step[t]), (name, t)
    for x, y in zip(outputs(c), outputs(a)):
        assert torch.equal(x, y), name
    assert not torch.equal(a.rows[0], a.rows[3]) and bool(torch.isfinite(a.rows).all())
    for v in (a, b, c):
        v.close()


@pytest.mark.parametrize("name", ["vmax_2", "friction_high"])
def test_pair_form_matches_the_oracle(name, directory):
    against_the_oracle(pc.group(name, directory), N_PAIR, 128)


def test_velocity_mode_pair_batch_matches_the_oracle(directory):
    """the even batch of the group with VELOCITY joints (whichever form the launch takes with control modes set)"""
    against_the_oracle(pc.group("vmax_2_velocity", directory), N_PAIR, None)


# ---------------------------------------------------------------- 3. episode ends under moved parameters
@pytest.mark.parametrize("name", ["all_moved", "all_moved_deep_chain"])
def test_episode_end_inside_the_launch(name, directory):
    """max_episode_steps = 2: step 1 is the oracle's; step 2 ends every episode inside the launch - state and observation are the
    group's oracle reset (at the tolerance of test_gpu_parity.py::test_reset_matches_oracle); step 3 is the oracle's step after
    its reset, under the same action"""
    g = pc.group(name, directory)
    b, cases, exp = g["built"], g["cases"], pc.expected(g)
    v, acts, idx = load(g, N_SINGLE, max_episode_steps=2)
    worst = Worst()
    obs, rew, done = v.step_tensor(acts)
    assert not bool(done.any())
    obs, rew, cnt = obs.cpu().numpy(), rew.cpu().numpy(), gpu_support.contact_counts(v).cpu().numpy()
    for e, k in enumerate(idx):
        check(b, "%s env %d step 1" % (name, e), obs[e], rew[e], cnt[e], exp[k][0], worst)
    obs, rew, done = v.step_tensor(acts)
    assert bool(done.all())
    first, state, _ = pc.reset_expectation(b.o64, b.om, cases[0]["action"])
    np.testing.assert_allclose(obs.cpu().numpy(), np.tile(first, (N_SINGLE, 1)), atol=2e-6, rtol=0)
    np.testing.assert_allclose(v.get_state().cpu().numpy(), np.tile(state, (N_SINGLE, 1)), atol=2e-6, rtol=0)
    obs, rew, done = v.step_tensor(acts)
    assert not bool(done.any())
    obs, rew, cnt = obs.cpu().numpy(), rew.cpu().numpy(), gpu_support.contact_counts(v).cpu().numpy()
    for k, c in enumerate(cases):
        want = pc.reset_expectation(b.o64, b.om, c["action"])[2]
        want32 = pc.reset_expectation(b.o32, b.om, c["action"])[2]
        check(b, "%s env %d, the step after the reset" % (name, k), obs[k], rew[k], cnt[k],
              dict(want, tau_extra=fc.tau_extra(b, want, want32)), worst)
    print("ENGINE-PARAMS %s episode end: largest deviation / bound: q %.3f qd %.3f tau %.3f" % (name, worst.q, worst.qd, worst.tau))
    v.close()


# ---------------------------------------------------------------- 4. two batches with different parameters do not bleed
@pytest.mark.parametrize("pair", [("gravity_low", "gravity_high"), ("dt_half", "dt_double")])
def test_two_parameter_sets_alive_at_once(pair, directory):
    """both batches created before either steps, stepped in turn: each is bitwise the same batch stepped alone"""
    groups = [pc.group(n, directory) for n in pair]
    both = [load(g, N_PAIR) for g in groups]
    together = [[], []]
    for t in range(pc.N_STEPS):
        for i, (v, acts, _) in enumerate(both):
            v.step_tensor(acts)
            together[i].append(outputs(v))
    assert not torch.equal(together[0][0][0], together[1][0][0])
    for v, _, _ in both:
        v.close()
    for i, g in enumerate(groups):
        v, acts, _ = load(g, N_PAIR)
        for t in range(pc.N_STEPS):
            v.step_tensor(acts)
            for x, y in zip(outputs(v), together[i][t]):
                assert torch.equal(x, y), (pair[i], t)
        v.close()


# ---------------------------------------------------------------- 5. the row the trainer reads follows the parameters
@pytest.mark.parametrize("name", ["dt_half", "substeps_3"])
def test_reward_and_penalties_are_the_closed_form(name, directory):
    """r = -w_d (2.5 - z)^2 - w_k (x^2 + y^2) - w_e sum |qd tau| with the head COM, recomputed in f64 from what the step returned,
    at the tolerances of test_gpu_parity.py::test_reward_is_the_reference_formula; the penalties are its three terms. (tau is the
    motor impulse over the group's OWN dt: test_group_matches_the_oracle compares it with the oracle's.)"""
    g = pc.group(name, directory)
    J = g["built"].J
    v, acts, _ = load(g, N_SINGLE)
    for t in range(pc.N_STEPS):
        obs, rew, _ = v.step_tensor(acts)
        head = v.head_position().double()
        power = (obs[:, J:2 * J].double() * obs[:, 2 * J:].double()).abs().sum(1)
        terms = torch.stack([1.0 * (2.5 - head[:, 2]) ** 2, 0.002 * (head[:, 0] ** 2 + head[:, 1] ** 2), 0.005 * power], 1)
        assert torch.allclose(rew.double(), -terms.sum(1), rtol=2e-4, atol=1e-3), (name, t)
        assert torch.allclose(v.penalties.double(), terms, rtol=2e-4, atol=1e-3), (name, t)
        assert torch.allclose(v.penalties.double().sum(1), -rew.double(), rtol=1e-5, atol=1e-4), (name, t)
        assert float(power.max()) > 1.0
    v.close()
