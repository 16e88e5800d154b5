"""The PGS warm start and the external wrench on the GPU against the f64 oracle, env-step by env-step: the case groups of
tests/feature_cases.py (generated and qualified on the CPU, tests/test_oracle_features_host.py), every kept case asserted.

Per env and env-step: parity_helpers.assert_step_close at its stated tolerances (loosen = 1; the generated models' torque floor as
in tests/test_gpu_synthetic_models.py), the reward, the contact count; with the contact sensor on also the per-body contact wrench
at the rule of tests/test_gpu_contact_wrench.py::test_sensor_matches_the_oracle (4 x the f32 oracle's spread over the group, floor
1e-3 M g) - the impulses themselves, not only what they do to qd. Every group runs in the pair form (even batch) and padded to an
odd batch (single-env form). Measured deviations: profiles/r15_feature_oracle.txt; the groups warm_fallen and wrench_fallen (from
the fallen states of tests/episode_cases.py): profiles/r18_episode_states.txt."""
import numpy as np
import pytest
import torch

import feature_cases as fc
import gpu_support
from gpu_support import DEV
from parity_helpers import assert_step_close

pytestmark = pytest.mark.gpu
GROUPS = ["warm_trex", "warm_factor_1.0", "warm_factor_0.3", "warm_slab", "warm_many_hulls", "warm_max_contacts_4", "warm_margin_0.5",
          "warm_primitives", "wrench_trex", "wrench_deep_chain", "wrench_bushy", "wrench_warm", "warm_fallen", "wrench_fallen"]


@pytest.fixture(scope="module")
def groups(tmp_path_factory):
    return fc.groups(tmp_path_factory.mktemp("feature_models"))


def make_vec(b, n, warm, **kw):
    params = dict(b.params)
    if warm:
        params["warmstart"] = warm
    return gpu_support.make_vec(n, b.urdf, params=params or None, collision=b.collision, **kw)


def contact_counts(v):
    return gpu_support.contact_counts(v).cpu().numpy()


def batch_size(n_cases, form):
    """even (pair form: two envs per workgroup) or odd (single-env form), padded with copies of the first cases"""
    return n_cases + (n_cases % 2 if form == "pair" else 1 - n_cases % 2)


def load(group, form, sensor=False, **kw):
    """the group's cases in one batch of the given form (env e holds case e % len(cases)): domain, wrench, then the states"""
    b, cases = group["built"], group["cases"]
    n = batch_size(len(cases), form)
    idx = np.arange(n) % len(cases)
    v = make_vec(b, n, group["warm"], **kw)
    assert v.batch.launch_info()["block"] == (128 if form == "pair" else 64)
    v.reset()
    if any(c.get("mass_scale") is not None for c in cases):
        v.set_domain(torch.tensor(np.array([np.ones(b.nb, np.float32) if cases[k].get("mass_scale") is None else cases[k]["mass_scale"] for k in idx])))
    if any(c.get("wrench") is not None for c in cases):
        v.set_external_wrench(torch.tensor(wrenches(b, cases, idx)))
    if sensor:
        v.enable_contact_sensor()
    v.set_state(torch.tensor(np.array([cases[k]["state"] for k in idx])))
    acts = torch.tensor(np.array([cases[k]["action"] for k in idx]), device=DEV)
    return v, acts, idx


def wrenches(b, cases, idx):
    return np.array([np.zeros((b.nb, 6), np.float32) if cases[k].get("wrench") is None else cases[k]["wrench"] for k in idx])


class Worst:
    """largest deviations of a run as shares of their tolerances (printed: the numbers of profiles/r15_feature_oracle.txt)"""

    def __init__(self):
        self.q = self.qd = self.tau = self.sensor = 0.0

    def step(self, b, g, o, extra):
        J = b.J
        self.q = max(self.q, np.abs(g[:J] - o[:J]).max() / 1e-4)
        self.qd = max(self.qd, np.abs(g[J:2 * J] - o[J:2 * J]).max() / (3e-3 * max(1.0, np.abs(o[J:2 * J]).max())))
        unsat = np.abs(o[2 * J:]) < 0.999 * b.max_force
        if unsat.any():
            self.tau = max(self.tau, np.abs(g[2 * J:] - o[2 * J:])[unsat].max() / (3e-3 * np.abs(o[2 * J:][unsat]).max() + b.tau_floor + extra + 1e-30))


def check_env_step(b, what, g_obs, g_rew, g_cnt, want, worst):
    worst.step(b, g_obs, want["obs"], want["tau_extra"])
    assert_step_close(g_obs, want["obs"], g_rew, want["rew"], what, J=b.J, max_force=b.max_force, tau_floor=b.tau_floor,
                      tau_extra=want["tau_extra"])
    assert g_cnt == want["cnt"], (what, g_cnt, want["cnt"])


def sensor_tolerance(b, group):
    """the rule of test_sensor_matches_the_oracle over the group: 4 x the largest f32 - f64 spread, floor 1e-3, in units of M g"""
    spread = max(np.abs(x["wrench32"] - x["wrench"]).max() / case_weight(b, c)
                 for c, e in zip(group["cases"], fc.expected(group)) for x in e if x is not None)
    return max(4 * spread, 1e-3)


def case_weight(b, c):
    ms = c.get("mass_scale")
    return b.weight if ms is None else float((b.om["mass"] * ms).sum()) * fc.G


@pytest.mark.parametrize("sensor", [False, True], ids=["plain", "sensor"])
@pytest.mark.parametrize("form", ["pair", "single"])
@pytest.mark.parametrize("name", GROUPS)
def test_group_matches_the_oracle(name, form, sensor, groups):
    group = groups[name]
    b, cases, exp = group["built"], group["cases"], fc.expected(group)
    v, acts, idx = load(group, form, sensor)
    worst, tol = Worst(), sensor_tolerance(b, group)
    in_contact = 0
    for t in range(max(c["steps"] for c in cases)):
        obs, rew, _ = v.step_tensor(acts)
        obs, rew, cnt = obs.cpu().numpy(), rew.cpu().numpy(), contact_counts(v)
        gw = v.contact_wrench().cpu().numpy().astype(np.float64) if sensor else None
        for e, k in enumerate(idx):
            if t >= cases[k]["steps"]:
                continue
            want = exp[k][t]
            what = "%s case %d (%s, %s) env %d step %d" % (name, k, cases[k]["origin"], cases[k].get("what", ""), e, t + 1)
            check_env_step(b, what, obs[e], rew[e], cnt[e], want, worst)
            in_contact += want["cnt"] > 0
            if sensor:
                err = np.abs(gw[e] - want["wrench"]).max() / case_weight(b, cases[k])
                worst.sensor = max(worst.sensor, err / tol)
                assert err <= tol, (what, err, tol)
                assert set(np.flatnonzero(gw[e][:, 2] > 0.01 * case_weight(b, cases[k]))) <= set(np.flatnonzero(want["wrench"][:, 2] > 0)), what
    print("FEATURE-ORACLE %s %s %s: %d envs; largest deviation / tolerance: q %.3f qd %.3f tau %.3f sensor %.3f (sensor tolerance %.2e M g)"
          % (name, form, "sensor" if sensor else "plain", len(idx), worst.q, worst.qd, worst.tau, worst.sensor, tol))
    assert in_contact >= len(cases) // 2
    v.close()


@pytest.mark.parametrize("form", ["pair", "single"])
def test_containment_through_set_state(form, groups):
    """A warm batch steps once from the cases' earlier states (every record populated); set_state then puts the f64 oracle's states
    after that step - env CONTAINED's made non-finite. That env: done = 1, reward 0, and from then on the oracle's steps from
    `reset` with an empty record. The others: the oracle's steps from those states (set_state emptied their records; the records
    they build from then on are theirs - a containment next door in the workgroup must not touch them)."""
    group = groups["contained_set_state"]
    b, cases, exp = group["built"], group["cases"], fc.expected(group)
    n = batch_size(len(cases), form)
    idx = np.arange(n) % len(cases)
    v = make_vec(b, n, group["warm"])
    assert v.batch.launch_info()["block"] == (128 if form == "pair" else 64)
    v.reset()
    acts = torch.tensor(np.array([cases[k]["action"] for k in idx]), device=DEV)
    v.set_state(torch.tensor(np.array([cases[k]["before"] for k in idx])))
    v.step_tensor(acts)
    assert (contact_counts(v) > 0).all()                  # records populated
    states = np.array([cases[k]["state"] for k in idx])
    states[fc.CONTAINED, 13 + 4] = np.nan
    v.set_state(torch.tensor(states))
    s = b.o64.new_state()
    b.o64.set_warmstart(s, group["warm"])
    first = b.o64.reset(s)
    worst = Worst()
    for t in range(3):
        obs, rew, done = v.step_tensor(acts)
        obs, rew, done, cnt = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), contact_counts(v)
        assert done.tolist() == [t == 0 and e == fc.CONTAINED for e in range(n)]
        for e, k in enumerate(idx):
            what = "contained_set_state env %d step %d" % (e, t + 1)
            if e != fc.CONTAINED:
                check_env_step(b, what, obs[e], rew[e], cnt[e], exp[k][t], worst)
            elif t == 0:
                assert rew[e] == 0.0 and np.abs(obs[e] - first).max() <= 1e-5, what
            else:
                check_env_step(b, what, obs[e], rew[e], cnt[e], dict(fc.step(b.o64, b.om, s, cases[k]["action"]), tau_extra=0.0), worst)
    print("FEATURE-ORACLE contained_set_state %s: largest deviation / tolerance: q %.3f qd %.3f tau %.3f" % (form, worst.q, worst.qd, worst.tau))
    v.close()


@pytest.mark.parametrize("form", ["pair", "single"])
def test_containment_with_a_populated_record(form, groups):
    """The floor raised to the feet of the start pose; after CONTAIN_AT warm steps env CONTAINED gets a non-finite wrench for one
    step (done = 1, reward 0, the start pose: include/trex_batch.h), then a zero wrench again. Its next solve meets the vertices of
    the record it had: it must start cold - the oracle's steps from the start pose with an empty record. The others keep theirs."""
    group = groups["contained_wrench"]
    b, cases, exp = group["built"], group["cases"], fc.expected(group)
    n = batch_size(len(cases), form)
    v, acts, idx = load(group, form)
    zero = torch.zeros(n, b.nb, 6)
    v.set_external_wrench(zero)
    worst = Worst()
    for t in range(cases[0]["steps"]):
        if t == fc.CONTAIN_AT:
            bad = zero.clone()
            bad[fc.CONTAINED, 3, 1] = float("nan")
            v.set_external_wrench(bad)
        obs, rew, done = v.step_tensor(acts)
        obs, rew, done, cnt = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), contact_counts(v)
        if t == fc.CONTAIN_AT:
            v.set_external_wrench(zero)
        assert done.tolist() == [t == fc.CONTAIN_AT and e == fc.CONTAINED for e in range(n)]
        for e, k in enumerate(idx):
            what = "contained_wrench env %d step %d" % (e, t + 1)
            if e == fc.CONTAINED and t == fc.CONTAIN_AT:
                assert rew[e] == 0.0 and np.isfinite(obs[e]).all(), what
                np.testing.assert_allclose(v.get_state()[e].cpu().numpy(), fc.start_state(b.om), atol=1e-6, rtol=0, err_msg=what)
            elif e == fc.CONTAINED or "contain_at" not in cases[k]:
                check_env_step(b, what, obs[e], rew[e], cnt[e], exp[k][t], worst)
    print("FEATURE-ORACLE contained_wrench %s: largest deviation / tolerance: q %.3f qd %.3f tau %.3f" % (form, worst.q, worst.qd, worst.tau))
    v.close()


def test_settle_substeps_do_not_feel_the_wrench(groups):
    """With a wrench set: the observation after reset, and that of an env whose episode ends inside a step launch, are the
    oracle's reset (which ignores the wrench); the envs that go on take the forced step."""
    group = groups["settle_wrench"]
    b, cases = group["built"], group["cases"]
    n = len(cases)
    v = make_vec(b, n, 0.0, max_episode_steps=5)
    v.set_external_wrench(torch.tensor(wrenches(b, cases, np.arange(n))))
    acts = torch.tensor(np.array([c["action"] for c in cases]), device=DEV)
    want = [fc.settle_run(b.o64, b.om, c) for c in cases]
    first = v.reset_tensor().cpu().numpy()
    for e in range(n):
        assert np.abs(first[e] - want[e][0]).max() <= 1e-5, e
    v.set_episode_steps(torch.tensor([0, 4, 0, 0], dtype=torch.int32))
    obs, rew, done = v.step_tensor(acts)
    obs, rew, cnt = obs.cpu().numpy(), rew.cpu().numpy(), contact_counts(v)
    assert done.tolist() == [False, True, False, False]
    worst = Worst()
    for e in range(n):
        if e == 1:      # the reward of the forced step, the observation of the new episode
            assert np.abs(obs[e] - want[e][0]).max() <= 1e-5
            assert abs(rew[e] - want[e][1]["rew"]) <= 2e-3 * abs(want[e][1]["rew"]) + 1e-3
        else:
            check_env_step(b, "settle env %d" % e, obs[e], rew[e], cnt[e], dict(want[e][1], tau_extra=0.0), worst)
    v.close()
