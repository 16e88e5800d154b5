"""The step kernel on the states that bench.py and every training run spend their time in: the fallen, thrashing T-rex of a
1000-step episode under uniform random actions (tests/episode_cases.py; qualified on the CPU by tests/test_episode_cases_host.py).
The root body - the floating base, with the model's longest hull scan of 840 vertices - and the cranium touch here at every base
orientation; in the landing states of the other parity tests the cranium never touches and the root body only in the last two.

a. one env-step of every accepted case against the f64 oracle at the stated tolerances of tests/test_gpu_parity.py, three groups;
b. the contact sensor's per-body wrench on the same cases, at the rule of test_gpu_contact_wrench.py::test_sensor_matches_the_oracle;
c. warm start and external wrench from fallen states: the groups warm_fallen / wrench_fallen of tests/test_gpu_feature_oracle.py;
d. the launch forms bitwise equal through a whole 1000-step episode;
e. 4 096 envs at the benchmark's stationary mix of episode ages: determinism, permutation, and an oracle sample.
No tolerance here is new: each is an existing rule of the suite applied to new states. Measured: profiles/r18_episode_states.txt."""
import numpy as np
import pytest
import torch

import episode_cases as ec
from gpu_support import DEV, action_limits as limits, contact_counts, make_vec
from parity_helpers import assert_step_close

pytestmark = pytest.mark.gpu
NB, J = 26, 25
EPISODE = 1000


def up_axis(state):
    """[n] z component of the base's z axis, from get_state()"""
    return 1.0 - 2.0 * (state[:, 3] ** 2 + state[:, 4] ** 2)


class Deviation:
    """largest deviations from the f64 oracle over a group: |dq| rad, |dqd| / max(1, |qd|_inf), |dtau| over the unsaturated joints /
    their largest, |dreward| / max(1, |reward|)"""

    def __init__(self):
        self.q = self.qd = self.tau = self.rew = 0.0

    def add(self, obs, rew, want, max_force=3.0e5):
        o = want["obs"]
        self.q = max(self.q, np.abs(obs[:J] - o[:J]).max())
        self.qd = max(self.qd, np.abs(obs[J:2 * J] - o[J:2 * J]).max() / max(1.0, np.abs(o[J:2 * J]).max()))
        unsat = np.abs(o[2 * J:]) < 0.999 * max_force
        if unsat.any():
            self.tau = max(self.tau, np.abs(obs[2 * J:] - o[2 * J:])[unsat].max() / max(1.0, np.abs(o[2 * J:][unsat]).max()))
        self.rew = max(self.rew, abs(rew - want["rew"]) / max(1.0, abs(want["rew"])))

    def __str__(self):
        return "q %.2e qd %.2e tau %.2e reward %.2e" % (self.q, self.qd, self.tau, self.rew)


def load(g, sensor=False, extra=()):
    """the accepted cases of a group (and then `extra`) as one batch: domain, then the states (motors enabled); -> (env, actions)"""
    b, cases = g["built"], g["cases"] + list(extra)
    v = make_vec(len(cases), collision=b.collision)
    v.reset()
    if cases[0].get("mass_scale") is not None:
        v.set_domain(torch.tensor(np.array([c["mass_scale"] for c in cases])), torch.tensor(np.array([c["friction"] for c in cases])))
    if sensor:
        v.enable_contact_sensor()
    v.set_state(torch.tensor(np.array([c["state"] for c in cases])), motors_enabled=True)
    return v, torch.tensor(np.array([c["action"] for c in cases]), device=DEV)


def domain_of(c):
    if c.get("mass_scale") is None:
        return None
    return lambda orc, s: orc.set_domain(s, c["mass_scale"].astype(np.float64), float(c["friction"]))


def judged_by_f32_spread(o32, obs, o, state, action, seed, what, setup=None):
    """the way out of test_gpu_parity.py::test_config4_size_on_one_gpu, unchanged: a state on which f32 ITSELF is the limit - the
    spread of seven evaluations of the oracle's f32 build exceeds 1e-3 of the rate scale - is judged by 3 x that spread.
    -> error / spread"""
    spread = ec.f32_spread(o32, o, state, action, seed, setup)
    assert spread[J:].max() > 1e-3 * max(1.0, np.abs(o[J:2 * J]).max()), "well-conditioned state out of tolerance: " + what
    err = np.abs(obs[:2 * J] - o[:2 * J])
    assert (err <= 3 * spread + 1e-6).all(), what + " beyond 3x the f32 spread"
    return float((err / (spread + 1e-6)).max())


# ---------------------------------------------------------------- a. one-step parity
@pytest.mark.parametrize("name", ["hulls", "hulls_domain", "primitives"])
def test_one_step_parity_on_episode_states(name):
    """Every accepted case, one env-step from set_state: assert_step_close at its default tolerances (reward included) and the
    oracle's contact count. At most 1 case in 50 may be judged by the f32 spread instead (counted and printed).
    Measured on an MI355X (kernel | the f32 oracle on the same cases): see profiles/r18_episode_states.txt."""
    g = ec.group(name)
    b, cases = g["built"], g["cases"]
    v, acts = load(g, extra=g["set_aside"])
    obs, rew, _ = v.step_tensor(acts)
    obs, rew, cnt = obs.cpu().numpy(), rew.cpu().numpy(), contact_counts(v).cpu().numpy()
    v.close()
    gpu, f32, fallback, worst_ratio = Deviation(), Deviation(), [], 0.0
    for k, c in enumerate(cases):
        want = c["r64"]
        what = "%s case %d (%s, up %.2f, touched %s)" % (name, k, c["origin"], c["up"], sorted(c["touched"]))
        gpu.add(obs[k], rew[k], want)
        f32.add(c["r32"]["obs"], c["r32"]["rew"], want)
        try:
            assert_step_close(obs[k], want["obs"], rew[k], want["rew"], what)
        except AssertionError:
            worst_ratio = max(worst_ratio, judged_by_f32_spread(b.o32, obs[k], want["obs"], c["state"], c["action"], k, what, domain_of(c)))
            fallback.append(k)
        assert cnt[k] == want["cnt"], (what, cnt[k], want["cnt"])
    root = sum(g["root"] in c["touched"] for c in cases)
    cranium = sum(g["cranium"] in c["touched"] for c in cases)
    print("EPISODE-STATES %s: %d cases (root body touches in %d, cranium in %d); largest deviation from the f64 oracle: kernel %s | f32 oracle %s; "
          "%d judged by the f32 spread %s, worst error / spread %.2f" % (name, len(cases), root, cranium, gpu, f32, len(fallback), fallback, worst_ratio))
    assert len(fallback) <= len(cases) // 50, "too many states outside the stated tolerance: %s" % fallback
    for k, c in enumerate(g["set_aside"], len(cases)):      # (episode_cases.F32_LIMITED: measured, not judged by a tolerance)
        o = c["r64"]["obs"]
        assert np.isfinite(obs[k]).all() and cnt[k] == c["r64"]["cnt"]
        print("EPISODE-STATES %s, set aside (%s): kernel |dq| %.2e |dqd| %.2e = %.2f x the rate tolerance" % (name, c["origin"], np.abs(obs[k][:J] - o[:J]).max(),
              np.abs(obs[k][J:2 * J] - o[J:2 * J]).max(), np.abs(obs[k][J:2 * J] - o[J:2 * J]).max() / (3e-3 * max(1.0, np.abs(o[J:2 * J]).max()))))
    if name == "hulls":         # the compared set still is the sample of tests/test_episode_cases_host.py
        assert root >= 200 and cranium >= 60 and sum(c["up"] < 0.5 for c in cases) >= 600


# ---------------------------------------------------------------- b. the contact sensor
@pytest.mark.parametrize("name,root_floor,cranium_floor", [("hulls", 50, 20), ("primitives", 33, 20)])
def test_sensor_on_episode_states(name, root_floor, cranium_floor):
    """The per-env, per-body contact wrench of the step against the f64 oracle's (parity_helpers.oracle_wrench), at the rule of
    test_sensor_matches_the_oracle: at most 4 x the largest f32 - f64 oracle spread over the group, floor 1e-3, in units of M g;
    the same touching bodies - those whose normal force exceeds 1 % of the weight on one side carry a positive one on the other.
    Root-body and cranium wrenches are among those compared: a normal force above 1 % of the weight in at least 50 / 20 cases
    (primitives: 33 root cases - the f64 oracle alone gives 37 there, tests/test_episode_cases_host.py, less a tenth)."""
    g = ec.group(name)
    b, cases = g["built"], g["cases"]
    v, acts = load(g, sensor=True)
    v.step_tensor(acts)
    gw = v.contact_wrench().cpu().numpy().astype(np.float64)
    v.close()
    err, spread, seen = [], [], {g["root"]: 0, g["cranium"]: 0}
    for k, c in enumerate(cases):
        w64, w32, Mg = c["r64"]["wrench"], c["r32"]["wrench"], ec.weight(b, c)
        err.append(np.abs(gw[k] - w64).max() / Mg)
        spread.append(np.abs(w32 - w64).max() / Mg)
        for body in range(NB):
            if w64[body, 2] > 0.01 * Mg:
                assert gw[k, body, 2] > 0, (name, k, body)
            if gw[k, body, 2] > 0.01 * Mg:
                assert body in c["touched"] and w64[body, 2] > 0, (name, k, body)
        for body in seen:
            seen[body] += bool(w64[body, 2] > 0.01 * Mg and gw[k, body, 2] > 0.01 * Mg)
    err, spread = np.array(err), np.array(spread)
    tol = max(4 * spread.max(), 1e-3)
    print("EPISODE-STATES sensor %s: %d cases; contact wrench / Mg: kernel - f64 max %.2e median %.2e | f32 - f64 oracle max %.2e median %.2e; "
          "tolerance %.2e; normal force above 1 %% of the weight: root body %d cases, cranium %d"
          % (name, len(cases), err.max(), np.median(err), spread.max(), np.median(spread), tol, seen[g["root"]], seen[g["cranium"]]))
    assert err.max() <= tol, (int(err.argmax()), err.max(), tol)
    assert seen[g["root"]] >= root_floor and seen[g["cranium"]] >= cranium_floor


# ---------------------------------------------------------------- d. the launch forms through a whole episode
@pytest.mark.parametrize("variant", ["default", "warmstart", "sensor_and_wrench"])
def test_launch_forms_stay_bitwise_equal_through_an_episode(variant, model):
    """1000 steps of uniform random actions from a reset, episode limit 1000 with the ages staggered by i * 1000 // 64 (episodes
    end inside the launches throughout): the pair form (n = 64) and the single-env form (n = 65, the same first 64 envs), step_rows
    and step_many (blocks of 100 steps), wave balance 0 and 1 give bitwise the same rows at every step, and the same final state,
    contact_stats and episode counts (and contact_wrench() at every block end, with the sensor on). The run goes where it is meant
    to: at step 500 more than half of the envs older than 200 steps lie (up axis below 0.5)."""
    n, S, block = 64, EPISODE, 100
    lo, hi = limits(model)
    gen = torch.Generator(device=DEV).manual_seed(31)
    acts = (lo + (hi - lo) * torch.rand(S, n + 1, J, device=DEV, generator=gen)).contiguous()
    kw = dict(params={"warmstart": 0.8}) if variant == "warmstart" else {}
    sensor = variant == "sensor_and_wrench"
    wrench = torch.zeros(n + 1, NB, 6)
    wrench[:, 0, :3] = 0.1 * float(model["mass"].sum()) * 9.81 * torch.nn.functional.normalize(torch.randn(n + 1, 3, generator=torch.Generator().manual_seed(32)), dim=1)

    def run(m, many, balance):
        v = make_vec(m, max_episode_steps=EPISODE, **kw)
        assert v.batch.launch_info()["block"] == (128 if m % 2 == 0 else 64)
        v.batch.set_wave_balance(balance)
        if sensor:
            v.enable_contact_sensor()
            v.set_external_wrench(wrench[:m])
        v.reset_tensor()
        v.set_episode_steps(((torch.arange(m) * EPISODE // n) % EPISODE).to(torch.int32))
        a = acts[:, :m].contiguous()
        rows, wr, mid = [], [], None
        for t0 in range(0, S, block):
            if many:
                rows.append(v.step_many_tensor(a[t0:t0 + block])[:, :n].clone())
            else:
                for t in range(t0, t0 + block):
                    v.step_tensor(a[t])
                    rows.append(v.rows[:n].clone())
            if sensor:
                wr.append(v.contact_wrench()[:n].clone())
            if t0 + block == 500:
                mid = (v.get_state()[:n].clone(), v.episode_steps[:n].clone())
        rows = torch.cat(rows) if many else torch.stack(rows)
        out = dict(rows=rows, wrench=wr, mid=mid, state=v.get_state()[:n].clone(), cnt=contact_counts(v)[:n].clone(), steps=v.episode_steps[:n].clone())
        v.close()
        return out

    ref = run(n, False, 0)
    for m, many, balance in ((n + 1, False, 1), (n, True, 1), (n + 1, True, 0)):
        got = run(m, many, balance)
        what = "n %d, %s, wave balance %d" % (m, "step_many" if many else "step_rows", balance)
        same = (got["rows"] == ref["rows"]).flatten(1).all(1)
        assert bool(same.all()), (what, "first step that differs", int((~same).nonzero()[0]))
        assert torch.equal(got["state"], ref["state"]) and torch.equal(got["cnt"], ref["cnt"]) and torch.equal(got["steps"], ref["steps"]), what
        assert torch.equal(got["mid"][0], ref["mid"][0]) and torch.equal(got["mid"][1], ref["mid"][1]), what
        assert len(got["wrench"]) == len(ref["wrench"]) and all(torch.equal(x, y) for x, y in zip(got["wrench"], ref["wrench"])), what
    assert torch.isfinite(ref["rows"]).all()
    assert int(ref["rows"][:, :, 3 * J + 1].sum()) == n              # every env's episode ended once, inside a launch
    state, age = ref["mid"]
    old = age > 200
    lying = int((up_axis(state)[old] < 0.5).sum())
    print("EPISODE-STATES launch forms %s: at step 500 %d of %d envs older than 200 steps lie; contact counts at the end up to %d"
          % (variant, lying, int(old.sum()), int(ref["cnt"].max())))
    assert int(old.sum()) >= n // 2 and 2 * lying > int(old.sum())
    if sensor:
        loaded = max(int((w[:, 0, 2] > 0).sum()) for w in ref["wrench"])
        print("EPISODE-STATES launch forms %s: the root body carries a normal force in up to %d of %d envs at a block end" % (variant, loaded, n))
        assert 10 * loaded > n


# ---------------------------------------------------------------- e. the benchmark's stationary mix
@pytest.mark.parametrize("warm", [0.0, 0.8], ids=["cold", "warmstart"])
def test_stationary_mix_at_4096_envs(warm, oracle64, oracle32, model):
    """bench.py's workload: 4 096 envs, episode limit 1000, ages staggered as ids * 1000 // n, a pre-roll of 1000 random-action steps.
    Then 20 steps three ways: two runs from the same saved state and episode counts (set_state empties the warm-start record on
    both sides) give the same bits; a permuted batch gives the permuted rows, bitwise; everything is finite, contact counts <= 13.
    And one step of 64 envs of that mix - the 32 with the most contacts, 32 spread over the batch - against the f64 oracle, exactly
    as test_gpu_parity.py::test_config4_size_on_one_gpu does it: the same qtol, the same f32-spread rule, the same cap of 3."""
    n, steps = 4096, 20
    lo, hi = limits(model)
    gen = torch.Generator(device=DEV).manual_seed(41)
    v = make_vec(n, max_episode_steps=EPISODE, **(dict(params={"warmstart": warm}) if warm else {}))
    v.reset_tensor()
    ids = torch.arange(n)
    v.set_episode_steps((ids * EPISODE // n).to(torch.int32))
    for t in range(EPISODE):
        v.step_tensor((lo + (hi - lo) * torch.rand(n, J, device=DEV, generator=gen)).contiguous())
    st, age = v.get_state().clone(), v.episode_steps.clone()
    assert torch.equal(age.cpu(), (ids * EPISODE // n).to(torch.int32))        # one full episode later: the same ages
    acts = (lo + (hi - lo) * torch.rand(steps, n, J, device=DEV, generator=gen)).contiguous()

    def run(order):
        v.set_state(st[order].contiguous())
        v.set_episode_steps(age[order])
        rows, first = [], None
        for t in range(steps):
            v.step_tensor(acts[t][order].contiguous())
            rows.append(v.rows.clone())
            cnt = contact_counts(v)
            assert 0 <= int(cnt.min()) and int(cnt.max()) <= 13
            first = cnt if first is None else first
        return torch.stack(rows), v.get_state().clone(), first

    ident = torch.arange(n, device=DEV)
    rows_a, st_a, cnt = run(ident)
    rows_b, st_b, _ = run(ident)
    assert torch.equal(rows_a, rows_b) and torch.equal(st_a, st_b)                          # determinism
    perm = torch.randperm(n, device=DEV, generator=gen)
    rows_p, st_p, _ = run(perm)
    assert torch.equal(rows_p, rows_a[:, perm]) and torch.equal(st_p, st_a[perm])           # permutation equivariance
    assert torch.isfinite(rows_a).all() and torch.isfinite(st_a).all()
    ended = int(rows_a[:, :, 3 * J + 1].sum())
    lying = int((up_axis(st)[age > 200] < 0.5).sum())
    assert ended >= steps * n // EPISODE - 8 and int(cnt.max()) >= 8 and 2 * lying > int((age > 200).sum())
    v.close()
    # the oracle sample: the first of the 20 steps (envs whose episode ended with it show the next episode's reset: not sampled)
    going = rows_a[0][:, 3 * J + 1] == 0
    by_cnt = torch.argsort(torch.where(going, cnt, -1), descending=True)[:32]
    spread_over = torch.arange(0, n, n // 32, device=DEV)[:32]
    idx = torch.cat([by_cnt, spread_over[going[spread_over]]]).cpu().numpy()
    st_h, a_h, o_h, r_h, c_h = st.cpu().numpy(), acts[0].cpu().numpy(), rows_a[0][:, :3 * J].cpu().numpy(), rows_a[0][:, 3 * J].cpu().numpy(), cnt.cpu().numpy()

    def setup(orc, s):
        orc.set_warmstart(s, warm)
    fallback, worst_ratio, touched_root = [], 0.0, 0
    for e in idx:
        s = oracle64.new_state()
        setup(oracle64, s)
        oracle64.set_state(s, st_h[e].astype(np.float64))
        o, r, _ = oracle64.step(s, a_h[e].astype(np.float64))
        what = "stationary-mix env %d (%d contacts)" % (e, c_h[e])
        qtol = 1e-4 + 0.01 * 5e-3 * max(1.0, np.abs(o[J:2 * J]).max())      # derived in test_config4_size_on_one_gpu
        try:
            assert_step_close(o_h[e], o, r_h[e], r, what, q_atol=qtol)
        except AssertionError:
            worst_ratio = max(worst_ratio, judged_by_f32_spread(oracle32, o_h[e], o, st_h[e], a_h[e], int(e), what, setup))
            fallback.append(int(e))
        assert len(oracle64.contacts(s)[0]) == c_h[e], what
        touched_root += 0 in oracle64.contacts(s)[0]
    print("EPISODE-STATES stationary mix, warm start %.1f: %d envs lie of %d older than 200 steps, %d episodes ended in %d steps; sample of %d: "
          "contacts up to %d, root body touches in %d; %d judged by the f32 spread %s, worst error / spread %.2f"
          % (warm, lying, int((age > 200).sum()), ended, steps, len(idx), c_h[idx].max(), touched_root, len(fallback), fallback, worst_ratio))
    assert len(idx) >= 60 and touched_root >= 10
    assert len(fallback) <= 3, "too many states outside the stated tolerance: %s" % fallback
