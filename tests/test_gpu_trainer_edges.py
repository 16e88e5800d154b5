"""The trainer-side kernels (csrc/policy_step.hip, csrc/ppo_learner.hip) at the shapes their padding, clamping and multi-trip
loops exist for, on the cases of tests/trainer_cases.py (checked on the CPU by tests/test_trainer_cases_host.py): every
comparison is against the f64 oracle (oracle/ppo_oracle.py), with f32 PyTorch (MlpPolicy, autograd) as a second witness.

Every output buffer has a guard region of GUARD rows behind it, filled with a sentinel that must survive the call.

Tolerances are the project's own (header of tests/test_gpu_policy.py): policy outputs, advantages, returns, losses 1e-5 relative
with that file's absolute floors; obs_out 1e-6; f64 running statistics 1e-10, return statistics 2e-6; gradient rtol 1e-4 +
1e-5 max|g| against the oracle; update 2 % of lr everywhere, 1e-3 relative where |g| > 1e-3 max|g|. Adam over 30 steps: the
bound of test_adam_kernel_is_tensorflows_adam..., 1e-5 lr per step + 2e-7 max|theta|.
Every case prints the deviation of the kernel and of f32 PyTorch from the oracle (-s); profiles/r14_trainer_edges.txt keeps them."""
import math

import numpy as np
import pytest
import torch

import trainer_cases as tc
from gpu_support import DEV
from oracle import ppo_oracle as P

pytestmark = pytest.mark.gpu
GUARD = 64
SENT = -12345.0
LR, EPS, MAXN = tc.LR, tc.ADAM_EPS, tc.MAX_GRAD_NORM


def guarded(rows, *shape, dtype=torch.float32):
    """(view of the first `rows` rows, whole buffer): GUARD sentinel rows lie behind the view"""
    full = torch.full((rows + GUARD,) + shape, SENT, dtype=dtype, device=DEV)
    return full[:rows], full


def guard_intact(*fulls_and_rows):
    for full, rows in fulls_and_rows:
        assert bool((full[rows:] == SENT).all()), "the guard region behind a [%d, ...] output was written" % rows


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def make_policy(kern, params):
    """MlpPolicy (f32 PyTorch) holding exactly the case's parameters, packed with kern.layout"""
    from trex_gym.ppo import MlpPolicy
    pol = MlpPolicy(kern.layout, kern.param_count, torch.device(DEV))
    with torch.no_grad():
        pol.theta.copy_(torch.from_numpy(tc._params_to_theta(kern.layout, kern.param_count, params)).to(DEV))
    return pol


# ================================================================ act
def _check_act(case, label):
    from trex_gym import _capi
    D, A, n = case["D"], case["A"], case["n"]
    kern = _capi.Policy(n, D, A, 64, 0)
    pol = make_policy(kern, case["params"])
    assert tc.layout_rule(D, A) == ({k: (o, tuple(s)) for k, (o, s) in kern.layout.items()}, kern.param_count)
    kern.set_stats(case["stats"])
    rows, noise = dev32(case["rows"]), dev32(case["noise"])
    (actions, F_a), (obs_n, F_o), (act_b, F_b) = guarded(n, A), guarded(n, D), guarded(n, A)
    (logp, F_l), (val, F_v) = guarded(n), guarded(n)
    kern.act(pol.theta, rows, noise, actions, obs_n, act_b, logp, val, clip_obs=tc.CLIP_OBS)
    guard_intact((F_a, n), (F_o, n), (F_b, n), (F_l, n), (F_v, n))
    got = {k: v.cpu().double().numpy() for k, v in dict(actions=actions, obs=obs_n, logp=logp, val=val).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    # ---- the f64 oracle
    mean64, ls64, _ = P.policy_forward(case["params"], case["obs_n"])
    nlp_at_got = P.neglogp(mean64, ls64, got["actions"])
    print("%s: max |d| vs oracle: obs %.2e actions %.2e value %.2e logp %.2e" % (
        label, np.abs(got["obs"] - case["obs_n"]).max(), np.abs(got["actions"] - case["actions"]).max(),
        np.abs(got["val"] - case["value"]).max(), np.abs(-got["logp"] - case["neglogp"]).max()))
    assert (np.abs(got["obs"]) == tc.CLIP_OBS).any()
    np.testing.assert_allclose(got["obs"], case["obs_n"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["actions"], case["actions"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got["val"], case["value"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(-got["logp"], nlp_at_got, rtol=1e-5, atol=3e-4)
    np.testing.assert_allclose(-got["logp"], case["neglogp"], rtol=1e-5, atol=3e-4)
    assert torch.equal(act_b, actions)
    # ---- f32 PyTorch, the second witness (tolerances of test_policy_kernel_matches_f32_torch_and_the_oracle)
    with torch.no_grad():
        mean32 = dev32(case["stats"]["obs_mean"])
        rstd32 = dev32(1.0 / np.sqrt(case["stats"]["obs_var"] + 1e-8))
        o = ((rows[:, :D] - mean32) * rstd32).clamp(-tc.CLIP_OBS, tc.CLIP_OBS)
        d = pol.dist(o)
        a = d.loc + d.scale * noise
        lp, v = d.log_prob(a).sum(-1), pol.value(o)
    print("%s: max |d| of f32 torch vs oracle: actions %.2e value %.2e logp %.2e" % (
        label, np.abs(a.cpu().double().numpy() - case["actions"]).max(), np.abs(v.cpu().double().numpy() - case["value"]).max(),
        np.abs(-lp.cpu().double().numpy() - case["neglogp"]).max()))
    torch.testing.assert_close(obs_n, o, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(actions, a, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(val, v, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(logp, lp, rtol=1e-5, atol=2e-4)
    # ---- the optional outputs left out: the same actions, nothing else
    actions2, F_a2 = guarded(n, A)
    kern.act(pol.theta, rows, noise, actions2, None, None, None, None, clip_obs=tc.CLIP_OBS)
    assert torch.equal(actions2, actions)
    guard_intact((F_a2, n))
    # ---- value_only: the same values bitwise, and nothing else is touched
    keep = [f.clone() for f in (F_a, F_o, F_b, F_l)]
    val2, F_v2 = guarded(n)
    kern.act(pol.theta, rows, None, None, value_out=val2, value_only=True, clip_obs=tc.CLIP_OBS)
    assert torch.equal(val2, val)
    guard_intact((F_v2, n))
    assert all(torch.equal(k, f) for k, f in zip(keep, (F_a, F_o, F_b, F_l)))
    # (with every buffer given, value_only still writes the values alone)
    kern.act(pol.theta, rows, noise, actions, obs_n, act_b, logp, val2, clip_obs=tc.CLIP_OBS, value_only=True)
    assert torch.equal(val2, val) and all(torch.equal(k, f) for k, f in zip(keep, (F_a, F_o, F_b, F_l)))
    kern.close()


@pytest.mark.parametrize("index", range(len(tc.ACT_CASES)), ids=["D%d_A%d_n%d" % c for c in tc.ACT_CASES])
def test_act_at_the_edges_of_its_tiling(index):
    """trex_policy_act at n < 32, n = 32 k + 1, D = 1 ... 126 (16 k-chunks, 29 staging slots), A = 1 ... 32, three row strides,
    non-trivial statistics: every output against the oracle and f32 PyTorch; lanes past n of a ragged tile write nothing."""
    D, A, n = tc.ACT_CASES[index]
    _check_act(tc.act_case(D, A, n, index), "act D=%d A=%d n=%d" % (D, A, n))


@pytest.mark.parametrize("mode", tc.ACT_TANH_CASES)
def test_act_in_both_ends_of_the_fast_tanh(mode):
    """(75, 25, 33) with every hidden pre-activation below 0.1 (the series branch) and with most units beyond +-20, a part of
    them beyond +-44.4 where exp2 overflows to inf (the saturated branch): finite, and the oracle's values."""
    _check_act(tc.act_case(75, 25, 33, tc.ACT_TANH_CASES.index(mode), mode), "act tanh " + mode)


# ================================================================ observe
@pytest.mark.parametrize("n,D,extra", tc.OBSERVE_CASES, ids=["n%d_D%d" % (c[0], c[1]) for c in tc.OBSERVE_CASES])
def test_observe_is_vecnormalize_at_one_to_64_workgroups(n, D, extra):
    """trex_policy_observe == the oracle's VecNormalize after every step of: a reset (with_reward = False, which must leave the
    return side bitwise alone), then reward steps with no, all, 20 % and only the last env done, then with_reward = False again
    on non-trivial returns. n = 4096 / 2049: 64 / 33
    workgroup partials, two trips of the merge. A second Policy object fed the same sequence ends bitwise equal."""
    from trex_gym import _capi
    steps = tc.observe_sequence(n, D, extra)
    kerns = [_capi.Policy(n, D, 3, 64, 0) for _ in range(2)]
    finals = []
    for which, kern in enumerate(kerns):
        vn = P.VecNormalize(n, D, gamma=0.99)
        (raw, F_raw), (done, F_done), (scale, F_scale), (ret, F_ret) = guarded(n), guarded(n), guarded(1), guarded(n)
        for t, rows64 in enumerate(steps):
            rows = dev32(rows64)
            if t == 0:
                st0 = kern.get_stats()
                kern.get_returns(ret)
                ret0 = ret.clone()
                kern.observe(rows, with_reward=False)
                vn.obs(rows64[:, :D])
                st = kern.get_stats()
                kern.get_returns(ret)
                assert all(st[k] == st0[k] for k in ("ret_mean", "ret_var", "ret_count", "raw_reward_sum")) and torch.equal(ret, ret0)
            else:
                kern.observe(rows, True, 0.99, raw, done, scale)
                vn.obs(rows64[:, :D])
                want_r = vn.reward(rows64[:, D], rows64[:, D + 1] != 0)
                st = kern.get_stats()
                kern.get_returns(ret)
                assert abs(st["ret_count"] - vn.ret_rms.count) < 1e-9
                np.testing.assert_allclose(st["ret_mean"], vn.ret_rms.mean, rtol=2e-6)
                np.testing.assert_allclose(st["ret_var"], vn.ret_rms.var, rtol=2e-6)
                assert torch.equal(raw, rows[:, D]) and torch.equal(done, rows[:, D + 1])
                assert abs(scale.item() - 1.0 / math.sqrt(vn.ret_rms.var + 1e-8)) <= 2e-6 * scale.item()
                np.testing.assert_allclose(np.clip(raw.cpu().numpy() * scale.item(), -10, 10), want_r, rtol=2e-6)
                np.testing.assert_allclose(ret.cpu().numpy(), vn.ret, rtol=1e-5, atol=1e-4)
                assert bool((ret[rows[:, D + 1] != 0] == 0).all())
            np.testing.assert_allclose(st["obs_mean"], vn.ob_rms.mean, rtol=1e-10)
            np.testing.assert_allclose(st["obs_var"], vn.ob_rms.var, rtol=1e-10)
            assert abs(st["obs_count"] - vn.ob_rms.count) < 1e-9
            guard_intact((F_raw, n), (F_done, n), (F_scale, 1), (F_ret, n))
        assert abs(st["raw_reward_sum"] - sum(float(r[:, D].sum()) for r in steps[1:])) <= 1e-9 * abs(st["raw_reward_sum"])
        # with_reward = False once more, now that the returns and their statistics are far from their initial values (the
        # reward / done columns of this block are not zero: they must not be looked at)
        st0, ret0 = kern.get_stats(), ret.clone()
        assert st0["ret_count"] > n and st0["ret_mean"] < -1.0 and (n == 1 or float(ret0.abs().max()) > 0)
        kern.observe(dev32(steps[2]), with_reward=False)
        vn.obs(steps[2][:, :D])
        st = kern.get_stats()
        kern.get_returns(ret)
        assert all(st[k] == st0[k] for k in ("ret_mean", "ret_var", "ret_count", "raw_reward_sum")) and torch.equal(ret, ret0)
        np.testing.assert_allclose(st["obs_mean"], vn.ob_rms.mean, rtol=1e-10)
        np.testing.assert_allclose(st["obs_var"], vn.ob_rms.var, rtol=1e-10)
        assert abs(st["obs_count"] - vn.ob_rms.count) < 1e-9
        guard_intact((F_raw, n), (F_done, n), (F_scale, 1), (F_ret, n))
        finals.append((kern.get_stats(), ret.clone()))
    (sa, ra), (sb, rb) = finals
    assert all(np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])) for k in sa) and torch.equal(ra, rb)
    for kern in kerns:
        kern.close()


# ================================================================ GAE
@pytest.mark.parametrize("pattern", tc.GAE_DONE_PATTERNS)
@pytest.mark.parametrize("T,n", tc.GAE_SHAPES, ids=["T%d_n%d" % s for s in tc.GAE_SHAPES])
def test_gae_at_short_and_ragged_rollouts(T, n, pattern):
    from trex_gym import _capi
    kern = _capi.Policy(n, 4, 2, 64, 0)
    case = tc.gae_case(T, n, pattern, 10 * tc.GAE_SHAPES.index((T, n)) + tc.GAE_DONE_PATTERNS.index(pattern))
    raw, scale, done, val = (dev32(case[k]) for k in ("raw", "scale", "done", "val"))
    rew64 = np.clip(case["raw"] * case["scale"][:, None], -10, 10)
    assert (np.abs(rew64) == 10).any()
    for gamma, lam in tc.GAE_GAMMA_LAM:
        (adv, F_adv), (ret, F_ret) = guarded(T, n), guarded(T, n)
        kern.gae(raw, scale, done, val, adv, ret, gamma, lam, 10.0)
        a64, r64 = P.gae(rew64, case["val"][:T], case["val"][T], case["done"], gamma, lam)
        np.testing.assert_allclose(adv.cpu().numpy(), a64, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(ret.cpu().numpy(), r64, rtol=1e-5, atol=1e-5)
        guard_intact((F_adv, T), (F_ret, T))
    kern.close()


# ================================================================ Adam
@pytest.mark.parametrize("max_norm", [0.5, 0.0])
@pytest.mark.parametrize("D,A", tc.ADAM_DIMS)
def test_adam_over_30_steps(D, A, max_norm):
    """trex_policy_adam for 30 consecutive steps (bias correction at t > 4) against the oracle's Adam; gradients below and above
    the clip norm and tiny ones; an all-zero gradient first (theta bitwise unchanged, norm 0) and at step 17 (the moments
    alone move theta); max_grad_norm = 0 is the no-clip branch (the reference skips the clip); after adam_reset the next step
    is a t = 1 step again. theta at every step within the bound of test_adam_kernel_is_tensorflows_adam...:
    1e-5 lr per step + 2e-7 max|theta|."""
    from trex_gym import _capi
    kern = _capi.Policy(64, D, A, 64, 0)
    Pn = kern.param_count
    assert Pn == tc.layout_rule(D, A)[1]
    g = torch.Generator(device=DEV).manual_seed(40 + D)
    (theta, F_t), (grad, F_g), (m, F_m), (v, F_v), (norm, F_n) = guarded(Pn), guarded(Pn), guarded(Pn), guarded(Pn), guarded(1)
    # theta at the scale of what 30 steps move it by (30 lr = 0.009): the bound then measures the update, not the f32 rounding of
    # a large theta, which at |theta| ~ 0.4 alone takes an f32 PyTorch evaluation of these steps to 0.7 - 1.1 of the bound by
    # step 16 (here: 0.18 - 0.27; profiles/r14_trainer_edges.txt)
    theta.copy_(0.01 * torch.randn(Pn, device=DEV, generator=g))
    m.zero_(); v.zero_()

    def run(steps, theta, m, v, label):
        p64 = {"w": theta.cpu().double().numpy().copy()}
        opt = P.Adam(p64, lr=LR, epsilon=EPS)
        t32, m32, v32 = theta.clone(), torch.zeros_like(m), torch.zeros_like(v)      # the same steps in f32 PyTorch: printed, not asserted
        worst, worst32 = 0.0, 0.0
        for it in range(steps):
            gscale = 0.0 if it in (0, 17) else (1e-3, 1.0, 1e-6, 0.3)[it % 4]
            grad.copy_(gscale * torch.randn(Pn, device=DEV, generator=g))
            g64 = {"w": grad.cpu().double().numpy().copy()}
            g32 = grad.clone()
            before = theta.clone()
            kern.adam(theta, grad, m, v, lr=LR, eps=EPS, max_grad_norm=max_norm, grad_norm_out=norm)
            n64 = math.sqrt(float(np.sum(g64["w"] ** 2)))
            gc = P.clip_by_global_norm(g64, max_norm)[0] if max_norm > 0 else g64
            p64 = opt.step(p64, gc)
            if max_norm > 0:
                g32 = g32 * (max_norm / max(float(g32.norm()), max_norm))
            m32 = 0.9 * m32 + (1.0 - 0.9) * g32
            v32 = 0.999 * v32 + (1.0 - 0.999) * g32 * g32
            t32 = t32 - float(LR * math.sqrt(1.0 - 0.999 ** (it + 1)) / (1.0 - 0.9 ** (it + 1))) * m32 / (v32.sqrt() + EPS)
            assert abs(norm.item() - n64) <= 1e-5 * n64
            assert float(grad.abs().max()) == 0.0                       # zeroed for the next accumulation
            if it == 0:
                assert norm.item() == 0.0 and torch.equal(theta, before)
            atol = 1e-5 * LR * (it + 1) + 2e-7 * np.abs(p64["w"]).max()          # test_adam_kernel_is_tensorflows_adam...'s bound
            worst = max(worst, np.abs(theta.cpu().numpy() - p64["w"]).max() / atol)
            worst32 = max(worst32, np.abs(t32.cpu().numpy() - p64["w"]).max() / atol)
            np.testing.assert_allclose(theta.cpu().numpy(), p64["w"], rtol=0, atol=atol)
            # (the betas cross the C-ABI as f32: 1 - (float)0.999 is 1.3e-5 away from 0.001, relative - hence 1e-4 on the moments)
            np.testing.assert_allclose(m.cpu().numpy(), opt.m["w"], rtol=1e-4, atol=1e-6 * np.abs(opt.m["w"]).max() + 1e-30)
            np.testing.assert_allclose(v.cpu().numpy(), opt.v["w"], rtol=1e-4, atol=1e-6 * np.abs(opt.v["w"]).max() + 1e-30)
            guard_intact((F_t, Pn), (F_g, Pn), (F_m, Pn), (F_v, Pn), (F_n, 1))
        print("adam %s, %d steps: largest |theta - oracle| in units of the bound: kernel %.3f, f32 torch %.3f" % (label, steps, worst, worst32))

    run(tc.ADAM_STEPS, theta, m, v, "D=%d A=%d max_norm=%g" % (D, A, max_norm))
    kern.adam_reset()
    m.zero_(); v.zero_()
    run(3, theta, m, v, "after reset")            # (a step count left at 30 would put the second of these a fifth of lr off)
    kern.close()


# ================================================================ advantage statistics
@pytest.mark.parametrize("nmb", tc.STATS_NMB)
@pytest.mark.parametrize("mb", tc.STATS_MB)
def test_minibatch_stats_against_numpy(mb, nmb):
    from trex_gym import _capi
    kern = _capi.Policy(64, 4, 2, 64, 0)
    rng = np.random.default_rng(900 + mb + nmb)
    N = nmb * mb + 50
    adv64 = tc.f32r(2.0 * rng.standard_normal(N) + 0.5)
    perm64 = rng.permutation(N).astype(np.int64)
    stats, F_s = guarded(nmb, 2)
    kern.minibatch_stats(dev32(adv64), torch.from_numpy(perm64).to(DEV), nmb, mb, stats)
    guard_intact((F_s, nmb))
    for k in range(nmb):
        a = adv64[perm64[k * mb:(k + 1) * mb]]
        assert abs(stats[k, 0].item() - a.mean()) < 1e-6
        if mb == 1:
            assert stats[k, 1].item() == 1e8                           # std = 0: 1 / (0 + 1e-8)
        else:
            assert abs(stats[k, 1].item() - 1.0 / (a.std() + 1e-8)) < 1e-5 * stats[k, 1].item()
    kern.close()


# ================================================================ the learner
_DEVICE_CASES = {}


def learner_inputs(name):
    """(case, device tensors of its rollout buffers): uploaded once, shared, never written by a test"""
    if name not in _DEVICE_CASES:
        case = tc.learn_case_by_name(name)
        t = {k: dev32(case[k]) for k in ("obs", "act", "logp_old", "value_old", "adv", "ret")}
        t["perm"] = torch.from_numpy(case["perm"]).to(DEV)
        t["stats"] = torch.from_numpy(case["adv_stats"]).to(DEV)
        _DEVICE_CASES[name] = (case, t)
    return _DEVICE_CASES[name]


class LearnerRun:
    """fresh theta / m / v / grad / loss sums, each with a guard region; one native call; the results as f64 numpy"""

    def __init__(self, kern, case, t, sums="zero", first=None, mb=None, grad_scale=None, theta=None):
        Pn = kern.param_count
        (self.theta, self.F_t), (self.grad, self.F_g), (self.m, self.F_m), (self.v, self.F_v) = (guarded(Pn) for _ in range(4))
        self.sums, self.F_s = guarded(2)
        self.Pn = Pn
        self.theta.copy_(torch.from_numpy(tc._params_to_theta(kern.layout, Pn, case["params"])).to(DEV) if theta is None else theta)
        self.theta0 = self.theta.clone()
        self.grad.fill_(7.0)                # whatever it held is overwritten, not accumulated
        self.m.zero_(); self.v.zero_(); self.sums.zero_()
        first = case["first"] if first is None else first
        mb = case["mb"] if mb is None else mb
        s = None if sums is None else self.sums
        if grad_scale is None:
            kern.minibatch_step(self.theta, self.grad, self.m, self.v, t["obs"], t["act"], t["logp_old"], t["value_old"], t["adv"],
                                t["ret"], t["perm"], first, mb, t["stats"], cliprange=tc.CLIPRANGE, ent_coef=case["ent_coef"],
                                vf_coef=tc.VF_COEF, lr=LR, eps=EPS, max_grad_norm=MAXN, loss_sums=s)
        else:
            kern.minibatch_grad(self.theta, self.grad, t["obs"], t["act"], t["logp_old"], t["value_old"], t["adv"], t["ret"],
                                t["perm"], first, mb, t["stats"], cliprange=tc.CLIPRANGE, ent_coef=case["ent_coef"],
                                vf_coef=tc.VF_COEF, grad_scale=grad_scale, loss_sums=s)
        torch.cuda.synchronize()
        guard_intact((self.F_t, Pn), (self.F_g, Pn), (self.F_m, Pn), (self.F_v, Pn), (self.F_s, 2))

    def same_as(self, other):
        return all(torch.equal(a, b) for a, b in ((self.F_g, other.F_g), (self.F_t, other.F_t), (self.F_s, other.F_s),
                                                  (self.F_m, other.F_m), (self.F_v, other.F_v)))


def grad_violation(got, want, rtol):
    """max over the elements of |got - want| / (rtol |want| + 1e-5 max|want|): <= 1 is assert_allclose's pass"""
    return float((np.abs(got - want) / (rtol * np.abs(want) + 1e-5 * np.abs(want).max())).max())


def autograd_gradient(kern, case, t):
    """f32 PyTorch autograd of the same loss on the same parameters: the second witness"""
    pol = make_policy(kern, case["params"])
    idx = torch.from_numpy(case["idx"]).to(DEV)
    obs, act, logp0, val0, adv, ret = (t[k].index_select(0, idx) for k in ("obs", "act", "logp_old", "value_old", "adv", "ret"))
    c = tc.CLIPRANGE
    a_n = (adv - t["stats"][0]) * t["stats"][1]
    dd = pol.dist(obs)
    ratio = (dd.log_prob(act).sum(-1) - logp0).exp()
    pg = torch.max(-a_n * ratio, -a_n * ratio.clamp(1 - c, 1 + c)).mean()
    v = pol.value(obs)
    vclip = val0 + (v - val0).clamp(-c, c)
    vf = 0.5 * torch.max((v - ret) ** 2, (vclip - ret) ** 2).mean()
    (pg - case["ent_coef"] * dd.entropy().sum(-1).mean() + tc.VF_COEF * vf).backward()
    return pol.grad.detach().cpu().double().numpy(), pg.item(), vf.item()


def check_learner_step(kern, case, t, run, label):
    """grad_dev (unclipped), both loss sums and the parameter update of one minibatch_step against the oracle; the gradient also
    against autograd. Prints the measured deviations of the kernel and of f32 PyTorch."""
    q = case["q"]
    out, gflat = q["out"], tc._grads_to_flat(kern, q["grads"])
    got = run.grad.cpu().double().numpy()
    g_auto, pg32, vf32 = autograd_gradient(kern, case, t)
    sums = run.sums.cpu().double().numpy()
    print("%s: gradient vs oracle, in units of the tolerance: kernel %.3f, f32 torch %.3f; max|g| %.3e; loss rel: kernel %.1e %.1e, "
          "torch %.1e %.1e" % (label, grad_violation(got, gflat, 1e-4), grad_violation(g_auto, gflat, 1e-4), np.abs(gflat).max(),
                               abs(sums[0] - out["pg_loss"]) / max(1.0, abs(out["pg_loss"])), abs(sums[1] - out["vf_loss"]) / max(1.0, abs(out["vf_loss"])),
                               abs(pg32 - out["pg_loss"]) / max(1.0, abs(out["pg_loss"])), abs(vf32 - out["vf_loss"]) / max(1.0, abs(out["vf_loss"]))))
    scale = np.abs(gflat).max()
    assert np.isfinite(got).all() and scale > 0
    np.testing.assert_allclose(got, gflat, rtol=1e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(got, g_auto, rtol=1e-3, atol=1e-5 * scale)
    assert abs(sums[0] - out["pg_loss"]) <= 1e-5 * max(1.0, abs(out["pg_loss"]))
    assert abs(sums[1] - out["vf_loss"]) <= 1e-5 * max(1.0, abs(out["vf_loss"]))
    theta0 = run.theta0.cpu().double().numpy()
    gc, _ = P.clip_by_global_norm({"w": gflat}, MAXN)
    want = P.Adam({"w": theta0}, lr=LR, epsilon=EPS).step({"w": theta0.copy()}, gc)["w"]
    step = run.theta.cpu().double().numpy() - theta0
    big = np.abs(gc["w"]) > 1e-3 * np.abs(gc["w"]).max()
    print("%s: update: max |d| %.2e lr; where |g| > 1e-3 max|g| (%d elements): max rel %.1e" % (
        label, np.abs(step - (want - theta0)).max() / LR, big.sum(), (np.abs(step - (want - theta0))[big] / np.abs(want - theta0)[big]).max()))
    np.testing.assert_allclose(step, want - theta0, rtol=0, atol=0.02 * LR)
    np.testing.assert_allclose(step[big], (want - theta0)[big], rtol=1e-3, atol=1e-5 * LR)


@pytest.mark.parametrize("D,A", tc.LEARN_DIMS, ids=["D%d_A%d" % c for c in tc.LEARN_DIMS])
def test_learner_at_every_dimension_edge(D, A):
    """trex_policy_minibatch_step at mb = 70 (three tiles, the last holding 6 samples), first = 7 (not a multiple of the tile),
    ent_coef 0.01, for D on either side of 8, 32, 64 and at 96 (all staged columns, ~151 KB of LDS), A = 1 ... 32."""
    from trex_gym import _capi
    name = "dims_D%d_A%d" % (D, A)
    case, t = learner_inputs(name)
    kern = _capi.Policy(64, D, A, 64, 0)
    check_learner_step(kern, case, t, LearnerRun(kern, case, t), name)
    kern.close()


@pytest.mark.parametrize("mb,first", tc.LEARN_MBS, ids=["mb%d_first%d" % c for c in tc.LEARN_MBS])
def test_learner_at_every_minibatch_size_edge(mb, first):
    """D = 75, A = 25 at less than one tile, one tile +- 1 sample, and 64 / 65 / 128 tiles: one trip of learn_reduce_kernel, one
    trip and a tile, two trips (the trainer's real minibatch)."""
    from trex_gym import _capi
    name = "mb%d_first%d" % (mb, first)
    case, t = learner_inputs(name)
    kern = _capi.Policy(64, 75, 25, 64, 0)
    check_learner_step(kern, case, t, LearnerRun(kern, case, t), name)
    kern.close()


def test_learner_workspace_is_reused_by_smaller_minibatches():
    """One Policy object, minibatches of 33, 4096, 33, 1000 samples: the partial buffer grows once and the later, smaller
    minibatches read only their own tiles of it. Every call against the oracle; the second mb = 33 call bitwise as the first."""
    from trex_gym import _capi
    kern = _capi.Policy(64, 75, 25, 64, 0)
    runs = []
    for mb in tc.LEARN_REUSE_MBS:
        case, t = learner_inputs("reuse_mb%d" % mb)
        kern.adam_reset()
        runs.append(LearnerRun(kern, case, t))
        check_learner_step(kern, case, t, runs[-1], "reuse call %d (mb %d)" % (len(runs), mb))
    assert runs[2].same_as(runs[0])
    kern.close()


@pytest.mark.parametrize("name", ["mb4096_first5", "dims_D64_A25"])
def test_learner_is_bitwise_repeatable_and_adds_its_loss_sums(name):
    """the fixed-order reductions (learn_reduce_kernel, learn_adam_kernel): the same call on fresh copies gives the same bits, on
    the same and on another Policy object; loss_sums are ADDED to (x + x = 2 x exactly); loss_sums = None changes nothing else."""
    from trex_gym import _capi
    case, t = learner_inputs(name)
    kern = _capi.Policy(64, case["D"], case["A"], 64, 0)
    a = LearnerRun(kern, case, t)
    kern.adam_reset()
    b = LearnerRun(kern, case, t)
    other = _capi.Policy(64, case["D"], case["A"], 64, 0)
    c = LearnerRun(other, case, t)
    assert b.same_as(a) and c.same_as(a)
    kern.adam_reset()
    d = LearnerRun(kern, case, t, sums=None)
    assert torch.equal(d.F_g, a.F_g) and torch.equal(d.F_t, a.F_t) and float(d.sums.abs().max()) == 0.0
    # a second call into the same sums buffer
    kern.adam_reset()
    kern.minibatch_step(d.theta0.clone(), d.grad, torch.zeros_like(d.m), torch.zeros_like(d.v), t["obs"], t["act"], t["logp_old"],
                        t["value_old"], t["adv"], t["ret"], t["perm"], case["first"], case["mb"], t["stats"], cliprange=tc.CLIPRANGE,
                        ent_coef=case["ent_coef"], vf_coef=tc.VF_COEF, lr=LR, eps=EPS, max_grad_norm=MAXN, loss_sums=a.sums)
    assert torch.equal(a.sums, 2 * b.sums) and float(b.sums.abs().min()) > 0
    guard_intact((a.F_s, 2))
    kern.close(); other.close()


def test_minibatch_grad_scales_splits_and_leaves_the_step_count():
    """trex_policy_minibatch_grad on the 64-sample case: grad_scale = 0.5 gives bitwise half of minibatch_step's grad_dev and
    loss sums; theta is not touched and the Adam step count does not move (a following minibatch_step is the t = 1 update);
    the two 32-sample halves, each at grad_scale 0.5 with the WHOLE minibatch's advantage statistics, sum to the oracle's
    whole-minibatch gradient, their loss sums to its losses."""
    from trex_gym import _capi
    case, t = learner_inputs("split64")
    kern = _capi.Policy(64, case["D"], case["A"], 64, 0)
    whole = LearnerRun(kern, case, t)
    check_learner_step(kern, case, t, whole, "split64 whole")
    fresh = _capi.Policy(64, case["D"], case["A"], 64, 0)
    half = LearnerRun(fresh, case, t, grad_scale=0.5)
    assert torch.equal(half.grad, 0.5 * whole.grad) and torch.equal(half.sums, 0.5 * whole.sums)
    assert torch.equal(half.theta, half.theta0) and float(half.m.abs().max()) == 0.0 and float(half.v.abs().max()) == 0.0
    one = LearnerRun(fresh, case, t, grad_scale=1.0)
    assert torch.equal(one.grad, whole.grad) and torch.equal(one.sums, whole.sums)
    after = LearnerRun(fresh, case, t)                        # two minibatch_grad calls later: still the first Adam step
    assert after.same_as(whole)
    # the two halves
    q = case["q"]
    gflat = tc._grads_to_flat(kern, q["grads"])
    lo = LearnerRun(fresh, case, t, first=0, mb=32, grad_scale=0.5)
    hi = LearnerRun(fresh, case, t, first=32, mb=32, grad_scale=0.5)
    total = (lo.grad + hi.grad).cpu().double().numpy()
    print("split64 halves: gradient vs oracle in units of the tolerance: %.3f" % grad_violation(total, gflat, 1e-4))
    np.testing.assert_allclose(total, gflat, rtol=1e-4, atol=1e-5 * np.abs(gflat).max())
    sums = (lo.sums + hi.sums).cpu().double().numpy()
    assert abs(sums[0] - q["out"]["pg_loss"]) <= 1e-5 * max(1.0, abs(q["out"]["pg_loss"]))
    assert abs(sums[1] - q["out"]["vf_loss"]) <= 1e-5 * max(1.0, abs(q["out"]["vf_loss"]))
    # ... and the data-parallel recipe end to end: the summed gradient through trex_policy_adam is the whole minibatch's update
    theta, m, v = whole.theta0.clone(), torch.zeros_like(whole.m), torch.zeros_like(whole.v)
    fresh.adam_reset()
    fresh.adam(theta, lo.grad + hi.grad, m, v, lr=LR, eps=EPS, max_grad_norm=MAXN)
    np.testing.assert_allclose((theta - whole.theta0).cpu().numpy(), (whole.theta - whole.theta0).cpu().numpy(), rtol=0, atol=0.02 * LR)
    kern.close(); fresh.close()


def test_learner_refusals_stay():
    """TrexError, and nothing is launched: the gradient buffer keeps its fill. first < 0, mb = 0 and D = 97 are refused by the C host
    entry (csrc/ppo_learner.hip); a perm shorter than first + mb by the binding's length check (trex_gym/_capi.py, _ptr) - the
    C-ABI takes no perm length, so that is where the rule lives."""
    from trex_gym import _capi
    case, t = learner_inputs("split64")
    kern = _capi.Policy(64, case["D"], case["A"], 64, 0)
    wide = _capi.Policy(64, 97, 2, 64, 0)                    # D = 97: one column more than the learner stages
    Pn = max(kern.param_count, wide.param_count)
    theta, grad, m, v = torch.zeros(Pn, device=DEV), torch.full((Pn,), SENT, device=DEV), torch.zeros(Pn, device=DEV), torch.zeros(Pn, device=DEV)

    def step(k, tt, first, mb, perm):
        k.minibatch_step(theta[:k.param_count], grad[:k.param_count], m[:k.param_count], v[:k.param_count], tt["obs"], tt["act"], tt["logp_old"],
                         tt["value_old"], tt["adv"], tt["ret"], perm, first, mb, tt["stats"], loss_sums=None)

    for first, mb, perm in ((-1, 32, t["perm"]), (0, 0, t["perm"]), (-32, 32, t["perm"]), (case["N"] - 10, 32, t["perm"]),
                            (0, 64, t["perm"][:63].clone())):
        with pytest.raises(_capi.TrexError):
            step(kern, t, first, mb, perm)
        with pytest.raises(_capi.TrexError):
            kern.minibatch_grad(theta, grad, t["obs"], t["act"], t["logp_old"], t["value_old"], t["adv"], t["ret"], perm, first, mb, t["stats"])
    z = torch.zeros(64, device=DEV)
    tw = dict(obs=torch.zeros(64, 97, device=DEV), act=torch.zeros(64, 2, device=DEV), logp_old=z, value_old=z, adv=z, ret=z,
              stats=torch.tensor([0.0, 1.0], device=DEV))
    with pytest.raises(_capi.TrexError, match="obs_dim <= 96"):
        step(wide, tw, 0, 64, torch.arange(64, device=DEV))
    torch.cuda.synchronize()
    assert bool((grad == SENT).all()) and float(theta.abs().max()) == 0.0
    kern.close(); wide.close()
