"""The privileged critic on the device (include/trex_policy_critic.h; the CRITIC instantiations of act_kernel and learn_grad_kernel in
csrc/policy_step.hip and csrc/ppo_learner.hip, the statistics kernels on a second block) on the cases of tests/critic_cases.py,
which tests/test_critic_ref.py qualifies on the CPU: every comparison is against the f64 reference tests/critic_ref.py, and - bit
for bit - against the symmetric kernels fed one half each, whose order of accumulation the critic instantiations share.

Every output buffer has a guard region of GUARD rows behind it, filled with a sentinel that must survive the call.

Tolerances are the project's own (header of tests/test_gpu_policy.py, restated in tests/test_gpu_trainer_edges.py): policy outputs
and values 1e-5 relative with that file's absolute floors (actions, value 2e-5; log-probability 3e-4); obs_out and obs_v_out 1e-6;
f64 running moments 1e-10; gradient rtol 1e-4 + 1e-5 max|g| against the reference; losses 1e-5; minibatch_step against
minibatch_grad + adam 2 % of lr."""
import numpy as np
import pytest
import torch

import critic_cases as cc
import critic_ref as CR
import trainer_cases as tc
from gpu_support import DEV, make_vec, replay_equals_eager
from oracle import ppo_oracle as P
from test_gpu_trainer_edges import EPS, LR, MAXN, SENT, dev32, grad_violation, guard_intact, guarded

pytestmark = pytest.mark.gpu


def _capi():
    from trex_gym import _capi, critic_capi
    return _capi, critic_capi


def critic_policy(n, D, Dv, A):
    """(Policy, PolicyCritic) with the critic width set; the layout is the header's"""
    K, CC = _capi()
    kern = K.Policy(n, D, A, 64, 0)
    crit = CC.PolicyCritic(kern)
    assert crit.set(Dv) == Dv
    assert CR.layout_rule(D, A, Dv) == ({k: (o, tuple(s)) for k, (o, s) in crit.layout.items()}, crit.param_count)
    return kern, crit


def theta_of(layout, count, params):
    return torch.from_numpy(tc._params_to_theta(layout, count, params)).to(DEV)


def flat_grads(layout, count, grads):
    class _L:
        pass
    k = _L()
    k.layout, k.param_count = layout, count
    return tc._grads_to_flat(k, grads)


def block(layout, flat, name):
    off, shape = layout[name]
    return flat[off:off + int(np.prod(shape))]


# ================================================================ act
class ActRun:
    def __init__(self, crit, theta, rows, rows_v, noise, n, D, Dv, A, **kw):
        (self.actions, self.F_a), (self.obs, self.F_o), (self.obs_v, self.F_ov) = guarded(n, A), guarded(n, D), guarded(n, Dv)
        (self.act_b, self.F_b), (self.logp, self.F_l), (self.val, self.F_v) = guarded(n, A), guarded(n), guarded(n)
        crit.act(theta, rows, rows_v, noise, self.actions, self.obs, self.obs_v, self.act_b, self.logp, self.val, clip_obs=tc.CLIP_OBS, **kw)
        torch.cuda.synchronize()
        self.fulls = ((self.F_a, n), (self.F_o, n), (self.F_ov, n), (self.F_b, n), (self.F_l, n), (self.F_v, n))
        guard_intact(*self.fulls)

    def policy_side(self):
        return (self.F_a, self.F_o, self.F_b, self.F_l)


@pytest.mark.parametrize("index", range(len(cc.ACT_CASES)), ids=["D%d_Dv%d_A%d_n%d" % c for c in cc.ACT_CASES])
def test_act_with_a_critic_row(index):
    K, CC = _capi()
    D, Dv, A, n = cc.ACT_CASES[index]
    c = cc.act_case(D, Dv, A, n, index)
    kern, crit = critic_policy(n, D, Dv, A)
    theta = theta_of(crit.layout, crit.param_count, c["params"])
    kern.set_stats(c["stats"])
    crit.set_stats(c["stats_v"])
    got_st = crit.get_stats()
    assert np.array_equal(got_st["mean"], c["stats_v"]["mean"]) and np.array_equal(got_st["var"], c["stats_v"]["var"]) and got_st["count"] == 100.0
    rows, rows_v, noise = dev32(c["rows"]), dev32(c["rows_v"]), dev32(c["noise"])
    assert rows.shape[1] == c["row_stride"] and rows_v.shape[1] == c["stride_v"] != c["row_stride"]
    r = ActRun(crit, theta, rows, rows_v, noise, n, D, Dv, A)
    got = {k: v.cpu().double().numpy() for k, v in dict(actions=r.actions, obs=r.obs, obs_v=r.obs_v, logp=r.logp, val=r.val).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    # ---- the f64 reference
    mean64, ls64, _ = CR.forward(c["params"], c["obs_n"], c["obs_v_n"])
    print("act D=%d Dv=%d A=%d n=%d: max |d| vs reference: obs %.2e obs_v %.2e actions %.2e value %.2e logp %.2e" % (
        D, Dv, A, n, np.abs(got["obs"] - c["obs_n"]).max(), np.abs(got["obs_v"] - c["obs_v_n"]).max(),
        np.abs(got["actions"] - c["actions"]).max(), np.abs(got["val"] - c["value"]).max(), np.abs(-got["logp"] - c["neglogp"]).max()))
    np.testing.assert_allclose(got["obs"], c["obs_n"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["obs_v"], c["obs_v_n"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["actions"], c["actions"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got["val"], c["value"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(-got["logp"], P.neglogp(mean64, ls64, got["actions"]), rtol=1e-5, atol=3e-4)
    np.testing.assert_allclose(-got["logp"], c["neglogp"], rtol=1e-5, atol=3e-4)
    assert torch.equal(r.act_b, r.actions)
    # ---- bit for bit the symmetric kernels, one half each
    sym_p, sym_v = K.Policy(n, D, A, 64, 0), K.Policy(n, Dv, A, 64, 0)
    sym_p.set_stats(c["stats"])
    sym_v.set_stats(c["vf"]["stats"])
    th_p, th_v = theta_of(sym_p.layout, sym_p.param_count, c["pi"]["params"]), theta_of(sym_v.layout, sym_v.param_count, c["vf"]["params"])
    (a_p, _), (o_p, _), (l_p, _), (v_p, _), (a_v, _), (o_v, _), (v_v, _) = (guarded(n, A), guarded(n, D), guarded(n), guarded(n),
                                                                         guarded(n, A), guarded(n, Dv), guarded(n))
    sym_p.act(th_p, rows, noise, a_p, o_p, None, l_p, v_p, clip_obs=tc.CLIP_OBS)
    sym_v.act(th_v, rows_v, noise, a_v, o_v, None, None, v_v, clip_obs=tc.CLIP_OBS)
    assert torch.equal(r.actions, a_p) and torch.equal(r.logp, l_p) and torch.equal(r.obs, o_p)
    assert torch.equal(r.val, v_v) and torch.equal(r.obs_v, o_v)
    assert not torch.equal(r.val, v_p)
    # ---- independence: other critic rows leave the policy's outputs alone, other policy rows leave the value alone
    g = torch.Generator(device=DEV).manual_seed(index)
    r2 = ActRun(crit, theta, rows, torch.randn(rows_v.shape, device=DEV, generator=g), noise, n, D, Dv, A)
    assert all(torch.equal(x, y) for x, y in zip(r2.policy_side(), r.policy_side())) and not torch.equal(r2.val, r.val)
    r3 = ActRun(crit, theta, torch.randn(rows.shape, device=DEV, generator=g), rows_v, noise, n, D, Dv, A)
    assert torch.equal(r3.F_v, r.F_v) and torch.equal(r3.F_ov, r.F_ov) and not torch.equal(r3.actions, r.actions)
    # ---- rows_v = None: the policy alone - the same actions, nothing else
    actions2, F_a2 = guarded(n, A)
    crit.act(theta, rows, None, noise, actions2, clip_obs=tc.CLIP_OBS)
    assert torch.equal(actions2, r.actions)
    guard_intact((F_a2, n))
    # ---- value_only: the same values bitwise, with no policy row at all, and nothing else is touched
    keep = [f.clone() for f in (r.F_a, r.F_o, r.F_ov, r.F_b, r.F_l)]
    val2, F_v2 = guarded(n)
    crit.act(theta, None, rows_v, None, None, value_out=val2, value_only=True, clip_obs=tc.CLIP_OBS)
    assert torch.equal(val2, r.val)
    guard_intact((F_v2, n))
    val2.fill_(SENT)
    crit.act(theta, rows, rows_v, noise, r.actions, r.obs, r.obs_v, r.act_b, r.logp, val2, clip_obs=tc.CLIP_OBS, value_only=True)
    assert torch.equal(val2, r.val) and all(torch.equal(k, f) for k, f in zip(keep, (r.F_a, r.F_o, r.F_ov, r.F_b, r.F_l)))
    for k in (kern, sym_p, sym_v):
        k.close()


# ================================================================ critic observe
@pytest.mark.parametrize("n,Dv", cc.OBSERVE_CASES, ids=["n%d_Dv%d" % c for c in cc.OBSERVE_CASES])
def test_critic_observe_is_a_running_mean_std_of_its_own(n, Dv):
    """trex_policy_critic_observe == RunningMeanStd over Dv columns after every block; the columns behind Dv hold NaN; the
    observation and return statistics, the raw-reward sum and the discounted returns - moved off their initial values by a reward
    step first - stay bitwise as they were. n = 2049: 33 workgroup partials, two trips of the merge."""
    D = 5
    kern, crit = critic_policy(n, D, Dv, 3)
    rng = np.random.default_rng(n + Dv)
    first = np.asarray(rng.standard_normal((n, D + 2)), np.float32)
    first[:, D + 1] = 0.0
    kern.observe(torch.from_numpy(first).to(DEV), True, 0.99)
    st0 = kern.get_stats()
    ret0, F_r = guarded(n)
    kern.get_returns(ret0)
    ret0 = ret0.clone()
    assert st0["ret_count"] > 1.0 and st0["raw_reward_sum"] != 0.0
    fresh = crit.get_stats()
    assert (fresh["mean"] == 0).all() and (fresh["var"] == 1).all() and fresh["count"] == 1e-4
    rms = P.RunningMeanStd((Dv,))
    for rows64 in cc.observe_sequence(n, Dv):
        assert np.isnan(rows64[:, Dv:]).all()
        crit.observe(dev32(rows64))
        rms.update(rows64[:, :Dv])
        st = crit.get_stats()
        np.testing.assert_allclose(st["mean"], rms.mean, rtol=1e-10)
        np.testing.assert_allclose(st["var"], rms.var, rtol=1e-10)
        assert abs(st["count"] - rms.count) < 1e-9
    st1 = kern.get_stats()
    assert all(np.array_equal(np.asarray(st1[k]), np.asarray(st0[k])) for k in st0)
    ret1, _ = guarded(n)
    kern.get_returns(ret1)
    assert torch.equal(ret1, ret0)
    # a second object fed the same blocks ends bitwise equal (fixed-order merge)
    kern2, crit2 = critic_policy(n, D, Dv, 3)
    for rows64 in cc.observe_sequence(n, Dv):
        crit2.observe(dev32(rows64))
    a, b = crit.get_stats(), crit2.get_stats()
    assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    # setting the width again starts the moments afresh and leaves the Adam step count and the other statistics alone
    crit.set(Dv)
    again = crit.get_stats()
    assert (again["mean"] == 0).all() and (again["var"] == 1).all() and again["count"] == 1e-4
    assert all(np.array_equal(np.asarray(kern.get_stats()[k]), np.asarray(st0[k])) for k in st0)
    kern.close(); kern2.close()


# ================================================================ the learner
_DEVICE_CASES = {}


def learner_inputs(index):
    """(case, device tensors of its rollout buffers): uploaded once, shared, never written by a test"""
    if index not in _DEVICE_CASES:
        case = cc.learn_case_by_index(index)
        t = {k: dev32(case[k]) for k in ("obs", "obs_v", "act", "logp_old", "value_old", "adv", "ret")}
        t["perm"] = torch.from_numpy(case["perm"]).to(DEV)
        t["stats"] = torch.from_numpy(case["adv_stats"]).to(DEV)
        for half in ("pi", "vf"):       # what the symmetric witnesses read: that half's own buffers
            t[half] = {k: dev32(case[half][k]) for k in ("obs", "value_old", "ret")}
        _DEVICE_CASES[index] = (case, t)
    return _DEVICE_CASES[index]


class Run:
    """fresh theta / m / v / grad / loss sums, each with a guard region; one native call; `call` picks the entry point"""

    def __init__(self, count, theta, call):
        (self.theta, self.F_t), (self.grad, self.F_g), (self.m, self.F_m), (self.v, self.F_v) = (guarded(count) for _ in range(4))
        self.sums, self.F_s = guarded(2)
        self.theta.copy_(theta)
        self.theta0 = self.theta.clone()
        self.grad.fill_(7.0)
        self.m.zero_(); self.v.zero_(); self.sums.zero_()
        call(self)
        torch.cuda.synchronize()
        guard_intact((self.F_t, count), (self.F_g, count), (self.F_m, count), (self.F_v, count), (self.F_s, 2))

    def same_as(self, other):
        return all(torch.equal(a, b) for a, b in ((self.F_g, other.F_g), (self.F_t, other.F_t), (self.F_s, other.F_s),
                                                  (self.F_m, other.F_m), (self.F_v, other.F_v)))


def _step_kw(case):
    return dict(cliprange=tc.CLIPRANGE, ent_coef=case["ent_coef"], vf_coef=tc.VF_COEF, lr=LR, eps=EPS, max_grad_norm=MAXN)


@pytest.mark.parametrize("index", range(len(cc.LEARN_CASES)), ids=["D%d_Dv%d_A%d_mb%d_first%d" % c for c in cc.LEARN_CASES])
def test_learner_with_a_critic_buffer(index):
    K, CC = _capi()
    case, t = learner_inputs(index)
    D, Dv, A, mb, first = cc.LEARN_CASES[index]
    kern, crit = critic_policy(64, D, Dv, A)
    lay, count = crit.layout, crit.param_count
    theta = theta_of(lay, count, case["params"])

    def step(r):
        crit.minibatch_step(r.theta, r.grad, r.m, r.v, t["obs"], t["obs_v"], t["act"], t["logp_old"], t["value_old"], t["adv"], t["ret"],
                            t["perm"], first, mb, t["stats"], loss_sums=r.sums, **_step_kw(case))

    run = Run(count, theta, step)
    # ---- the gradient and the losses against the f64 reference
    q = case["q"]
    want = flat_grads(lay, count, q["grads"])
    got = run.grad.cpu().double().numpy()
    sums = run.sums.cpu().double().numpy()
    scale = np.abs(want).max()
    print("learner D=%d Dv=%d mb=%d: gradient vs reference, in units of the tolerance: %.3f; max|g| %.3e; loss rel %.1e %.1e" % (
        D, Dv, mb, grad_violation(got, want, 1e-4), scale, abs(sums[0] - q["out"]["pg_loss"]) / max(1.0, abs(q["out"]["pg_loss"])),
        abs(sums[1] - q["out"]["vf_loss"]) / max(1.0, abs(q["out"]["vf_loss"]))))
    assert np.isfinite(got).all() and scale > 0
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * scale)
    assert abs(sums[0] - q["out"]["pg_loss"]) <= 1e-5 * max(1.0, abs(q["out"]["pg_loss"]))
    assert abs(sums[1] - q["out"]["vf_loss"]) <= 1e-5 * max(1.0, abs(q["out"]["vf_loss"]))
    # ---- bit for bit the symmetric learner: the pi blocks and logstd at D on the policy half, the vf blocks at Dv fed obs_v
    kw = dict(cliprange=tc.CLIPRANGE, ent_coef=case["ent_coef"], vf_coef=tc.VF_COEF)
    sym_p, sym_v = K.Policy(64, D, A, 64, 0), K.Policy(64, Dv, A, 64, 0)
    g_p, g_v = torch.zeros(sym_p.param_count, device=DEV), torch.zeros(sym_v.param_count, device=DEV)
    sym_p.minibatch_grad(theta_of(sym_p.layout, sym_p.param_count, case["pi"]["params"]), g_p, t["obs"], t["act"], t["logp_old"],
                         t["pi"]["value_old"], t["adv"], t["pi"]["ret"], t["perm"], first, mb, t["stats"], **kw)
    sym_v.minibatch_grad(theta_of(sym_v.layout, sym_v.param_count, case["vf"]["params"]), g_v, t["obs_v"], t["act"], t["logp_old"],
                         t["value_old"], t["adv"], t["ret"], t["perm"], first, mb, t["stats"], **kw)
    for name in tc.PARAM_NAMES:
        if name.startswith("vf."):
            assert torch.equal(block(lay, run.grad, name), block(sym_v.layout, g_v, name)), name
        else:
            assert torch.equal(block(lay, run.grad, name), block(sym_p.layout, g_p, name)), name
    # ---- two runs are bitwise equal; minibatch_grad gives the step's gradient and moves nothing; grad + adam is the step
    kern.adam_reset()
    assert Run(count, theta, step).same_as(run)

    def grad_only(r):
        crit.minibatch_grad(r.theta, r.grad, t["obs"], t["obs_v"], t["act"], t["logp_old"], t["value_old"], t["adv"], t["ret"], t["perm"],
                            first, mb, t["stats"], loss_sums=r.sums, grad_scale=1.0, **kw)

    g = Run(count, theta, grad_only)
    assert torch.equal(g.grad, run.grad) and torch.equal(g.sums, run.sums) and torch.equal(g.theta, g.theta0)
    assert float(g.m.abs().max()) == 0.0 and float(g.v.abs().max()) == 0.0
    kern.adam_reset()
    crit.adam(g.theta, g.grad, g.m, g.v, lr=LR, eps=EPS, max_grad_norm=MAXN)
    np.testing.assert_allclose((g.theta - g.theta0).cpu().numpy(), (run.theta - run.theta0).cpu().numpy(), rtol=0, atol=0.02 * LR)
    assert float((run.theta - run.theta0).abs().max()) > 0.1 * LR
    for k in (kern, sym_p, sym_v):
        k.close()


# ================================================================ refusals
def test_refusals_by_name_with_nothing_launched():
    K, CC = _capi()
    E = K.TrexError
    case, t = learner_inputs(2)                     # (33, 64, 25)
    D, Dv, A, mb, first = cc.LEARN_CASES[2]
    n = 64
    kern, crit = critic_policy(n, D, Dv, A)
    plain = K.Policy(n, D, A, 64, 0)
    bare = CC.PolicyCritic(plain)
    count = max(crit.param_count, plain.param_count)
    theta, m, v = (torch.zeros(count, device=DEV) for _ in range(3))
    grad = torch.full((count,), SENT, device=DEV)
    rows, rows_v, noise = torch.zeros(n, D + 2, device=DEV), torch.zeros(n, Dv + 3, device=DEV), torch.zeros(n, A, device=DEV)
    (actions, F_a), (obs_o, F_o), (obs_vo, F_ov), (val, F_v) = guarded(n, A), guarded(n, D), guarded(n, Dv), guarded(n)
    st_v, st = crit.get_stats(), kern.get_stats()

    def learn(obj, with_v, first=first, mb=mb, step=True, **over):
        a = dict(t, **over)
        args = [a["obs"]] + ([a["obs_v"]] if with_v else []) + [a["act"], a["logp_old"], a["value_old"], a["adv"], a["ret"], a["perm"], first, mb, a["stats"]]
        if step:
            obj.minibatch_step(theta, grad, m, v, *args)
        else:
            obj.minibatch_grad(theta, grad, *args)

    # the plain calls on an object with a critic width
    with pytest.raises(E, match="critic width set"):
        kern.act(theta, rows, noise, actions, obs_o, None, None, val)
    for step in (True, False):
        with pytest.raises(E, match="critic width set"):
            learn(kern, False, step=step)
    # the critic calls on an object without one
    for call in (lambda: bare.observe(rows_v), lambda: bare.get_stats(), lambda: bare.set_stats(dict(mean=[], var=[], count=1.0)),
                 lambda: bare.act(theta, rows, rows_v, noise, actions, obs_o, None, None, None, val),
                 lambda: learn(bare, True), lambda: learn(bare, True, step=False)):
        with pytest.raises(E, match="no critic width is set"):
            call()
    # a width outside [0, 126]: the object unchanged
    for bad in (-1, 127, 1000):
        with pytest.raises(E, match="critic_dim must be in"):
            crit.set(bad)
        assert K.lib.trex_policy_critic_dim(kern.h) == Dv and K.lib.trex_policy_param_count(kern.h) == crit.param_count
    crit.dim = Dv
    # stride_v < Dv
    with pytest.raises(E, match="stride_v < critic_dim"):
        crit.observe(torch.zeros(n, Dv - 1, device=DEV))
    with pytest.raises(E, match="stride_v < critic_dim"):
        crit.act(theta, rows, torch.zeros(n, Dv - 1, device=DEV), noise, actions, obs_o, obs_vo, None, None, val)
    with pytest.raises(E, match="row_stride < obs_dim"):
        crit.act(theta, torch.zeros(n, D - 1, device=DEV), rows_v, noise, actions, obs_o, obs_vo, None, None, val)
    # the policy alone writes no value; value_only needs the critic row and a place for the values
    with pytest.raises(E, match="value_out and obs_v_out must be null"):
        crit.act(theta, rows, None, noise, actions, obs_o, None, None, None, val)
    with pytest.raises(E, match="value_out and obs_v_out must be null"):
        crit.act(theta, rows, None, noise, actions, obs_o, obs_vo)
    with pytest.raises(E, match="value_only needs"):
        crit.act(theta, rows, None, noise, actions, value_out=val, value_only=True)
    with pytest.raises(E, match="value_only needs"):
        crit.act(theta, rows, rows_v, noise, actions, value_only=True)
    with pytest.raises(E):
        crit.act(theta, None, rows_v, noise, actions)
    # host pointers and short buffers: the binding's check, and the C entry's own on the raw pointer
    with pytest.raises(E, match="device memory"):
        crit.observe(rows_v.cpu())
    with pytest.raises(E, match="device memory"):
        crit.act(theta, rows, rows_v.cpu(), noise, actions)
    with pytest.raises(E, match="at least"):
        crit.act(theta, rows, rows_v, noise, actions, obs_v_out=torch.zeros(n * Dv - 1, device=DEV))
    with pytest.raises(E, match="at least"):
        crit.act(theta[:crit.param_count - 1], rows, rows_v, noise, actions)
    with pytest.raises(E, match="at least"):
        learn(crit, True, obs_v=t["obs_v"][:-1])
    with pytest.raises(E, match="expected a tensor of shape"):
        crit.observe(torch.zeros(n - 1, Dv, device=DEV))
    host = np.zeros((n, Dv), np.float32)
    assert K.lib.trex_policy_critic_observe(kern.h, host.ctypes.data, Dv, None) == K.E_INVALID
    host_st = crit.get_stats()
    assert all(np.array_equal(np.asarray(host_st[k]), np.asarray(st_v[k])) for k in st_v)
    # the learner's own refusals hold with a critic: sizes, perm length, and Dv > 96
    for f, b in ((-1, 32), (0, 0)):
        with pytest.raises(E):
            learn(crit, True, first=f, mb=b)
    with pytest.raises(E):
        learn(crit, True, first=0, mb=64, perm=t["perm"][:63].clone())
    wide_k, wide = critic_policy(n, 4, 97, 2)
    z = torch.zeros(n, device=DEV)
    with pytest.raises(E, match="critic_dim <= 96"):
        wide.minibatch_step(theta, grad, m, v, torch.zeros(n, 4, device=DEV), torch.zeros(n, 97, device=DEV), torch.zeros(n, 2, device=DEV),
                            z, z, z, z, torch.arange(n, device=DEV), 0, n, torch.tensor([0.0, 1.0], device=DEV))
    # ... while the act launch takes the wide critic (126 is the object's limit, 96 the learner's)
    wide.act(theta, torch.zeros(n, 4, device=DEV), torch.zeros(n, 97, device=DEV), torch.zeros(n, 2, device=DEV), torch.zeros(n, 2, device=DEV),
             value_out=z.clone())
    torch.cuda.synchronize()
    # nothing was launched, nothing moved
    assert bool((grad == SENT).all()) and float(theta.abs().max()) == 0.0 and float(m.abs().max()) == 0.0
    guard_intact((F_a, n), (F_o, n), (F_ov, n), (F_v, n))
    assert all(bool((x == SENT).all()) for x in (actions, obs_o, obs_vo, val))
    now_v, now = crit.get_stats(), kern.get_stats()
    assert all(np.array_equal(np.asarray(now_v[k]), np.asarray(st_v[k])) for k in st_v)
    assert all(np.array_equal(np.asarray(now[k]), np.asarray(st[k])) for k in st)
    # clearing the width gives the plain calls back, with the symmetric layout
    assert crit.set(0) == 0 and crit.param_count == plain.param_count
    kern.act(theta[:plain.param_count], rows, noise, actions, obs_o, None, None, val)
    for k in (kern, plain, wide_k):
        k.close()


# ================================================================ the object's lifetime
def _lifetime_inputs(n, D, A, widths, seed=11):
    """finite inputs of a rollout of one step: bitwise comparisons only, so any numbers do"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    t = dict(rows=r(n, D + 2), noise=r(n, A), obs=r(n, D), act=r(n, A), logp=r(n) - 3.0, val=r(n), adv=r(n), ret=r(n),
             tmean=r(n, A), tvalue=r(n), tlogstd=0.1 * r(A), perm=torch.randperm(n, generator=g).to(DEV),
             stats=torch.tensor([0.1, 0.9], device=DEV))
    for Dv in widths:
        t["rows_v%d" % Dv], t["obs_v%d" % Dv] = r(n, Dv + 3), r(n, Dv)
    return t


def test_one_object_through_its_lifetime_is_a_fresh_object_at_every_stage():
    """What the object owns - the moments of both blocks, the learner workspace, which trex_policy_set_critic drops because its
    row is as long as the parameter vector - through a life of one policy object: a plain minibatch step; a critic of width 5
    (observe, act, step); a critic of width 17 (the workspace goes, the moments start afresh; the same three calls); no critic
    again (a plain step, a distillation step). After every stage theta, m, v, the gradient, the loss sums, what the act wrote and
    the critic's moments are BITWISE those of the same calls on a freshly created object (the Adam step count of the long-lived
    one reset, as trex_policy_adam_reset does). n = 33: two tiles, the second ragged; mb = 33.

    Then 8 objects live and die, each through a critic and a 4096-sample step (a workspace of 5 MB: larger than the granule), and
    the device's free memory is where it started, to within one allocation granule (2 MiB, the fragment the driver maps device
    memory in; what an object of this size holds besides its workspace is below that resolution). Measured on an MI355X, with the
    parent's library and with this one: +0 bytes after the 8 objects - and +0 while one of them lives (the figure is printed), so
    the runtime serves allocations of this size from memory it already holds, and the check catches a leak only once it outgrows
    that; the bitwise stages above are what pins the ownership paths."""
    K, CC = _capi()
    from trex_gym import distill_capi
    n, D, A, mb = 33, 9, 3, 33
    t = _lifetime_inputs(n, D, A, (5, 17))
    kw = dict(cliprange=tc.CLIPRANGE, ent_coef=0.01, vf_coef=tc.VF_COEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
    dkw = dict(loss="kl", vf_coef=tc.VF_COEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
    def theta_for(count):
        return (0.1 * torch.randn(count, generator=torch.Generator(device="cpu").manual_seed(count))).to(DEV)

    def plain_step(kern):
        return Run(kern.param_count, theta_for(kern.param_count), lambda r: kern.minibatch_step(
            r.theta, r.grad, r.m, r.v, t["obs"], t["act"], t["logp"], t["val"], t["adv"], t["ret"], t["perm"], 0, mb, t["stats"],
            loss_sums=r.sums, **kw))

    def distill_step(kern):
        return Run(kern.param_count, theta_for(kern.param_count), lambda r: distill_capi.PolicyDistill(kern).minibatch_step(
            r.theta, r.grad, r.m, r.v, t["obs"], t["tmean"], t["tvalue"], t["tlogstd"], t["perm"], 0, mb, loss_sums=r.sums, **dkw))

    def critic_stage(kern, crit, Dv):
        """set, observe, act, step -> (the step's Run, the act's outputs, the moments)"""
        assert crit.set(Dv) == Dv
        rows_v, obs_v = t["rows_v%d" % Dv], t["obs_v%d" % Dv]
        crit.observe(rows_v)
        theta = theta_for(crit.param_count)
        act = ActRun(crit, theta, t["rows"], rows_v, t["noise"], n, D, Dv, A)
        run = Run(crit.param_count, theta, lambda r: crit.minibatch_step(
            r.theta, r.grad, r.m, r.v, t["obs"], obs_v, t["act"], t["logp"], t["val"], t["adv"], t["ret"], t["perm"], 0, mb, t["stats"],
            loss_sums=r.sums, **kw))
        return run, [f for f, _ in act.fulls], crit.get_stats()

    def fresh():
        kern = K.Policy(n, D, A, 64, 0)
        return kern, CC.PolicyCritic(kern)

    def same_stage(a, b):
        return a[0].same_as(b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and \
            all(np.array_equal(np.asarray(a[2][k]), np.asarray(b[2][k])) for k in a[2])

    old, old_crit = fresh()
    # 1: a plain step
    w, _ = fresh()
    first = plain_step(old)
    assert first.same_as(plain_step(w)) and float((first.theta - first.theta0).abs().max()) > 0.1 * LR
    w.close()
    # 2, 3: a critic, then a wider one
    for Dv in (5, 17):
        old.adam_reset()
        got = critic_stage(old, old_crit, Dv)
        w, w_crit = fresh()
        want = critic_stage(w, w_crit, Dv)
        assert same_stage(got, want), Dv
        assert got[2]["count"] == 1e-4 + n and float((got[0].theta - got[0].theta0).abs().max()) > 0.1 * LR
        w.close()
    # 4: no critic again
    assert old_crit.set(0) == 0 and old_crit.param_count == old.param_count
    for step in (plain_step, distill_step):
        old.adam_reset()
        w, _ = fresh()
        got = step(old)
        assert got.same_as(step(w)) and float((got.theta - got.theta0).abs().max()) > 0.1 * LR, step.__name__
        w.close()
    old.adam_reset()
    assert plain_step(old).same_as(first)
    old.close()

    # ---- 8 objects live and die
    N = 4096
    big = _lifetime_inputs(N, D, A, (5,), seed=12)

    def a_life(alive=None):
        kern, crit = fresh()
        crit.set(5)
        crit.observe(t["rows_v5"])
        count, plain = crit.param_count, kern.param_count
        th, gr, m, v = (torch.zeros(max(count, plain), device=DEV) for _ in range(4))
        crit.minibatch_step(th[:count], gr[:count], m[:count], v[:count], big["obs"], big["obs_v5"], big["act"], big["logp"], big["val"], big["adv"], big["ret"], big["perm"],
                            0, N, big["stats"], **kw)
        crit.set(0)
        kern.minibatch_step(th[:plain], gr[:plain], m[:plain], v[:plain], t["obs"], t["act"],
                            t["logp"], t["val"], t["adv"], t["ret"], t["perm"], 0, mb, t["stats"], **kw)
        torch.cuda.synchronize()
        if alive is not None:
            alive.append(torch.cuda.mem_get_info()[0])
        kern.close()

    a_life()                                   # (what the runtime allocates on a first use is not the object's)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    alive = []
    for _ in range(8):
        a_life(alive)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print("free device memory before and after 8 objects: %d -> %d bytes (%+d); while one lives: %+d" % (
        free0, free1, free1 - free0, min(alive) - free0))
    assert free0 - free1 <= 2 << 20


# ================================================================ capture
def test_act_and_observe_replay_from_a_graph():
    """act with a critic passes gpu_support.replay_equals_eager (the rows change between capture and replay); the critic observe
    followed by the act - a launch chain that moves the moments - replays bitwise what the same chain gives eagerly from the same
    moments."""
    D, Dv, A, n = 75, 96, 25, 97
    c = cc.act_case(D, Dv, A, n, 5)
    kern, crit = critic_policy(n, D, Dv, A)
    theta = theta_of(crit.layout, crit.param_count, c["params"])
    kern.set_stats(c["stats"])
    crit.set_stats(c["stats_v"])
    rows, rows_v, noise = dev32(c["rows"]), dev32(c["rows_v"]), dev32(c["noise"])
    rows0, rows_v0 = rows.clone(), rows_v.clone()
    outs = [torch.zeros(n, A, device=DEV), torch.zeros(n, D, device=DEV), torch.zeros(n, Dv, device=DEV), torch.zeros(n, device=DEV),
            torch.zeros(n, device=DEV)]

    def act(o):
        crit.act(theta, rows, rows_v, noise, o[0], o[1], o[2], None, o[3], o[4], clip_obs=tc.CLIP_OBS)

    def other_rows():
        rows.mul_(0.5); rows_v.mul_(-0.7)

    replay_equals_eager(act, outs, other_rows, replays=2, changed=[0, 1, 2, 4])     # (the log-probability is the noise's: it need not move)
    # ---- observe + act: eager from the case's moments, then the captured chain from the same moments
    def chain(o):
        crit.observe(rows_v)
        act(o)

    results = []
    graph = None
    for mode in ("eager", "replay", "eager other rows", "replay other rows"):
        if "other" in mode:
            rows.copy_(rows0 * 1.5); rows_v.copy_(rows_v0 * 0.25)
        else:
            rows.copy_(rows0); rows_v.copy_(rows_v0)
        crit.set_stats(c["stats_v"])
        fresh = [torch.zeros_like(o) for o in outs]
        if mode.startswith("eager"):
            chain(fresh)
        else:
            if graph is None:
                torch.cuda.synchronize()
                side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(graph, stream=side):
                        chain(outs)
            for o in outs:
                o.zero_()
            graph.replay()
            fresh = [o.clone() for o in outs]
        torch.cuda.synchronize()
        results.append((fresh, crit.get_stats()))
    for (a, sa), (b, sb) in ((results[0], results[1]), (results[2], results[3])):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert all(np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])) for k in sa) and sa["count"] > n
    assert not torch.equal(results[0][0][4], results[2][0][4]) and not np.array_equal(results[0][1]["mean"], results[2][1]["mean"])
    del graph
    kern.close()


# ================================================================ the env's critic row and the trainer
PPO_KW = dict(nsteps=4, nminibatches=2, noptepochs=1)


def test_privileged_rows_follow_the_env():
    """critic.attach / critic.privileged on an env with the sensor model, the episode randomisation and the contact sensor: the
    row is clean_obs, then friction, the push force, the foot contact forces - refilled by step_tensor and reset_tensor - and a
    source that does not fit is left out whole and named."""
    from trex_gym import critic as C, randomize as Z, sensing as S
    from trex_gym.termination import foot_links
    n = 64
    env = make_vec(n, max_episode_steps=25)
    env.enable_contact_sensor(True)
    S.attach(env, S.typical(env), seed=1)
    Z.attach(env, Z.typical(env), seed=2)
    env.reset_tensor()
    C.privileged(env)
    feet = foot_links(env)
    Dv = 75 + 1 + 2 + 3 * len(feet)
    assert env.critic_rows.shape == (n, Dv) and len(env.critic_names) == Dv and env.critic_spec["dim"] == Dv
    assert env.critic_spec["left_out"] == [] and [s[0] for s in env.critic_spec["sources"]] == ["clean", "random", "push_force", "contact"]
    g = torch.Generator(device=DEV).manual_seed(0)
    lo, hi = torch.tensor(env.model.lower, device=DEV), torch.tensor(env.model.upper, device=DEV)
    touched = 0.0
    for _ in range(30):                             # (0.6 s: the robot, hung 0.39 m over the floor, lands; episodes end at 25 steps)
        env.step_tensor(lo + (hi - lo) * torch.rand(n, env.J, device=DEV, generator=g))
        assert torch.equal(env.critic_rows[:, :75], env.clean_obs) and not torch.equal(env.clean_obs, env.obs)
        env.random_api.info(values=env.random_values)
        t = [i for i, x in enumerate(env.randomization["terms"]) if x[0] == 1][0]
        assert torch.equal(env.critic_rows[:, 75], env.random_values[:, t, 0]) and float(env.critic_rows[:, 75].min()) >= 0.5
        force = torch.zeros(n, env.random_api.num_pushes, 3, device=DEV)
        env.random_api.info(push_force=force)
        assert torch.equal(env.critic_rows[:, 76:78], force[:, 0, :2])
        w = env.contact_wrench()
        bodies = [int(b) for b in env._link_bodies(feet)]
        assert torch.equal(env.critic_rows[:, 78:], w[:, bodies, :3].reshape(n, -1))
        touched = max(touched, float(env.critic_rows[:, 78:].abs().max()))
    assert touched > 0
    env.reset_tensor()
    assert torch.equal(env.critic_rows[:, :75], env.clean_obs)
    # a budget that the contact forces no longer fit in: left out whole
    C.privileged(env, max_width=80)
    assert env.critic_rows.shape == (n, 78) and env.critic_spec["left_out"] == ["foot_contact"]
    with pytest.raises(ValueError):
        C.attach(env, C.random("command"))
    C.attach(env, None)
    assert env.critic_rows is None and env.critic_spec is None
    env.step_tensor(torch.zeros(n, env.J, device=DEV))
    env.close()


def _agent(critic, seed=3, sensing=False, **kw):
    from trex_gym import critic as C, sensing as S
    from trex_gym.ppo import PPO
    env = make_vec(64, max_episode_steps=6)
    if sensing:
        S.attach(env, S.typical(env), seed=5)
    if critic:
        C.attach(env, C.clean())
    return PPO(env, seed=seed, critic=critic, **PPO_KW, **kw)


def test_ppo_with_the_clean_row_and_no_sensors_is_the_symmetric_trainer():
    """critic.attach(env, [clean()]) without a sensor model: Dv = D and the two rows are equal, so theta after one update is bit
    for bit the symmetric trainer's at the same seed - rollout, statistics, learner and all."""
    a = _agent(True)                               # (each agent seeds the generator when it is made: one after the other)
    th_a = a.policy.theta.clone()
    ia = a.update(a.collect())
    b = _agent(False)
    assert a.critic_dim == 75 and a.crit.param_count == b.kern.param_count and torch.equal(th_a, b.policy.theta)
    ib = b.update(b.collect())
    assert not torch.equal(th_a, a.policy.theta)
    assert torch.equal(a.b_obs_v, a.b_obs) and torch.equal(a.b_obs, b.b_obs) and torch.equal(a.b_val, b.b_val)
    assert torch.equal(a.policy.theta, b.policy.theta) and ia == ib
    sv, so = a.crit.get_stats(), a.kern.get_stats()
    assert np.array_equal(sv["mean"], so["obs_mean"]) and np.array_equal(sv["var"], so["obs_var"]) and sv["count"] == so["obs_count"]
    a.env.close(); b.env.close()


def test_ppo_reads_the_clean_row_beside_the_sensors():
    """with sensing.typical attached, b_obs_v[0] of a rollout is env.clean_obs as it was before the rollout, normalised with the critic
    moments of that instant and clipped - at obs_out's tolerance, 1e-6; the reference takes the moments as the kernel does, from
    their f32 image (csrc/policy_step.hip: `norm`) - and it is not what the policy read."""
    a = _agent(True, sensing=True)
    a.collect()                                   # (one rollout first: the envs and the moments leave the reset state)
    clean0, rows0 = a.env.clean_obs.clone(), a.env.obs.clone()
    st, so = a.crit.get_stats(), a.kern.get_stats()
    batch = a.collect()
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    want_v = np.clip((clean0.cpu().double().numpy() - f32(st["mean"])) * f32(1.0 / np.sqrt(st["var"] + 1e-8)), -10.0, 10.0)
    want_p = np.clip((rows0.cpu().double().numpy() - f32(so["obs_mean"])) * f32(1.0 / np.sqrt(so["obs_var"] + 1e-8)), -10.0, 10.0)
    print("b_obs_v[0] vs normalised clean_obs: max |d| %.2e; b_obs[0] vs normalised obs: %.2e" % (
        np.abs(a.b_obs_v[0].cpu().numpy() - want_v).max(), np.abs(a.b_obs[0].cpu().numpy() - want_p).max()))
    np.testing.assert_allclose(a.b_obs_v[0].cpu().numpy(), want_v, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(a.b_obs[0].cpu().numpy(), want_p, rtol=1e-6, atol=1e-6)
    assert not torch.equal(a.b_obs_v[0], a.b_obs[0]) and float((a.b_obs_v[0] - a.b_obs[0]).abs().max()) > 1e-3
    info = a.update(batch)
    assert all(np.isfinite(v) for v in info.values())
    with pytest.raises(ValueError, match="no critic row"):
        from trex_gym.ppo import PPO
        PPO(make_vec(8), critic=True, **PPO_KW)
    a.env.close()


def test_ppo_graph_update_is_the_eager_update():
    """use_graphs=True - the rollout with its critic launches and the env's critic fill captured, the epoch captured - against the
    eager trainer: the rollout buffers and theta after the update bit for bit. The captured epoch draws its permutation at the
    generator state its warm-up leaves (two draws of N numbers); the eager side is put at the same state."""
    e = _agent(True, sensing=True)                  # (each agent seeds the generator when it is made: one after the other)
    be = e.collect()
    g = _agent(True, sensing=True, use_graphs=True)
    bg = g.collect()
    for x, y in zip(be[:6] + (e.b_obs_v,), bg[:6] + (g.b_obs_v,)):
        assert torch.equal(x, y)
    N, before = be[0].shape[0], e.policy.theta.clone()
    torch.manual_seed(77)
    torch.rand(N, device=DEV); torch.rand(N, device=DEV)
    ie = e.update(be)
    torch.manual_seed(77)
    ig = g.update(bg)
    assert torch.equal(e.policy.theta, g.policy.theta) and torch.equal(e.adam_m, g.adam_m)
    assert ie == ig and not torch.equal(e.policy.theta, before)
    # a second replayed rollout and update still run and agree on the rollout
    torch.manual_seed(78)
    be = e.collect()
    torch.manual_seed(78)
    bg = g.collect()
    assert all(torch.equal(x, y) for x, y in zip(be[:6], bg[:6])) and torch.equal(e.b_obs_v, g.b_obs_v)
    e.env.close(); g.env.close()


def test_autograd_path_trains_a_critic_wider_than_the_learner(tmp_path):
    """Dv = 100 > 96: the native learner is refused by name at construction, the autograd path trains - and its gradient of a
    minibatch is the reference's (the f32 witness of MlpPolicy with a layout of Dv rows)."""
    from trex_gym import critic as C
    from trex_gym.ppo import PPO
    env = make_vec(64, max_episode_steps=6)
    extra = torch.randn(64, 25, device=DEV)
    C.attach(env, [C.clean(), C.tensor(extra)])
    with pytest.raises(ValueError, match="native learner"):
        PPO(env, critic=True, **PPO_KW)
    a = PPO(env, critic=True, native_learner=False, **PPO_KW)
    assert a.critic_dim == 100 and a.policy.p("vf.W1").shape == (100, 64)
    th0 = a.policy.theta.clone()
    info = a.update(a.collect())
    assert all(np.isfinite(v) for v in info.values()) and not torch.equal(a.policy.theta, th0)
    assert torch.equal(a.env.critic_rows[:, 75:], extra)
    env.close()


def test_world_size_above_one_with_a_critic_is_refused_by_name():
    from trex_gym.ppo import PPO

    class Env:
        rank, world_size, process_group, device = 0, 2, None, torch.device(DEV)
    with pytest.raises(ValueError, match="critic moments"):
        e = Env()
        e.num_envs = 8
        import types
        e.observation_space = types.SimpleNamespace(shape=(75,))
        e.action_space = types.SimpleNamespace(shape=(25,))
        PPO(e, critic=True, **PPO_KW)


def test_checkpoint_round_trips_the_critic(tmp_path):
    """trex_train with critic="clean" and the sensor model: Dv, the spec and the moments go into the checkpoint and come back; the
    loaded agent plays policy-only (no critic row on its env)."""
    from trex_gym import trex_train
    args = trex_train.parse_args(["--critic", "clean", "--sensing", "typical"])
    env = trex_train.build_environment(64, device=DEV, max_episode_steps=6, sensing=trex_train.sensing_args(args), critic=args.critic)
    assert env.critic_rows.shape == (64, 75) and env.critic_config["preset"] == "clean"
    path = str(tmp_path / "policy.pt")
    agent, hist = trex_train.train(env, 2 * 64 * 4, 0, nsteps=4, noptepochs=1, save_path=path, log=lambda s: None)
    assert len(hist) == 2 and agent.crit is not None and all(np.isfinite(h["value_loss"]) for h in hist)
    ck = torch.load(path, map_location=DEV, weights_only=True)
    st = agent.crit.get_stats()
    assert ck["critic"]["dim"] == 75 and ck["critic"]["preset"] == "clean" and ck["critic"]["spec"] == env.critic_spec
    assert ck["critic"]["names"] == env.critic_names
    assert np.array_equal(ck["critic"]["mean"].cpu().numpy(), st["mean"]) and np.array_equal(ck["critic"]["var"].cpu().numpy(), st["var"])
    assert float(ck["critic"]["count"]) == st["count"] > 64
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    assert again.crit.dim == 75 and again.env.critic_rows is None and again.critic_config["spec"] == env.critic_spec
    st2 = again.crit.get_stats()
    assert np.array_equal(st2["mean"], st["mean"]) and np.array_equal(st2["var"], st["var"]) and st2["count"] == st["count"]
    assert torch.equal(again.policy.theta, agent.policy.theta)
    _, rewards = trex_train.play(again, 3, log=lambda *a: None)
    assert len(rewards) == 3 and np.isfinite(rewards).all()
    env.close(); again.env.close()
