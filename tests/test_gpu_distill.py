"""Policy distillation on the device (include/trex_policy_distill.h; the LOSS_DISTILL instantiation of learn_grad_kernel in
csrc/ppo_learner.hip; trex_gym.distill) on the cases of tests/distill_cases.py, against the f64 reference tests/distill_ref.py that
tests/test_distill_ref.py qualifies on the CPU - and, bit for bit, against the PPO learner where the two must agree.

Every output buffer is gpu_support.guarded: guard elements on either side, which must survive the call.

Tolerances are the project's own for the PPO learner's gradient (tests/test_gpu_policy.py): rtol 1e-4 + 1e-5 max|g| against the
reference; the loss sums rtol 1e-5. Everything else is bitwise."""
import numpy as np
import pytest
import torch

import distill_cases as dc
import distill_ref as DR
import trainer_cases as tc
from gpu_support import DEV, guarded, guards_intact, make_vec, replay_equals_eager

pytestmark = pytest.mark.gpu

LR, EPS, MAXN = tc.LR, tc.ADAM_EPS, tc.MAX_GRAD_NORM


def _api():
    from trex_gym import _capi, distill_capi
    return _capi, distill_capi


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


_DEVICE_CASES = {}


def inputs(name):
    """(case, device tensors of its buffers): uploaded once, shared, never written by a test"""
    if name not in _DEVICE_CASES:
        c = dc.case_by_name(name)
        t = {k: dev32(c[k]) for k in ("obs", "tmean", "tvalue", "tlogstd")}
        t["perm"] = torch.from_numpy(c["perm"]).to(DEV)
        _DEVICE_CASES[name] = (c, t)
    return _DEVICE_CASES[name]


def student(c, n=64):
    K, DC = _api()
    kern = K.Policy(n, c["D"], c["A"], 64, 0)
    assert dc.layout_rule(c["D"], c["A"]) == ({k: (o, tuple(s)) for k, (o, s) in kern.layout.items()}, kern.param_count)
    theta = torch.from_numpy(tc._params_to_theta(kern.layout, kern.param_count, c["params"])).to(DEV)
    return kern, DC.PolicyDistill(kern), theta


def block(layout, flat, name):
    off, shape = layout[name]
    return flat[off:off + int(np.prod(shape))]


class Run:
    """fresh theta / grad / m / v / loss sums, each guarded; one native call"""

    def __init__(self, count, theta, call):
        (self.W_t, self.theta), (self.W_g, self.grad), (self.W_m, self.m), (self.W_v, self.v) = (guarded((count,)) for _ in range(4))
        self.W_s, self.sums = guarded((2,))
        self.count = count
        self.theta.copy_(theta)
        self.grad.fill_(3.0)
        self.m.zero_(); self.v.zero_(); self.sums.zero_()
        call(self)
        torch.cuda.synchronize()
        self.check_guards()

    def check_guards(self):
        assert all(guards_intact(w, (self.count,)) for w in (self.W_t, self.W_g, self.W_m, self.W_v)) and guards_intact(self.W_s, (2,))


def grad_run(c, t, dist, theta, kind, vf_coef, grad_scale=1.0, tvalue="given", count=None):
    tv = t["tvalue"] if tvalue == "given" else tvalue
    return Run(count or theta.numel(), theta, lambda r: dist.minibatch_grad(
        r.theta, r.grad, t["obs"], t["tmean"], tv, t["tlogstd"] if kind == DR.KL else None, t["perm"], c["first"], c["mb"], kind, vf_coef,
        grad_scale, r.sums))


# ================================================================ 1. gradient and loss sums against the f64 reference
@pytest.mark.parametrize("kind_name,kind", dc.KINDS, ids=[k for k, _ in dc.KINDS])
@pytest.mark.parametrize("name", list(dc.shapes()))
def test_gradient_and_losses_are_the_reference_s(name, kind_name, kind):
    c, t = inputs(name)
    kern, dist, theta = student(c)
    worst, lrel = [], []
    for vf_coef in dc.VF_COEFS:
        out, grads = dc.reference(name, kind, vf_coef)
        want1 = tc._grads_to_flat(kern, grads)
        for gs in dc.GRAD_SCALES:
            r = grad_run(c, t, dist, theta, kind, vf_coef, gs)
            got, sums, want = r.grad.cpu().double().numpy(), r.sums.cpu().double().numpy(), want1 * gs
            scale = np.abs(want).max()
            worst.append(np.max(np.abs(got - want) / (1e-4 * np.abs(want) + 1e-5 * scale)))
            lrel.append(max(abs(sums[0] / (gs * out["pi_loss"]) - 1), abs(sums[1] / (gs * out["vf_loss"]) - 1)))
            assert np.isfinite(got).all() and scale > 0
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * scale)
            np.testing.assert_allclose(sums, [gs * out["pi_loss"], gs * out["vf_loss"]], rtol=1e-5)
            assert torch.equal(r.theta, theta)
    print("%s %s: worst gradient element at %.3f of the tolerance, worst loss sum off by %.1e (relative)" % (name, kind_name, max(worst), max(lrel)))
    kern.close()


# ================================================================ 2. exact zeros
@pytest.mark.parametrize("name", ["dims_D64_A25", "dims_D96_A32", "mb1_first0", "mb31_first5", "mb33_first5", "mb2049_first5"])
def test_exact_zeros(name):
    """MSE: the logstd gradient is zero; vf_coef = 0: the vf blocks are zero, with the teacher's values given or absent (the same
    bits, and L_vf reported as 0 without them); the pad elements between the blocks are zero; on ragged last tiles too."""
    c, t = inputs(name)
    kern, dist, theta = student(c)
    lay = kern.layout
    used = torch.zeros(kern.param_count, dtype=torch.bool, device=DEV)
    for k in lay:
        block(lay, used, k).fill_(True)
    for kind in (DR.MSE, DR.KL):
        a = grad_run(c, t, dist, theta, kind, 0.0)
        b = grad_run(c, t, dist, theta, kind, 0.0, tvalue=None)
        h = grad_run(c, t, dist, theta, kind, 0.5)
        for r in (a, b, h):
            assert bool((~used).any()) and float(r.grad[~used].abs().max()) == 0.0
            assert (float(block(lay, r.grad, "logstd").abs().max()) == 0.0) == (kind == DR.MSE)
            assert float(block(lay, r.grad, "pi.W1").abs().max()) > 0
        for k in lay:
            if k.startswith("vf."):
                assert float(block(lay, a.grad, k).abs().max()) == 0.0 and float(block(lay, b.grad, k).abs().max()) == 0.0, k
                assert float(block(lay, h.grad, k).abs().max()) > 0, k
            else:
                assert torch.equal(block(lay, a.grad, k), block(lay, h.grad, k)), k
        assert torch.equal(a.grad, b.grad) and a.sums[0] == b.sums[0] == h.sums[0]
        assert float(b.sums[1]) == 0.0 and a.sums[1] == h.sums[1] and float(a.sums[1]) > 0
    kern.close()


# ================================================================ 3. identity with the PPO kernel's value head
@pytest.mark.parametrize("name", ["dims_D33_A1", "dims_D75_A25", "mb33_first5", "mb2049_first5"])
def test_vf_blocks_are_the_ppo_kernel_s(name):
    """trex_policy_minibatch_grad with ret = teacher_value, val0 = 0 and cliprange = 1e30: vclip = 0 + (v - 0) is exactly v, both
    branches of the clipped value loss give v - R, and the vf blocks and the value loss sum are the distillation call's bits."""
    c, t = inputs(name)
    kern, dist, theta = student(c)
    N = c["N"]
    zero, one = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    act = torch.zeros(N, c["A"], device=DEV)
    stats = torch.tensor([0.0, 1.0], device=DEV)
    for vf_coef in (0.5, 1.0):
        d = grad_run(c, t, dist, theta, DR.KL, vf_coef)
        p = Run(kern.param_count, theta, lambda r: kern.minibatch_grad(
            r.theta, r.grad, t["obs"], act, zero, zero, one, t["tvalue"], t["perm"], c["first"], c["mb"], stats, cliprange=1e30, ent_coef=0.0,
            vf_coef=vf_coef, grad_scale=1.0, loss_sums=r.sums))
        for k in kern.layout:
            if k.startswith("vf."):
                assert torch.equal(block(kern.layout, d.grad, k), block(kern.layout, p.grad, k)), k
        assert d.sums[1] == p.sums[1] and float(d.sums[1]) > 0
    kern.close()


# ================================================================ 4. repeatability, isolation, step = grad + adam
def _ppo_call(kern):
    """a PPO minibatch_grad on the same object and shape (tests/trainer_cases.py's mb33_first5)"""
    lc = tc.learn_case_by_name("mb33_first5")
    lt = {k: dev32(lc[k]) for k in ("obs", "act", "logp_old", "value_old", "adv", "ret")}
    lperm, lstats = torch.from_numpy(lc["perm"]).to(DEV), torch.from_numpy(lc["adv_stats"]).to(DEV)

    def ppo(r):
        kern.minibatch_grad(r.theta, r.grad, lt["obs"], lt["act"], lt["logp_old"], lt["value_old"], lt["adv"], lt["ret"], lperm, lc["first"],
                            lc["mb"], lstats, cliprange=tc.CLIPRANGE, ent_coef=0.01, vf_coef=tc.VF_COEF, loss_sums=r.sums)
    return ppo


def test_repeatable_and_isolated():
    """two calls give the same bits; a PPO minibatch_grad on the same policy object before and after the distillation calls too"""
    c, t = inputs("mb33_first5")
    kern, dist, theta = student(c)
    ppo = _ppo_call(kern)
    before = Run(kern.param_count, theta, ppo)
    for kind in (DR.MSE, DR.KL):
        a, b = grad_run(c, t, dist, theta, kind, 0.5), grad_run(c, t, dist, theta, kind, 0.5)
        assert torch.equal(a.grad, b.grad) and torch.equal(a.sums, b.sums)
    after = Run(kern.param_count, theta, ppo)
    assert torch.equal(before.grad, after.grad) and torch.equal(before.sums, after.sums) and float(before.grad.abs().max()) > 0
    kern.close()


def _two_updates(kind):
    """(two _step calls, two (_grad, trex_policy_adam) pairs) from the same parameters, moments and Adam count; the second update
    agrees only if each step moved the count by exactly one (the step size depends on it)"""
    c, t = inputs("mb33_first5")
    kern, dist, theta = student(c)
    tl = t["tlogstd"] if kind == DR.KL else None

    def steps(r):
        for _ in range(2):
            dist.minibatch_step(r.theta, r.grad, r.m, r.v, t["obs"], t["tmean"], t["tvalue"], tl, t["perm"], c["first"], c["mb"], kind, 0.5, LR,
                                0.9, 0.999, EPS, MAXN, r.sums)

    def pairs(r):
        for i in range(2):
            dist.minibatch_grad(r.theta, r.grad, t["obs"], t["tmean"], t["tvalue"], tl, t["perm"], c["first"], c["mb"], kind, 0.5, 1.0, r.sums)
            r.last_grad = r.grad.clone()
            kern.adam(r.theta, r.grad, r.m, r.v, lr=LR, eps=EPS, max_grad_norm=MAXN)

    s = Run(kern.param_count, theta, steps)
    kern.adam_reset()
    g = Run(kern.param_count, theta, pairs)
    return kern, theta, s, g


@pytest.mark.parametrize("kind", [DR.MSE, DR.KL], ids=["mse", "kl"])
def test_step_has_the_gradient_of_grad_and_moves_the_adam_count_by_one(kind):
    """_step leaves in grad_dev and loss_sums the bits of _grad; its update is that of _grad + trex_policy_adam (at the tolerance
    tests/test_gpu_critic.py uses for the PPO step, 2 % of lr, here; bit for bit in the test below); and it advances the policy
    object's Adam count by exactly one:
    the same trex_policy_adam call behind two steps gives the bits it gives behind two trex_policy_adam calls."""
    kern, theta, s, g = _two_updates(kind)
    assert torch.equal(s.grad, g.last_grad) and torch.equal(s.sums, g.sums)
    np.testing.assert_allclose((s.theta - theta).cpu().numpy(), (g.theta - theta).cpu().numpy(), rtol=0, atol=0.02 * LR)
    assert float((s.theta - theta).abs().max()) > 0.1 * LR
    # ---- the count: a probe update by trex_policy_adam (fixed inputs) behind two steps, behind two adam calls, behind one
    c, t = inputs("mb33_first5")
    dist, P = _api()[1].PolicyDistill(kern), kern.param_count
    tl = t["tlogstd"] if kind == DR.KL else None

    def probe():
        th = theta.clone()
        kern.adam(th, torch.full((P,), 0.01, device=DEV), torch.zeros(P, device=DEV), torch.zeros(P, device=DEV), lr=LR, eps=EPS, max_grad_norm=MAXN)
        return th

    def scratch():
        return [theta.clone()] + [torch.zeros(P, device=DEV) for _ in range(3)]

    kern.adam_reset()
    for _ in range(2):
        dist.minibatch_step(*scratch(), t["obs"], t["tmean"], t["tvalue"], tl, t["perm"], c["first"], c["mb"], kind, 0.5, LR, 0.9, 0.999, EPS, MAXN)
    behind_steps = probe()
    kern.adam_reset()
    for _ in range(2):
        kern.adam(*scratch(), lr=LR, eps=EPS, max_grad_norm=MAXN)
    behind_adams = probe()
    kern.adam_reset()
    kern.adam(*scratch(), lr=LR, eps=EPS, max_grad_norm=MAXN)
    behind_one = probe()
    assert torch.equal(behind_steps, behind_adams) and not torch.equal(behind_steps, behind_one)
    kern.close()


@pytest.mark.parametrize("kind", [DR.MSE, DR.KL], ids=["mse", "kl"])
def test_step_is_grad_plus_adam_bit_for_bit(kind):
    """_step == _grad + trex_policy_adam, bit for bit, after two updates: theta, both Adam moments, the gradient and the loss sums.
    The step runs learn_adam_kernel, trex_policy_adam the single-workgroup adam_kernel; both take Adam's moments from
    policy_common.h's adam_moments, which states the rounding (left to the compiler, the two kernels contracted the second moment
    differently: v was off by one unit in the last place, 9.1e-13 with the squared error and 1.8e-12 with the KL, theta by 3.7e-9)."""
    kern, theta, s, g = _two_updates(kind)
    print("kind %d: step vs grad + adam after two updates: max |d theta| %.3e, |d m| %.3e, |d v| %.3e; theta moved %.3e" % (
        kind, float((s.theta - g.theta).abs().max()), float((s.m - g.m).abs().max()), float((s.v - g.v).abs().max()),
        float((s.theta - theta).abs().max())))
    assert torch.equal(s.grad, g.last_grad) and torch.equal(s.sums, g.sums) and torch.equal(s.m, g.m)
    assert torch.equal(s.v, g.v) and torch.equal(s.theta, g.theta)
    kern.close()


# ================================================================ 5. refusals
def test_refusals_with_nothing_launched():
    K, DC = _api()
    from trex_gym import critic_capi
    c, t = inputs("dims_D75_A25")
    kern, dist, theta0 = student(c)
    W_t, theta = guarded((kern.param_count + 4096,))
    theta[:kern.param_count].copy_(theta0)
    W_g, grad = guarded((kern.param_count + 4096,))
    m, v = torch.zeros_like(grad), torch.zeros_like(grad)
    keep_theta = theta.clone()

    def call(d, step, kind=DR.KL, vf_coef=0.5, tvalue=t["tvalue"], tlogstd=t["tlogstd"], obs=t["obs"], tmean=t["tmean"], first=c["first"], mb=c["mb"]):
        if step:
            d.minibatch_step(theta, grad, m, v, obs, tmean, tvalue, tlogstd, t["perm"], first, mb, kind, vf_coef)
        else:
            d.minibatch_grad(theta, grad, obs, tmean, tvalue, tlogstd, t["perm"], first, mb, kind, vf_coef)

    crit = critic_capi.PolicyCritic(kern)
    crit.set(40)
    wide = K.Policy(64, 97, c["A"], 64, 0)
    wide_d = DC.PolicyDistill(wide)
    for step in (True, False):
        with pytest.raises(K.TrexError, match="critic width set") as e:
            call(dist, step)
        assert e.value.code == K.E_INVALID
    crit.set(0)
    for step in (True, False):
        for match, kw in (("unknown loss kind", dict(kind=2)), ("unknown loss kind", dict(kind=-1)), ("needs teacher_logstd", dict(tlogstd=None)),
                          ("teacher_value may be null only", dict(tvalue=None)), ("bad sizes", dict(mb=0)), ("bad sizes", dict(first=-1))):
            with pytest.raises(K.TrexError, match=match) as e:
                call(dist, step, **kw)
            assert e.value.code == K.E_INVALID
        with pytest.raises(K.TrexError, match="obs_dim <= 96") as e:
            call(wide_d, step, obs=torch.zeros(c["N"], 97, device=DEV))
        assert e.value.code == K.E_INVALID
        with pytest.raises(K.TrexError, match="at least"):
            call(dist, step, tmean=t["tmean"][:-1])
        with pytest.raises(K.TrexError, match="device memory"):
            call(dist, step, obs=t["obs"].cpu())
    with pytest.raises(ValueError):
        DC.kind_of("huber")
    torch.cuda.synchronize()
    assert torch.equal(theta, keep_theta) and bool((grad == 7.0).all()) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
    assert guards_intact(W_t, theta.shape) and guards_intact(W_g, grad.shape)
    # ... and the object still works: the KL step without a teacher value at vf_coef 0, the MSE step without a teacher logstd
    call(dist, True, vf_coef=0.0, tvalue=None)
    call(dist, True, kind=DR.MSE, tlogstd=None)
    torch.cuda.synchronize()
    assert not torch.equal(theta, keep_theta) and bool(torch.isfinite(theta).all())
    kern.close(); wide.close()


# ================================================================ 6. capture
def test_step_replays_from_a_graph():
    """_step captured (after a warm-up call that sizes the workspace) and replayed twice from given theta / m / v and Adam count
    equals two eager calls from the same state, bit for bit; gpu_support.replay_equals_eager on the gradient call (the teacher's
    means change between capture and replay)."""
    c, t = inputs("mb2049_first5")
    kern, dist, theta0 = student(c)
    P = kern.param_count
    tmean = t["tmean"].clone()

    def grad_call(outs):
        dist.minibatch_grad(theta0, outs[0], t["obs"], tmean, t["tvalue"], t["tlogstd"], t["perm"], c["first"], c["mb"], DR.KL, 0.5, 1.0, None)

    replay_equals_eager(grad_call, [torch.zeros(P, device=DEV)], lambda: tmean.mul_(0.5), replays=2)
    bufs = [torch.zeros(P, device=DEV) for _ in range(4)] + [torch.zeros(2, device=DEV)]

    def step(b):
        dist.minibatch_step(b[0], b[1], b[2], b[3], t["obs"], t["tmean"], t["tvalue"], t["tlogstd"], t["perm"], c["first"], c["mb"], DR.KL, 0.5,
                            LR, 0.9, 0.999, EPS, MAXN, b[4])

    def fresh(b):
        b[0].copy_(theta0)
        for x in b[1:]:
            x.zero_()
        kern.adam_reset()

    eager = [torch.zeros_like(x) for x in bufs]
    fresh(eager)
    step(eager); step(eager)
    fresh(bufs)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(bufs)
    fresh(bufs)
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, eager)) and not torch.equal(bufs[0], theta0)
    del graph
    kern.close()


# ================================================================ 7. the driver
N_ENVS, T = 64, 4
KW = dict(nsteps=T, nminibatches=2, noptepochs=2)


def _teacher_source(D, A, seed=5):
    lay, count = dc.layout_rule(D, A)
    params = tc.make_params(D, A, np.random.default_rng(seed))
    theta = torch.from_numpy(tc._params_to_theta(lay, count, params)).to(DEV)
    stats = dict(obs_mean=np.zeros(D), obs_var=np.ones(D), obs_count=100.0, ret_mean=0.0, ret_var=1.0, ret_count=100.0)
    return theta, stats


def _agent(loss="kl", beta=1.0, sensing=True, **kw):
    from trex_gym import distill as D, sensing as S
    env = make_vec(N_ENVS, max_episode_steps=6)
    if sensing:
        S.attach(env, S.typical(env), seed=5)
    teacher = D.Teacher(env, _teacher_source(75, 25), rows="clean")
    return D.Distill(env, teacher, loss=loss, beta=beta, beta_decay=0.5, seed=3, **dict(KW, **kw))


def test_rollout_follows_the_mask_and_leaves_the_teacher_alone():
    a = _agent(beta=1.0)
    st0 = a.teacher.kern.get_stats()
    so0 = a.kern.get_stats()
    a.collect()
    assert bool(a.mask.all()) and torch.equal(a.actions, a.b_tmean[-1]) and not torch.equal(a.actions, a.student_actions)
    assert a.last_beta == 1.0 and a.beta == 0.5
    a.beta = 0.0
    a.collect()
    assert not bool(a.mask.any()) and torch.equal(a.actions, a.student_actions) and not torch.equal(a.actions, a.b_tmean[-1])
    mask = torch.arange(N_ENVS, device=DEV) % 3 == 0
    a.collect(mask=mask)
    assert torch.equal(a.actions, torch.where(mask[:, None], a.b_tmean[-1], a.student_actions))
    assert torch.equal(a.actions[0], a.b_tmean[-1][0]) and torch.equal(a.actions[1], a.student_actions[1])
    # the teacher read the clean row, the student the sensors' row; the teacher's moments never moved, the student's did
    assert not torch.equal(a.env.clean_rows, a.env.rows)
    st1, so1 = a.teacher.kern.get_stats(), a.kern.get_stats()
    assert all(np.array_equal(np.asarray(st0[k]), np.asarray(st1[k])) for k in st0)
    assert so1["obs_count"] > so0["obs_count"] and bool(torch.isfinite(a.b_tval).all())
    # the teacher's value and mean of the last step are what its act call gives on the row of that moment: finite, and not the student's
    assert float((a.b_tmean[-1] - a.student_actions).abs().max()) > 1e-3
    a.env.close()


def test_teacher_refusals():
    from trex_gym import distill as D
    env = make_vec(8)
    theta, stats = _teacher_source(75, 25)
    with pytest.raises(ValueError, match="actions"):
        D.Teacher(env, _teacher_source(75, 24))
    with pytest.raises(ValueError, match="reads 80 columns"):
        D.Teacher(env, _teacher_source(80, 25), rows="rows")
    with pytest.raises(ValueError, match="no critic row"):
        D.Teacher(env, (theta, stats), rows="critic")
    with pytest.raises(ValueError, match="at most 126"):
        D.Teacher(env, _teacher_source(127, 25), rows=torch.zeros(8, 127, device=DEV))
    with pytest.raises(ValueError, match="expected a"):
        D.Teacher(env, (theta, stats), rows=torch.zeros(8, 74, device=DEV))
    with pytest.raises(ValueError, match="expected one of"):
        D.Teacher(env, (theta, stats), rows="noisy")
    t = D.Teacher(env, (theta, stats), rows=torch.zeros(8, 80, device=DEV))
    assert t.obs_dim == 75 and t.rows_choice == "tensor"

    class Two:
        world_size = 2
    with pytest.raises(ValueError, match="single process"):
        D.Distill(Two(), t)
    env.close()


@pytest.mark.parametrize("loss", ["kl", "mse"])
def test_update_is_the_sequence_of_c_abi_calls(loss):
    K, DC = _api()
    a = _agent(loss=loss)
    batch = a.collect()
    N, mb = N_ENVS * T, N_ENVS * T // KW["nminibatches"]
    theta = a.policy.theta.clone()
    state = torch.cuda.get_rng_state()
    info = a.update(batch)
    # ---- the same calls on a second student object (Adam count 0, as the agent's was)
    torch.cuda.set_rng_state(state)
    kern = K.Policy(N_ENVS, 75, 25, 64, 0)
    dist = DC.PolicyDistill(kern)
    grad, m, v, sums = torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros(2, device=DEV)
    total = torch.zeros(2, device=DEV)
    for _ in range(KW["noptepochs"]):
        perm = torch.rand(N, device=DEV).argsort()
        sums.zero_()
        for i in range(KW["nminibatches"]):
            dist.minibatch_step(theta, grad, m, v, a.b_obs.view(N, 75), a.b_tmean.view(N, 25), a.b_tval.view(N),
                                a.teacher.logstd if loss == "kl" else None, perm, i * mb, mb, loss, 0.5, 3e-4, 0.9, 0.999, 1e-5, 0.5, sums)
        total += sums
    assert torch.equal(theta, a.policy.theta) and torch.equal(m, a.adam_m) and torch.equal(v, a.adam_v)
    pi, vf = (total / (KW["noptepochs"] * KW["nminibatches"])).tolist()
    assert info == dict(policy_loss=pi, value_loss=vf, beta=1.0) and pi > 0 and vf > 0
    kern.close(); a.env.close()


def test_graph_update_is_the_eager_update():
    """use_graphs=True - the rollout with both act calls and the where captured, the epoch captured - against the eager driver: the
    rollout buffers and theta after the update bit for bit (the generator is put at the same state on both sides, as
    tests/test_gpu_critic.py does for PPO)."""
    e = _agent(noptepochs=1)
    be = e.collect()
    g = _agent(noptepochs=1, use_graphs=True)
    bg = g.collect()
    assert torch.equal(e.b_obs, g.b_obs) and torch.equal(e.b_tmean, g.b_tmean) and torch.equal(e.b_tval, g.b_tval)
    N, before = N_ENVS * T, e.policy.theta.clone()
    torch.manual_seed(77)
    torch.rand(N, device=DEV); torch.rand(N, device=DEV)
    ie = e.update(be)
    torch.manual_seed(77)
    ig = g.update(bg)
    assert torch.equal(e.policy.theta, g.policy.theta) and torch.equal(e.adam_m, g.adam_m)
    assert ie == ig and not torch.equal(e.policy.theta, before)
    # a second replayed rollout with another mask (refilled outside the capture) agrees too
    mask = torch.arange(N_ENVS, device=DEV) % 2 == 0
    torch.manual_seed(78)
    e.collect(mask=mask)
    torch.manual_seed(78)
    g.collect(mask=mask)
    assert torch.equal(e.b_obs, g.b_obs) and torch.equal(e.b_tmean, g.b_tmean) and torch.equal(e.actions, g.actions)
    assert torch.equal(g.actions, torch.where(mask[:, None], g.b_tmean[-1], g.student_actions))
    e.env.close(); g.env.close()


def test_ten_mse_updates_lower_the_loss_on_a_held_out_batch():
    """64 envs, ten updates with the squared-error loss, the teacher driving (beta 1, no decay: every rollout visits the states the
    held-out batch comes from). The held-out batch is fixed and of the run's own first rollout, which no update sees: the raw
    rows the envs stand on when it ends and the teacher's means there. L_pi on it is computed by the f64 reference from the
    student's means alone - the student as it is after the update, its running moments (which move from rollout to rollout) and
    theta, both in f64 - and is lower after the last update than after the first."""
    a = _agent(loss="mse", beta=1.0, lr=1e-3)
    a.beta_decay = 1.0
    a.collect()                                            # held out: never passed to update
    raw = a.env.rows[:, :75].cpu().double().numpy()
    tmean_dev = torch.zeros(N_ENVS, 25, device=DEV)
    a.teacher.act(tmean_dev)
    tmean = tmean_dev.cpu().double().numpy()

    def held_out():
        st = a.kern.get_stats()
        obs = np.clip((raw - st["obs_mean"]) / np.sqrt(st["obs_var"] + 1e-8), -10.0, 10.0)
        mean, logstd, _ = DR.forward(tc._theta_to_params(a.kern, a.policy.theta), obs)
        return float(np.mean(DR.policy_terms(DR.MSE, mean, logstd, tmean, None)))

    seen = []
    for _ in range(10):
        info = a.update(a.collect())
        seen.append((held_out(), info["policy_loss"]))
    print("held-out L_pi after each update: " + " ".join("%.5f" % h for h, _ in seen))
    print("training L_pi of each update:    " + " ".join("%.5f" % p for _, p in seen))
    assert all(np.isfinite(h) and np.isfinite(p) for h, p in seen) and seen[-1][0] < seen[0][0]
    # the student is an ordinary policy: PPO takes its parameters and moments over and updates
    from trex_gym.ppo import PPO
    st = a.kern.get_stats()
    ppo = PPO(a.env, **KW)
    with torch.no_grad():
        ppo.policy.theta.copy_(a.policy.theta)
    ppo.kern.set_stats(st)
    out = ppo.update(ppo.collect())
    assert all(np.isfinite(x) for x in out.values())
    a.env.close()


def test_checkpoint_records_the_teacher_and_plays(tmp_path):
    """trex_train: a teacher trained by PPO on the clean env and saved; --distill with --sensing trains a student onto it; the
    checkpoint stores the teacher's path and row choice and loads and plays as any other."""
    from trex_gym import trex_train
    tpath, spath = str(tmp_path / "teacher.pt"), str(tmp_path / "student.pt")
    env = trex_train.build_environment(N_ENVS, device=DEV, max_episode_steps=6)
    trex_train.train(env, N_ENVS * T, 0, nsteps=T, noptepochs=1, save_path=tpath, log=lambda s: None)
    env.close()
    args = trex_train.parse_args(["--distill", tpath, "--sensing", "typical", "--distill_loss", "mse", "--dagger_beta", "0.8", "0.5"])
    assert trex_train.distill_args(args) == dict(teacher=tpath, rows="clean", loss="mse", beta=0.8, decay=0.5)
    env = trex_train.build_environment(N_ENVS, device=DEV, max_episode_steps=6, sensing=trex_train.sensing_args(args))
    lines = []
    agent, hist = trex_train.train(env, 2 * N_ENVS * T, 0, nsteps=T, noptepochs=1, save_path=spath, log=lines.append,
                                   distill=trex_train.distill_args(args))
    assert len(hist) == 2 and [h["beta"] for h in hist] == [0.8, 0.4] and all(np.isfinite(h["policy_loss"]) for h in hist)
    assert any("L_pi" in l and "L_vf" in l and "beta" in l for l in lines)
    ck = torch.load(spath, map_location=DEV, weights_only=True)
    assert ck["distill"] == dict(teacher=tpath, rows="clean", loss="mse") and ck["critic"] is None
    again = trex_train.load_agent(spath, num_envs=4, device=DEV)
    assert torch.equal(again.policy.theta, agent.policy.theta)
    _, rewards = trex_train.play(again, 3, log=lambda *a: None)
    assert len(rewards) == 3 and np.isfinite(rewards).all()
    env.close(); again.env.close()
