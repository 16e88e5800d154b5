"""The mirror maps on the device (include/trex_symmetry.h, csrc/symmetry.hip) through the C-ABI, against tests/symmetry_ref.py: the
two row launches bit for bit - they move words and flip sign bits, nothing is rounded -, the moments bit for bit in the header's
order of f64 operations, guards and every column the header does not name untouched, the refusals, stream capture, the channels of
a generated exactly symmetric biped, and the trainer with symmetry="augment", "loss" and "both" (trex_gym.symmetry.MirrorPPO)."""
import numpy as np
import pytest
import torch

import symmetry_models as SM
import symmetry_ref as R
from gpu_support import DEV, guarded, guards_intact, refused, replay_equals_eager, same_bits

pytestmark = pytest.mark.gpu

INVALID = -1
SPECIAL = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7f800001, 0x00000001], np.uint32)


def random_table(rng, W, involution):
    """a signed permutation of W columns; involution: made of fixed points and swapped pairs whose two signs agree"""
    if not involution:
        return rng.permutation(W).astype(np.int32), rng.choice([-1, 1], W).astype(np.int8)
    src, sign = np.arange(W, dtype=np.int32), rng.choice([-1, 1], W).astype(np.int8)
    order = rng.permutation(W)
    for a, b in zip(order[0:2 * (W // 3):2], order[1:2 * (W // 3):2]):
        src[a], src[b] = b, a
        sign[b] = sign[a]
    return src, sign


def random_words(rng, shape):
    """f32 with every exponent, and NaNs with payloads, infinities and zeros of both signs sprinkled in"""
    w = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    at = rng.integers(0, flat.size, size=max(1, flat.size // 7))
    flat[at] = SPECIAL[rng.integers(0, len(SPECIAL), size=at.size)]
    return w.view(np.float32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("width", [1, 2, 75, 93, 126, 517])
def test_mirror_rows_bitwise(width):
    """n below, at and above a wave and a tile; packed and padded rows; in place and out of place; the columns beyond the width and
    the guards keep their fill; an involution applied twice reproduces the input"""
    from trex_gym.symmetry_capi import MirrorTable
    rng = np.random.default_rng(width)
    src, sign = random_table(rng, width, False)
    table = MirrorTable(src, sign)
    isrc, isign = random_table(rng, width, True)
    itable = MirrorTable(isrc, isign)
    assert not table.involution or width <= 2
    assert itable.involution
    for n in (1, 63, 64, 65, 257):
        for stride in (width, width + 3):
            x = random_words(rng, (n, stride))
            want = R.mirror_rows(src, sign, x[:, :width])
            xin = dev(x)
            whole, out = guarded((n, stride))
            table.rows(xin.reshape(-1), out.reshape(-1), n=n, in_stride=stride, out_stride=stride)
            got = bits(out)
            assert (got[:, :width] == want.view(np.uint32)).all(), (n, stride)
            assert (out[:, width:] == 7.0).all() and guards_intact(whole, (n, stride))
            assert (bits(xin) == x.view(np.uint32)).all()                # the input is read only
            # out of place into rows of another stride
            whole2, out2 = guarded((n, width + 1))
            table.rows(xin.reshape(-1), out2.reshape(-1), n=n, in_stride=stride, out_stride=width + 1)
            assert (bits(out2)[:, :width] == want.view(np.uint32)).all() and (out2[:, width:] == 7.0).all() and guards_intact(whole2, (n, width + 1))
            # in place
            whole3, buf = guarded((n, stride))
            buf.copy_(xin)
            table.rows(buf.reshape(-1), buf.reshape(-1), n=n, in_stride=stride, out_stride=stride)
            got = bits(buf)
            assert (got[:, :width] == want.view(np.uint32)).all(), (n, stride, "in place")
            assert (got[:, width:] == x.view(np.uint32)[:, width:]).all() and guards_intact(whole3, (n, stride))
            # the involution, twice, in place
            buf.copy_(xin)
            itable.rows(buf.reshape(-1), buf.reshape(-1), n=n, in_stride=stride, out_stride=stride)
            assert (bits(buf)[:, :width] == R.mirror_rows(isrc, isign, x[:, :width]).view(np.uint32)).all()
            itable.rows(buf.reshape(-1), buf.reshape(-1), n=n, in_stride=stride, out_stride=stride)
            assert (bits(buf) == x.view(np.uint32)).all(), (n, stride, "twice")


@pytest.mark.parametrize("N,D,A,Dv", [(1, 1, 1, 0), (15, 75, 25, 0), (160, 93, 25, 96), (5000, 93, 25, 0)])
def test_mirror_augment_bitwise(N, D, A, Dv):
    """the second halves are the reference's bit for bit, the first halves and the guards untouched; (5000, ..): more copy
    workgroups than one and a last tile that is not full"""
    from trex_gym import symmetry_capi as S
    rng = np.random.default_rng(N + D)
    tabs = [random_table(rng, w, True) for w in (D, A)] + ([random_table(rng, Dv, True)] if Dv else [])
    handles = [S.MirrorTable(*t) for t in tabs]
    shapes = [(2 * N, D), (2 * N, A), (2 * N,), (2 * N,), (2 * N,), (2 * N,)] + ([(2 * N, Dv)] if Dv else [])
    host = [random_words(rng, s) for s in shapes]
    bufs = [guarded(s) for s in shapes]
    for (whole, view), h in zip(bufs, host):
        view.copy_(dev(h))
    views = [v for _, v in bufs]
    S.augment(handles[0], handles[1], *views[:6], N, critic_table=handles[2] if Dv else None, obs_v=views[6] if Dv else None)
    want = R.augment(tabs[0], tabs[1], *host[:6], N, critic_t=tabs[2] if Dv else None, obs_v=host[6] if Dv else None)
    for k, ((whole, view), h, w) in enumerate(zip(bufs, host, want)):
        got = bits(view)
        assert (got[:N] == h.view(np.uint32)[:N]).all(), k
        assert (got[N:] == w.view(np.uint32)[N:]).all(), k
        assert guards_intact(whole, shapes[k]), k


@pytest.mark.parametrize("D", [1, 75, 126])
def test_symmetrize_stats_bitwise(D):
    """the moments against the reference in the header's order, the count and the return moments untouched, a second application
    changes nothing; after it `act` normalises the mirrored rows to the mirror image of the normalised rows, bit for bit"""
    from trex_gym import _capi, symmetry_capi as S
    rng = np.random.default_rng(D)
    n, A = 67, min(D, 25)
    src, sign = random_table(rng, D, True)
    table = S.MirrorTable(src, sign)
    k = _capi.Policy(n, D, A, 64, 0)
    st = dict(obs_mean=rng.normal(size=D) * 3, obs_var=rng.uniform(0.01, 9.0, D), obs_count=12345.0, ret_mean=0.7, ret_var=2.5, ret_count=99.0,
              raw_reward_sum=-3.25)
    k.set_stats(st)
    S.symmetrize_stats(k, table)
    got = k.get_stats()
    mean, var = R.symmetrize_stats(src, sign, st["obs_mean"], st["obs_var"])
    assert got["obs_mean"].tobytes() == mean.tobytes() and got["obs_var"].tobytes() == var.tobytes()
    for name in ("obs_count", "ret_mean", "ret_var", "ret_count", "raw_reward_sum"):
        assert got[name] == st[name], name
    S.symmetrize_stats(k, table)
    again = k.get_stats()
    assert again["obs_mean"].tobytes() == mean.tobytes() and again["obs_var"].tobytes() == var.tobytes()
    # normalising commutes with mirroring
    theta = torch.zeros(k.param_count, device=DEV)
    rows = dev((rng.normal(size=(n, D)) * 4).astype(np.float32))
    noise = torch.zeros(n, A, device=DEV)
    outs = []
    for r in (rows, table.rows(rows)):
        actions, obs_out = torch.empty(n, A, device=DEV), torch.empty(n, D, device=DEV)
        k.act(theta, r, noise, actions, obs_out, torch.empty(n, A, device=DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV))
        outs.append(obs_out)
    assert same_bits(outs[1], table.rows(outs[0]))
    assert not same_bits(outs[1], outs[0]) or D == 1
    other = S.MirrorTable(*random_table(rng, D + 1, True))
    refused(INVALID, S.symmetrize_stats, k, other)
    refused(INVALID, S.symmetrize_stats, k, table, table)          # no critic is set


def test_refusals_on_the_device():
    from trex_gym import symmetry_capi as S
    from trex_gym.symmetry_capi import MirrorTable, lib
    import ctypes as C
    rng = np.random.default_rng(0)
    W, n = 75, 16
    table = MirrorTable(*random_table(rng, W, True))
    x, out = torch.zeros(n, W, device=DEV), torch.zeros(n, W, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw = lambda a, sa, b, sb, rows, width: lib.trex_mirror_rows(table.h, a, sa, b, sb, rows, width, stream)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)
    assert raw(p(x), W, p(out), W, n, W) == 0
    assert raw(p(x), W, p(x), W, n, W) == 0                               # in place
    assert raw(p(x), W, p(x, 1), W, n - 1, W) == INVALID                  # shifted by one float: overlap
    assert raw(p(x), W, p(x), W + 1, n - 1, W) == INVALID                 # the same base, another stride
    # (a short buffer: refused by the tensor's length - the raw pointer lies in a larger block of torch's allocator)
    refused(INVALID, table.rows, x.reshape(-1), out.reshape(-1), n=n + 1, in_stride=W, out_stride=W)
    assert raw(p(x), W, p(out), W, n, W - 1) == INVALID
    assert raw(p(x), W - 1, p(out), W, n, W) == INVALID
    assert raw(None, W, p(out), W, n, W) == INVALID
    host = np.zeros((n, W), np.float32)
    assert raw(C.c_void_p(host.ctypes.data), W, p(out), W, n, W) == INVALID
    assert (out == 0).all()
    with pytest.raises(Exception):
        MirrorTable([0, 0, 1], [1, 1, 1])
    with pytest.raises(Exception):
        MirrorTable([0, 1], [1, 2])
    act = MirrorTable(*random_table(rng, 25, True))
    N = 8
    bufs = [torch.zeros(2 * N, W, device=DEV), torch.zeros(2 * N, 25, device=DEV)] + [torch.zeros(2 * N, device=DEV) for _ in range(4)]
    S.augment(table, act, *bufs, N)
    refused(INVALID, S.augment, act, table, *bufs, N)                     # the tables swapped: the widths do not fit
    for k in range(6):
        short = list(bufs)
        short[k] = bufs[k][:2 * N - 1].clone()
        refused(INVALID, S.augment, table, act, *short, N)
    h = [C.c_void_p(b.data_ptr()) for b in bufs]
    assert lib.trex_mirror_augment(table.h, act.h, None, *h, None, N, W, 25, 0, stream) == 0
    assert lib.trex_mirror_augment(table.h, act.h, None, *h[:5], None, None, N, W, 25, 0, stream) == INVALID       # ret is null
    assert lib.trex_mirror_augment(table.h, act.h, None, *h, None, 0, W, 25, 0, stream) == INVALID
    assert lib.trex_mirror_augment(table.h, act.h, act.h, *h, None, N, W, 25, 25, stream) == INVALID               # a critic table without obs_v
    assert lib.trex_mirror_augment(table.h, None, None, *h, None, N, W, 25, 0, stream) == INVALID


def test_stream_capture():
    """rows, rows in place and augment, captured on a side stream and replayed on new data, are bitwise the eager calls"""
    from trex_gym import symmetry_capi as S
    rng = np.random.default_rng(2)
    D, A, N = 93, 25, 300
    obs_t, act_t = S.MirrorTable(*random_table(rng, D, True)), S.MirrorTable(*random_table(rng, A, True))
    src = torch.randn(N, D + 2, device=DEV)
    seeds = [torch.randn(2 * N, D, device=DEV), torch.randn(2 * N, A, device=DEV)] + [torch.randn(2 * N, device=DEV) for _ in range(4)]

    def call(outs):
        obs_t.rows(src.reshape(-1), outs[0].reshape(-1), n=N, in_stride=D + 2, out_stride=D)
        for o, s in zip(outs[1:], seeds):
            o.copy_(s)
        S.augment(obs_t, act_t, *outs[1:], N)
        obs_t.rows(outs[1], outs[1])

    outs = [torch.zeros(N, D, device=DEV)] + [torch.zeros_like(s) for s in seeds]

    def change():
        src.normal_()
        for s in seeds:
            s.normal_()

    replay_equals_eager(call, outs, change)


@pytest.mark.parametrize("lateral", [0, 1])
def test_channels_on_the_device(lateral, tmp_path):
    """On the exactly symmetric biped: a state and its mirror image set with set_state, the locomotion-style rows composed on the
    device; mirror.rows(rows(s)) against rows(mirror s) within the tolerances of tests/test_gpu_observations.py (TOL over
    max(1, |value|), times the channel's |scale|), the PREV_ACTION and EXTERNAL columns bit for
    bit; the tables are the reference's; mirror.state is the reference's"""
    from tolerances import LINK_TOL as TOL
    from trex_gym import observations as O
    from trex_gym.symmetry import Mirror
    from trex_gym.vec_env import TrexVecEnv
    path, props, model = SM.compile_biped(tmp_path, lateral)
    chans = SM.locomotion_channels(model, lateral) + [(R.PREV_ACTION, 0, (0, 0, 0), 1.0), (R.EXTERNAL, 3, (0, 0, 0), 1.0)]
    es, eg = [1, 0, 2], [1, 1, -1]
    n = 12
    states = SM.random_states(model, n, seed=11, lateral=lateral)
    ext = torch.randn(2 * n, 3, device=DEV)
    ext[n:] = ext[:n][:, es] * torch.tensor(eg, dtype=torch.float32, device=DEV)
    spec = [O.Channel(k, l, tuple(x), s) for k, l, x, s in chans]
    env = TrexVecEnv(2 * n, urdf_path=path, device=DEV, params=props["params"], observations=spec, external=ext)
    env.reset_tensor()
    mirror = Mirror(env, external=(es, eg), log=None)
    mm = R.model_table(model)
    want_src, want_sign = R.row_table(model, mm, chans, SM.NJ, 2, extern_src=es, extern_sign=eg)
    assert mirror.lateral == lateral and mirror.row_table.src.tolist() == want_src.tolist() and mirror.row_table.sign.tolist() == want_sign.tolist()
    assert all(v == 0.0 for v in mirror.residual.values())
    st = torch.tensor(states, dtype=torch.float64, device=DEV)
    image = mirror.state(st)
    ref_image = np.array([R.mirror_state(model, mm, s) for s in states])
    flip = np.sign((ref_image[:, 3:7] * image.cpu().numpy()[:, 3:7]).sum(1))[:, None]
    ref_image[:, 3:7] *= flip
    assert np.abs(image.cpu().numpy() - ref_image).max() < 1e-12
    env.set_state(torch.cat([st, image]).float())
    act = torch.randn(2 * n, SM.NJ, device=DEV)
    act[n:] = mirror.actions(act[:n].contiguous())
    assert same_bits(mirror.actions(act[n:].contiguous()), act[:n])
    rows = torch.zeros(2 * n, mirror.width, device=DEV)
    base = torch.zeros(2 * n, 3 * SM.NJ + 2, device=DEV)
    base[:, :2 * SM.NJ] = env.get_state()[:, 13:]
    env.batch.compose_rows(base, rows, act, ext)
    got = mirror.rows(rows[:n].contiguous()).cpu().numpy().astype(np.float64)
    want = rows[n:].cpu().numpy().astype(np.float64)
    col, worst = 3 * SM.NJ, 0.0
    assert (got[:, :col] == want[:, :col]).all() and (got[:, -2:] == want[:, -2:]).all()
    for kind, link, xyz, scale in chans:
        w = R.channel_width(kind, link, SM.NJ)
        g, r = got[:, col:col + w], want[:, col:col + w]
        if kind in (R.PREV_ACTION, R.EXTERNAL, R.CONTACT_FORCE):
            assert g.tobytes() == r.tobytes(), kind
        else:
            tol = TOL["velocity"] if kind in (R.BASE_LINEAR_VELOCITY, R.BASE_ANGULAR_VELOCITY, R.POINT_VELOCITY) else TOL["pose"]
            dev_ = (np.abs(g - r) / np.maximum(1.0, np.abs(r).max(1, keepdims=True))).max() / abs(scale)
            worst = max(worst, dev_ / tol)
            assert dev_ <= tol, (kind, dev_, tol)
        col += w
    print("lateral %d: the largest channel deviation is %.3g of its tolerance" % (lateral, worst))
    assert col == mirror.obs_dim


def _tiny_trainer(symmetry=None, use_graphs=False, with_arg=True, seed=3, **more):
    from trex_gym.ppo import PPO
    from trex_gym.symmetry import Mirror, MirrorPPO
    from trex_gym.vec_env import TrexVecEnv
    env = TrexVecEnv(16, device=DEV)
    kw = dict(nsteps=4, nminibatches=2, noptepochs=2, seed=seed, use_graphs=use_graphs)
    if not with_arg:
        return env, PPO(env, **kw)
    return env, MirrorPPO(env, Mirror(env, log=None) if symmetry else None, symmetry=symmetry, **kw, **more)


def _mirror_loss_gradient(ppo, obs, tgt, perm, mb):
    """(the launch's gradient, autograd's of the definition sym_coef (1 / mb) sum_i |mu(s_i) - target_i|^2 / 2)"""
    grad = torch.zeros_like(ppo.policy.theta)
    ppo._distill.minibatch_grad(ppo.policy.theta, grad, obs, tgt, torch.zeros(obs.shape[0], device=DEV), None, perm, 0, mb, "mse", 0.0,
                                ppo.sym_coef, ppo.sym_sums)
    idx = perm[:mb]
    ppo.policy.grad.zero_()
    loss = ppo.sym_coef * 0.5 * ((ppo.policy.mean(obs.index_select(0, idx)) - tgt.index_select(0, idx)) ** 2).sum(-1).mean()
    loss.backward()
    want = ppo.policy.grad.detach().clone()
    ppo.policy.grad.zero_()
    return grad, want, loss.item()


@pytest.mark.parametrize("mode", ["loss", "both"])
def test_mirror_loss_target_and_gradient(mode):
    """symmetry="loss" / "both" at T = 4, n = 16: the stored target is M_a mu_old(M_o s) of every sample the learner reads (the
    mirrored ones too), against MlpPolicy in torch at the act kernel's tolerance of tests/test_gpu_policy.py (1e-5); the gradient of
    the mirror loss against torch autograd of its definition at that file's autograd tolerance (rtol 1e-3, atol 1e-5 of the largest
    entry); an update runs and moves the parameters"""
    env, ppo = _tiny_trainer(mode, sym_coef=0.7)
    with torch.no_grad():
        ppo.policy.theta.add_(0.05 * torch.randn_like(ppo.policy.theta))
    batch = ppo.collect()
    obs = batch[0]
    N = obs.shape[0]
    assert N == (128 if mode == "both" else 64) and ppo.b_tgt.shape[0] * 16 == N
    tgt = ppo.b_tgt.reshape(N, 25)
    with torch.no_grad():
        want_tgt = ppo.mirror.actions(ppo.policy.mean(ppo.mirror.rows(obs.contiguous())).contiguous())
    torch.testing.assert_close(tgt, want_tgt, rtol=1e-5, atol=1e-5)
    assert (tgt - ppo.policy.mean(obs)).abs().max().item() > 1e-3          # a policy that is not symmetric: the loss is there
    mb = ppo._mb(N)
    perm = torch.rand(N, device=DEV).argsort()
    grad, want, loss = _mirror_loss_gradient(ppo, obs, tgt, perm, mb)
    assert loss > 0
    torch.testing.assert_close(grad, want, rtol=1e-3, atol=1e-5 * float(want.abs().max()))
    before = ppo.policy.theta.detach().clone()
    info = ppo.update(batch)
    assert not same_bits(before, ppo.policy.theta) and torch.isfinite(ppo.policy.theta).all() and np.isfinite(info["policy_loss"])
    # the step is PPO's gradient plus the mirror loss': with sym_coef 0 it is the plain step's gradient
    g0, g1 = torch.zeros_like(grad), torch.zeros_like(grad)
    ppo.kern.minibatch_stats(batch[4], perm, ppo._steps, mb, ppo.mb_stats)
    ppo.kern.minibatch_grad(ppo.policy.theta, g0, *batch[:6], perm, 0, mb, ppo.mb_stats[0], ppo.cliprange, ppo.ent_coef, ppo.vf_coef)
    ppo._distill.minibatch_grad(ppo.policy.theta, g1, obs, tgt, batch[3], None, perm, 0, mb, "mse", 0.0, 0.0, ppo.sym_sums)
    assert (g1 == 0).all() and g0.abs().max().item() > 0


def test_symmetrized_parameters_have_no_mirror_loss():
    """for symmetrize_theta'd parameters mu(s) == M_a mu(M_o s): the targets are the means and the mirror loss and its gradient are
    zero at the tolerance above - 1e-5 on the means, and on the gradient 1e-5 of the largest entry the same launch gives against
    targets of zero; symmetric_action is then the mean itself"""
    from trex_gym.symmetry import symmetrize_theta
    env, ppo = _tiny_trainer("loss")
    with torch.no_grad():
        ppo.policy.theta.add_(0.05 * torch.randn_like(ppo.policy.theta))
    raw = ppo.policy.theta.detach().clone()
    symmetrize_theta(ppo.policy, ppo.mirror, ppo.kern.layout)
    assert not same_bits(raw, ppo.policy.theta)
    once = ppo.policy.theta.detach().clone()
    symmetrize_theta(ppo.policy, ppo.mirror, ppo.kern.layout)
    torch.testing.assert_close(ppo.policy.theta.detach(), once, rtol=0, atol=1e-7)          # a projection
    batch = ppo.collect()
    obs, N = batch[0], batch[0].shape[0]
    tgt = ppo.b_tgt.reshape(N, 25)
    with torch.no_grad():
        mu = ppo.policy.mean(obs)
    torch.testing.assert_close(tgt, mu, rtol=1e-5, atol=1e-5)
    perm = torch.rand(N, device=DEV).argsort()
    grad, want, loss = _mirror_loss_gradient(ppo, obs, tgt, perm, N // 2)
    scale, _, _ = _mirror_loss_gradient(ppo, obs, torch.zeros_like(tgt), perm, N // 2)
    assert loss <= 25 * 0.5 * 1e-10 and grad.abs().max().item() <= 1e-5 * scale.abs().max().item()
    sa = ppo.mirror.symmetric_action(ppo)
    mean = torch.empty_like(sa)
    ppo.kern.act(ppo.policy.theta, env.rows, torch.zeros_like(sa), mean, clip_obs=ppo.clip_obs)
    torch.testing.assert_close(sa, mean, rtol=1e-5, atol=1e-5)


def test_symmetric_action_is_equivariant_bitwise():
    """symmetric_action(M_o s) == M_a symmetric_action(s), bit for bit, for parameters that are NOT symmetric, on rows of a rollout"""
    env, ppo = _tiny_trainer("augment")
    with torch.no_grad():
        ppo.policy.theta.add_(0.05 * torch.randn_like(ppo.policy.theta))
    ppo.collect()
    rows = env.rows.clone()
    mirrored = ppo.mirror.rows(rows)
    a, b = ppo.mirror.symmetric_action(ppo, rows), ppo.mirror.symmetric_action(ppo, mirrored)
    assert same_bits(b, ppo.mirror.actions(a)) and not same_bits(a, b)
    assert same_bits(ppo.mirror.rows(mirrored), rows)


def test_trainer_without_symmetry_is_unchanged():
    """MirrorPPO(symmetry=None) is plain PPO of this tree: two updates give the same parameters bit for bit. (That plain PPO is what
    it was before the mirror maps is not shown here: scripts/symmetry_bench.py times it against a build of the parent.)"""
    thetas = []
    for with_arg in (False, True):
        env, ppo = _tiny_trainer(None, with_arg=with_arg)
        for _ in range(2):
            ppo.update(ppo.collect())
        assert ppo.b_obs.shape[0] == 4 and ppo.b_val.shape[0] == 5
        thetas.append(ppo.policy.theta.detach().clone())
    assert same_bits(*thetas)


def test_trainer_augment_matches_the_concatenated_data():
    """MirrorPPO(symmetry="augment") on the T-rex at T = 4, n = 16, D = 75, A = 25, nminibatches = 2: the rollout buffers' second halves
    are the reference's images of the first; the running moments are symmetric; an epoch runs 4 steps of the plain minibatch size;
    the gradient of the first minibatch is that of oracle/ppo_oracle.py on the explicitly concatenated data, at the tolerance of
    tests/test_gpu_policy.py"""
    from oracle import ppo_oracle as PO
    import test_gpu_policy as TP
    env, ppo = _tiny_trainer("augment")
    mirror = ppo.mirror
    batch = ppo.collect()
    obs, act, logp, val, adv, ret = [b.cpu().numpy() for b in batch[:6]]
    N = 64
    assert obs.shape == (2 * N, 75) and act.shape == (2 * N, 25) and all(b.shape == (2 * N,) for b in (logp, val, adv, ret))
    o_t, a_t = (mirror.obs_table.src, mirror.obs_table.sign), (mirror.act_table.src, mirror.act_table.sign)
    assert obs[N:].tobytes() == R.mirror_rows(*o_t, obs[:N]).tobytes() and act[N:].tobytes() == R.mirror_rows(*a_t, act[:N]).tobytes()
    for b in (logp, val, adv, ret):
        assert b[N:].tobytes() == b[:N].tobytes()
    st = ppo.kern.get_stats()
    m, v = R.symmetrize_stats(*o_t, st["obs_mean"], st["obs_var"])
    assert m.tobytes() == st["obs_mean"].tobytes() and v.tobytes() == st["obs_var"].tobytes()
    assert ppo._steps == 4 and ppo.mb_stats.shape[0] == 4
    # the gradient of the first minibatch: the native launch on the device buffers against the f64 oracle on data concatenated here
    full = [np.concatenate([obs[:N], R.mirror_rows(*o_t, obs[:N])]), np.concatenate([act[:N], R.mirror_rows(*a_t, act[:N])])] + \
        [np.concatenate([b[:N], b[:N]]) for b in (logp, val, adv, ret)]
    mb = ppo._mb(2 * N)
    assert mb == N // 2
    perm = torch.rand(2 * N, device=DEV).argsort()
    ppo.kern.minibatch_stats(batch[4], perm, ppo._steps, mb, ppo.mb_stats)
    grad = torch.zeros_like(ppo.policy.theta)
    ppo.kern.minibatch_grad(ppo.policy.theta, grad, *batch[:6], perm, 0, mb, ppo.mb_stats[0], ppo.cliprange, ppo.ent_coef, ppo.vf_coef)
    idx = perm[:mb].cpu().numpy()
    assert (idx >= N).any() and (idx < N).any()          # the minibatch mixes real and mirrored samples
    h = [x[idx].astype(np.float64) for x in full]
    prm = TP._theta_to_params(ppo.kern, ppo.policy.theta)
    out, grads = PO.ppo_loss_and_grads(prm, h[0], h[1], -h[2], h[3], h[4], h[5], cliprange=ppo.cliprange, ent_coef=ppo.ent_coef, vf_coef=ppo.vf_coef)
    gflat = TP._grads_to_flat(ppo.kern, grads)
    np.testing.assert_allclose(grad.cpu().double().numpy(), gflat, rtol=1e-4, atol=1e-5 * np.abs(gflat).max())
    before = ppo.policy.theta.detach().clone()
    ppo.update(batch)
    assert not same_bits(before, ppo.policy.theta) and torch.isfinite(ppo.policy.theta).all()


def test_trainer_both_under_graphs_replays_the_eager_run():
    """use_graphs=True with symmetry="both" - the rollout with its symmetrize launches, the mirror targets' act calls, GAE and the
    augment launch captured, the epoch of 2 x nminibatches steps of two gradient launches, their sum and Adam captured - against the eager trainer: the augmented rollout buffers and theta after the update bit for bit.
    The captured epoch draws its permutation at the generator state its warm-up leaves (two draws of 2 T n numbers); the eager side
    is put at the same state (the scheme of tests/test_gpu_critic.py)."""
    _, e = _tiny_trainer("both", seed=5)
    be = e.collect()
    _, g = _tiny_trainer("both", use_graphs=True, seed=5)
    bg = g.collect()
    for x, y in zip(be[:6] + (e.b_tgt,), bg[:6] + (g.b_tgt,)):
        assert torch.equal(x, y)
    N, before = be[0].shape[0], e.policy.theta.clone()
    assert N == 2 * 4 * 16
    torch.manual_seed(77)
    torch.rand(N, device=DEV); torch.rand(N, device=DEV)
    ie = e.update(be)
    torch.manual_seed(77)
    ig = g.update(bg)
    assert torch.equal(e.policy.theta, g.policy.theta) and torch.equal(e.adam_m, g.adam_m)
    assert ie == ig and not torch.equal(e.policy.theta, before)
    torch.manual_seed(78)
    be = e.collect()
    torch.manual_seed(78)
    bg = g.collect()
    assert all(torch.equal(x, y) for x, y in zip(be[:6], bg[:6])) and torch.equal(e.b_tgt, g.b_tgt)
    e.env.close(); g.env.close()


def test_training_script_stores_the_tables(tmp_path):
    """trex_train.train(symmetry="augment") trains MirrorPPO and the checkpoint carries the option and the mirror tables as plain
    values (it loads with weights_only)"""
    from trex_gym import trex_train
    args = trex_train.parse_args(["--symmetry", "augment"]) if hasattr(trex_train, "parse_args") else None
    assert args is None or args.symmetry == "augment"
    env = trex_train.build_environment(64, device=DEV)
    path = str(tmp_path / "ck.pt")
    agent, hist = trex_train.train(env, 2 * 64 * 4, 0, nsteps=4, noptepochs=1, save_path=path, log=lambda *_: None, symmetry="augment")
    assert agent.symmetry == "augment" and agent.b_obs.shape[0] == 8 and len(hist) == 2
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sym = ck["symmetry"]
    assert sym["mode"] == "augment" and sym["pair"] == agent.mirror.pair.tolist() and sym["sign"] == agent.mirror.sign.tolist()
    assert sym["obs_dim"] == 75 and len(sym["row_src"]) == 77 and sym["lateral"] == agent.mirror.lateral
    plain, _ = trex_train.train(trex_train.build_environment(64, device=DEV), 64 * 4, 0, nsteps=4, noptepochs=1, save_path=path, log=lambda *_: None)
    assert torch.load(path, map_location="cpu", weights_only=True)["symmetry"] is None and type(plain).__name__ == "PPO"


def test_mirrored_clips():
    """symmetry.mirrored_clip on the T-rex: every frame is mirror.state of the clip's; twice gives the clip back (a quaternion up to its
    sign); a looping clip is shifted by half a cycle, closes on itself and keeps the mirrored displacement"""
    from trex_gym.motion import Clip
    from trex_gym.symmetry import Mirror, clip_with_mirror, mirrored_clip
    from trex_gym.vec_env import TrexVecEnv
    env = TrexVecEnv(2, device=DEV)
    mirror = Mirror(env, log=None)
    rng = np.random.default_rng(4)
    F, J = 9, 25
    lo, hi = np.asarray(env.model.lower), np.asarray(env.model.upper)
    frames = np.zeros((F, 7 + J))
    frames[:, :3] = np.cumsum(rng.uniform(0.0, 0.1, (F, 3)), 0) + (0, 0, 3.0)
    q = rng.normal(size=(F, 4)) * (0.1, 0.1, 0.1, 1.0)
    frames[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    frames[:, 7:] = rng.uniform(lo, hi, (F, J)) * 0.5
    vel = rng.normal(size=(F, 6 + J))
    clip = Clip(frames, 0.02, False, vel)
    once = mirrored_clip(clip, mirror)
    st = np.zeros((F, 13 + 2 * J))
    st[:, :7], st[:, 13:13 + J], st[:, 7:13], st[:, 13 + J:] = frames[:, :7], frames[:, 7:], vel[:, :6], vel[:, 6:]
    want = mirror.state(torch.tensor(st, dtype=torch.float64)).numpy()
    assert np.abs(once.frames - np.concatenate([want[:, :7], want[:, 13:13 + J]], 1)).max() < 1e-12
    assert np.abs(once.velocities - np.concatenate([want[:, 7:13], want[:, 13 + J:]], 1)).max() < 1e-12
    assert np.abs(once.frames[:, 7:] - clip.frames[:, 7:][:, mirror.pair] * mirror.sign).max() == 0 and not np.allclose(once.frames, clip.frames)
    twice = mirrored_clip(once, mirror)
    flip = np.sign((twice.frames[:, 3:7] * frames[:, 3:7]).sum(1))[:, None]
    twice.frames[:, 3:7] *= flip
    assert np.abs(twice.frames - frames).max() < 1e-12 and np.abs(twice.velocities - vel).max() < 1e-12
    both = clip_with_mirror(clip, mirror)
    assert both.num_frames == 2 * F and (both.frames[:F] == frames).all() and np.abs(both.frames[F, :2] - frames[-1, :2]).max() < 1e-12
    assert np.abs(both.frames[F:, 2:] - once.frames[:, 2:]).max() == 0 and both.velocities.shape == (2 * F, 6 + J)
    assert np.abs(np.diff(both.frames[F:, :2], axis=0) - np.diff(once.frames[:, :2], axis=0)).max() < 1e-12
    loop_frames = frames.copy()
    loop_frames[-1, 3:] = loop_frames[0, 3:]
    loop = Clip(loop_frames, 0.02, True)
    m = mirrored_clip(loop, mirror)
    plain = mirrored_clip(Clip(loop_frames, 0.02, False), mirror)
    P, h = F - 1, (F - 1) // 2
    disp = plain.frames[-1, :3] - plain.frames[0, :3]
    assert m.loop and m.num_frames == F and np.abs(m.frames[0] - plain.frames[h]).max() == 0
    assert np.abs(m.frames[-1, 3:] - m.frames[0, 3:]).max() == 0 and np.abs(m.frames[-1, :3] - m.frames[0, :3] - disp).max() < 1e-12
    assert np.abs(m.frames[P - h, :3] - (plain.frames[0, :3] + disp)).max() < 1e-12
    joined = clip_with_mirror(loop, mirror)
    assert joined.loop and joined.num_frames == 2 * F - 1 and np.abs(joined.frames[F - 1, :2] - loop_frames[-1, :2]).max() == 0
    from trex_gym import motion as M
    M.attach(env, joined, terms=M.imitation(env.model, end_effectors=False))      # the device takes the joined clip
    env.reset_tensor()
    env.step_tensor(torch.zeros(2, 25, device=DEV))
    assert torch.isfinite(env.rew).all()
    env.close()


def test_trainer_augments_the_critic_rows():
    """MirrorPPO(symmetry="augment", critic=True) at T = 4, n = 16: the critic table is the observation table for clean() and the
    caller's rule for tensor(); the second half of b_obs_v is the table's image of the first, bit for bit; the critic's running
    moments are symmetric under it; an update runs. A tensor() source without a rule, a drawn element whose partner is not drawn
    and the mirror loss with critic= are refused."""
    from trex_gym import critic as C
    from trex_gym.symmetry import Mirror, MirrorPPO
    from trex_gym.vec_env import TrexVecEnv
    env = TrexVecEnv(16, device=DEV)
    extra = torch.randn(16, 4, device=DEV)
    C.attach(env, [C.clean(), C.tensor(extra)])
    mirror = Mirror(env, log=None)
    rule = ([1, 0, 2, 3], [1, 1, -1, 1])
    kw = dict(nsteps=4, nminibatches=2, noptepochs=1, seed=3, critic=True)
    with pytest.raises(ValueError, match="caller rule"):
        MirrorPPO(env, mirror, **kw)
    with pytest.raises(ValueError, match="permute"):
        MirrorPPO(env, mirror, critic_tensor_rules=[([0, 0, 2, 3], [1, 1, 1, 1])], **kw)
    with pytest.raises(ValueError, match="refused together with critic"):
        MirrorPPO(env, mirror, symmetry="loss", critic_tensor_rules=[rule], **kw)
    ppo = MirrorPPO(env, mirror, critic_tensor_rules=[rule], **kw)
    t = mirror.critic_table
    assert t.width == 79 and t.src.tolist() == mirror.obs_table.src.tolist() + [76, 75, 77, 78]
    assert t.sign.tolist() == mirror.obs_table.sign.tolist() + [1, 1, -1, 1] and t.involution
    batch = ppo.collect()
    N = 64
    v = ppo.b_obs_v.reshape(2 * N, 79).cpu().numpy()
    assert v[N:].tobytes() == R.mirror_rows(t.src, t.sign, v[:N]).tobytes() and np.abs(v[:N, 75:]).max() > 0
    obs = batch[0].cpu().numpy()
    assert obs[N:].tobytes() == R.mirror_rows(mirror.obs_table.src, mirror.obs_table.sign, obs[:N]).tobytes()
    st = ppo.crit.get_stats()
    m, var = R.symmetrize_stats(t.src, t.sign, st["mean"], st["var"])
    assert m.tobytes() == np.asarray(st["mean"]).tobytes() and var.tobytes() == np.asarray(st["var"]).tobytes()
    before = ppo.policy.theta.detach().clone()
    ppo.update(batch)
    assert not same_bits(before, ppo.policy.theta) and torch.isfinite(ppo.policy.theta).all()
    # the rules of the other sources, on a stand-in for the env's records: a mass term on a body without its partner is refused
    import types
    fake = types.SimpleNamespace(critic_spec=dict(sources=[["random", [0, [1, 2]]]], dim=2), randomization=dict(terms=[(0, 6, 0, 0)]),
                                 _links=env._links)
    with pytest.raises(ValueError, match="its mirror partner"):
        mirror.critic_rules(fake)
    a, b = 1, int(mirror.body_pair[1])
    fake.critic_spec = dict(sources=[["random", [0, [a, b]]], ["command", None], ["random", [1, [2, 3]]]], dim=7)
    fake.randomization = dict(terms=[(0, 0, 0, 0), (2, 0, 0, 0)])
    src, sign = mirror.critic_rules(fake)
    assert int(mirror.pair[2]) == 3                      # femur left / right
    assert src.tolist() == [1, 0, 2, 3, 4, 6, 5] and sign.tolist() == [1, 1] + mirror.command_table[1].tolist() + [1, 1]
    env.close()
