"""External wrench per env and body (trex_batch_set_external_wrench, include/trex_batch.h) on the GPU: pinned against the f64
oracle through an exact restatement of gravity, momentum balance in free flight, bitwise identities for the zero wrench, the
launch forms, resets and step_many, refusals, containment, and the Python surface (trex_gym.perturb, TrexVecEnv).
The exact comparison - one-hot forces and torques per body, in contact, against the oracle's own wrench: tests/test_gpu_feature_oracle.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import ASSET_URDF
from gpu_support import DEV, contact_counts, make_vec, random_actions
from parity_helpers import GOLD, assert_step_close
from state_sets import landing_states

pytestmark = pytest.mark.gpu
NB, J = 26, 25


@pytest.fixture(scope="module")
def capi():
    from trex_gym import _capi
    return _capi


# ---------------------------------------------------------------- 1. the oracle, through gravity g + delta
@pytest.mark.parametrize("delta", [4.9, -4.9])
@pytest.mark.parametrize("randomised_mass", [False, True])
def test_vertical_wrench_is_a_change_of_gravity(delta, randomised_mass, oracle64, model):
    """F_b = (0, 0, -delta m_b s_b) on every body restates gravity g + delta exactly (gravity enters the oracle nowhere else):
    one step from landing and crouch states against Oracle(gravity = g + delta), contact counts included."""
    from oracle import oracle as O
    g = oracle64.params["gravity"]
    orc = O.Oracle(model, params={"gravity": g + delta})
    ls, la = landing_states(oracle64, model)
    states = np.concatenate([ls, GOLD["crouch_state"][30:36].astype(np.float32)])
    acts = np.concatenate([la, GOLD["crouch_actions"][:6].astype(np.float32)])
    n = len(states)
    rng = np.random.default_rng(3)
    ms = rng.uniform(0.8, 1.2, (n, NB)).astype(np.float32) if randomised_mass else np.ones((n, NB), np.float32)
    w = np.zeros((n, NB, 6), np.float32)
    w[:, :, 2] = -delta * model["mass"][None, :] * ms
    v = make_vec(n)
    v.reset()
    if randomised_mass:
        v.set_domain(torch.tensor(ms))
    v.set_external_wrench(torch.tensor(w))
    v.set_state(torch.tensor(states))
    obs, rew, _, _ = v.step(acts)
    cnt = contact_counts(v).cpu().numpy()
    changed = 0
    for e in range(n):
        s = orc.new_state()
        if randomised_mass:
            orc.set_domain(s, ms[e].astype(np.float64))
        orc.set_state(s, states[e].astype(np.float64))
        o, r, _ = orc.step(s, acts[e].astype(np.float64))
        assert_step_close(obs[e], o, rew[e], r, "delta %g state %d" % (delta, e))
        assert cnt[e] == len(orc.contacts(s)[0]), e
        s0 = oracle64.new_state()
        if randomised_mass:
            oracle64.set_domain(s0, ms[e].astype(np.float64))
        oracle64.set_state(s0, states[e].astype(np.float64))
        o0, _, _ = oracle64.step(s0, acts[e].astype(np.float64))
        changed += np.abs(o0 - o).max() > 1e-3
    assert changed >= n // 2          # the changed gravity really changes the step
    assert (cnt > 0).sum() > 10


# ---------------------------------------------------------------- 2. free flight: momentum balance
def test_free_flight_momentum_balance(model, oracle64):
    """Over one env-step T: d(linear momentum) = T sum F_b, d(angular momentum about the world origin) =
    T sum (c_b x F_b + tau_b) (forced minus unforced, from the GPU states): world axes, force at the COM, torque about it."""
    m = make_vec(4, params={"link_damping": 0.0})
    m.reset()
    st = m.get_state().clone()
    st[:, 2] += 5.0
    m.set_state(st)
    mtot = float(model["mass"].sum())
    g = oracle64.params["gravity"]
    rng = np.random.default_rng(11)
    w = np.zeros((4, NB, 6), np.float32)
    mb = model["mass"][:, None]
    for e in (0, 1):   # random forces and torques on every body, scaled with its mass (sum |F| ~ 0.5 M g, base torque ~ 1e3 N m)
        w[e, :, :3] = rng.normal(size=(NB, 3)) * 0.5 * g * mb
        w[e, :, 3:] = rng.normal(size=(NB, 3)) * 1e3 * mb / mb.max()
    w[3, 0, 3:] = [2e3, -1e3, 3e3]            # a pure torque on the base
    s0 = st[0].cpu().numpy().astype(np.float64)
    s = oracle64.new_state()
    oracle64.set_state(s, s0)
    pos, rot = oracle64.body_poses(s)
    c = pos + np.einsum("bij,bj->bi", rot, model["com"])          # body COMs at the start

    def momenta(row):
        s = oracle64.new_state()
        oracle64.set_state(s, row.astype(np.float64))
        h = oracle64.energy(s)["momentum"]
        p0, _ = oracle64.body_poses(s)
        return h[3:6], h[0:3] + np.cross(p0[0], h[3:6])          # linear; angular about the world origin
    m.set_external_wrench(torch.tensor(w))
    m.step_tensor(torch.tensor(model["q_start"][model["obs_order"]], dtype=torch.float32, device=DEV).repeat(4, 1))
    st1 = m.get_state().cpu().numpy()
    T = oracle64.params["substeps"] * oracle64.params["dt"]
    l0, a0 = momenta(s0)
    lu, au = momenta(st1[2])                  # unforced
    for e in (0, 1, 3):
        l1, a1 = momenta(st1[e])
        F = w[e, :, :3].astype(np.float64)
        want_l = T * F.sum(0)
        want_a = T * (np.cross(c, F) + w[e, :, 3:]).sum(0)
        dl, da = (l1 - l0) - (lu - l0), (a1 - a0) - (au - a0)
        if e == 3:
            assert np.linalg.norm(dl) <= 0.01 * T * 0.5 * mtot * g, dl
        else:
            assert np.linalg.norm(dl - want_l) <= 0.01 * np.linalg.norm(want_l), (dl, want_l)
        assert np.linalg.norm(da - want_a) <= 0.02 * np.linalg.norm(want_a), (e, da, want_a)


# ---------------------------------------------------------------- 3. the zero wrench is bitwise the plain step
@pytest.mark.parametrize("n,params", [(4096, None), (4097, None), (4096, {"warmstart": 0.85})])
def test_zero_wrench_is_bitwise_the_plain_step(n, params, model):
    plain, zero, cleared = (make_vec(n, params=params) for _ in range(3))
    for v in (plain, zero, cleared):
        v.reset_tensor()
    zero.set_external_wrench(torch.zeros(n, NB, 6))
    cleared.set_external_wrench(torch.randn(n, NB, 6) * 100)
    cleared.clear_external_wrench()
    gen = torch.Generator(device=DEV).manual_seed(7)
    for t in range(30):
        a = random_actions(model, n, gen)
        rows = []
        for v in (plain, zero, cleared):
            v.step_tensor(a)
            rows.append(v.rows.clone())
        assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2]), t
    assert torch.equal(plain.get_state(), zero.get_state()) and torch.equal(plain.get_state(), cleared.get_state())
    assert torch.equal(contact_counts(plain), contact_counts(zero)) and torch.equal(contact_counts(plain), contact_counts(cleared))
    assert contact_counts(plain).sum() > 0


# ---------------------------------------------------------------- 4. independence and launch forms
def test_wrench_acts_on_its_envs_only(model):
    n = 4096
    free, forced = make_vec(n), make_vec(n)
    for v in (free, forced):
        v.reset_tensor()
    gen = torch.Generator(device=DEV).manual_seed(2)
    half = torch.randperm(n, generator=gen, device=DEV)[: n // 2]
    w = torch.zeros(n, NB, 6, device=DEV)
    w[half, 0, :2] = 5e3 * torch.randn(n // 2, 2, generator=gen, device=DEV)
    w[half, 5, 3:] = 1e3 * torch.randn(n // 2, 3, generator=gen, device=DEV)
    forced.set_external_wrench(w)
    other = torch.ones(n, dtype=torch.bool, device=DEV)
    other[half] = False
    for t in range(20):
        a = random_actions(model, n, gen)
        free.step_tensor(a)
        forced.step_tensor(a)
        assert torch.equal(free.rows[other], forced.rows[other]), t
    assert not torch.equal(free.rows[~other], forced.rows[~other])


def test_pair_and_single_launch_forms_agree_bitwise(model):
    """4096 envs step in the pair form, 4097 in the single-env form: the same wrench, the same rows (wave balance on)."""
    a_pair, a_single = make_vec(4096), make_vec(4097)
    assert a_pair.batch.launch_info()["block"] == 128 and a_single.batch.launch_info()["block"] == 64
    gen = torch.Generator(device=DEV).manual_seed(4)
    w = torch.zeros(4097, NB, 6, device=DEV)
    w[:, 0, :3] = 3e3 * torch.randn(4097, 3, generator=gen, device=DEV)
    w[:, 9, 3:] = 5e2 * torch.randn(4097, 3, generator=gen, device=DEV)
    for v in (a_pair, a_single):
        v.batch.set_wave_balance(1)
        v.reset_tensor()
    a_single.set_external_wrench(w)
    a_pair.set_external_wrench(w[:4096])
    for t in range(60):
        a = random_actions(model, 4097, gen)
        a_single.step_tensor(a)
        a_pair.step_tensor(a[:4096])
        assert torch.equal(a_single.rows[:4096], a_pair.rows), t
    assert torch.equal(a_single.get_state()[:4096], a_pair.get_state())


# ---------------------------------------------------------------- 5. resets
def test_resets_do_not_feel_the_wrench():
    n = 8
    w = torch.zeros(n, NB, 6)
    w[:, 0, 0] = 2e4
    w[:, 3, 5] = 3e3
    plain, forced = make_vec(n), make_vec(n)
    forced.set_external_wrench(w)
    o0, o1 = plain.reset_tensor().clone(), forced.reset_tensor().clone()
    assert torch.equal(o0, o1)
    plain.batch.reset(obs := torch.zeros(n, 3 * J, device=DEV))
    forced.batch.reset(obs2 := torch.zeros(n, 3 * J, device=DEV))
    assert torch.equal(obs, obs2)
    a = torch.zeros(n, J, device=DEV)
    plain.step_tensor(a)
    forced.step_tensor(a)
    assert not torch.equal(plain.rows, forced.rows)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[::2] = 1
    plain.reset_tensor(mask)
    forced.reset_tensor(mask)
    assert torch.equal(plain.rows[::2], forced.rows[::2])
    assert torch.equal(plain.get_state()[::2], forced.get_state()[::2])


def test_episode_limit_reset_settles_without_the_wrench():
    """The env whose episode ends in the step: done = 1 and the reward of the FORCED step, then the observation of a plain
    reset (the settle substep feels no wrench)."""
    n = 4
    w = torch.zeros(n, NB, 6)
    w[:, 0, :3] = torch.tensor([3e4, -2e4, 1e4])
    a = torch.zeros(n, J, device=DEV)
    fresh = make_vec(n)
    first = fresh.reset_tensor().clone()
    v = make_vec(n, max_episode_steps=5)
    v.set_external_wrench(w)
    v.reset_tensor()
    v.set_episode_steps(torch.tensor([4, 0, 0, 0], dtype=torch.int32))
    ref_forced, ref_plain = make_vec(n), make_vec(n)
    ref_forced.set_external_wrench(w)
    for r in (ref_forced, ref_plain):
        r.reset_tensor()
    o, rew, d = v.step_tensor(a)
    of, rf, _ = ref_forced.step_tensor(a)
    op, rp, _ = ref_plain.step_tensor(a)
    assert d.tolist() == [True, False, False, False]
    assert rew[0].item() == rf[0].item() and rew[0].item() != rp[0].item()
    assert torch.equal(o[0], first[0])
    assert torch.equal(o[1:], of[1:]) and torch.equal(rew[1:], rf[1:])


# ---------------------------------------------------------------- 6. step_many
def test_step_many_is_bitwise_the_steps_one_by_one(model):
    n, S = 256, 8
    gen = torch.Generator(device=DEV).manual_seed(9)
    w = torch.zeros(n, NB, 6, device=DEV)
    w[:, :, :3] = 200 * torch.randn(n, NB, 3, generator=gen, device=DEV)
    w[:, :, 3:] = 50 * torch.randn(n, NB, 3, generator=gen, device=DEV)
    acts = torch.stack([random_actions(model, n, gen) for _ in range(S)])
    many, rows = make_vec(n, max_episode_steps=6), make_vec(n, max_episode_steps=6)
    for v in (many, rows):
        v.reset_tensor()
        v.set_episode_steps(torch.arange(n, dtype=torch.int32) % 6)
        v.set_external_wrench(w)
    out = many.step_many_tensor(acts)
    for s in range(S):
        rows.step_tensor(acts[s])
        assert torch.equal(out[s], rows.rows), s
    assert torch.equal(many.get_state(), rows.get_state())


# ---------------------------------------------------------------- 7. refusals and containment
def test_bad_wrench_buffers_and_debug_step_are_refused(capi):
    n = 16
    b = capi.Batch(capi.Model(ASSET_URDF), n, 0)
    need = n * NB * 6
    with pytest.raises(capi.TrexError):
        b.set_external_wrench(torch.zeros(n, NB, 6))                          # host tensor
    with pytest.raises(capi.TrexError):
        b.set_external_wrench(torch.zeros(n, NB, 5, device=DEV))              # short / wrong shape
    # the C-ABI itself: a host pointer and an exactly-sized short allocation
    host = np.zeros(need, np.float32)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert capi.lib.trex_batch_set_external_wrench(b.h, C.c_void_p(host.ctypes.data), s) == capi.E_INVALID
    hip = C.CDLL("libamdhip64.so")
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(4 * need - 4)) == 0
    try:
        assert capi.lib.trex_batch_set_external_wrench(b.h, p, s) == capi.E_INVALID
    finally:
        torch.cuda.synchronize()
        hip.hipFree(p)
    # debug_step: fine without a wrench, refused while one is set, fine again once it is cleared
    a, obs, dbg = torch.zeros(n, J, device=DEV), torch.zeros(n, 3 * J, device=DEV), torch.zeros(4096, device=DEV)
    b.reset()
    b.debug_step(a, obs, dbg)
    b.set_external_wrench(torch.zeros(n, NB, 6, device=DEV))
    with pytest.raises(capi.TrexError) as ei:
        b.debug_step(a, obs, dbg)
    assert ei.value.code == capi.E_INVALID
    b.set_external_wrench(None)
    b.debug_step(a, obs, dbg)
    torch.cuda.synchronize()
    b.close()


def test_non_finite_wrench_is_contained():
    n = 6
    w = torch.zeros(n, NB, 6)
    w[2, 4, 1] = float("nan")
    v, ref = make_vec(n), make_vec(n)
    for x in (v, ref):
        x.reset_tensor()
    v.set_external_wrench(w)
    a = torch.zeros(n, J, device=DEV)
    o, r, d = v.step_tensor(a)
    o0, r0, _ = ref.step_tensor(a)
    assert d.tolist() == [False, False, True, False, False, False]
    assert torch.isfinite(v.rows).all() and torch.isfinite(v.get_state()).all()
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(v.rows[keep], ref.rows[keep])


# ---------------------------------------------------------------- 8. Python surface
def test_apply_external_force_on_the_head(model, oracle64):
    n = 3
    v = make_vec(n)
    v.reset()
    hb = int(v.model.array("head_body")[0])
    link = [k for k, (_, b) in enumerate(v.model.links()) if b == hb][0]
    F = torch.tensor([[100.0, -50.0, 20.0], [0.0, 0.0, -300.0], [7.0, 8.0, 9.0]])
    pose = v.link_transforms()[:, link, :3].cpu()
    P = pose + torch.tensor([0.3, -0.2, 0.1])
    w = v.apply_external_force(link, F, P).cpu().numpy().astype(np.float64)
    st = v.get_state().cpu().numpy()
    for e in range(n):
        s = oracle64.new_state()
        oracle64.set_state(s, st[e].astype(np.float64))
        pos, rot = oracle64.body_poses(s)
        c = pos[hb] + rot[hb] @ model["com"][hb]
        want = np.zeros((NB, 6))
        want[hb, :3] = F[e].numpy()
        want[hb, 3:] = np.cross(P[e].numpy() - c, F[e].numpy())
        np.testing.assert_allclose(w[e], want, atol=1e-3 * np.abs(want).max())
    # it is what the next step applies: the same as set_external_wrench with that tensor
    other = make_vec(n)
    other.reset()
    other.set_external_wrench(torch.tensor(w, dtype=torch.float32))
    a = torch.zeros(n, J, device=DEV)
    v.step_tensor(a)
    other.step_tensor(a)
    assert torch.equal(v.rows, other.rows)
    v.clear_external_wrench()


def test_ppo_update_with_random_pushes():
    from trex_gym import trex_train
    env = trex_train.build_environment(4096, max_episode_steps=200, push_force=3000.0, push_interval=8, push_duration=3)
    assert env.pushes is not None
    agent, hist = trex_train.train(env, num_timesteps=4096 * 32, seed=0, nsteps=32, noptepochs=1, log=lambda s: None)
    assert len(hist) == 1
    for h in hist:
        assert all(math.isfinite(v) for v in (h["policy_loss"], h["value_loss"], h["entropy"], h["mean_step_reward"]))
    assert torch.isfinite(agent.obs).all()
