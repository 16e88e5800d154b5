"""Contact sensor (trex_batch_set_contact_sensor / trex_batch_contact_wrench, include/trex_batch.h) on the GPU: the per-body
floor-contact wrench against the f64 and f32 oracles (hulls and primitives, with and without domains), the one-substep
identity with contact_stats, statics, the friction pyramid, bitwise read-only-ness across the launch forms, reset semantics,
containment and refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ASSET_URDF
from gpu_support import DEV, make_vec, random_actions
from parity_helpers import GOLD, oracle_wrench
from state_sets import landing_states

pytestmark = pytest.mark.gpu
NB, J = 26, 25


@pytest.fixture(scope="module")
def capi():
    from trex_gym import _capi
    return _capi


def sensing(n, **kw):
    v = make_vec(n, **kw)
    v.enable_contact_sensor()
    return v


def weight(model, mass_scale=None, g=9.81):
    m = model["mass"] if mass_scale is None else model["mass"] * mass_scale
    return float(m.sum()) * g


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("collision", ["hulls", "primitives"])
@pytest.mark.parametrize("domain", [False, True])
def test_sensor_matches_the_oracle(collision, domain, model):
    """One env-step from landing and crouch states, per env and body, against the f64 oracle. Tolerance: the spread
    between the f32 and the f64 oracle on the same states is MEASURED here (the 60-sweep PGS is far from converged, so
    rounding moves impulses between the points of a body and between bodies); the GPU may differ from f64 by at most
    4 x that spread, with a floor of 1e-3 M g (forces) / 1e-3 M g x 1 m (moments), M g the env's weight. Measured on an
    MI355X: f32 - f64 up to 3.0e-4 .. 4.8e-4 M g over the four cases, GPU - f64 up to 2.2e-4 .. 6.0e-4 M g (medians
    below 1e-5): the GPU sits within the f32 oracle's own spread. Also: > 10 envs in contact, and the same touching bodies - those whose normal
    force exceeds 1 % of the weight on one side carry a positive normal force on the other."""
    from oracle import oracle as O, trex_model as tm
    om = tm.use_primitive_collision(model, 0.2, 3, 4) if collision == "primitives" else model
    o64, o32 = O.Oracle(om, precision="f64"), O.Oracle(om, precision="f32")
    ls, la = landing_states(o64, om)
    states = np.concatenate([ls, GOLD["crouch_state"][30:36].astype(np.float32)])
    acts = np.concatenate([la, GOLD["crouch_actions"][:6].astype(np.float32)])
    n = len(states)
    rng = np.random.default_rng(11)
    ms = rng.uniform(0.8, 1.2, (n, NB)).astype(np.float32) if domain else None
    fr = rng.uniform(0.6, 1.2, n).astype(np.float32) if domain else None
    v = sensing(n, collision=collision)
    v.reset()
    if domain:
        v.set_domain(torch.tensor(ms), torch.tensor(fr))
    v.set_state(torch.tensor(states))
    v.step(acts)
    gw = v.contact_wrench().cpu().numpy().astype(np.float64)
    err, spread, in_contact = [], [], 0
    for k in range(n):
        msk = None if ms is None else ms[k]
        frk = None if fr is None else float(fr[k])
        w64, touched = oracle_wrench(o64, om, states[k], acts[k], msk, frk)
        w32, _ = oracle_wrench(o32, om, states[k], acts[k], msk, frk)
        Mg = weight(om, msk)
        err.append(np.abs(gw[k] - w64).max() / Mg)
        spread.append(np.abs(w32 - w64).max() / Mg)
        in_contact += bool(touched)
        for b in range(NB):
            if w64[b, 2] > 0.01 * Mg:
                assert gw[k, b, 2] > 0, (k, b)
            if gw[k, b, 2] > 0.01 * Mg:
                assert b in touched and w64[b, 2] > 0, (k, b)
    err, spread = np.array(err), np.array(spread)
    tol = max(4 * spread.max(), 1e-3)
    print("contact wrench / Mg: gpu-f64 max %.2e median %.2e; f32-f64 max %.2e median %.2e; tol %.2e"
          % (err.max(), np.median(err), spread.max(), np.median(spread), tol))
    assert in_contact > 10
    assert err.max() <= tol


def test_one_substep_identity_with_contact_stats(model):
    """substeps = 1: sum_b F_z dt is the summed normal impulse of contact_stats (the same impulses summed in another order)."""
    n = 512
    v = sensing(n, params={"substeps": 1})
    v.reset_tensor()
    dt = v.model.get_param("dt")
    gen = torch.Generator(device=DEV).manual_seed(3)
    seen = 0
    for t in range(150):
        v.step_tensor(random_actions(model, n, gen))
        if t % 10 == 9:
            imp = torch.zeros(n, device=DEV)
            v.batch.contact_stats(None, imp)
            fz = v.contact_wrench()[:, :, 2].double().sum(1) * dt
            assert torch.allclose(fz, imp.double(), rtol=1e-5, atol=1e-9), t
            seen += int((imp > 0).sum())
    assert seen > 100


# ---------------------------------------------------------------- 2. statics, pyramid
def test_statics_of_the_standing_pose(model, oracle64):
    """Holding the start pose for 400 steps: the floor carries the weight (sum F = (0, 0, M g) within 1 %), the moments
    about the system COM balance (sum_b tau_b + (c_b - C) x F_b within 2e-2 M g x 1 m: a 2 cm centre-of-pressure offset,
    for a body that still sways slightly), bodies off the floor report exact zeros; an airborne env reports all zeros."""
    v = sensing(2)
    v.reset()
    q0 = model["q_start"][model["obs_order"]].astype(np.float32)
    a = np.tile(q0, (2, 1))
    for _ in range(400):
        v.step(a)
    w = v.contact_wrench().cpu().numpy().astype(np.float64)
    Mg = weight(model, g=oracle64.params["gravity"])
    for k in range(2):
        F = w[k, :, :3].sum(0)
        assert abs(F[2] - Mg) <= 0.01 * Mg and abs(F[0]) <= 0.01 * Mg and abs(F[1]) <= 0.01 * Mg, F
        s = oracle64.new_state()
        oracle64.set_state(s, v.get_state()[k].cpu().numpy().astype(np.float64))
        pos, rot = oracle64.body_poses(s)
        com = pos + np.einsum("bij,bj->bi", rot, model["com"])
        Cs = (model["mass"][:, None] * com).sum(0) / model["mass"].sum()
        M = (w[k, :, 3:] + np.cross(com - Cs, w[k, :, :3])).sum(0)
        assert np.abs(M).max() <= 2e-2 * Mg, M
        off = w[k, :, 2] <= 0
        assert off.any() and (w[k][off] == 0).all()
        assert (w[k, ~off, 2] > 0).all()
    st = v.get_state()
    st[1, 2] = 50.0
    v.set_state(st)
    v.step(a)
    w = v.contact_wrench()
    assert (w[1] == 0).all() and (w[0, :, 2] > 0).any()


def test_friction_pyramid_under_random_actions(model):
    n = 4096
    v = sensing(n)
    v.reset_tensor()
    mu = v.model.get_param("friction")
    gen = torch.Generator(device=DEV).manual_seed(5)
    touching = 0
    for t in range(40):
        v.step_tensor(random_actions(model, n, gen))
        if t % 4 == 3:
            w = v.contact_wrench()
            assert torch.isfinite(w).all()
            fz = w[..., 2]
            assert (fz >= 0).all()
            eps = 1e-4 * fz + 1e-3
            assert (w[..., 0].abs() <= mu * fz + eps).all() and (w[..., 1].abs() <= mu * fz + eps).all()
            touching += int((fz > 0).any(1).sum())
    assert touching > n


# ---------------------------------------------------------------- 3. read-only and the launch forms, bitwise
def outputs(v):
    cnt, imp = torch.zeros(v.num_envs, dtype=torch.int32, device=DEV), torch.zeros(v.num_envs, device=DEV)
    v.batch.contact_stats(cnt, imp)
    return [v.rows.clone(), v.done.clone(), v.get_state(), cnt, imp, v.episode_steps if v.max_episode_steps else cnt]


@pytest.mark.parametrize("n,kw,wrench", [(64, {}, False), (63, {}, False), (64, {"params": {"warmstart": 0.85}}, False),
                                         (63, {"params": {"warmstart": 0.85}}, True), (64, {"max_episode_steps": 7}, True),
                                         (63, {"max_episode_steps": 7, "penalties_in_rows": True}, False)])
def test_sensor_is_read_only(n, kw, wrench, model):
    """Sensor on against off: rows (obs | reward | done), done flags, state, contact_stats and episode counts bitwise, in the
    pair form (even n) and the single-env form (odd n), warm, with an external wrench, across episode-limit resets."""
    off, on = make_vec(n, **kw), sensing(n, **kw)
    gen = torch.Generator(device=DEV).manual_seed(n)
    w = 2e3 * torch.randn(n, NB, 6, generator=gen, device=DEV) if wrench else None
    for v in (off, on):
        v.reset_tensor()
        if w is not None:
            v.set_external_wrench(w)
        if v.max_episode_steps:
            v.set_episode_steps(torch.arange(n, dtype=torch.int32) % 7)
    for t in range(25):
        a = random_actions(model, n, gen)
        off.step_tensor(a)
        on.step_tensor(a)
        for x, y in zip(outputs(off), outputs(on)):
            assert torch.equal(x, y), t
    assert (on.contact_wrench()[..., 2] > 0).any()


def test_pair_single_and_step_many_agree_bitwise(model):
    """The sensor values: 4096 envs (pair form) against the first 4096 of 4097 (single-env form); step_many against the
    last of its S steps taken one by one; step_many's rows against the plain kernels'."""
    pair, single = sensing(4096), sensing(4097)
    assert pair.batch.launch_info()["block"] == 128 and single.batch.launch_info()["block"] == 64
    gen = torch.Generator(device=DEV).manual_seed(8)
    for v in (pair, single):
        v.batch.set_wave_balance(1)
        v.reset_tensor()
    for t in range(30):
        a = random_actions(model, 4097, gen)
        single.step_tensor(a)
        pair.step_tensor(a[:4096])
        assert torch.equal(single.contact_wrench()[:4096], pair.contact_wrench()), t
    n, S = 256, 6
    acts = torch.stack([random_actions(model, n, gen) for _ in range(S)])
    many, one, plain = sensing(n, max_episode_steps=5), sensing(n, max_episode_steps=5), make_vec(n, max_episode_steps=5)
    for v in (many, one, plain):
        v.reset_tensor()
        v.set_episode_steps(torch.arange(n, dtype=torch.int32) % 5)
    out = many.step_many_tensor(acts).clone()
    ref = plain.step_many_tensor(acts)
    assert torch.equal(out, ref)
    for s in range(S):
        one.step_tensor(acts[s])
    assert torch.equal(many.contact_wrench(), one.contact_wrench())
    assert torch.equal(many.get_state(), one.get_state())


# ---------------------------------------------------------------- 4. resets, containment
def lowered_start(model):
    """The highest start height (5 mm grid below the model's) whose settle substep pushes the body out of the floor with
    more than 20 % of its weight on the oracle (a start pose just inside the contact margin has points with zero impulse)."""
    from oracle import oracle as O
    z0 = float(model["base_start_pos"][2])
    for z in np.arange(z0, 0.0, -0.005):
        om = dict(model)
        om["base_start_pos"] = np.array([0.0, 0.0, z])
        orc = O.Oracle(om)
        s = orc.new_state()
        orc.reset(s)
        body, lam, _, _ = orc.contacts(s)
        if len(body) >= 2 and lam[:, 0].sum() / orc.params["dt"] > 0.2 * weight(model, g=orc.params["gravity"]):
            return om, orc, float(z)
    raise AssertionError("no start height touches the floor")


def settle_wrench(om, orc):
    """The oracle's reset: the un-actuated settle substep from the start pose; COMs at the start pose."""
    nj = NB - 1
    pre = np.zeros(13 + 2 * nj)
    pre[:3] = om["base_start_pos"]
    pre[3:7] = om["base_start_quat"]
    pre[13:13 + nj] = om["q_start"][om["obs_order"]]
    s = orc.new_state()
    orc.set_state(s, pre)
    pos, rot = orc.body_poses(s)
    com = pos + np.einsum("bij,bj->bi", rot, om["com"])
    orc.reset(s)
    body, lam, pt, _ = orc.contacts(s)
    W = np.zeros((NB, 6))
    for b, l, p in zip(body, lam, pt):
        f = np.array([l[1], l[2], l[0]])
        W[b, :3] += f
        W[b, 3:] += np.cross(p - com[b], f)
    return W / orc.params["dt"]


def test_reset_reports_the_settle_substep(capi, model, oracle64):
    """With a start pose low enough that the settle substep touches the floor: the reset launch and the episode-limit
    reset inside a step launch both report that substep (oracle, 5e-3 M g and M g x 1 m), a masked reset leaves the other
    envs' values bitwise alone."""
    om, orc, z = lowered_start(model)
    want = settle_wrench(om, orc)
    Mg = weight(model)
    assert want[:, 2].sum() > 0.2 * Mg
    m = capi.Model(ASSET_URDF)
    m.set_start_pose((0.0, 0.0, z), (0.0, 0.0, 0.0))
    n = 6
    b = capi.Batch(m, n, 0)
    b.set_contact_sensor(True)
    obs = torch.zeros(n, 3 * J, device=DEV)
    b.reset(obs)
    got = b.contact_wrench().cpu().numpy()
    for k in range(n):
        assert np.abs(got[k] - want).max() <= 5e-3 * Mg, k
    # a few steps, then a masked reset of env 2: the others keep their values
    a = torch.tensor(np.tile(model["q_start"][model["obs_order"]], (n, 1)), dtype=torch.float32, device=DEV)
    rew, done = torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    for _ in range(3):
        b.step(a, obs, rew, done)
    before = b.contact_wrench().clone()
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[2] = 1
    b.reset(obs, mask)
    after = b.contact_wrench()
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(before[keep], after[keep]) and not torch.equal(before[2], after[2])
    assert np.abs(after[2].cpu().numpy() - want).max() <= 5e-3 * Mg
    # the episode limit: env 4 ends its episode with the next step and reports the settle substep
    b.set_episode_limit(10, torch.tensor([0, 0, 0, 0, 9, 0], dtype=torch.int32, device=DEV))
    b.step(a, obs, rew, done)
    assert done.tolist() == [0, 0, 0, 0, 1, 0]
    w = b.contact_wrench()
    assert np.abs(w[4].cpu().numpy() - want).max() <= 5e-3 * Mg
    assert torch.equal(w[4], after[2]) or np.abs((w[4] - after[2]).cpu().numpy()).max() <= 1e-4 * Mg
    torch.cuda.synchronize()
    b.close()


def test_contained_env_reports_zeros(model):
    n = 6
    w = torch.zeros(n, NB, 6)
    w[3, 4, 1] = float("nan")
    v, ref = sensing(n), sensing(n)
    for x in (v, ref):
        x.reset_tensor()
    v.set_external_wrench(w)
    ref.set_external_wrench(torch.zeros(n, NB, 6))
    a = torch.tensor(np.tile(model["q_start"][model["obs_order"]], (n, 1)), dtype=torch.float32, device=DEV)
    for _ in range(60):
        _, _, d = v.step_tensor(a)
        ref.step_tensor(a)
    assert d.tolist() == [False, False, False, True, False, False]
    cw, rw = v.contact_wrench(), ref.contact_wrench()
    assert (cw[3] == 0).all()
    keep = [0, 1, 2, 4, 5]
    assert torch.equal(cw[keep], rw[keep]) and (rw[keep, :, 2] > 0).any()


# ---------------------------------------------------------------- 5. refusals, Python surface
def test_refusals(capi):
    n = 16
    b = capi.Batch(capi.Model(ASSET_URDF), n, 0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = torch.zeros(n, NB, 6, device=DEV)
    gp = C.c_void_p(good.data_ptr())
    assert capi.lib.trex_batch_contact_wrench(b.h, gp, s) == capi.E_INVALID           # never enabled
    b.set_contact_sensor(True)
    assert capi.lib.trex_batch_contact_wrench(b.h, gp, s) == 0
    host = np.zeros(n * NB * 6, np.float32)
    assert capi.lib.trex_batch_contact_wrench(b.h, C.c_void_p(host.ctypes.data), s) == capi.E_INVALID
    hip = C.CDLL("libamdhip64.so")
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(4 * n * NB * 6 - 4)) == 0
    try:
        assert capi.lib.trex_batch_contact_wrench(b.h, p, s) == capi.E_INVALID        # one float short
    finally:
        torch.cuda.synchronize()
        hip.hipFree(p)
    with pytest.raises(capi.TrexError):
        b.contact_wrench(torch.zeros(n, NB, 6))                                          # host tensor
    a, obs, dbg = torch.zeros(n, J, device=DEV), torch.zeros(n, 3 * J, device=DEV), torch.zeros(4096, device=DEV)
    b.reset()
    with pytest.raises(capi.TrexError) as ei:
        b.debug_step(a, obs, dbg)
    assert ei.value.code == capi.E_INVALID
    assert (b.contact_wrench() == b.contact_wrench()).all()
    b.set_contact_sensor(False)
    assert capi.lib.trex_batch_contact_wrench(b.h, gp, s) == capi.E_INVALID           # off again
    b.debug_step(a, obs, dbg)
    torch.cuda.synchronize()
    b.close()


def test_python_surface(model):
    from trex_gym.trex_env import TrexBulletEnv
    v = sensing(4)
    assert (v.contact_wrench() == 0).all()
    v.reset()
    a = np.tile(model["q_start"][model["obs_order"]].astype(np.float32), (4, 1))
    for _ in range(200):
        v.step(a)
    names = [name for name, _ in v.model.links()]
    w = v.contact_wrench()
    flags = v.in_contact()
    assert flags.shape == (4, NB) and flags.dtype == torch.bool and flags.device == w.device
    touching = flags[0].nonzero().flatten().tolist()
    assert touching
    body_of = v.model.array("link_body").astype(int)
    feet = [[names[i] for i in range(len(names)) if body_of[i] == b] for b in touching]
    f = v.contact_forces(feet)
    assert f.shape == (4, len(touching), 3)
    assert torch.allclose(f.sum(1), w[:, :, :3].sum(1), rtol=1e-5, atol=1e-2)
    e = TrexBulletEnv(urdf_path=ASSET_URDF, contact_sensor=True)
    for _ in range(200):
        e.step(a[0])
    cw = e.contact_wrench()
    assert cw.shape == (NB, 6) and cw[:, 2].sum() > 0
