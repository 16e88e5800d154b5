"""The actuator model on the GPU: per-joint control modes, per-env motor gains, stiffness actions
(trex_batch_set_control_mode / _set_motor_gains / _set_stiffness_actions, include/trex_batch.h)."""
import numpy as np
import pytest
import torch

from conftest import ASSET_URDF
from gpu_support import DEV, contact_counts, make_vec, random_actions
from parity_helpers import GOLD, assert_step_close
from state_sets import landing_states

pytestmark = pytest.mark.gpu
NB, J = 26, 25
KP0, KD0, F0 = 5e-3, 0.1, 3e5


def rollout(v, acts, keep_state=True):
    """the rows of every step of `acts` [S, n, A] from a reset, and the final state"""
    v.reset()
    rows = []
    for a in acts:
        v.step_tensor(a)
        rows.append(v.rows.clone())
    st = torch.zeros(v.num_envs, v.batch.state_width, device=DEV)
    v.batch.get_state(st)
    return torch.stack(rows), st


def mixed_modes():
    return ["velocity" if k % 5 == 1 else ("torque" if k % 5 == 3 else "position") for k in range(J)]


def mixed_actions(n, steps, model, gen, modes):
    a = torch.stack([random_actions(model, n, gen) for _ in range(steps)])
    m = torch.tensor([{"position": 0, "velocity": 1, "torque": 2}[x] for x in modes], device=DEV)
    vel = 4.0 * (torch.rand(steps, n, J, generator=gen, device=DEV) - 0.5)
    tor = 400.0 * (torch.rand(steps, n, J, generator=gen, device=DEV) - 0.5)
    return torch.where(m == 1, vel, torch.where(m == 2, tor, a)).contiguous()


# ---------------------------------------------------------------- gains against the oracle
def test_uniform_gains_per_env_match_the_oracle_with_those_parameters(oracle64, model):
    """kp / kd / max_force uniform over the joints of an env, a different triple per env in one batch, the full 5 substeps,
    from landing and crouch states: each env against Oracle(params = its triple) within assert_step_close, contact counts equal."""
    from oracle import oracle as O
    ls, la = landing_states(oracle64, model)
    states = np.concatenate([ls, GOLD["crouch_state"][30:36].astype(np.float32)])
    acts = np.concatenate([la, GOLD["crouch_actions"][:6].astype(np.float32)])
    n = len(states)
    rng = np.random.default_rng(11)
    kp = (KP0 * rng.uniform(0.2, 5.0, n)).astype(np.float32)
    kd = (KD0 * rng.uniform(0.2, 3.0, n)).astype(np.float32)
    # before the GPU sees anything, on the CPU: a state stays only if the f32 ORACLE with the env's gains passes the same
    # comparison against the f64 one (a state where f32 arithmetic itself decides a contact or a saturation proves nothing)
    keep = []
    for e in range(n):
        prm = {"motor_kp": float(kp[e]), "motor_kd": float(kd[e])}
        res = []
        for prec in ("f64", "f32"):
            orc = O.Oracle(model, params=prm, precision=prec)
            s = orc.new_state()
            orc.set_state(s, states[e].astype(np.float64))
            o, r, _ = orc.step(s, acts[e].astype(np.float64))
            res.append((o, r, len(orc.contacts(s)[0])))
        try:
            assert_step_close(res[1][0].astype(np.float32), res[0][0], res[1][1], res[0][1])
            ok = res[0][2] == res[1][2]
        except AssertionError:
            ok = False
        if ok:
            keep.append(e)
    print("gains against the oracle: %d of %d states kept after the f32-oracle check" % (len(keep), n))
    assert len(keep) >= 2 * n // 3
    states, acts, kp, kd = states[keep], acts[keep], kp[keep], kd[keep]
    n = len(keep)
    v = make_vec(n)
    v.reset()
    v.set_motor_gains(kp=np.repeat(kp[:, None], J, 1), kd=np.repeat(kd[:, None], J, 1))
    v.set_state(torch.tensor(states))
    obs, rew, _, _ = v.step(acts)
    cnt = contact_counts(v).cpu().numpy()
    changed = 0
    for e in range(n):
        orc = O.Oracle(model, params={"motor_kp": float(kp[e]), "motor_kd": float(kd[e])})
        s = orc.new_state()
        orc.set_state(s, states[e].astype(np.float64))
        o, r, _ = orc.step(s, acts[e].astype(np.float64))
        assert_step_close(obs[e], o, rew[e], r, "env %d kp %g kd %g" % (e, kp[e], kd[e]))
        assert cnt[e] == len(orc.contacts(s)[0]), e
        s0 = oracle64.new_state()
        oracle64.set_state(s0, states[e].astype(np.float64))
        o0, _, _ = oracle64.step(s0, acts[e].astype(np.float64))
        changed += np.abs(o0 - o).max() > 1e-3
    assert changed >= n // 2          # the gains really change the step


def test_max_force_bounds_the_reported_torque():
    """|tau_obs_j| <= F_j everywhere; joints driven far from their target report exactly +- F_j; F_j = 0 reports 0."""
    n = 8
    v = make_vec(n)
    rng = np.random.default_rng(2)
    F = rng.uniform(5.0, 50.0, (n, J)).astype(np.float32)
    F[:, 3] = 0.0
    v.reset()
    v.set_motor_gains(max_force=F)
    lo, hi = v.model.lower.astype(np.float32), v.model.upper.astype(np.float32)
    a = np.where(rng.random((n, J)) < 0.5, lo, hi).astype(np.float32)      # targets at the stops: far from the start pose
    dt, kp = v.model.get_param("dt"), v.model.get_param("motor_kp")
    first = None
    for _ in range(3):
        obs, _, _, _ = v.step(a)
        tau = obs[:, 2 * J:]
        assert (np.abs(tau) <= F * (1 + 1e-6)).all()
        assert (tau[:, 3] == 0).all()
        first = obs if first is None else first
    # a motor row that is NOT at its bound is satisfied: the joint moves at the velocity the motor asks for, kp (a - q) / dt plus
    # what is left of its rate. A joint far from its target that moves at less than half of kp |a - q| / dt is therefore at the bound.
    obs = first
    tau, err = obs[:, 2 * J:], a - obs[:, :J]
    far = (np.abs(err) > 0.2) & (np.abs(obs[:, J:2 * J]) < 0.5 * kp * np.abs(err) / dt)
    far[:, 3] = False
    print("max_force: %d of %d joints far from following their motor" % (far.sum(), far.size))
    assert far.sum() > n * J // 4
    np.testing.assert_allclose(np.abs(tau[far]), F[far], rtol=2e-6)     # (F dt) (1 / dt): two roundings
    assert (np.sign(tau[far]) == np.sign(err[far])).all()


# ---------------------------------------------------------------- torque mode
def free_flight_state(oracle64):
    s = oracle64.new_state()
    oracle64.reset(s)
    st = oracle64.get_state(s)
    st[2] += 3.0                      # well above the floor: no contact within a step
    return st


def test_torque_mode_free_flight_is_forward_dynamics(oracle64, oracle32, model):
    """substeps = 1, link_damping = 0, no joint at a stop, no contact: velocities after the step = v + a dt with a from
    forward_dynamics(s, tau, with_damping=True); random tau on all joints and one joint at a time. Tolerance: 3 x the f32
    oracle's own deviation from the f64 one on the same cases, floored at 1e-5 relative to the largest velocity change so that
    an exact f32 oracle does not ask for the impossible; the same rule for the base twist (v, w). Measured (profiles/r10_actuators.txt), relative to the largest velocity
    change of the case: joints f32 oracle 2.0e-5 .. 4.6e-4, the kernel 2.7e-8 .. 1.3e-6; base f32 oracle 2.8e-7 .. 7.7e-6,
    the kernel 2.9e-7 .. 6.1e-7."""
    from oracle import oracle as O
    prm = {"substeps": 1, "link_damping": 0.0}
    o64, o32 = O.Oracle(model, params=prm), O.Oracle(model, params=prm, precision="f32")
    dt = o64.params["dt"]
    rng = np.random.default_rng(4)
    st = free_flight_state(o64)
    st[13 + J:] = rng.normal(size=J) * 0.3       # joint rates
    st[7:13] = rng.normal(size=6) * 0.2
    taus = [rng.uniform(-200, 200, J)] + [np.eye(J)[k] * 150.0 for k in (0, 7, 19)] + [np.zeros(J)]
    n = len(taus)
    v = make_vec(n, params=prm, control_mode="torque")
    v.reset()
    v.set_state(torch.tensor(np.tile(st.astype(np.float32), (n, 1))))
    obs, _, _, _ = v.step(np.array(taus, np.float32))
    got = torch.zeros(n, 13 + 2 * J, device=DEV)
    v.batch.get_state(got)
    got = got.cpu().numpy().astype(np.float64)
    worst_gpu = worst_f32 = 0.0
    for e, tau in enumerate(taus):
        def expect(orc):
            s = orc.new_state()
            orc.set_state(s, st.astype(np.float32).astype(np.float64))
            qdd, ba = orc.forward_dynamics(s, tau, with_damping=True)
            return qdd * dt, ba * dt
        dq64, db64 = expect(o64)
        dq32, db32 = expect(o32)
        s = o64.new_state()
        o64.set_state(s, st.astype(np.float32).astype(np.float64))
        base = o64.get_state(s)
        scale = max(np.abs(dq64).max(), 1e-3)
        f32_dev = np.abs(dq32 - dq64).max() / scale
        gpu_dev = np.abs((got[e, 13 + J:] - base[13 + J:]) - dq64).max() / scale
        worst_gpu, worst_f32 = max(worst_gpu, gpu_dev), max(worst_f32, f32_dev)
        # the base twist: state words 7..9 = v, 10..12 = w; forward_dynamics returns (dw, dv), world axes
        want_b = np.concatenate([db64[3:], db64[:3]])
        f32_b = np.concatenate([db32[3:], db32[:3]])
        bscale = max(np.abs(want_b).max(), 1e-3)
        gpu_bdev = np.abs((got[e, 7:13] - base[7:13]) - want_b).max() / bscale
        f32_bdev = np.abs(f32_b - want_b).max() / bscale
        print("torque free flight case %d base: gpu %.3e f32 oracle %.3e (relative to %.3e)" % (e, gpu_bdev, f32_bdev, bscale))
        assert gpu_bdev <= max(3 * f32_bdev, 1e-5 + 3 * np.finfo(np.float32).eps * np.abs(base[7:13]).max() / bscale), e
        print("torque free flight case %d: gpu %.3e f32 oracle %.3e (relative to %.3e rad/s)" % (e, gpu_dev, f32_dev, scale))
        assert gpu_dev <= max(3 * f32_dev, 1e-5 + 3 * np.finfo(np.float32).eps * np.abs(base[13 + J:]).max() / scale), e
        np.testing.assert_allclose(obs[e, 2 * J:], tau, rtol=1e-6, atol=0)       # the torque column: the command
    # joint torques are internal: with the positions held at the common start state, the total linear and angular momentum of the
    # new velocities (Oracle.energy) is that of the step with tau = 0. (At the NEW positions it is not: they differ by qd dt between
    # the cases, a first-order term of the integrator, not of the torques.) Bound: every one of the 26 bodies' terms is a product of
    # f32-stored velocities, relative error 2^-23 each after the kernel's own rounding, on the scale of the total: 3 x 26 x 2^-23.
    mom = []
    for e in range(n):
        s = o64.new_state()
        mixed = st.astype(np.float32).astype(np.float64)
        mixed[7:13] = got[e, 7:13]
        mixed[13 + J:] = got[e, 13 + J:]
        o64.set_state(s, mixed)
        mom.append(o64.energy(s)["momentum"])
    mom = np.array(mom)
    mscale = max(np.abs(mom[-1]).max(), 1.0)
    print("torque free flight: momentum deviation %.3e on a scale of %.3e" % (np.abs(mom[:-1] - mom[-1]).max(), mscale))
    assert np.abs(mom[:-1] - mom[-1]).max() <= 3 * 26 * 2.0 ** -23 * mscale, np.abs(mom[:-1] - mom[-1]).max()


def test_torque_is_clipped_to_max_force_and_reported():
    n = 4
    v = make_vec(n, control_mode="torque")
    v.reset()
    F = np.full((n, J), 20.0, np.float32)
    v.set_motor_gains(max_force=F)
    a = np.linspace(-60, 60, n * J, dtype=np.float32).reshape(n, J)
    obs, _, _, _ = v.step(a)
    np.testing.assert_array_equal(obs[:, 2 * J:], np.clip(a, -20.0, 20.0))
    assert v.action_space.shape == (J,)


# ---------------------------------------------------------------- stiffness actions
def test_stiffness_actions_equal_the_same_gains_bitwise(model):
    """[a, kp] rows == set_motor_gains(kp, sqrt(2 kp)) with J-wide actions, bitwise (both reach the row set-up as the same two
    f32 numbers: the action decode forms sqrt(2 kp) with the correctly rounded f32 square root, as torch does). With
    kp = 5e-3 everywhere: close to the default step, not bitwise - sqrt(2 * 5e-3f) in f32 is not the f32 of 0.1."""
    n, steps = 64, 12
    gen = torch.Generator(device=DEV).manual_seed(7)
    acts = torch.stack([random_actions(model, n, gen) for _ in range(steps)])
    kp = (KP0 * (0.2 + 4.8 * torch.rand(n, J, generator=gen, device=DEV))).contiguous()
    vs = make_vec(n, variable_stiffness=True, kp_max=1.0)
    assert vs.action_space.shape == (2 * J,)
    rs, ss = rollout(vs, torch.cat([acts, kp.expand(steps, n, J)], dim=2).contiguous())
    vg = make_vec(n)
    vg.reset()
    vg.set_motor_gains(kp=kp, kd=torch.sqrt(2.0 * kp))
    rg, sg = rollout(vg, acts)
    assert torch.equal(rs, rg) and torch.equal(ss, sg)
    rs2, _ = rollout(vs, torch.cat([acts, torch.full((steps, n, J), KP0, device=DEV)], dim=2).contiguous())
    vd = make_vec(n)
    rd, _ = rollout(vd, acts)
    # (the first step, within the parity suite's one-step tolerances: kd differs from the model's 0.1 in its last bit)
    q2, qd2, q0, qd0 = rs2[0, :, :J], rs2[0, :, J:2 * J], rd[0, :, :J], rd[0, :, J:2 * J]
    assert (q2 - q0).abs().max() <= 1e-4 and (qd2 - qd0).abs().max() <= 3e-3 * max(1.0, float(qd0.abs().max()))
    with pytest.raises(ValueError):
        vs.step_tensor(acts[0])          # J-wide actions are refused while stiffness actions are on


# ---------------------------------------------------------------- identities, bitwise
@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("params", [None, {"warmstart": 0.8}])
def test_gains_set_to_the_model_parameters_are_the_default_step(n, params, model):
    gen = torch.Generator(device=DEV).manual_seed(1)
    acts = torch.stack([random_actions(model, n, gen) for _ in range(40)])
    vd = make_vec(n, params=params, max_episode_steps=25)
    rd, sd = rollout(vd, acts)
    va = make_vec(n, params=params, max_episode_steps=25)
    va.reset()
    va.set_motor_gains(kp=KP0, kd=KD0, max_force=F0)
    ra, sa = rollout(va, acts)
    assert torch.equal(rd, ra) and torch.equal(sd, sa)
    assert torch.equal(contact_counts(vd), contact_counts(va))
    va.set_motor_gains()                 # cleared: the default kernels again
    rc, sc = rollout(va, acts)
    assert torch.equal(rd, rc) and torch.equal(sd, sc)


@pytest.mark.parametrize("n", [2, 64, 2500, 4096])
@pytest.mark.parametrize("params", [None, {"warmstart": 0.8}])
@pytest.mark.parametrize("extras", [False, True])
def test_launch_forms_agree_for_mixed_modes_and_random_gains(n, params, extras, model):
    """pair (even n) == single (odd n, the same envs first) == step_many, for a mixed-mode batch with randomised gains,
    with and without warm start, wrench and sensor, through landing and episode ends."""
    steps = 30 if n <= 64 else 24
    modes = mixed_modes()
    gen = torch.Generator(device=DEV).manual_seed(3)
    acts = mixed_actions(n + 1, steps, model, gen, modes)
    kp = KP0 * (0.2 + 4.8 * torch.rand(n + 1, J, generator=gen, device=DEV))
    kd = KD0 * (0.2 + 2.8 * torch.rand(n + 1, J, generator=gen, device=DEV))
    w = torch.zeros(n + 1, NB, 6, device=DEV)
    w[:, 0, 0] = 30.0

    def make(m):
        v = make_vec(m, params=params, control_mode=modes, max_episode_steps=20)
        v.reset()
        v.set_motor_gains(kp=kp[:m], kd=kd[:m])
        if extras:
            v.set_external_wrench(w[:m].contiguous())
            v.batch.set_contact_sensor(True)
        return v
    vp, vs, vm = make(n), make(n + 1), make(n)
    rp, sp = rollout(vp, acts[:, :n].contiguous())
    rs, ss = rollout(vs, acts)
    assert torch.equal(rp, rs[:, :n]) and torch.equal(sp, ss[:n])
    vm.reset()
    rm = vm.step_many_tensor(acts[:, :n].contiguous())
    assert torch.equal(rm, rp)
    if extras:
        assert torch.equal(vp.batch.contact_wrench(), vs.batch.contact_wrench()[:n])
    assert torch.isfinite(rp).all() and (rp[:, :, 3 * J + 1] != 0).any()      # episode ends happened


def test_settle_substep_ignores_modes_and_gains(model):
    """a reset's first observation does not depend on modes or gains; neither does the episode-limit reset inside a launch."""
    n = 16
    vd = make_vec(n)
    o0 = vd.reset_tensor().clone()
    va = make_vec(n, control_mode=mixed_modes(), max_episode_steps=3)
    va.set_motor_gains(kp=3 * KP0, max_force=50.0)
    assert torch.equal(va.reset_tensor(), o0)
    gen = torch.Generator(device=DEV).manual_seed(5)
    acts = mixed_actions(n, 3, model, gen, mixed_modes())
    for a in acts:
        obs, _, done = va.step_tensor(a)
    assert done.all() and torch.equal(obs, o0)


# ---------------------------------------------------------------- refusals and containment
def test_refusals():
    from trex_gym import _capi
    n = 4
    v = make_vec(n)
    v.reset()
    b = v.batch
    with pytest.raises(_capi.TrexError):
        b.set_control_mode([0] * (J - 1) + [3])
    with pytest.raises(_capi.TrexError):
        b.set_control_mode([-1] + [0] * (J - 1))
    with pytest.raises(_capi.TrexError):
        b.set_motor_gains(kp=torch.zeros(n, J))                        # host memory
    with pytest.raises(_capi.TrexError):
        b.set_motor_gains(kd=torch.zeros(n, J - 1, device=DEV))         # short
    for name in ("kp", "kd", "max_force"):
        with pytest.raises(_capi.TrexError):
            b.set_motor_gains(**{name: torch.zeros(n, J)})                              # host memory
        with pytest.raises(_capi.TrexError):
            b.set_motor_gains(**{name: torch.zeros(n * J - 1, device=DEV)})             # short (through the C call: no shape check)
        if torch.cuda.device_count() > 1:
            with pytest.raises(_capi.TrexError):
                b.set_motor_gains(**{name: torch.zeros(n, J, device="cuda:1")})         # another device's memory
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(_capi.TrexError):
            b.set_stiffness_actions(True, bad)
    dbg, obs, a = torch.zeros(4096, device=DEV), torch.zeros(n, 3 * J, device=DEV), torch.zeros(n, J, device=DEV)
    b.debug_step(a, obs, dbg)                                           # allowed while nothing is active
    b.set_control_mode(["velocity"] + ["position"] * (J - 1))
    with pytest.raises(_capi.TrexError):
        b.debug_step(a, obs, dbg)
    b.set_control_mode(None)
    b.set_motor_gains(kp=torch.full((n, J), KP0, device=DEV))
    with pytest.raises(_capi.TrexError):
        b.debug_step(a, obs, dbg)
    b.set_motor_gains()
    b.debug_step(a, obs, dbg)
    b.set_stiffness_actions(True, 1.0)
    with pytest.raises(_capi.TrexError):
        b.step(a, obs, torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV))   # J-wide buffer: short


@pytest.mark.parametrize("what", ["gain", "inf_force", "torque"])
def test_a_non_finite_gain_or_torque_ends_only_its_env(what, model):
    n = 8
    gen = torch.Generator(device=DEV).manual_seed(9)
    modes = ["torque" if k == 4 else "position" for k in range(J)]
    acts = mixed_actions(n, 3, model, gen, modes)
    ref = make_vec(n, control_mode=modes)
    rr, _ = rollout(ref, acts)
    v = make_vec(n, control_mode=modes)
    if what == "gain":
        kp = torch.full((n, J), KP0, device=DEV)
        kp[5, 7] = float("nan")
        v.reset()
        v.set_motor_gains(kp=kp)
    elif what == "inf_force":
        F = torch.full((n, J), F0, device=DEV)
        F[5, 2] = float("inf")
        v.reset()
        v.set_motor_gains(max_force=F)
    else:
        acts = acts.clone()
        acts[:, 5, 4] = float("nan")
    rb, _ = rollout(v, acts)
    others = [e for e in range(n) if e != 5]
    assert torch.equal(rb[:, others], rr[:, others])
    assert (rb[:, 5, 3 * J + 1] == 1).all() and (rb[:, 5, 3 * J] == 0).all() and torch.isfinite(rb).all()


# ---------------------------------------------------------------- Python surface
def test_action_spaces_and_named_modes():
    v = make_vec(2, control_mode={"joint_cranium": "torque", "joint_atlas_axis": "velocity"})
    k_t, k_v = v.model.joint_names.index("joint_cranium"), v.model.joint_names.index("joint_atlas_axis")
    assert v.control_modes[k_t] == 2 and v.control_modes[k_v] == 1 and sum(v.control_modes) == 3
    assert v.action_space.high[k_t] == np.float32(3e5) and v.action_space.low[k_v] == -100.0
    others = [k for k in range(J) if k not in (k_t, k_v)]
    np.testing.assert_array_equal(v.action_space.low[others], v.model.lower.astype(np.float32)[others])
    with pytest.raises(KeyError):
        make_vec(2, control_mode={"no_such_joint": "torque"})
    with pytest.raises(ValueError):
        v.step(np.zeros((2, 2 * J), np.float32))


# ---------------------------------------------------------------- per-joint rows against the oracle's restated targets
def restated_cases(model, oracle64):
    """landing + crouch + joint-limit states (one stop, several stops), with actions"""
    import joint_limit_states as jl
    ls, la = landing_states(oracle64, model)
    s1, a1 = jl.one_stop_states(model, oracle64)
    s2, a2, _ = jl.several_stop_states(model, oracle64)
    states = np.concatenate([ls, GOLD["crouch_state"][30:36].astype(np.float32), s1[::4], s2[::3]])
    acts = np.concatenate([la, GOLD["crouch_actions"][:6].astype(np.float32), a1[::4], a2[::3]])
    return states, acts


def test_per_joint_gains_and_mixed_position_velocity_rows_match_the_restated_oracle(model):
    """substeps = 1, link_damping = 0. A row (t_j, vt_j, kp_j, kd_j) is the oracle's row (kp0, kd0) with the raw target
    t'_j = q_j + (dt / kp0) [kp_j (t_j - q_j) / dt + kd_j (vt_j - nqd_j) + kd0 nqd_j], nqd the oracle's own unconstrained rate
    (forward_dynamics with damping, clamped). Random per-joint kp (0.2 - 5 x default) and kd, POSITION joints (vt = 0, t clipped
    to the limits) and VELOCITY joints (kp = 0, vt clipped to +- max_coordinate_velocity, some commands beyond it), on landing,
    crouch and joint-limit states; contact counts equal; assert_step_close with its tolerances. On the CPU, before the GPU sees
    anything, a state stays only if the f32 oracle fed the same restated targets passes against the f64 one; a state that then
    misses may be judged by 3 x the f32 oracle's deviation on that case, for at most 1 state in 16, counted and printed."""
    from oracle import oracle as O
    import joint_limit_states as jl
    prm = {"substeps": 1, "link_damping": 0.0}
    o64, o32 = O.Oracle(model, params=prm), O.Oracle(model, params=prm, precision="f32")
    dt, vmax = o64.params["dt"], o64.params["max_coordinate_velocity"]
    lo, hi = jl.limits(model)
    states, acts = restated_cases(model, O.Oracle(model))
    n0 = len(states)
    rng = np.random.default_rng(21)
    velj = rng.random((n0, J)) < 0.4                                   # VELOCITY joints, a different set per case
    kp = (KP0 * rng.uniform(0.2, 5.0, (n0, J))).astype(np.float32)
    kd = (KD0 * rng.uniform(0.2, 3.0, (n0, J))).astype(np.float32)
    cmd = np.where(velj, rng.uniform(-3.0, 3.0, (n0, J)), acts).astype(np.float32)
    cmd[velj & (rng.random((n0, J)) < 0.05)] = 150.0                   # beyond the velocity clip
    oo = np.asarray(model["obs_order"])

    def restated(orc, e):
        s = orc.new_state()
        orc.set_state(s, states[e].astype(np.float64))
        orc.set_motors_on(s, True)
        st = orc.get_state(s)
        q, qd = st[13:13 + J], st[13 + J:]
        qdd, _ = orc.forward_dynamics(s, None, with_damping=True)
        nqd = np.clip(qd + qdd * dt, -vmax, vmax)
        c = cmd[e].astype(np.float64)
        t = np.where(velj[e], q, np.clip(c, lo, hi))
        vt = np.where(velj[e], np.clip(c, -vmax, vmax), 0.0)
        kpe = np.where(velj[e], 0.0, kp[e].astype(np.float64))
        kde = kd[e].astype(np.float64)
        tp = q + (dt / KP0) * (kpe * (t - q) / dt + kde * (vt - nqd) + KD0 * nqd)
        orc.substep(s, tp)
        r, _ = orc.reward(s)
        return orc.observe(s), r, len(orc.contacts(s)[0])
    # (forward_dynamics returns the joint accelerations in observation order, like the states: checked below on one case)
    ref64, ref32, keep = [], [], []
    for e in range(n0):
        a, b = restated(o64, e), restated(o32, e)
        ref64.append(a); ref32.append(b)
        try:
            assert_step_close(b[0].astype(np.float32), a[0], b[1], a[1])
            if a[2] == b[2]:
                keep.append(e)
        except AssertionError:
            pass
    print("restated rows: %d of %d states kept after the f32-oracle check" % (len(keep), n0))
    assert len(keep) >= 2 * n0 // 3
    n = len(keep)
    # the modes are batch-wide: one batch per distinct mode set would be n batches; instead every case runs in its own
    # 2-env batch (the pair form) with its mode set
    fallback = 0
    for e in keep:
        v = make_vec(2, params=prm, control_mode=[1 if x else 0 for x in velj[e]])
        v.reset()
        v.set_motor_gains(kp=kp[e], kd=kd[e])
        v.set_state(torch.tensor(np.tile(states[e], (2, 1))))
        obs, rew, _, _ = v.step(np.tile(cmd[e], (2, 1)))
        cnt = contact_counts(v).cpu().numpy()
        assert (obs[0] == obs[1]).all()
        o, r, c = ref64[e]
        assert cnt[0] == c, e
        try:
            assert_step_close(obs[0], o, rew[0], r, "case %d" % e)
        except AssertionError:
            f = jl.step_errors(ref32[e][0], o, ref32[e][1], r)
            g = jl.step_errors(obs[0].astype(np.float64), o, float(rew[0]), r)
            print("restated rows: case %d judged by 3 x the f32 oracle: gpu %s f32 %s" % (e, g, f))
            assert all(gk <= 3 * fk for gk, fk in zip(g, f)), (e, g, f)
            fallback += 1
        v.close()
    print("restated rows: %d of %d cases judged by the f32 oracle's deviation" % (fallback, n))
    assert fallback * 16 <= n


def test_uniform_max_force_per_env_matches_the_oracle(oracle64, model):
    """max_force uniform over the joints of an env, a different value per env (1e3 .. 3e5 N m: the motors saturate in the
    landing states), the full 5 substeps, against Oracle(params={"motor_max_force": F}); same CPU-side pruning as above."""
    from oracle import oracle as O
    ls, la = landing_states(oracle64, model)
    states = np.concatenate([ls, GOLD["crouch_state"][30:36].astype(np.float32)])
    acts = np.concatenate([la, GOLD["crouch_actions"][:6].astype(np.float32)])
    n0 = len(states)
    rng = np.random.default_rng(13)
    F = np.exp(rng.uniform(np.log(1e3), np.log(3e5), n0)).astype(np.float32)
    refs, keep = [], []
    for e in range(n0):
        res = []
        for prec in ("f64", "f32"):
            orc = O.Oracle(model, params={"motor_max_force": float(F[e])}, precision=prec)
            s = orc.new_state()
            orc.set_state(s, states[e].astype(np.float64))
            o, r, _ = orc.step(s, acts[e].astype(np.float64))
            res.append((o, r, len(orc.contacts(s)[0])))
        refs.append(res[0])
        try:
            assert_step_close(res[1][0].astype(np.float32), res[0][0], res[1][1], res[0][1])
            if res[0][2] == res[1][2]:
                keep.append(e)
        except AssertionError:
            pass
    print("max_force against the oracle: %d of %d states kept after the f32-oracle check" % (len(keep), n0))
    assert len(keep) >= 2 * n0 // 3
    v = make_vec(len(keep))
    v.reset()
    v.set_motor_gains(max_force=np.repeat(F[keep][:, None], J, 1))
    v.set_state(torch.tensor(states[keep]))
    obs, rew, _, _ = v.step(acts[keep])
    cnt = contact_counts(v).cpu().numpy()
    at_bound = 0
    for k, e in enumerate(keep):
        o, r, c = refs[e]
        assert_step_close(obs[k], o, rew[k], r, "env %d F %g" % (e, F[e]))
        assert cnt[k] == c, e
        assert (np.abs(obs[k, 2 * J:]) <= F[e] * (1 + 1e-6)).all()
        at_bound += int((np.abs(o[2 * J:]) >= 0.999 * F[e]).sum())
    assert at_bound > len(keep)      # the bound is active in these states


def test_zero_max_force_moves_like_the_oracle_without_motors(model):
    """F_j = 0 on every joint of an env: that env moves as the oracle with its motors off (substeps = 1: Oracle.substep with
    motors off), on landing, crouch and joint-limit states - a null row must not reach the limit row riding on it either -
    and reports torque 0."""
    from oracle import oracle as O
    prm = {"substeps": 1}
    o64, o32 = O.Oracle(model, params=prm), O.Oracle(model, params=prm, precision="f32")
    states, acts = restated_cases(model, O.Oracle(model))

    def off(orc, e):
        s = orc.new_state()
        orc.set_state(s, states[e].astype(np.float64))
        orc.set_motors_on(s, False)
        orc.substep(s, None)
        r, _ = orc.reward(s)
        return orc.observe(s), r, len(orc.contacts(s)[0]), orc.limit_rows(s)
    refs, keep = [], []
    for e in range(len(states)):
        a, b = off(o64, e), off(o32, e)
        refs.append(a)
        try:
            assert_step_close(b[0].astype(np.float32), a[0], b[1], a[1])
            if a[2] == b[2]:
                keep.append(e)
        except AssertionError:
            pass
    print("motors off: %d of %d states kept after the f32-oracle check" % (len(keep), len(states)))
    assert len(keep) >= 2 * len(states) // 3
    v = make_vec(len(keep), params=prm)
    v.reset()
    v.set_motor_gains(max_force=0.0)
    v.set_state(torch.tensor(states[keep]))
    obs, rew, _, _ = v.step(acts[keep])
    cnt = contact_counts(v).cpu().numpy()
    assert (obs[:, 2 * J:] == 0).all()
    with_limits = 0
    for k, e in enumerate(keep):
        o, r, c, lim = refs[e]
        assert np.abs(o[2 * J:]).max() == 0
        assert_step_close(obs[k], o, rew[k], r, "state %d" % e)
        assert cnt[k] == c, e
        with_limits += lim > 0
    assert with_limits > 10          # joints on their stops are among the cases


def test_torque_mode_in_contact_is_the_wrench_path(model, oracle64):
    """Contact states, substeps = 1: a torque tau on joint j is the couple + tau a_j on the child body and - tau a_j on the parent
    body (a_j the joint's world axis at the state), fed through the external wrench to an env without motors (max_force 0, which
    test_zero_max_force_moves_like_the_oracle_without_motors ties to the oracle). Within assert_step_close; the torque column is
    excluded (the torque env reports its command, the wrench env 0)."""
    prm = {"substeps": 1}
    ls, la = landing_states(oracle64, model)
    states = np.concatenate([ls, GOLD["crouch_state"][30:36].astype(np.float32)])
    n = len(states)
    rng = np.random.default_rng(17)
    tau = rng.uniform(-300, 300, (n, J)).astype(np.float32)
    tau[::3] = 0.0
    for e in range(0, n, 3):
        tau[e, rng.integers(J)] = 250.0           # one joint at a time
    oo = np.asarray(model["obs_order"])
    w = np.zeros((n, NB, 6), np.float32)
    for e in range(n):
        s = oracle64.new_state()
        oracle64.set_state(s, states[e].astype(np.float64))
        _, rot = oracle64.body_poses(s)
        for k in range(J):
            b = int(oo[k])
            a = rot[b] @ np.asarray(model["joint_axis"][b], float)
            w[e, b, 3:] += tau[e, k] * a
            w[e, int(model["parent"][b]), 3:] -= tau[e, k] * a
    vt = make_vec(n, params=prm, control_mode="torque")
    vt.reset()
    vt.set_state(torch.tensor(states))
    ot, rt, _, _ = vt.step(tau)
    vw = make_vec(n, params=prm)
    vw.reset()
    vw.set_motor_gains(max_force=0.0)
    vw.set_external_wrench(torch.tensor(w))
    vw.set_state(torch.tensor(states))
    ow, rw, _, _ = vw.step(np.zeros((n, J), np.float32))
    ct, cw = contact_counts(vt).cpu().numpy(), contact_counts(vw).cpu().numpy()
    assert (ct == cw).all() and (ct > 0).sum() > 10
    np.testing.assert_array_equal(ot[:, 2 * J:], tau)
    for e in range(n):
        a, b = ot[e].copy(), ow[e].astype(np.float64)
        a[2 * J:] = 0
        assert_step_close(a, b, what="state %d" % e)
    assert np.abs(ow - make_free(vw, states, n, prm)).max() > 1e-3      # the torques really change the step


def make_free(vw, states, n, prm):
    v0 = make_vec(n, params=prm)
    v0.reset()
    v0.set_motor_gains(max_force=0.0)
    v0.set_state(torch.tensor(states))
    o0, _, _, _ = v0.step(np.zeros((n, J), np.float32))
    return o0


# ---------------------------------------------------------------- the feature switched off is the code it was
@pytest.mark.parametrize("params", [None, {"warmstart": 0.8}])
def test_all_position_no_gains_is_the_default_step_at_4096_envs(params, model):
    """100 random-action steps of 4096 envs through landing with episode ends: modes set to all-POSITION, gains set and cleared,
    stiffness actions switched on and off again - then rows, state, contact stats and episode counts are bitwise those of a
    batch that never heard of actuators."""
    n, steps = 4096, 100
    gen = torch.Generator(device=DEV).manual_seed(6)
    vd = make_vec(n, params=params, max_episode_steps=40)
    va = make_vec(n, params=params, max_episode_steps=40)
    va.batch.set_control_mode(["velocity"] * J)
    va.batch.set_control_mode(["position"] * J)
    va.set_motor_gains(kp=2 * KP0)
    va.set_motor_gains()
    va.batch.set_stiffness_actions(True, 1.0)
    va.batch.set_stiffness_actions(False)
    assert va.A == J
    vd.reset(); va.reset()
    for t in range(steps):
        a = random_actions(model, n, gen)
        vd.step_tensor(a); va.step_tensor(a)
        if t % 10 == 9 or t == steps - 1:
            assert torch.equal(vd.rows, va.rows), t
    assert torch.equal(vd.get_state(), va.get_state())
    assert torch.equal(contact_counts(vd), contact_counts(va))
    assert torch.equal(vd.episode_steps, va.episode_steps)
    assert va.batch.launch_info() == vd.batch.launch_info()


def test_negative_gains_are_clamped_to_zero(model):
    n = 8
    gen = torch.Generator(device=DEV).manual_seed(12)
    acts = torch.stack([random_actions(model, n, gen) for _ in range(5)])
    neg, zero = make_vec(n), make_vec(n)
    neg.reset(); zero.reset()
    neg.set_motor_gains(kp=-1.0, kd=-0.5, max_force=-10.0)
    zero.set_motor_gains(kp=0.0, kd=0.0, max_force=0.0)
    rn, sn = rollout(neg, acts)
    rz, sz = rollout(zero, acts)
    assert torch.equal(rn, rz) and torch.equal(sn, sz) and torch.isfinite(rn).all()


def test_launch_info_of_a_warm_batch_with_actuators():
    v = make_vec(64, params={"warmstart": 0.8})
    pair = v.batch.launch_info()
    v.set_motor_gains(kp=KP0)
    single = v.batch.launch_info()
    assert pair["block"] == 128 and pair["grid"] == 32
    assert single["block"] == 64 and single["grid"] == 64 and single["lds_bytes"] < pair["lds_bytes"] // 2 + 64
    v.set_motor_gains()
    assert v.batch.launch_info() == pair


# ---------------------------------------------------------------- trainer, single env, RandomGains
def test_ppo_update_on_a_torque_mode_env():
    import math
    from trex_gym import trex_train
    env = trex_train.build_environment(4096, max_episode_steps=200, control_mode="torque", gain_scale=0.2)
    assert env.control_modes == [2] * J and env.gains is not None and env.action_space.shape == (J,)
    agent, hist = trex_train.train(env, num_timesteps=4096 * 32, seed=0, nsteps=32, noptepochs=1, log=lambda s: None)
    assert len(hist) == 1
    for h in hist:
        assert all(math.isfinite(x) for x in (h["policy_loss"], h["value_loss"], h["entropy"], h["mean_step_reward"]))
    assert torch.isfinite(agent.obs).all()
    with pytest.raises(ValueError):
        trex_train.build_environment(8, variable_stiffness=True)


def test_random_gains_are_redrawn_for_the_envs_that_reset():
    from trex_gym.perturb import RandomGains
    n = 16
    v = make_vec(n)
    v.gains = RandomGains(n, J, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    v.reset_tensor()
    s0 = v.gains.scale.clone()
    assert ((s0 >= 0.8) & (s0 <= 1.2)).all() and s0.std() > 0
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[3] = 1
    v.reset_tensor(mask)
    changed = (v.gains.scale != s0).any(0)
    assert changed[3] and changed.sum() == 1
    obs, _, _ = v.step_tensor(torch.zeros(n, J, device=DEV))
    assert torch.isfinite(obs).all() and not (obs == obs[0]).all()


def test_single_env_facade_takes_modes_and_stiffness():
    from trex_gym.trex_env import TrexBulletEnv
    e = TrexBulletEnv(urdf_path=ASSET_URDF, device=DEV, control_mode="torque")
    assert e.action_space.shape == (J,) and e.action_space.high[0] == np.float32(3e5)
    tau = np.linspace(-50, 50, J).astype(np.float32)
    obs, r, done, _ = e.step(tau)
    np.testing.assert_array_equal(np.asarray(obs[2 * J:], np.float32), tau)
    e2 = TrexBulletEnv(urdf_path=ASSET_URDF, device=DEV, variable_stiffness=True, kp_max=0.5)
    assert e2.action_space.shape == (2 * J,) and e2.action_space.high[-1] == np.float32(0.5)
    with pytest.raises(ValueError):
        e2.step(np.zeros(J, np.float32))
    obs, r, done, _ = e2.step(np.concatenate([np.zeros(J), np.full(J, KP0)]).astype(np.float32))
    assert np.isfinite(obs).all()
