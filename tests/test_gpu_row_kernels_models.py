"""The observation, reward and motion kernels (csrc/observation.hip, reward.hip, motion.hip) on the generated models of
tests/synthetic_models.py - deep_chain (J = 6), bushy (J = 25, nb = 26, six merged links), slab (J = 1) and mount_first, whose URDF
link 0 is welded behind a turned frame to a moving body at depth 2 - against the f64 references observation_ref, reward_ref and
motion_ref, with the checks of test_gpu_observations.py, test_gpu_rewards.py and test_gpu_motion.py themselves (their helpers take
the joint count). What the T-rex asset cannot reach: the base axes of a link outside the root, lanes and columns past a small J,
another obs_slot permutation, a step time and a floor height that are not the defaults.

Cases: tests/row_kernel_cases.py - N = 9 envs (one full 8-env workgroup and a ragged slot), landing and airborne states, every
kind of channel and term; tests/test_row_kernel_cases_host.py shows on the CPU that they reach their branches and that a kernel
with a wrong base body, joint order, Ts or floor_z would leave the references by 100 x the bounds applied here.

Tolerances: none of its own - tolerances.LINK_TOL as test_gpu_observations applies it, reward_ref.bound, motion_ref.sample_bound and
motion_ref.bound. The largest deviation as a fraction of its bound is printed per model and kernel (-s) and recorded in
profiles/r25_row_kernels_models.txt: measured on an MI355X, 0.61 at most (JOINT_ACC on mount_first), 0.32 for the observation
channels, 0.30 for a sampled column."""
import numpy as np
import pytest
import torch

import motion_ref as MR
import observation_ref as OR
import reward_ref as RR
import row_kernel_cases as RK
import test_gpu_motion as TM
import test_gpu_observations as TO
import test_gpu_rewards as TR
from gpu_support import DEV, guarded, guards_intact, make_vec, refused, same_bits
from state_sets import built_models
from tolerances import LINK_TOL

pytestmark = pytest.mark.gpu
N = RK.N


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return built_models(RK.MODELS, tmp_path_factory)


def env_of(m, n=N, other=False, **kw):
    """n envs of the generated model m under its own parameters (other: and RK.OTHER_PARAMS), the contact sensor on"""
    v = make_vec(n, urdf=m["path"], params=RK.params_of(m["props"], other), **kw)
    v.enable_contact_sensor(True)
    v.reset_tensor()
    return v


def case(m, name, other=False):
    params = RK.params_of(m["props"], other)
    st, act = RK.states(name, m["om"], params)
    return m["om"], m["om"]["nb"] - 1, params, st, act, RK.touch_link(name, m["om"], params)


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.array(x), dtype=dtype).to(DEV)             # (a copy: the cases are read-only arrays)


def fractions(name, kernel, worst):
    print("%s %s: largest deviation / bound  %s" % (name, kernel, "  ".join("%s %.3f" % (k, x) for k, x in worst.items())))


def reward_worst():
    return {TR.KIND_NAMES[k]: x for k, x in sorted(TR.WORST.items())}


def attach_clip(v, om, name, params):
    """the model's clip with its end effectors on the device -> (the reference's table, (links, points))"""
    frames, vel = RK.clip(om, RK.oracle_of(name, om, params))
    links, pts = RK.end_effectors(om)
    v.batch.set_link_probes(7, links, pts)
    assert TM.mapi(v).set_motion(frames, RK.DT, False, vel, 7) == RK.FRAMES
    assert TM.mapi(v).info() == dict(frames=RK.FRAMES, duration=(RK.FRAMES - 1) * RK.DT, terms=0, probes=len(links))
    return MR.device_table(MR.build_table(om, frames, vel, RK.DT, False)), (links, pts)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RK.MODELS)
def test_observations(name, built):
    """compose_rows after set_state and one step: pass-through and copied channels bitwise, computed ones within LINK_TOL; a
    padded stride and a guard row keep their NaN; the point channels agree with link_state(axes="base") within 2 x LINK_TOL"""
    om, J, params, st, act, touch = case(built[name], name)
    spec = RK.obs_spec(om, touch)
    v = env_of(built[name])
    E = v.batch.set_observation(spec)
    assert E == OR.extra_dim(spec, J) == v.batch.observation_dim() - 3 * J and v.rows.shape == (N, 3 * J + 2)
    v.set_state(dev(st))
    v.step_tensor(dev(act))
    a_in, ext = TO.inputs(N, seed=11, J=J)
    W = 3 * J + E + 2
    out = TO.compose(v, v.rows, a_in, ext, E, pad=5, guard_rows=1, J=J)
    assert out.shape == (N + 1, W + 5) and torch.isfinite(out[:N, :W]).all()
    assert torch.isnan(out[:N, W:]).all() and torch.isnan(out[N]).all()
    fz = v.contact_wrench()[:, :, 2]
    worst = TO.check_rows(om, spec, out[:N, :W], v.rows, v.get_state(), a_in, ext, fz, J=J, floor_z=params.get("floor_z", OR.FLOOR_Z))
    assert (fz[:, int(om["link_body"][touch])] > 0).any()                              # the CONTACT channel's body stands on the floor
    fractions(name, "observation", {k: x / LINK_TOL[k] for k, x in worst.items()})
    # the point channels against the link query of the same batch
    ln = RK.links_of(om)
    links = [0, ln["deepest"]] + ([ln["merged"]] if ln["merged"] is not None else []) + [touch]
    pts = np.array([[0.1, -0.2, 0.3], [0.05, 0.0, -0.02], [0.0, 0.0, 0.0], [0.25, 0.5, -0.125]], np.float32)[:len(links)]
    spec2 = [c for l, p in zip(links, pts) for c in ((OR.POINT_POS, l, tuple(p), 1.0), (OR.POINT_VEL, l, tuple(p), 1.0))]
    E2 = v.batch.set_observation(spec2)
    got = TO.compose(v, v.rows, None, None, E2, J=J)[:, 3 * J:3 * J + E2].reshape(N, len(links), 6).cpu().numpy().astype(np.float64)
    ls = v.link_state(v.link_probes(links, pts.astype(np.float64)), axes="base")
    pos, vel = ls.position.cpu().numpy().astype(np.float64), ls.linear_velocity.cpu().numpy().astype(np.float64)
    for e in range(N):
        assert np.abs(got[e, :, :3] - pos[e]).max() <= 2 * LINK_TOL["pose"] * max(1.0, np.abs(pos[e]).max()), e
        assert np.abs(got[e, :, 3:] - vel[e]).max() <= 2 * LINK_TOL["velocity"] * max(1.0, np.abs(vel[e]).max()), e
    v.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RK.MODELS)
def test_rewards(name, built):
    """three steps under actions outside the limits and random commands: every env and term within reward_ref.bound of the
    reference fed with the GPU's own rows and sensor forces; the column bitwise the ordered f32 sum; guards intact"""
    om, J, params, st, act, touch = case(built[name], name)
    spec = RK.reward_spec(om, touch)
    v = env_of(built[name])
    v.set_state(dev(st))
    Ts = TR.step_seconds(v)
    assert Ts == RR.step_seconds(params.get("dt", 0.002), params.get("substeps", 5))
    assert TR.api(v).set_reward(spec) == 32 == TR.api(v).reward_terms()
    hists = TR.histories(N, 32, J=J)
    TR.WORST.clear()
    tb = int(om["link_body"][touch])
    timers = limit = count = stood = 0
    for t in range(RK.WILD_STEPS):
        a, cmd = (dev(x) for x in RK.wild_inputs(N, J, t))
        v.step_tensor(a)
        rows = v.rows.clone()
        state, force = TR.instant(v)
        after, terms, ok = TR.compose(v, rows, a, cmd, 32)
        assert ok
        terms = TR.check(om, spec, rows, after, terms, state, force, hists, Ts, a, cmd, J=J)
        assert bool((terms[:, [RR.JOINT_ACC, RR.ACTION_RATE]] == 0).all()) == (t == 0)     # the rate terms: from the second step on
        stood += int((force[:, tb, 2] > RK.FORCE_MIN).sum())
        timers += sum(h["timer"][RR.FOOT_AIR_TIME] > 0 for h in hists)
        limit += int((terms[:, RR.JOINT_LIMIT] != 0).sum())
        count += int((terms[:, RR.CONTACT_COUNT] != 0).sum())
    assert (terms[:, RR.ACTION_RATE] != 0).all() and timers > 0 and limit > 0 and count > 0
    assert stood > 0                                                                    # FOOT_SLIP and the single-body count: in contact
    fractions(name, "reward", reward_worst())
    v.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RK.MODELS)
def test_motion(name, built):
    """motion_sample at knots, between them, at 0, T, beyond T and at a negative time, with the end effectors' points;
    compose_motion_reward twice on stepped states; motion_reset under an alternating mask: get_state() of the masked envs is
    bitwise what motion_sample gives - the obs_slot scatter -, the others and everything outside the row are untouched"""
    om, J, params, st, act, touch = case(built[name], name)
    v = env_of(built[name])
    v.set_state(dev(st))
    v.step_tensor(dev(act))
    tab, probes = attach_clip(v, om, name, params)
    K = len(probes[0])
    assert K == min(8, len(om["link_names"])) and probes[0][0] == 0
    TM.WORST.clear()
    times = RK.time_list(N, tab["duration"])
    state, points, phase = TM.sample(v, times, K, J=J)
    TM.check_sample(om, tab, probes, times, state, points, phase, J=J)
    # the terms, on the rows and the state of one instant; the clock moves on between the two calls
    spec = RK.motion_spec(om)
    assert TM.mapi(v).set_reward(spec, 0.5) == len(spec)
    clocks, helds = [MR.new_clock() for _ in range(N)], [np.zeros(len(spec)) for _ in range(N)]
    Ts = TM.step_seconds(v)
    rows = v.rows.clone()
    assert not bool((rows[:, 3 * J + 1] != 0).any())
    gstate = v.get_state().cpu().numpy().astype(np.float64)
    prev = None
    for step in range(2):
        after, terms, ok = TM.compose(v, rows, len(spec), pad=3 * step)
        assert ok
        prev = TM.check_compose(om, tab, probes, spec, 0.5, rows, after, terms, gstate, clocks, helds, Ts, prev, J=J)
    assert (np.abs(prev) > 1e-8).all()                                                  # no term has decayed to nothing
    # reference state initialisation
    mask = torch.zeros(N, dtype=torch.bool, device=DEV)
    mask[::2] = True
    before_state = v.get_state()
    whole, r = guarded((N, 3 * J + 2 + 3), fill=float("nan"))
    r[:, :3 * J + 2] = v.rows
    before_rows = r.clone()
    TM.mapi(v).reset(mask, dev(times), r)
    torch.cuda.synchronize()
    want = TM.sample(v, times, 0, J=J)[0]
    got = v.get_state()
    assert guards_intact(whole, (N, 3 * J + 5), fill=float("nan")) and bool(torch.isnan(r[:, 3 * J + 2:]).all())
    assert same_bits(got[mask], want[mask]) and same_bits(got[~mask], before_state[~mask])
    assert not same_bits(got[mask], before_state[mask]) and same_bits(r[~mask], before_rows[~mask])
    assert same_bits(r[mask][:, :J], want[mask][:, 13:13 + J]) and same_bits(r[mask][:, J:2 * J], want[mask][:, 13 + J:])
    assert float(r[mask][:, 2 * J:3 * J].abs().sum()) == 0.0 and same_bits(r[:, 3 * J:3 * J + 2], before_rows[:, 3 * J:3 * J + 2])
    own = TM.sample(v, None, 0, J=J)[0]                                                  # the clocks: t0 = the time, k = 0
    assert same_bits(own[mask], want[mask])
    fractions(name, "motion", dict(sorted(TM.WORST.items())))
    v.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_episode_ends(built):
    """deep_chain, an episode limit of 2 with staggered counts, rewards and a clip both attached, 5 steps: in every launch some
    envs end and others go on; done rows repeat the held values bitwise, timers and clocks restart as the two references say"""
    name = "deep_chain"
    om, J, params, st, act, touch = case(built[name], name)
    plan = RK.episode_plan(N, limit=2, steps=5)
    v = env_of(built[name], max_episode_steps=2)
    v.set_state(dev(st))
    v.set_episode_steps(torch.arange(N) % 2)
    Ts = TR.step_seconds(v)
    rspec = [RK.rterm(RR.STEP, 0.5), RK.rterm(RR.JOINT_VEL, -1e-3), RK.rterm(RR.JOINT_ACC, -2.5e-7), RK.rterm(RR.ACTION_RATE, -0.01),
             RK.rterm(RR.FOOT_AIR_TIME, 1.0, link=touch, p0=1e6), RK.rterm(RR.ORIENTATION, -1.0), RK.rterm(RR.BASE_HEIGHT, 1.0, p0=0.2),
             RK.rterm(RR.FOOT_AIR_TIME, 1.0, link=touch, p0=-1e6)]
    TR.api(v).set_reward(rspec)
    tab, probes = attach_clip(v, om, name, params)
    mspec = RK.motion_spec(om)
    TM.mapi(v).set_reward(mspec, 1.0)
    hists = TR.histories(N, len(rspec), J=J)
    clocks, helds = [MR.new_clock() for _ in range(N)], [np.zeros(len(mspec)) for _ in range(N)]
    TR.WORST.clear()
    TM.WORST.clear()
    prev_r = prev_m = None
    for t in range(5):
        a, cmd = TR.inputs(N, seed=90 + t, J=J)
        v.step_tensor(a)
        rows = v.rows.clone()
        done = (rows[:, 3 * J + 1] != 0).cpu().numpy()
        assert done.tolist() == plan[t].tolist() and done.any() and not done.all()
        state, force = TR.instant(v)
        after, terms, ok = TR.compose(v, rows, a, cmd, len(rspec))
        assert ok
        terms = TR.check(om, rspec, rows, after, terms, state, force, hists, Ts, a, cmd, prev_terms=prev_r, J=J)
        assert same_bits(torch.tensor(terms[:, 0]), 0.5 * rows[:, 3 * J].cpu())            # STEP comes from the row, done or not
        if prev_r is not None:
            assert terms[done, 1:].tobytes() == prev_r[done, 1:].tobytes()
        # (the timer of a foot that never "touches" - threshold 1e6 - restarts with every episode)
        assert all(hists[e]["timer"][4] == 0.0 for e in range(N) if done[e]) and all(hists[e]["timer"][4] > 0 for e in range(N) if not done[e])
        prev_r = terms
        after, mterms, ok = TM.compose(v, rows, len(mspec))
        assert ok
        mterms = TM.check_compose(om, tab, probes, mspec, 1.0, rows, after, mterms, state, clocks, helds, Ts, prev_m, J=J)
        if prev_m is not None:
            assert mterms[done].tobytes() == prev_m[done].tobytes()
        assert all(clocks[e]["k"] == 0 for e in range(N) if done[e])
        prev_m = mterms
    assert sorted(set(c["k"] for c in clocks)) == [0, 1]
    own = TM.sample(v, None, 0, J=J)[0]                                                  # the device's clocks are the reference's
    assert same_bits(own, TM.sample(v, np.array([MR.clock_time(c, Ts) for c in clocks], np.float32), 0, J=J)[0])
    fractions(name, "episode ends, reward", reward_worst())
    fractions(name, "episode ends, motion", dict(sorted(TM.WORST.items())))
    v.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_parameters_that_are_not_the_defaults(built):
    """deep_chain with dt = 1/200, substeps = 3, floor_z = 0.05: BASE_HEIGHT and POINT_HEIGHT of both kernels against that floor,
    JOINT_ACC and the FOOT_AIR_TIME timer against Ts = 0.015 s - three envs go through the lift-off and the landing of
    row_kernel_cases.air_time_case -, and the clip clock over 4 composes"""
    name = "deep_chain"
    m = built[name]
    om, J, params, st, act, _ = case(m, name, other=True)
    c = RK.air_time_case(name, om, params)
    touch = RK.link_of_body(om, c["body"])
    st, act = st.copy(), act.copy()
    lifted = [0, 4, 8]
    st[lifted], act[lifted] = c["state"], c["action"]
    v = env_of(m, other=True)
    Ts, floor_z = TR.step_seconds(v), params["floor_z"]
    assert Ts == RR.step_seconds(1.0 / 200.0, 3) == MR.step_seconds(1.0 / 200.0, 3) != RR.step_seconds(0.002, 5) and floor_z == 0.05
    assert v.model.get_param("floor_z") == 0.05
    v.set_state(dev(st))
    ospec, rspec, mspec = RK.obs_spec(om, touch), RK.reward_spec(om, touch), RK.motion_spec(om)
    E = v.batch.set_observation(ospec)
    TR.api(v).set_reward(rspec)
    tab, probes = attach_clip(v, om, name, params)
    TM.mapi(v).set_reward(mspec, 1.0)
    hists = TR.histories(N, 32, J=J)
    clocks, helds = [MR.new_clock() for _ in range(N)], [np.zeros(len(mspec)) for _ in range(N)]
    TR.WORST.clear()
    TM.WORST.clear()
    a, ext = dev(act), TO.inputs(N, seed=12, J=J)[1]
    cmd = TR.inputs(N, seed=13, J=J)[1]
    oworst = dict(pose=0.0, velocity=0.0)
    AIR = RR.FOOT_AIR_TIME
    prev_m, paid, flown, contact = None, 0, 0, []
    for t in range(max(c["steps"], 4)):
        v.step_tensor(a)
        rows = v.rows.clone()
        assert not bool((rows[:, 3 * J + 1] != 0).any())
        state, force = TR.instant(v)
        out = TO.compose(v, rows, a, ext, E, J=J)
        w = TO.check_rows(om, ospec, out, rows, v.get_state(), a, ext, v.contact_wrench()[:, :, 2], J=J, floor_z=floor_z)
        oworst = {k: max(oworst[k], w[k]) for k in w}
        before = [h["timer"][AIR] for h in hists]
        after, terms, ok = TR.compose(v, rows, a, cmd, 32)
        assert ok
        terms = TR.check(om, rspec, rows, after, terms, state, force, hists, Ts, a, cmd, J=J, floor_z=floor_z)
        paid += sum(1 for e in lifted if terms[e, AIR] != 0 and before[e] > 0)
        flown += sum(1 for e in lifted if hists[e]["timer"][AIR] > 0)
        contact.append(bool(force[0, c["body"], 2] > RK.FORCE_MIN))
        if t < 4:
            after, mterms, ok = TM.compose(v, rows, len(mspec))
            assert ok
            prev_m = TM.check_compose(om, tab, probes, mspec, 1.0, rows, after, mterms, state, clocks, helds, Ts, prev_m, J=J)
    # the body stood, left the floor and landed; the landing paid the timer: steps in the air x 0.015 s less the offset
    assert contact[0] and not all(contact) and paid >= 1 and flown >= 1, (contact, c["touch"])
    assert all(ck["k"] == 4 for ck in clocks)
    own = TM.sample(v, None, 0, J=J)[0]
    assert same_bits(own, TM.sample(v, np.full(N, MR.clock_time(clocks[0], Ts), np.float32), 0, J=J)[0])
    fractions(name, "other parameters, observation", {k: x / LINK_TOL[k] for k, x in oworst.items()})
    fractions(name, "other parameters, reward", reward_worst())
    fractions(name, "other parameters, motion", dict(sorted(TM.WORST.items())))
    v.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_ik_in_base_axes_is_refused_off_the_root(built):
    """mount_first: URDF link 0 does not belong to the base body, so targets in TREX_AXES_BASE are refused with TREX_E_INVALID
    before any launch - the guarded outputs keep their fill; targets in world axes are accepted"""
    from trex_gym import _capi
    m = built["mount_first"]
    om, J = m["om"], m["om"]["nb"] - 1
    assert om["link_body"][0] != 0
    n = 4
    v = env_of(m, n)
    b = v.batch
    links = [RK.links_of(om)["deepest"]]
    b.set_link_probes(0, links, np.array([[0.05, 0.0, -0.02]]))
    t = torch.zeros(n, 1, 7, device=DEV)
    t[..., :3] = torch.tensor([0.3, 0.1, 2.9], device=DEV)
    t[..., 6] = 1
    wq, q = guarded((n, J), fill=float("nan"))
    wi, info = guarded((n, 4), fill=float("nan"))
    refused(_capi.E_INVALID, b.inverse_kinematics, 0, [1], t, q, 2, None, None, info)          # frame = TREX_AXES_BASE
    assert "link 0" in _capi.lib.trex_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and torch.isnan(info).all()
    assert guards_intact(wq, (n, J), fill=float("nan")) and guards_intact(wi, (n, 4), fill=float("nan"))
    b.inverse_kinematics(0, [1], t, q, 0, None, None, info)                                     # frame = TREX_AXES_WORLD
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(info).all()
    assert guards_intact(wq, (n, J), fill=float("nan")) and guards_intact(wi, (n, 4), fill=float("nan"))
    v.close()
