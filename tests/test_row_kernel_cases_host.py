"""CPU checks that keep tests/test_gpu_row_kernels_models.py from being vacuous: the generated model mount_first is what it claims
(URDF link 0 welded, behind a turned frame, to a moving body at depth 2; joints that sort differently from the bodies); the cases
of tests/row_kernel_cases.py reach the branches they are meant to, by Oracle.contacts and the references; and a kernel that took
the base axes from body 0, the joint columns in body order, or Ts and floor_z at their defaults would be seen - the references
alone, evaluated with that mistake on the case states, leave the right values by at least 100 x the bound the GPU test applies, in
at least one env and one term or channel of every kind the mistake touches."""
import numpy as np
import pytest

import motion_ref as MR
import observation_ref as OR
import reward_ref as RR
import row_kernel_cases as RK
import synthetic_models as sm
from state_sets import built_models
from tolerances import LINK_TOL

SEPARATION = 100.0
POSE_KINDS = (OR.GRAVITY, OR.BASE_HEIGHT, OR.POINT_POS, OR.POINT_HEIGHT)
VEL_KINDS = (OR.BASE_LIN, OR.BASE_ANG, OR.POINT_VEL)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return built_models(RK.MODELS, tmp_path_factory)


def case(built, name, other=False):
    m = built[name]
    params = RK.params_of(m["props"], other)
    st, act = RK.states(name, m["om"], params)
    return m["om"], params, st, act, RK.touch_link(name, m["om"], params)


# ---------------------------------------------------------------- mount_first
def test_mount_first_is_what_it_claims(built):
    """(that the loader and the oracle's compiler agree on every array of it, link_body and link_tf included:
    tests/test_synthetic_models_host.py::test_loader_matches_the_oracle_compiler[mount_first])"""
    m = built["mount_first"]
    props, om = m["props"], m["om"]
    assert om["link_names"][0] == "imu" and om["nb"] == props["nb"]
    lb, depth = np.asarray(om["link_body"], int), np.asarray(om["depth"], int)
    tf0 = np.asarray(om["link_tf"], np.float64).reshape(-1, 12)[0]
    assert lb[0] >= 1 and lb[0] == props["link0_body"] and depth[lb[0]] >= 2 and depth[lb[0]] == props["link0_depth"]
    assert depth.max() == props["depth"] and len(lb) == 6 and om["nb"] == 5
    R0 = tf0[:9].reshape(3, 3)
    assert props["link0_turned"] and np.abs(R0 - np.eye(3))[~np.eye(3, dtype=bool)].min() > 1e-2 and np.abs(tf0[9:]).min() > 1e-2
    np.testing.assert_allclose(R0 @ R0.T, np.eye(3), atol=1e-12)
    oo = list(om["obs_order"])
    assert props["permuted_obs_order"] and oo != sorted(oo) and oo != sorted(oo, reverse=True)
    lo, hi = om["q_lower"][oo], om["q_upper"][oo]
    assert len(set(lo)) == len(lo) and len(set(hi)) == len(hi)                 # every joint its own limits: a permutation shows
    assert np.all(np.sort(np.abs(om["joint_axis"][1:]), axis=1)[:, 1] > 0.02)  # oblique axes
    assert "mount_first" not in sm.MODELS and "mount_first" in sm.KINEMATIC_MODELS
    # deep_chain keeps URDF link 0 in the root, turned against the body's axes (the inertial frame's rpy); on bushy and slab link 0
    # IS the root body's frame: there "the base axes are body 0's" is the same computation
    o = built["deep_chain"]["om"]
    assert o["link_body"][0] == 0 and np.abs(np.asarray(o["link_tf"], float).reshape(-1, 12)[0][:9] - np.eye(3).reshape(-1)).max() > 1e-2
    for name in ("bushy", "slab"):
        o = built[name]["om"]
        assert o["link_body"][0] == 0 and np.abs(np.asarray(o["link_tf"], float).reshape(-1, 12)[0] - np.r_[np.eye(3).reshape(-1), 0, 0, 0]).max() == 0


# ---------------------------------------------------------------- the cases reach their branches
@pytest.mark.parametrize("name", RK.MODELS)
def test_cases_reach_their_branches(name, built):
    om, params, st, act, touch = case(built, name)
    J = om["nb"] - 1
    assert st.shape == (RK.N, 13 + 2 * J) and act.shape == (RK.N, J) and (st == st.astype(np.float32)).all()
    bodies = RK.touching(name, om, params)
    assert sum(1 for b in bodies if b) >= 2 and sum(1 for b in bodies if not b) >= 2, bodies
    tb = int(om["link_body"][touch])
    assert sum(1 for b in bodies if tb in b) >= 1
    assert sum(1 for row in RK.touching_wild(name, om, params) for b in row if tb in b) >= 1       # and along the reward test's steps
    ospec, rspec = RK.obs_spec(om, touch), RK.reward_spec(om, touch)
    assert sorted(set(s[0] for s in ospec)) == list(range(OR.KINDS)) and len(rspec) <= RR.MAX_TERMS
    assert all(int(om["link_body"][s[1]]) == tb for s in ospec if s[0] == OR.CONTACT)
    assert all(int(om["link_body"][s[1]]) == tb for s in rspec if s[0] in (RR.FOOT_AIR_TIME, RR.FOOT_SLIP))
    assert all((s[2] >> tb) & 1 for s in rspec if s[0] == RR.CONTACT_COUNT)
    ln = RK.links_of(om)
    assert (ln["merged"] is not None) == (name in ("bushy", "mount_first"))
    links, pts = RK.end_effectors(om)
    assert len(links) == min(8, len(om["link_names"])) == len(set(links)) and links[0] == 0
    assert ln["merged"] is None or ln["merged"] in links
    # JOINT_LIMIT: some env stands inside the margin of a stop
    rows = RK.rows_of(om, st)
    force = np.zeros((om["nb"], 3))
    hit = 0
    for e in range(RK.N):
        v, _ = RR.evaluate(om, rspec, st[e], rows[e], RR.new_history(len(rspec), J, J), RR.step_seconds(params.get("dt", 0.002), 5),
                           action=act[e], command=np.zeros(3), force=force)
        hit += int(v[RR.JOINT_LIMIT] > 0)
    assert hit >= 1
    # the clip: a rollout inside the limits that moves
    frames, vel = RK.clip(om, RK.oracle_of(name, om, params))
    assert frames.shape == (RK.FRAMES, 7 + J) and vel.shape == (RK.FRAMES, 6 + J)
    assert MR.refusal(om, frames, vel, RK.DT) is None and np.abs(frames[-1] - frames[0]).max() > 1e-2
    assert len(RK.motion_spec(om)) == MR.MAX_TERMS and sorted(set(s[0] for s in RK.motion_spec(om))) == list(range(MR.KINDS))


def test_episode_plan_mixes_done_and_live_rows():
    done = RK.episode_plan(RK.N, limit=2, steps=5)
    assert done.shape == (5, RK.N) and all(row.any() and not row.all() for row in done)


def test_air_time_case_lifts_off_and_lands(built):
    om, params, _, _, _ = case(built, "deep_chain", other=True)
    c = RK.air_time_case("deep_chain", om, params)
    t = c["touch"]
    assert c["body"] >= 1 and c["steps"] == len(t) <= 10 and t[0] and t[-1] and not any(t[1:-1]) and len(t) >= 3


# ---------------------------------------------------------------- a wrong kernel would be seen
def obs_bounds(spec, want, J):
    """per channel, the bound check_rows of tests/test_gpu_observations.py applies to its columns (0: compared bitwise)"""
    out = []
    for (kind, _, _, scale), (c0, w) in zip(spec, OR.columns(spec, J)):
        r = want[c0:c0 + w]
        tol = LINK_TOL["pose"] if kind in POSE_KINDS else LINK_TOL["velocity"] if kind in VEL_KINDS else 0.0
        out.append(tol * abs(scale) * max(1.0, np.abs(r).max() / abs(scale)))
    return out


def obs_separation(om, spec, vm, vspec, st, floor_z, vfloor_z):
    """{kind: the largest |right - mistaken| / bound over the envs and the channels of that kind}"""
    J = om["nb"] - 1
    ext, fz = np.zeros(7), np.zeros(om["nb"])
    best = {}
    for e in range(len(st)):
        right = OR.channels(om, st[e], spec, extern=ext, contact_fz=fz, floor_z=floor_z)
        wrong = OR.channels(vm, st[e], vspec, extern=ext, contact_fz=fz, floor_z=vfloor_z)
        for (kind, _, _, _), (c0, w), b in zip(spec, OR.columns(spec, J), obs_bounds(spec, right, J)):
            if b > 0:
                best[kind] = max(best.get(kind, 0.0), np.abs(right[c0:c0 + w] - wrong[c0:c0 + w]).max() / b)
    return best


def reward_separation(om, spec, vm, vspec, st, rows, act, Ts, vTs, floor_z, vfloor_z, forces=None, steps=1):
    """{kind: the largest |right - mistaken| / bound}; `steps` calls per env on the rows [steps][n], so that the rate terms and the
    timers have a history"""
    J = om["nb"] - 1
    T = len(spec)
    best = {}
    cmd = np.array([0.3, -0.2, 0.4])
    for e in range(len(st[0])):
        hr, hw = RR.new_history(T, J, J), RR.new_history(T, J, J)
        for k in range(steps):
            f = np.zeros((om["nb"], 3)) if forces is None else forces[k][e]
            right, cases = RR.evaluate(om, spec, st[k][e], rows[k][e], hr, Ts, action=act[e] * (k + 1), command=cmd, force=f, floor_z=floor_z)
            wrong, _ = RR.evaluate(vm, vspec, st[k][e], rows[k][e], hw, vTs, action=act[e] * (k + 1), command=cmd, force=f, floor_z=vfloor_z)
            for t, (s, c) in enumerate(zip(spec, cases)):
                b = RR.bound(s[0], c) + 2 * RR.U * abs(right[t])
                if b > 0:
                    best[s[0]] = max(best.get(s[0], 0.0), abs(right[t] - wrong[t]) / b)
    return best


def motion_separation(om, tab, vtab, spec, st, rows, Ts, vTs, composes=1):
    J = om["nb"] - 1
    probes = RK.end_effectors(om)
    best = {}
    for e in range(len(st)):
        cr, cw, hr, hw = MR.new_clock(), MR.new_clock(), np.zeros(len(spec)), np.zeros(len(spec))
        for _ in range(composes):
            right, cases = MR.evaluate(om, tab, spec, st[e], rows[e], cr, hr, Ts, probes)
            wrong, _ = MR.evaluate(om, vtab, spec, st[e], rows[e], cw, hw, vTs, probes)
            for t, (s, c) in enumerate(zip(spec, cases)):
                b = MR.bound(s[0], c) + 2 * MR.U * abs(right[t])
                best[s[0]] = max(best.get(s[0], 0.0), abs(right[t] - wrong[t]) / b)
    return best


def clip_table(om, name, params):
    frames, vel = RK.clip(om, RK.oracle_of(name, om, params))
    return MR.device_table(MR.build_table(om, frames, vel, RK.DT, False))


@pytest.mark.parametrize("name", ["mount_first", "deep_chain"])
def test_base_axes_of_body_0_would_be_seen(name, built):
    """mount_first: link 0 in body 2; deep_chain: link 0 in the root, turned. On bushy and slab URDF link 0 IS the root's frame
    (asserted above)"""
    om, params, st, act, touch = case(built, name)
    Ts, fz = RR.step_seconds(0.002, 5), RR.FLOOR_Z
    vm, shift = RK.root_axes_variant(om)
    ospec, rspec = RK.obs_spec(om, touch), RK.reward_spec(om, touch)
    sep = obs_separation(om, ospec, vm, RK.shift_obs(ospec, shift), st, fz, fz)
    print(name, "base axes of body 0, observation channels:", sep)
    for kind in (OR.GRAVITY, OR.BASE_LIN, OR.BASE_ANG, OR.BASE_HEIGHT, OR.POINT_POS, OR.POINT_VEL):
        assert sep[kind] >= SEPARATION, (kind, sep[kind])
    assert sep[OR.POINT_HEIGHT] == 0.0                                         # a world height: no base axes in it
    rows = RK.rows_of(om, st)
    sep = reward_separation(om, rspec, vm, RK.shift_rew(rspec, shift), [st], [rows], act, Ts, Ts, fz, fz)
    print(name, "base axes of body 0, reward terms:", sep)
    for kind in (RR.TRACK_LIN, RR.TRACK_ANG, RR.LIN_VEL_Z, RR.ANG_VEL_XY, RR.ORIENTATION, RR.BASE_HEIGHT):
        assert sep[kind] >= SEPARATION, (kind, sep[kind])
    # END_EFFECTOR: the probes in the base axes, at the state and at the reference pose
    tab = clip_table(om, name, params)
    mspec = RK.motion_spec(om)
    links, pts = RK.end_effectors(om)
    best = 0.0
    for e in range(RK.N):
        right, cases = MR.evaluate(om, tab, mspec, st[e], rows[e], MR.new_clock(), np.zeros(8), Ts, (links, pts))
        wrong, _ = MR.evaluate(vm, tab, mspec, st[e], rows[e], MR.new_clock(), np.zeros(8), Ts, ([l + shift for l in links], pts))
        best = max(best, abs(right[2] - wrong[2]) / (MR.bound(MR.END_EFFECTOR, cases[2]) + 2 * MR.U * abs(right[2])))
    print(name, "base axes of body 0, END_EFFECTOR:", best)
    # (with link 0 in the root the mistake turns and moves both probe sets by one constant transform: the distances between them,
    # all the term reads, stay - the same value. On mount_first body 2 moves against body 0 between the state and the reference.)
    assert mspec[2][0] == MR.END_EFFECTOR and (best >= SEPARATION if om["link_body"][0] != 0 else best < 1.0)


@pytest.mark.parametrize("name", ["deep_chain", "bushy", "mount_first"])
def test_joint_columns_in_body_order_would_be_seen(name, built):
    """(slab has one joint: there is no other order)"""
    om, params, st, act, touch = case(built, name)
    J = om["nb"] - 1
    Ts, fz = RR.step_seconds(0.002, 5), RR.FLOOR_Z
    vm = RK.body_order_variant(om)
    assert list(vm["obs_order"]) != list(om["obs_order"]) and list(built["slab"]["om"]["obs_order"]) == [1]
    ospec, rspec, mspec = RK.obs_spec(om, touch), RK.reward_spec(om, touch), RK.motion_spec(om)
    sep = obs_separation(om, ospec, vm, ospec, st, fz, fz)
    print(name, "body order, observation channels:", sep)
    for kind in (OR.POINT_POS, OR.POINT_VEL, OR.POINT_HEIGHT):                 # the chain walk reads q by obs_slot
        assert sep[kind] >= SEPARATION, (kind, sep[kind])
    rows = RK.rows_of(om, st)
    sep = reward_separation(om, rspec, vm, rspec, [st], [rows], act, Ts, Ts, fz, fz)
    print(name, "body order, reward terms:", sep)
    assert sep[RR.POINT_HEIGHT] >= SEPARATION, sep[RR.POINT_HEIGHT]              # the chain walk again
    oo = np.asarray(om["obs_order"], int)
    if not (np.array_equal(om["q_lower"][oo], om["q_lower"][1:]) and np.array_equal(om["q_upper"][oo], om["q_upper"][1:])):
        assert sep[RR.JOINT_LIMIT] >= SEPARATION, sep[RR.JOINT_LIMIT]            # joint_body: the limits of the joint's own body
    else:
        assert name != "mount_first"                                           # (equal limits on every joint: the same computation)
    if not np.array_equal(om["q_start"][oo], om["q_start"][1:]):
        assert sep[RR.JOINT_POSE] >= SEPARATION, sep[RR.JOINT_POSE]
    # the clip's joint columns scattered into body order without obs_slot: the sampled state, and the terms that read it
    tab = clip_table(om, name, params)
    vtab = RK.body_order_table(om, tab)
    times = RK.time_list(RK.N, tab["duration"])
    worst = max((np.abs(MR.sample(tab, t)[0] - MR.sample(vtab, t)[0]) / MR.sample_bound(tab, t)).max() for t in times)
    assert worst >= SEPARATION, worst
    sep = motion_separation(om, tab, vtab, mspec, st, rows, Ts, Ts)
    print(name, "body order, motion terms:", sep)
    for kind in (MR.POSE, MR.VELOCITY, MR.END_EFFECTOR):
        assert sep[kind] >= SEPARATION, (kind, sep[kind])


def test_default_ts_and_floor_would_be_seen(built):
    """deep_chain under RK.OTHER_PARAMS: the references with the default Ts and floor_z against the right ones"""
    om, params, st, act, touch = case(built, "deep_chain", other=True)
    J = om["nb"] - 1
    Ts, fz = RR.step_seconds(params["dt"], params["substeps"]), params["floor_z"]
    dTs, dfz = RR.step_seconds(0.002, 5), RR.FLOOR_Z
    assert abs(Ts - 0.015) < 1e-8 and Ts != dTs and fz != dfz
    ospec, rspec, mspec = RK.obs_spec(om, touch), RK.reward_spec(om, touch), RK.motion_spec(om)
    sep = obs_separation(om, ospec, om, ospec, st, fz, dfz)
    for kind in (OR.BASE_HEIGHT, OR.POINT_HEIGHT):
        assert sep[kind] >= SEPARATION, (kind, sep[kind])
    # two steps of the oracle behind every case state: JOINT_ACC has a history
    orc = RK.oracle_of("deep_chain", om, params)
    nxt = []
    for s0, a in zip(st, act):
        s = orc.new_state()
        orc.set_state(s, s0)
        orc.set_motors_on(s, 1)
        orc.step(s, 0.5 * a)
        nxt.append(orc.get_state(s).astype(np.float32).astype(np.float64))
    nxt = np.array(nxt)
    sep = reward_separation(om, rspec, om, rspec, [st, nxt], [RK.rows_of(om, st), RK.rows_of(om, nxt)], act, Ts, dTs, fz, dfz, steps=2)
    print("default Ts and floor_z, reward terms:", sep)
    for kind in (RR.BASE_HEIGHT, RR.POINT_HEIGHT, RR.JOINT_ACC):
        assert sep[kind] >= SEPARATION, (kind, sep[kind])
    # FOOT_AIR_TIME through the lift-off and the landing of the air-time case: the payout is the timer
    c = RK.air_time_case("deep_chain", om, params)
    link = RK.link_of_body(om, c["body"])
    spec = [RK.rterm(RR.FOOT_AIR_TIME, 1.0, link=link, p0=RK.FORCE_MIN, p1=0.005)]
    hr, hw = RR.new_history(1, J, J), RR.new_history(1, J, J)
    row = RK.rows_of(om, c["state"][None])[0]
    best = 0.0
    for touch_now in c["touch"]:
        f = np.zeros((om["nb"], 3))
        f[c["body"], 2] = 10.0 if touch_now else 0.0
        right, cases = RR.evaluate(om, spec, c["state"], row, hr, Ts, force=f, floor_z=fz)
        wrong, _ = RR.evaluate(om, spec, c["state"], row, hw, dTs, force=f, floor_z=dfz)
        b = RR.bound(RR.FOOT_AIR_TIME, cases[0]) + 2 * RR.U * abs(right[0])
        if b > 0:
            best = max(best, abs(right[0] - wrong[0]) / b)
    assert best >= SEPARATION, best
    # the clip clock over 4 composes: every term reads the reference at t0 + k Ts
    tab = clip_table(om, "deep_chain", params)
    sep = motion_separation(om, tab, tab, mspec, st, RK.rows_of(om, st), Ts, dTs, composes=4)
    print("default Ts, motion terms:", sep)
    for kind in range(MR.KINDS):
        assert sep[kind] >= SEPARATION, (kind, sep[kind])
