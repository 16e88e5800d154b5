"""The case groups of tests/param_cases.py - the step under every engine parameter moved off its default - proven on the CPU
before they reach a GPU, on the oracle alone: every kept case is accepted (the f32 oracle within assert_step_close of the f64
oracle at loosen = 1, same contacts), at least half of a group's cases tell the moved parameter from its default by >= 10 x the
rate tolerance, at most half of the examined candidates were replaced, and the states are in the branch the group is about.
Each test prints its group's figures (pytest -s); measured: profiles/r26_engine_params.txt."""
import numpy as np
import pytest

import param_cases as pc

REPLACED_CAP = 0.5


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return tmp_path_factory.mktemp("param_models")


def group(name, directory):
    return pc.group(name, directory)


def test_groups_move_what_they_say():
    d, moved = pc.defaults(), pc.moved_parameters()
    for name, m in moved.items():
        assert all(m[k] != d[k] for k in m), name
        assert len(m) == 1 or name.startswith("all_moved"), name
    assert moved["dt_half"]["dt"] == 0.5 * d["dt"] and moved["dt_double"]["dt"] == 2.0 * d["dt"]
    assert set(moved["all_moved"]) == {k for n, m in moved.items() if not n.startswith("all_moved") for k in m}
    assert all(moved["all_moved"][k] in [m[k] for n, m in moved.items() if not n.startswith("all_moved") and k in m]
               for k in moved["all_moved"])


def test_velocity_restatement_without_velocity_joints_is_the_oracle_step(directory):
    """env_step's substep-by-substep restatement with no joint in VELOCITY mode is oracle_step itself, bitwise"""
    g = group("substeps_3", directory)
    b = g["built"]
    for c in g["cases"][:4]:
        plain = pc.run(b.o64, b.om, c)
        restated = pc.run(b.o64, b.om, dict(c, vel=np.zeros(b.J, bool)))
        for x, y in zip(plain, restated):
            assert np.array_equal(x["obs"], y["obs"]) and x["rew"] == y["rew"] and np.array_equal(x["state"], y["state"])


@pytest.mark.parametrize("name", pc.GROUPS)
def test_group_is_accepted_and_sensitive(name, directory):
    g = group(name, directory)
    b, base, cases, st = g["built"], g["base"], g["cases"], g["stats"]
    assert 8 <= len(cases) <= 16, (name, st)
    assert st["share"] <= REPLACED_CAP, (name, st)
    dev, gaps, sensitive = [], [], 0
    for k, c in enumerate(cases):
        ok, r64, r32 = pc.accept(b, c)                         # the group's own oracle, both builds
        assert ok, (name, k, c["origin"])
        dev.append(pc.rate_gap(b, r32, r64))
        fails, gap = pc.sensitivity(b, base, c, r64, r32)      # ... against the oracle with the moved parameter at its default
        gaps.append(gap)
        sensitive += bool(fails and gap >= pc.EFFECT)
    in_contact = sum(any(x["cnt"] > 0 for x in e) for e in pc.expected(g))
    print("PARAM-CASES %-22s kept %2d examined %2d replaced %2d (share %.2f) passed over %2d | in contact %2d | f32 - f64 |dqd| / tol max %.3f | "
          "default-parameter oracle |dqd| / tol: min %.1f median %.1f max %.0f, >= %g and failing in %d of %d"
          % (name, len(cases), st["examined"], st["replaced"], st["share"], st["passed_over"], in_contact, max(dev), min(gaps),
             np.median(gaps), max(gaps), pc.EFFECT, sensitive, len(cases)))
    assert 2 * sensitive >= len(cases), (name, sensitive, len(cases))


@pytest.mark.parametrize("name", ["cerp_low", "cerp_high"])
def test_contact_erp_cases_penetrate(name, directory):
    g = group(name, directory)
    b = g["built"]
    for c, e in zip(g["cases"], pc.expected(g)):
        assert min(x["dist_min"] for x in e) < 0 or pc.first_contacts(b.o64, b.om, c)[2].min() < 0, c["origin"]


@pytest.mark.parametrize("name", ["erp_low", "erp_high", "erp_low_deep_chain", "erp_high_deep_chain"])
def test_erp_cases_have_a_joint_beyond_its_stop(name, directory):
    g = group(name, directory)
    b = g["built"]
    rows = []
    for c in g["cases"]:
        assert pc.beyond_stop(b.om, c["state"]) > 0, c["origin"]
        s = b.o64.new_state()
        b.o64.set_state(s, c["state"].astype(np.float64))
        b.o64.step(s, c["action"].astype(np.float64))
        rows.append(b.o64.limit_rows(s))
    assert g["model"] == ("deep_chain" if name.endswith("deep_chain") else "trex") and b.nb == (7 if name.endswith("deep_chain") else 26)
    print("PARAM-CASES %s: limit rows at the end of the first env-step: %s" % (name, rows))


@pytest.mark.parametrize("name", ["iters_1", "iters_7", "iters_120"])
def test_iteration_cases_have_six_contact_points(name, directory):
    g = group(name, directory)
    assert all(e[0]["cnt"] >= 6 for e in pc.expected(g)), [e[0]["cnt"] for e in pc.expected(g)]
    assert int(g["built"].o64.params["iterations"]) % 2 == (0 if name == "iters_120" else 1)


@pytest.mark.parametrize("name", ["friction_low", "friction_high"])
def test_friction_cases_slide(name, directory):
    g = group(name, directory)
    b = g["built"]
    speeds = [pc.sliding_speed(b.o64, b.om, c) for c in g["cases"]]
    print("PARAM-CASES %s: tangential speed at a contact point, m/s: min %.2f max %.2f" % (name, min(speeds), max(speeds)))
    assert min(speeds) > pc.SLIDE
    assert "friction" in b.params and all("mass_scale" not in c for c in g["cases"])        # the model parameter: no domain


@pytest.mark.parametrize("name", ["floor_up", "floor_down", "all_moved"])
def test_floor_cases_touch_the_moved_floor(name, directory):
    g = group(name, directory)
    b = g["built"]
    fz = float(b.params["floor_z"])
    touching = 0
    for c in g["cases"]:
        body, pos, dist = pc.first_contacts(b.o64, b.om, c)
        if len(body):
            touching += 1
            assert np.abs(pos[:, 2] - dist - fz).max() <= 1e-9 + float(b.o64.params["contact_margin"]), c["origin"]
            assert pos[:, 2].max() <= fz + 2 * float(b.o64.params["contact_margin"])
    assert 2 * touching >= len(g["cases"]), (name, touching)


def test_gravity_zero_cases_start_airborne(directory):
    g = group("gravity_zero", directory)
    b = g["built"]
    assert all(len(pc.first_contacts(b.o64, b.om, c)[0]) == 0 for c in g["cases"])
    assert sum(e[2]["cnt"] > 0 for e in pc.expected(g)) >= len(g["cases"]) // 2       # ... and half of them touch down within 3 env-steps


def test_damping_cases_are_airborne_and_fast(directory):
    for name in ("damping_zero", "damping_high"):
        g = group(name, directory)
        b = g["built"]
        assert all(x["cnt"] == 0 for e in pc.expected(g) for x in e), name
        assert all(np.abs(c["state"][13 + b.J:]).max() > 4.0 for c in g["cases"]), name


def test_vmax_cases_are_clamped_where_the_kernel_clamps(directory):
    """vmax_2: in the 'rates' cases the unconstrained update of a joint rate exceeds the bound (the oracle clamps it: the rate the
    motor row starts from is +- 2); in the 'base' cases a component of the base's angular AND of its linear velocity does, the base
    is rolled and pitched by >= TILT, and the same world twist on an upright base (identity quaternion) gives rates >= EFFECT x the
    tolerance away and fails assert_step_close: a clamp made in the base's own frame cannot pass. vmax_2_velocity: commands beyond
    the bound on VELOCITY joints."""
    g = group("vmax_2", directory)
    b = g["built"]
    kinds = [c["kind"] for c in g["cases"]]
    assert kinds.count("rates") >= 4 and kinds.count("base") >= 4
    frame = []
    for c, e in zip(g["cases"], pc.expected(g)):
        w, v, nqd = pc.unconstrained_update(b.o64, b.om, c["state"])
        if c["kind"] == "rates":
            assert (np.abs(nqd) > 1.1 * pc.VMAX).sum() >= b.J // 2, c["origin"]
            assert np.abs(e[0]["obs"][b.J:2 * b.J]).max() < 100.0
        else:
            assert np.abs(w).max() > 1.1 * pc.VMAX and np.abs(v).max() > 1.1 * pc.VMAX, c["origin"]
            assert abs(c["roll"]) >= pc.TILT and abs(c["pitch"]) >= pc.TILT
            assert np.linalg.norm(c["state"][10:13]) > pc.VMAX and c["state"][9] < -pc.VMAX
            # after the step the free base still moves at the bound: nothing but the motors' reaction has touched it
            assert np.abs(e[0]["state"][7:13]).max() < pc.VMAX + 0.5
            fails, gap = pc.frame_gap(b, c)
            assert fails and gap >= pc.EFFECT, (c["origin"], gap)
            frame.append(gap)
    print("PARAM-CASES vmax_2: identity-quaternion variant of the %d base cases, |dqd| / tol: min %.1f median %.1f max %.0f"
          % (len(frame), min(frame), np.median(frame), max(frame)))
    gv = group("vmax_2_velocity", directory)
    vel = pc.velocity_mask(gv["built"].J)
    assert gv["modes"] is not None and sum(m == pc.MODE_VELOCITY for m in gv["modes"]) == vel.sum()
    for c in gv["cases"]:
        cmd = c["action"][vel]
        assert (np.abs(cmd) > pc.VMAX).sum() >= 3 and (np.abs(cmd) < pc.VMAX).any() and np.array_equal(c["vel"], vel)
