"""The oracle's warm start and external wrench (oracle/trex_oracle.c) on the CPU alone, and the case groups of
tests/feature_cases.py proven before they reach a GPU: every kept case is accepted (the f32 oracle within assert_step_close of the
f64 oracle, same contacts), the warm cases tell warm from cold, the wrenches are large enough to be seen.
Measured numbers: profiles/r15_feature_oracle.txt."""
import numpy as np
import pytest

import feature_cases as fc

J = 25
# largest |qd_warm - qd_cold| of the f64 oracle at 6000 sweeps over the states of test_converged_warm_and_cold_agree (rad/s),
# measured on the CPU (profiles/r15_feature_oracle.txt); the test allows 10 x
CONVERGED_MEASURED = 5.4e-3


@pytest.fixture(scope="module")
def groups(tmp_path_factory):
    return fc.groups(tmp_path_factory.mktemp("feature_models"))


def landing(oracle64, model, steps, seed=5, **setup):
    q0 = model["q_start"][model["obs_order"]]
    lo, hi = model["q_lower"][model["obs_order"]], model["q_upper"][model["obs_order"]]
    rng = np.random.default_rng(seed)
    s = oracle64.new_state()
    if "warm" in setup:
        oracle64.set_warmstart(s, setup["warm"])
    if "wrench" in setup:
        oracle64.set_external_wrench(s, setup["wrench"])
    out = [oracle64.reset(s)]
    for _ in range(steps):
        o, r, _ = oracle64.step(s, np.clip(q0 + 0.15 * rng.normal(size=J), lo, hi))
        out.append(np.append(o, r))
    return out, s


# ---------------------------------------------------------------- the oracle alone
def test_factor_zero_and_zero_wrench_are_the_plain_oracle(oracle64, model):
    plain, s0 = landing(oracle64, model, 50)
    off, s1 = landing(oracle64, model, 50, warm=0.0, wrench=np.zeros((26, 6)))
    assert all(np.array_equal(a, b) for a, b in zip(plain, off))
    assert np.array_equal(oracle64.get_state(s0), oracle64.get_state(s1))
    assert len(oracle64.contacts(s0)[0]) > 0


def test_empty_record_is_the_cold_substep(oracle64, model, groups):
    n = 0
    for c in groups["warm_trex"]["cases"]:
        out = []
        for warm in (0.0, fc.WARM):
            s = fc.start(oracle64, c, warm)
            assert len(oracle64.warm_record(s)[0]) == 0
            oracle64.set_motors_on(s, 1)
            oracle64.substep(s, c["action"].astype(np.float64))
            out.append((oracle64.get_state(s), oracle64.observe(s), oracle64.contacts(s)[1]))
            vert, lam = oracle64.warm_record(s)
            assert len(vert) == len(out[-1][2]) and np.array_equal(lam, out[-1][2])      # every solve writes its record
            n += len(vert) > 0
        assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert n > 20


def test_converged_warm_and_cold_agree(model):
    """At 6000 sweeps in f64 the warm solve (populated record) and the cold solve of the same state land on the same velocities:
    T-rex standing at rest (400 steps holding the start pose). The bound is 10 x the deviation measured on this very oracle."""
    from oracle import oracle as O
    rest = O.Oracle(model)
    conv = O.Oracle(model, params=dict(iterations=6000))
    q0 = model["q_start"][model["obs_order"]]
    s = rest.new_state()
    rest.set_warmstart(s, fc.WARM)
    rest.reset(s)
    worst = 0.0
    for t in range(460):
        rest.step(s, q0)
        if t >= 400 and t % 10 == 0:
            w = conv.copy_state(s)                     # carries the record and the factor
            assert len(conv.warm_record(w)[0]) >= 4
            c = conv.copy_state(s)
            conv.set_warmstart(c, 0.0)
            ow, oc = conv.step(w, q0)[0], conv.step(c, q0)[0]
            worst = max(worst, np.abs(ow[J:2 * J] - oc[J:2 * J]).max())
    print("converged warm - cold, largest |dqd|: %.3e rad/s" % worst)
    assert worst <= 10 * CONVERGED_MEASURED


@pytest.mark.parametrize("delta", [4.9, -4.9])
def test_vertical_wrench_is_a_change_of_gravity(delta, oracle64, model, groups):
    from oracle import oracle as O
    heavy = O.Oracle(model, params=dict(gravity=oracle64.params["gravity"] + delta))
    rng = np.random.default_rng(2)
    worst = 0.0
    for c in groups["warm_trex"]["cases"][:12]:
        ms = rng.uniform(0.8, 1.2, 26)
        w = np.zeros((26, 6))
        w[:, 2] = -delta * model["mass"] * ms
        a = fc.run(oracle64, model, dict(c, wrench=w, mass_scale=ms), 0.0)
        b = fc.run(heavy, model, dict(c, mass_scale=ms), 0.0)
        for x, y in zip(a, b):
            assert x["cnt"] == y["cnt"]
            worst = max(worst, np.abs(x["obs"][:2 * J] - y["obs"][:2 * J]).max() / max(1.0, np.abs(y["obs"][J:2 * J]).max()),
                        np.abs(x["obs"][2 * J:] - y["obs"][2 * J:]).max() / max(1.0, np.abs(y["obs"][2 * J:]).max()))
    print("wrench as gravity, largest relative deviation: %.3e" % worst)
    assert worst <= 1e-9


def test_free_flight_momentum_balance(model):
    """One substep in free flight, link_damping = 0, motors off: the velocity update is linear in the applied force at the pose it
    is made at, so (forced - unforced) spatial momentum, both taken at the OLD pose with the new velocities, is dt x the summed
    wrench about the base origin: sum F, sum (c_b x F_b + T_b). One-hot forces and torques on every body, and all at once."""
    from oracle import oracle as O
    orc = O.Oracle(model, params=dict(link_damping=0.0))
    dt = orc.params["dt"]
    rng = np.random.default_rng(4)
    st = fc.start_state(model)
    st[2] = 8.0
    st[3:7] = [0.1, -0.2, 0.05, 0.97]
    st[3:7] /= np.linalg.norm(st[3:7])
    st[7:13] = rng.normal(size=6)
    st[13 + J:] = 0.5 * rng.normal(size=J)
    s0 = orc.new_state()
    orc.set_state(s0, st)
    pos, rot = orc.body_poses(s0)
    c = pos + np.einsum("bij,bj->bi", rot, model["com"]) - pos[0]          # COMs relative to the base origin

    def momentum_after(w):
        s = orc.new_state()
        orc.set_external_wrench(s, w)
        orc.set_state(s, st)
        orc.substep(s)
        assert len(orc.contacts(s)[0]) == 0 and orc.limit_rows(s) == 0
        new = orc.get_state(s)
        mixed = st.copy()
        mixed[7:13], mixed[13 + J:] = new[7:13], new[13 + J:]
        orc.set_state(s, mixed)
        return orc.energy(s)["momentum"]
    free = momentum_after(None)
    ws = [fc.one_hot(26, b, sl, 1e3 * fc.unit(rng)) for b in range(26) for sl in (slice(0, 3), slice(3, 6))]
    ws.append(np.concatenate([1e3 * rng.normal(size=(26, 3)), 3e2 * rng.normal(size=(26, 3))], 1))
    for w in ws:
        d = momentum_after(w) - free
        want = dt * np.concatenate([(np.cross(c, w[:, :3]) + w[:, 3:]).sum(0), w[:, :3].sum(0)])
        assert np.linalg.norm(d - want) <= 1e-9 * np.linalg.norm(want), (d, want)


def test_set_state_reset_and_copy_handle_the_record(oracle64, model, groups):
    c = groups["warm_trex"]["cases"][0]
    s = fc.start(oracle64, c, fc.WARM)
    fc.step(oracle64, model, s, c["action"])
    vert, lam = oracle64.warm_record(s)
    assert len(vert) >= 4 and (lam[:, 0] > 0).any() and len(set(vert)) == len(vert)
    t = oracle64.copy_state(s)
    assert np.array_equal(oracle64.warm_record(t)[0], vert) and np.array_equal(oracle64.warm_record(t)[1], lam)
    a, b = fc.step(oracle64, model, s, c["action"]), fc.step(oracle64, model, t, c["action"])
    assert np.array_equal(a["obs"], b["obs"])                     # ... and the factor
    oracle64.set_state(t, oracle64.get_state(t))
    assert len(oracle64.warm_record(t)[0]) == 0
    # reset: the record is empty BEFORE the settle substep, which then writes its own - on a floor raised to the feet of the start
    # pose the settle solve has points, and a record left over from before would change it
    r = groups["contained_wrench"]["built"].o64
    used, fresh = fc.start(r, groups["contained_wrench"]["cases"][0], fc.WARM), r.new_state()
    r.set_warmstart(fresh, fc.WARM)
    fc.step(r, model, used, c["action"])
    assert (r.warm_record(used)[1][:, 0] > 0).any()
    assert np.array_equal(r.reset(used), r.reset(fresh)) and np.array_equal(r.get_state(used), r.get_state(fresh))
    assert len(r.warm_record(used)[0]) > 0 and np.array_equal(r.warm_record(used)[1], r.warm_record(fresh)[1])


def test_wrench_is_held_and_skips_the_settle_substep(oracle64, model):
    w = np.zeros((26, 6))
    w[0, :3] = [3e4, -2e4, 1e4]
    s, p = oracle64.new_state(), oracle64.new_state()
    oracle64.set_external_wrench(s, w)
    assert np.array_equal(oracle64.reset(s), oracle64.reset(p)) and np.array_equal(oracle64.get_state(s), oracle64.get_state(p))
    q0 = model["q_start"][model["obs_order"]]
    a, b = oracle64.step(s, q0)[0], oracle64.step(p, q0)[0]
    assert np.abs(a - b).max() > 1e-3
    oracle64.set_state(s, oracle64.get_state(p))                   # set_state keeps the wrench; None clears it
    assert not np.array_equal(oracle64.step(s, q0)[0], oracle64.step(oracle64.copy_state(p), q0)[0])
    oracle64.set_external_wrench(s, None)
    oracle64.set_state(s, oracle64.get_state(p))
    assert np.array_equal(oracle64.step(s, q0)[0], oracle64.step(p, q0)[0])


# ---------------------------------------------------------------- the case groups
def test_every_kept_case_is_accepted(groups):
    """f32 oracle against f64 oracle at loosen = 1, contact count and touched bodies, after every env-step of every case"""
    for name, g in groups.items():
        b = g["built"]
        if g["kind"] == "settle":
            assert all(fc.settle_close(b, fc.settle_run(b.o32, b.om, c), fc.settle_run(b.o64, b.om, c)) for c in g["cases"]), name
            continue
        dev = []
        for k, c in enumerate(g["cases"]):
            ok, r64, r32 = fc.accept(b, c, g["warm"])
            assert ok, (name, k, c["origin"])
            dev.append(fc.deviation(b, r64, r32))
        print("%s: %d cases, f32 - f64 oracle |dqd| / tolerance: max %.3f median %.3f" % (name, len(dev), max(dev), np.median(dev)))


def test_group_sizes_and_coverage(groups):
    assert len(groups["warm_trex"]["cases"]) == 24
    assert all(len(g["cases"]) <= 64 for g in groups.values())
    t = groups["wrench_trex"]
    hot = [np.flatnonzero(np.abs(c["wrench"]).max(1) > 0) for c in t["cases"][:58]]
    assert [int(h[0]) for h in hot[:52]] == [b for b in range(26) for _ in range(2)] and all(len(h) == 1 for h in hot)
    assert all((np.abs(c["wrench"][b, :3]).max() > 0) != (np.abs(c["wrench"][b, 3:]).max() > 0) for c, h in zip(t["cases"][:52], hot) for b in h)
    assert [int(np.flatnonzero(c["wrench"][7])[0]) for c in t["cases"][52:58]] == list(range(6))
    assert all(c["mass_scale"] is not None and (np.abs(c["wrench"]).max(1) > 0).all() for c in t["cases"][58:])
    assert {groups[n]["built"].nb for n in ("wrench_deep_chain", "wrench_bushy")} != {26}
    assert len({c["origin"] for c in t["cases"]}) == 12            # 12 landing states, cycled
    slab = groups["warm_slab"]                                          # one body with four points: the fourth point is recorded
    assert any(x["cnt"] >= 4 and len(x["touched"]) * 4 == x["cnt"] for e in fc.expected(slab) for x in e)
    for n in ("warm_max_contacts_4", "warm_margin_0.5"):                # more touching bodies than points per body allows: one each
        assert any(x["cnt"] == len(x["touched"]) >= 4 for e in fc.expected(groups[n]) for x in e), n


def test_warm_cases_tell_warm_from_cold(groups):
    sep = total = 0
    gaps = []
    for name in ("warm_trex", "warm_slab", "warm_many_hulls", "warm_max_contacts_4", "warm_margin_0.5", "warm_primitives"):
        g = groups[name]
        b = g["built"]
        for c, e in zip(g["cases"], fc.expected(g)):
            if e[0]["cnt"] == 0:
                continue
            cold = fc.run(b.o64, b.om, c, 0.0, steps=1)[0]
            total += 1
            sep += not fc.close(b, cold, e[0], e[0]["tau_extra"])
            gaps.append(np.abs(cold["obs"][b.J:2 * b.J] - e[0]["obs"][b.J:2 * b.J]).max() / (fc.QD_TOL * max(1.0, np.abs(e[0]["obs"][b.J:2 * b.J]).max())))
    print("warm - cold after one env-step: %d of %d in-contact cases fail assert_step_close; |dqd| / tolerance median %.2f max %.1f"
          % (sep, total, np.median(gaps), max(gaps)))
    assert 2 * sep >= total


def test_fallen_groups_are_what_they_claim(groups):
    """warm_fallen / wrench_fallen (from tests/episode_cases.py): the root body and the cranium touch, the contact set changes
    between the env-steps of a case, and the record is live - warm and cold give different rates in most cases in contact. (On
    these thrashing states, rates of 14 rad/s and a tolerance that scales with them, warm and cold seldom separate by
    assert_step_close: they are here for the record lookup under churning contact sets, and stay out of the share that
    test_warm_cases_tell_warm_from_cold asserts.) The wrench acts on exactly the root body and the cranium."""
    import episode_cases as ec
    g = groups["warm_fallen"]
    b = g["built"]
    root, cranium = ec.body(b.om, ec.ROOT), ec.body(b.om, ec.CRANIUM)
    exp = fc.expected(g)
    n_root = sum(any(root in x["touched"] for x in e) for e in exp)
    n_cranium = sum(any(cranium in x["touched"] for x in e) for e in exp)
    churn = sum(e[i]["cnt"] != e[i + 1]["cnt"] or e[i]["touched"] != e[i + 1]["touched"] for e in exp for i in range(len(e) - 1))
    live = sep = total = 0
    for c, e in zip(g["cases"], exp):
        if not any(x["cnt"] for x in e):
            continue
        cold = fc.run(b.o64, b.om, c, 0.0)
        total += 1
        live += any(not np.array_equal(x["obs"], y["obs"]) for x, y in zip(cold, e))
        sep += any(not fc.close(b, x, y) for x, y in zip(cold, e))
    print("warm_fallen: %d cases, root body touches in %d, cranium in %d, contact set changes between env-steps %d times; "
          "warm != cold in %d of %d in contact, beyond assert_step_close in %d" % (len(exp), n_root, n_cranium, churn, live, total, sep))
    assert len(exp) == 48 and max(c["up"] for c in g["cases"]) < 0.91 and n_root >= 10 and n_cranium >= 5 and churn >= 10
    assert total >= 30 and 2 * live >= total       # (a point that lives for one solve only meets no record: those cases start cold)
    w = groups["wrench_fallen"]
    assert len(w["cases"]) == 12
    for c in w["cases"]:
        assert set(np.flatnonzero(np.abs(c["wrench"]).max(1) > 0)) == {root, cranium}
    assert sum(any(root in x["touched"] for x in e) for e in fc.expected(w)) >= 6


def test_wrenches_are_large_enough_and_bounded(groups):
    for name, g in groups.items():
        if g["kind"] != "wrench":
            continue
        b = g["built"]
        vlim = float(b.o64.params["max_coordinate_velocity"])
        eff = []
        for c in g["cases"]:
            e, vmax = fc.wrench_effect(b, c, g["warm"])
            assert e >= fc.EFFECT and vmax < vlim, (name, c["what"], e, vmax)
            eff.append(e)
        print("%s: wrench effect on qd / tolerance: min %.1f median %.1f max %.0f" % (name, min(eff), np.median(eff), max(eff)))


def test_contained_env_continues_like_a_reset(groups):
    """What tests/test_gpu_feature_oracle.py::test_containment_through_set_state relies on: failure containment leaves the start
    pose WITHOUT a settle substep; the oracle's steps from reset (start pose + one free-fall substep, motors off) stay within
    assert_step_close of the steps from the start pose itself."""
    g = groups["contained_set_state"]
    b = g["built"]
    c = g["cases"][fc.CONTAINED]
    s, p = b.o64.new_state(), b.o64.new_state()
    b.o64.reset(s)
    b.o64.set_state(p, fc.start_state(b.om))
    for _ in range(2):
        assert fc.close(b, fc.step(b.o64, b.om, p, c["action"]), fc.step(b.o64, b.om, s, c["action"]))
