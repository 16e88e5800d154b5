"""CPU: the states and thresholds of tests/termination_cases.py are what they claim, on the f64 reference alone, and the reference
(tests/termination_ref.py) itself holds the properties that define a floor clearance."""
import numpy as np
import pytest

import termination_cases as TC
import termination_ref as TR

COLLISIONS = ("hulls", "primitives")


@pytest.mark.parametrize("collision", COLLISIONS)
def test_thresholds_qualify(collision):
    b, cases = TC.states(collision)
    thr = TC.search(collision)
    assert thr is not None, "no threshold set qualifies"
    c = TC.counts(thr["reasons"])
    print(collision, "head %.4f m, cos tilt %.4f, %s clear of %.4f m:" % (thr["head_height"], thr["cos_tilt"], thr["link"], thr["clear"]), c)
    assert c["n"] == len(cases)                                  # 0 cases left out
    assert min(c["head"], c["tilt"], c["clearance"]) >= 5, c     # each reason alone
    assert c["two"] >= 5, c
    assert 3 * c["none"] >= c["n"], c
    # every case at least CLEAR from every threshold in force
    v = thr["values"]
    dist = np.stack([np.abs(v[:, 0] - thr["head_height"]), np.abs(v[:, 1] - thr["cos_tilt"]), np.abs(v[:, 2])], 1)
    assert dist.min() >= TC.CLEAR, dist.min()
    # the reasons are those of the thresholds as the kernel will receive them (f32)
    hh, tilt = float(np.float32(thr["head_height"])), float(np.float32(thr["max_tilt"]))
    cm = thr["clear_min"].astype(np.float32).astype(np.float64)
    again = [TR.reason(TR.values(e, cm), hh, tilt) for e in TC.reference(collision)]
    assert (np.array(again) == thr["reasons"]).all()


def test_the_states_are_the_issues():
    _, hulls = TC.states("hulls")
    _, prims = TC.states("primitives")
    origins = [c["origin"] for c in hulls]
    assert sum(o.startswith("hulls episode") for o in origins) > 600 and sum(o.startswith("hulls_domain") for o in origins) > 600
    assert origins.count("start") == 1 and sum(o.startswith("case_states") for o in origins) == 33
    assert sum(c["origin"].startswith("primitives") for c in prims) > 300 and prims[-1]["origin"] == "start"
    assert len(TC.sample("hulls")) == 67 and len(TC.sample("primitives")) == 67
    assert TC.sample("hulls")[-1] == len(hulls) - 1


@pytest.mark.parametrize("collision", COLLISIONS)
def test_reference_clearance_properties(collision):
    b, cases = TC.states(collision)
    ref = TC.reference(collision)
    om, orc = b.om, b.o64
    floor_z = float(orc.params["floor_z"])
    rng = np.random.default_rng(11)
    for k in TC.sample(collision, 12):
        e, st = ref[k], cases[k]["state"].astype(np.float64)
        pts = TR.world_points(om, e["pos"], e["rot"])
        for bd, (w, r) in enumerate(pts):
            if len(w) == 0:
                assert np.isinf(e["clearance"][bd]) and np.isnan(e["lowest"][bd]).all()
                continue
            h = w[:, 2] - r
            assert (e["clearance"][bd] <= h - floor_z).all()               # <= the height of every one of its points
            assert (e["lowest"][bd][2] <= h).all()                         # the lowest point lies on or below every other
            assert abs((e["lowest"][bd][2] - floor_z) - e["clearance"][bd]) < 1e-12
        # invariant under base yaw about the world z axis and under xy translation
        yaw = rng.uniform(-np.pi, np.pi)
        qz = np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])
        x, y, z, w_ = st[3:7]
        moved = st.copy()
        moved[3:7] = [qz[3] * x - qz[2] * y, qz[3] * y + qz[2] * x, qz[3] * z + qz[2] * w_, qz[3] * w_ - qz[2] * z]   # qz * q
        c, s = np.cos(yaw), np.sin(yaw)
        moved[0:2] = [c * st[0] - s * st[1] + 3.7, s * st[0] + c * st[1] - 51.0]
        m = TR.evaluate(orc, om, moved, cases[k]["mass_scale"])
        fin = np.isfinite(e["clearance"])
        assert np.abs(m["clearance"][fin] - e["clearance"][fin]).max() < 1e-9
        assert abs(m["head"] - e["head"]) < 1e-9 and abs(m["cos_tilt"] - e["cos_tilt"]) < 1e-12
        # floor_z += d shifts every clearance by -d
        c2, _ = TR.clearance(om, floor_z + 0.125, e["pos"], e["rot"])
        assert np.abs(c2[fin] - (e["clearance"][fin] - 0.125)).max() < 1e-12


def test_reference_at_the_start_state():
    b, cases = TC.states("hulls")
    e = TC.reference("hulls")[[c["origin"] for c in cases].index("start")]
    assert abs(e["cos_tilt"] - 1.0) < 1e-12
    assert TR.reason(TR.values(e), head_height=None, max_tilt=None) == 0
    assert TR.reason(TR.values(e), head_height=e["head"] + 1e-6, max_tilt=None) == TR.HEAD
    assert TR.reason(TR.values(e), head_height=e["head"], max_tilt=None) == 0        # strict <
