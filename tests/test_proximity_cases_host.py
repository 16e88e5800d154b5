"""The synthetic cases of tests/proximity_cases.py qualified on the f64 reference alone: each is in the region of the (s, t) square
it names, at the test state and through the f32-rounded body-frame table; every case but the two fallback ones keeps its axes
more than 1e-3 m apart; and on the case states of the GPU tests no env's smallest default-table distance is near 0, so that
in_self_collision() has one right answer per env."""
import numpy as np
import pytest

import dynamics_ref as R
import proximity_cases as PC
import proximity_ref as PR
from state_sets import case_states

CASES = PC.cases()


@pytest.fixture(scope="module")
def state(model):
    return R.random_states(model, 8)[0][0]


def test_the_list_is_the_issues():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) == 13 + 2 * len(PC.ANGLES)
    assert sorted(abs(a) for a in PC.ANGLES) == [1e-5, 1e-5, 1e-4, 1e-4, 1e-3, 1e-3, 1e-2, 1e-2]
    assert [c["name"] for c in CASES if c["fallback"]] == ["crossing_axes", "concentric_spheres"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_is_in_its_region(case, model, state):
    bodies, caps, pairs = PC.table(model, state, case)
    assert np.array_equal(caps, caps.astype(np.float32).astype(np.float64))
    r = PR.proximity(model, state, bodies, caps, pairs)[0]
    # the table reproduces the design: the world capsules are the designed ones to the f32 rounding of the body-frame values
    wc = PR.world_capsules(model, state, bodies, caps)
    c = PC.centre(state)
    for got, want in zip(wc, (case["a"], case["b"])):
        assert np.abs(got[0] - (c + want[0])).max() < 1e-6 and np.abs(got[1] - (c + want[1])).max() < 1e-6
    designed = PR.capsule_closest((c + case["a"][0], c + case["a"][1], case["a"][2]), (c + case["b"][0], c + case["b"][1], case["b"][2]))
    assert abs(designed["distance"] - r["distance"]) < 1e-6
    # the region, on the design itself (between axes 1e-4 rad apart the rounding of the table, 1e-8 m, moves the closest points
    # from the middle to an end for 1e-8 m of distance: the table is held to the design's distance, above)
    for u, which, cap in ((designed["s"], 0, caps[0]), (designed["t"], 1, caps[1])):
        want = case["region"][which]
        if want != "any":
            assert PC.region_of(u, np.array_equal(cap[0:3], cap[3:6])) == want, (case["name"], which, u)
            if want == "interior":
                assert 0.05 < u < 0.95
    if case["fallback"]:
        assert r["axis"] < PR.EPS / 4 and np.array_equal(r["normal"], [0, 0, 1])
        assert abs(r["distance"] + case["a"][2] + case["b"][2]) < 1e-6
    else:
        assert r["axis"] > 1e-3, (case["name"], r["axis"])
    if case["name"] == "capsule_inside_capsule":
        assert r["distance"] < -0.25
    if case["name"].startswith("near_parallel"):
        d1, d2 = wc[0][1] - wc[0][0], wc[1][1] - wc[1][0]
        ang = np.arcsin(np.linalg.norm(np.cross(d1, d2)) / np.linalg.norm(d1) / np.linalg.norm(d2))
        want = abs(float(case["name"].rsplit("_", 1)[1]))
        assert abs(ang - want) < 0.02 * want + 1e-6          # (the rounding of the table turns an axis by 1e-7 rad)
        # lengthwise overlap: B's ends project inside A
        for e in wc[1][:2]:
            assert 0.0 < (e - wc[0][0]) @ d1 / (d1 @ d1) < 1.0


def test_no_case_state_has_its_minimum_near_zero(oracle64, model):
    """the reference's smallest distance over the default pairs, on the 67 case states of the GPU tests: none within 1e-4 m of 0
    (the GPU tolerance is 1e-5 x the env's scale, a few 1e-5 m)"""
    bodies, caps = PR.fitted_table(model)
    pairs = PR.default_pairs(model, bodies, caps)
    mins = [min(r["distance"] for r in PR.proximity(model, s, bodies, caps, pairs)) for s, _ in case_states(oracle64, model, 67)]
    assert min(abs(m) for m in mins) > 1e-4, sorted(mins, key=abs)[:3]
    assert any(m < 0 for m in mins) and any(m > 0 for m in mins)
