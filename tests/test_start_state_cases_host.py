"""The cases of tests/start_state_cases.py, qualified on the reference and the oracle alone: in every floor-placement case the two
lowest candidate points differ by more than the comparison bound of the heights, so the deciding point is unambiguous and the f32
and f64 runs name the same one; after the placement no point of the reference state lies below floor_z; every case starts every
env at its first apply and a third of them at its second; the joint limit is reached where a case means to reach it; and the
reference's f32 run passes the comparison a device run has to pass. Host-only."""
import numpy as np
import pytest

import start_state_cases as SC
import start_state_ref as SR
from start_state_ref import FLOOR_CLEARANCE, JOINT_POSITION


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return SC.build(tmp_path_factory.mktemp("start_state_models"))


@pytest.fixture(scope="module")
def runs(built):
    """{case name: (case, found, (one32, two32), (one64, two64))}, computed once"""
    out = {}
    for case in SC.cases(built):
        b = built[case.model]
        found = SC.found_state(b)
        out[case.name] = (case, found, SC.reference(case, b, found, True), SC.reference(case, b, found, False))
    return out


def test_the_models_are_the_ones_named(built):
    for name in SC.MODELS:
        assert built[name].om["nb"] == SC.NB[name]
    assert len(np.asarray(built["trex_primitives"].om["hull_radius"]).nonzero()[0]) > 0      # points with a radius
    assert not np.asarray(built["trex"].om["hull_radius"]).any()


def test_every_case_qualifies(built, runs):
    names = set()
    for name, (case, found, r32, r64) in runs.items():
        names.add(name)
        b = built[case.model]
        fz = SC.floor_z(b)
        for a32, a64 in zip(r32, r64):
            assert np.array_equal(a32.first, a64.first) and a32.first.any()
            bound = SC.bounds(a32, a64, case)
            if SC.has(case, FLOOR_CLEARANCE):
                f = a64.first
                assert (a64.lowest[f] >= 0).all() and np.array_equal(a32.lowest, a64.lowest), name
                assert a64.gap[f].min() > 2 * bound["z"], (name, a64.gap[f].min(), bound["z"])     # unambiguous on either side of the bound
                for e in np.flatnonzero(f):
                    h = SR.point_heights(b.om, a64.state[e], np.float64) + a64.state[e, 2]
                    assert h.min() >= fz and abs(h.min() - fz - a64.values[e, [t[0] for t in case.terms].index(FLOOR_CLEARANCE), 0]) < 1e-9
            else:
                assert (a64.lowest == -1).all() and (a64.shift == 0).all()
        assert r32[0].first.all() and np.array_equal(r32[1].first, SC.done_flags(case) != 0)
        assert (r32[1].ep == 1 + (SC.done_flags(case) != 0)).all()
    assert len(names) == len(runs) == 15


def test_the_joint_limit_is_reached(built, runs):
    case, found, r32, _ = runs["trex_n65_masks"]
    om = built["trex"].om
    slot = SC.last_slot(om)
    q = r32[0].state[:, 13 + slot]
    lo, hi = np.float32(om["q_lower"][om["nb"] - 1]), np.float32(om["q_upper"][om["nb"] - 1])
    assert (q == lo).any() and (q == hi).any() and ((q > lo) & (q < hi)).any()


def test_the_f32_run_passes_its_own_comparison(runs):
    for name, (case, found, r32, r64) in runs.items():
        rows = np.tile(found, (case.n, 1))
        for a32, a64 in zip(r32, r64):
            out = SC.compare(case, a32, a64, rows, a32.state, a32.values, a32.shift, a32.lowest)
            assert not out["failures"], (name, out["failures"])
            assert max(out["share"].values()) <= 0.25 + 1e-12
            rows = a32.state.astype(np.float32)
        # and a run whose quaternion is the found one's fails it
        a32, a64 = r32[0], r64[0]
        if SC.has(case, SR.BASE_RPY):
            wrong = a32.state.copy()
            wrong[:, 3:7] = found[3:7]
            assert SC.compare(case, a32, a64, np.tile(found, (case.n, 1)), wrong, a32.values, a32.shift, a32.lowest)["failures"]
