"""Pins tests/reward_ref.py - the f64 restatement the GPU's reward terms are compared with - without a GPU: hand-computed answers
on a two-joint synthetic model, the values the table of include/trex_reward.h names at states where they are known, and the history
rules (air time, done rows, the first step of an episode)."""
import numpy as np
import pytest

import reward_ref as RR
import synthetic_models as sm
from oracle import trex_model as tm

Z = (0.0, 0.0, 0.0)
TS = RR.step_seconds()


@pytest.fixture(scope="module")
def two(tmp_path_factory):
    """a box with two hinged plates, both about y: joints "a" (limits -1 .. 1) and "b" (-0.5 .. 2)"""
    b = sm.Builder(tmp_path_factory.mktemp("two_joint"), "two_joint")
    half = (0.2, 0.1, 0.05)
    rng = np.random.default_rng(7)
    b.link("root", 3.0, half, hulls=[(sm.box_verts(rng, half), (0, 0, 0), (0, 0, 0))])
    for name, x, lo, hi in (("a", 0.2, -1.0, 1.0), ("b", -0.2, -0.5, 2.0)):
        b.link("plate_" + name, 1.0, (0.1, 0.05, 0.02), com=(0.1, 0, 0), hulls=[(sm.box_verts(rng, (0.1, 0.05, 0.02)), (0.1, 0, 0), (0, 0, 0))])
        b.joint(name, "root", "plate_" + name, xyz=(x, 0, 0), axis=(0, 1, 0), lower=lo, upper=hi)
    m = tm.compile_model(b.write())
    assert m["nb"] == 3 and list(m["obs_order"]) == [1, 2]
    return m


def state(q=(0.0, 0.0), qd=(0.0, 0.0), z=1.0, quat=(0, 0, 0, 1), v=(0, 0, 0), w=(0, 0, 0)):
    return np.concatenate([[0.0, 0.0, z], quat, v, w, q, qd]).astype(np.float64)


def row_of(s, tau=(0.0, 0.0), reward=0.0, done=0.0):
    return np.concatenate([s[13:15], s[15:17], tau, [reward, done]])


def run(model, spec, s, row=None, hist=None, **kw):
    hist = RR.new_history(len(spec), 2, 2) if hist is None else hist
    v, cases = RR.evaluate(model, spec, s, row_of(s) if row is None else row, hist, TS, **kw)
    return v, cases, hist


def term(kind, weight=1.0, link=0, mask=0, xyz=Z, p0=0.0, p1=0.0):
    return (kind, link, mask, xyz, weight, p0, p1)


def test_hand_computed_joint_sums(two):
    s = state(q=(0.5, -0.25), qd=(2.0, -4.0))
    row = row_of(s, tau=(3.0, 0.5), reward=-1.5)
    spec = [term(RR.STEP), term(RR.ALIVE), term(RR.TORQUE), term(RR.TORQUE, mask=2), term(RR.JOINT_VEL), term(RR.POWER),
            term(RR.JOINT_POSE, mask=1), term(RR.JOINT_VEL, mask=1)]
    v, cases, _ = run(two, spec, s, row)
    assert list(v) == [-1.5, 1.0, 9.25, 0.25, 20.0, 8.0, 0.25, 4.0]
    assert [c.get("n") for c in cases[2:]] == [2, 1, 2, 2, 1, 1]
    prod, total = RR.compose([term(RR.STEP, 2.0), term(RR.ALIVE, 0.5)], [-1.5, 1.0])
    assert list(prod) == [-3.0, 0.5] and total == -2.5 and prod.dtype == np.float32
    assert list(RR.ordered_sum(np.array([[1.0, 2.0, 4.0], [0.5, 0.25, 0.0]], np.float32))) == [7.0, 0.75]


def test_orientation_upright_and_on_its_side(two):
    spec = [term(RR.ORIENTATION)]
    assert run(two, spec, state())[0][0] == 0.0
    h = np.sqrt(0.5)
    assert abs(run(two, spec, state(quat=(h, 0, 0, h)))[0][0] - 1.0) <= 1e-15          # rolled a quarter turn
    assert abs(run(two, spec, state(quat=(0, h, 0, h)))[0][0] - 1.0) <= 1e-15          # pitched a quarter turn
    assert abs(run(two, spec, state(quat=(0, 0, h, h)))[0][0]) <= 1e-15                # yawed: still upright


def test_tracking_is_one_at_the_command(two):
    s = state(v=(0.5, -0.25, 0.125), w=(0.0, 0.0, 0.75))
    spec = [term(RR.TRACK_LIN, p0=0.25), term(RR.TRACK_ANG, p0=0.25), term(RR.LIN_VEL_Z), term(RR.ANG_VEL_XY)]
    v, cases, _ = run(two, spec, s, command=(0.5, -0.25, 0.75))
    assert list(v) == [1.0, 1.0, 0.125 ** 2, 0.0]
    v, _, _ = run(two, spec, s, command=(0.0, -0.25, 0.25))
    assert abs(v[0] - np.exp(-1.0)) <= 1e-15 and abs(v[1] - np.exp(-1.0)) <= 1e-15
    assert RR.bound(RR.TRACK_LIN, cases[0]) > 0 and RR.bound(RR.LIN_VEL_Z, cases[2]) > 0


def test_heights(two):
    s = state(z=0.75)
    v, _, _ = run(two, [term(RR.BASE_HEIGHT, p0=0.5), term(RR.POINT_HEIGHT, link=1, xyz=(0.125, 0.0, 0.25), p0=0.0)], s)
    assert abs(v[0] - (0.75 - RR.FLOOR_Z - 0.5) ** 2) <= 1e-15
    assert abs(v[1] - (0.75 + 0.25 - RR.FLOOR_Z) ** 2) <= 1e-15


def test_joint_limit_zero_inside_linear_outside(two):
    """soft = 0.5: joint a (-1 .. 1) is free in -0.5 .. 0.5, joint b (-0.5 .. 2) in 0.125 .. 1.375"""
    spec = [term(RR.JOINT_LIMIT, p0=0.5)]
    for q in ((0.0, 0.75), (0.5, 0.125), (-0.5, 1.375)):
        assert run(two, spec, state(q=q))[0][0] == 0.0
    assert abs(run(two, spec, state(q=(0.75, 0.75)))[0][0] - 0.25) <= 1e-15
    assert abs(run(two, spec, state(q=(1.0, 0.75)))[0][0] - 0.5) <= 1e-15
    assert abs(run(two, spec, state(q=(-0.75, 1.5)))[0][0] - (0.25 + 0.125)) <= 1e-15
    assert run(two, [term(RR.JOINT_LIMIT, p0=1.0)], state(q=(1.0, -0.5)))[0][0] == 0.0
    assert abs(run(two, [term(RR.JOINT_LIMIT, p0=0.5, mask=2)], state(q=(0.75, 0.0)))[0][0] - 0.125) <= 1e-15


def test_air_time_fly_fly_land(two):
    foot = 1                                                  # URDF link of plate_a
    body = int(two["link_body"][foot])
    spec = [term(RR.FOOT_AIR_TIME, link=foot, p0=1.0, p1=0.01), term(RR.CONTACT_COUNT, mask=1 << body, p0=1.0)]
    air, floor = np.zeros((3, 3)), np.zeros((3, 3))
    floor[body] = (0.0, 0.0, 5.0)
    s, hist, got = state(), None, []
    for f in (air, air, floor, floor, air, floor):
        v, _, hist = run(two, spec, s, hist=hist, force=f)
        got.append(tuple(v))
    p1 = float(np.float32(0.01))
    want = [(0.0, 0.0), (0.0, 0.0), (2 * TS - p1, 1.0), (0.0, 1.0), (0.0, 0.0), (TS - p1, 1.0)]
    assert np.abs(np.array(got) - np.array(want, np.float64)).max() <= 1e-15


def test_foot_slip_needs_contact(two):
    foot = 1
    body = int(two["link_body"][foot])
    s = state(v=(0.5, -1.0, 3.0))
    f = np.zeros((3, 3))
    spec = [term(RR.FOOT_SLIP, link=foot, p0=1.0)]
    assert run(two, spec, s, force=f)[0][0] == 0.0
    f[body, 2] = 2.0
    assert abs(run(two, spec, s, force=f)[0][0] - 1.25) <= 1e-15


def test_done_row_holds_and_invalidates(two):
    spec = [term(RR.STEP), term(RR.JOINT_VEL), term(RR.JOINT_ACC), term(RR.ACTION_RATE), term(RR.FOOT_AIR_TIME, link=1, p0=1.0)]
    f = np.zeros((3, 3))
    s1, s2 = state(qd=(1.0, 2.0)), state(qd=(1.5, 2.0))
    v1, _, hist = run(two, spec, s1, action=(0.0, 0.0), force=f)
    assert list(v1) == [0.0, 5.0, 0.0, 0.0, 0.0]                              # the first step: no rate terms
    v2, _, hist = run(two, spec, s2, hist=hist, action=(0.5, 0.0), force=f)
    assert np.abs(v2 - [0.0, 6.25, (0.5 / TS) ** 2, 0.25, 0.0]).max() <= 1e-9 and hist["timer"][4] == 2 * TS
    # the episode ends: the row's state is the new episode's - everything but STEP repeats, the history is invalid afterwards
    v3, cases, hist = run(two, spec, state(qd=(9.0, 9.0)), row=row_of(state(qd=(9.0, 9.0)), reward=-7.0, done=1.0), hist=hist,
                          action=(3.0, 3.0), force=f)
    assert list(v3) == [-7.0] + list(v2[1:]) and hist["valid"] == 0 and (hist["timer"] == 0).all()
    assert all(RR.bound(k, c) == 0.0 for k, c in zip([t[0] for t in spec], cases))
    v4, _, hist = run(two, spec, s1, hist=hist, action=(1.0, 1.0), force=f)
    assert list(v4) == [0.0, 5.0, 0.0, 0.0, 0.0] and hist["valid"] == 1 and hist["timer"][4] == TS
    RR.reset_history(hist)
    assert hist["valid"] == 0 and (hist["held"] == 0).all() and (hist["timer"] == 0).all()


def test_table_of_a_specification(two):
    spec = [term(RR.TORQUE), term(RR.POWER, mask=2), term(RR.FOOT_SLIP, link=2, xyz=(0.1, 0.0, 0.0), p0=1.0),
            term(RR.CONTACT_COUNT, mask=6, p0=1.0), term(RR.TRACK_ANG, p0=0.5), term(RR.ACTION_RATE)]
    t = RR.reward_table(two, spec)
    assert list(t["mask"]) == [3, 2, 0, 6, 0, 0] and list(t["joint_body"][:3]) == [1, 2, 0]
    assert t["body"][2] == int(two["link_body"][2]) and t["body_mask"] == 1 << int(two["link_body"][2])
    assert t["contact"] and t["actions"] and t["command"]
