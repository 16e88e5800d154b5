"""Pins tests/motion_ref.py - the f64 restatement the GPU's motion launches are compared with - without a GPU: hand-computed
answers on a two-joint synthetic model at states where the values are known, the clock rules (wrap, clamp, done rows), and the
slerp against a rotation-matrix construction."""
import numpy as np
import pytest

import dynamics_ref as R
import motion_ref as MR
import synthetic_models as sm
from oracle import trex_model as tm

TS = MR.step_seconds()
DT = 1.0 / 32.0


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


def frame(pos=(0.0, 0.0, 1.0), quat=(0, 0, 0, 1), q=(0.0, 0.0)):
    return np.concatenate([pos, quat, q]).astype(np.float64)


def table(model, frames, loop=False, velocities=None, dt=DT):
    return MR.device_table(MR.build_table(model, np.array(frames), velocities, dt, loop))


def row_of(s, reward=0.0, done=0.0):
    return np.concatenate([s[13:15], s[15:17], [0.0, 0.0], [reward, done]])


ALL = [(MR.POSE, 0, 1.0, 2.0, 0.0), (MR.VELOCITY, 0, 1.0, 0.1, 0.0), (MR.END_EFFECTOR, 0, 1.0, 40.0, 0.0),
       (MR.ROOT_POSE, 0, 1.0, 10.0, 1.0), (MR.ROOT_VELOCITY, 0, 1.0, 1.0, 1.0)]
PROBES = ([1, 2], np.array([[0.2, 0.0, 0.0], [0.2, 0.0, 0.0]]))      # the tips of the two plates


def still_clip(two, q=(0.25, 0.5)):
    """4 frames of one pose: the reference is that pose at every time, all velocities 0"""
    return table(two, [frame(q=q)] * 4)


def state_at(tab, t):
    return MR.sample(tab, t)[0].astype(np.float32).astype(np.float64)


def test_reference_equals_state_all_terms_are_one(two):
    tab = still_clip(two)
    s = state_at(tab, TS)
    v, cases = MR.evaluate(two, tab, ALL, s, row_of(s), MR.new_clock(), np.zeros(5), TS, PROBES)
    assert np.abs(v - 1.0).max() <= 1e-12
    for (kind, *_), c in zip(ALL, cases):
        assert 0 < MR.bound(kind, c) < 2e-4          # a bound of roundings, not of the value's size


def test_offset_of_a_tenth_of_a_radian(two):
    tab = still_clip(two)
    s = state_at(tab, TS)
    s[13] += 0.1
    s = s.astype(np.float32).astype(np.float64)
    d = s[13] - np.float64(np.float32(0.25))
    v, _ = MR.evaluate(two, tab, ALL, s, row_of(s), MR.new_clock(), np.zeros(5), TS, PROBES)
    assert abs(v[0] - np.exp(-2.0 * d * d)) <= 1e-15 and abs(v[0] - np.exp(-0.02)) < 1e-7
    assert v[1] == 1.0 and v[3] == 1.0 and v[4] == 1.0
    # plate "a" turns about y by d at a lever of 0.2: its tip moves by the chord 2 * 0.2 sin(d / 2); plate "b" stays
    assert abs(v[2] - np.exp(-40.0 * (0.4 * np.sin(0.5 * d)) ** 2)) <= 1e-12
    one = [(MR.POSE, 2, 1.0, 2.0, 0.0), (MR.POSE, 1, 1.0, 2.0, 0.0)]          # masks: joint 1 alone sees nothing
    v, _ = MR.evaluate(two, tab, one, s, row_of(s), MR.new_clock(), np.zeros(2), TS)
    assert v[0] == 1.0 and abs(v[1] - np.exp(-2.0 * d * d)) <= 1e-15


def test_quarter_turn_of_the_base(two):
    tab = still_clip(two)
    s = state_at(tab, TS)
    h = np.sqrt(0.5)
    s[3:7] = (0, 0, h, h)
    s[0] += 0.5
    s = s.astype(np.float32).astype(np.float64)
    spec = [(MR.ROOT_POSE, 0, 1.0, 0.5, 0.25), (MR.END_EFFECTOR, 0, 1.0, 40.0, 0.0)]
    v, _ = MR.evaluate(two, tab, spec, s, row_of(s), MR.new_clock(), np.zeros(2), TS, PROBES)
    assert abs(v[0] - np.exp(-0.5 * (0.25 + 0.25 * (np.pi / 2) ** 2))) < 1e-7      # theta = 90 degrees
    assert abs(v[1] - 1.0) <= 1e-12                         # relative to the base: its drift and its turn do not enter
    s[3:7] = (0, 0, -h, -h)                                 # the same rotation, the other sign
    v2, _ = MR.evaluate(two, tab, spec, s.astype(np.float32).astype(np.float64), row_of(s), MR.new_clock(), np.zeros(2), TS, PROBES)
    assert abs(v2[0] - v[0]) < 1e-12
    assert abs(MR.quat_angle(np.array([0, 0, 0, 1.0]), np.array([1.0, 0, 0, 0])) - np.pi) < 1e-15


def moving_clip(two, loop):
    """5 frames, T = 1/8 s: joint a from 0 to 0.4 and back to 0, the base 0.25 m along x per frame and 1 m along y in all"""
    qa = [0.0, 0.2, 0.4, 0.2, 0.0]
    return table(two, [frame(pos=(0.25 * k, 0.25 * k, 1.0), q=(qa[k], 0.5)) for k in range(5)], loop=loop)


def test_a_clock_that_wraps(two):
    tab = moving_clip(two, loop=True)
    assert tab["duration"] == 0.125 and tab["disp"].tolist() == [1.0, 1.0]
    assert MR.map_time(tab, 0.0625)[:3] == (2, 0.0, 0.0)               # on a knot: the segment that begins there
    assert MR.map_time(tab, 0.125 + 0.03125 * 1.5)[:3] == (1, 0.5, 1.0)  # second cycle, halfway between frames 1 and 2
    s, phase = MR.sample(tab, 0.125 + 0.03125 * 1.5)
    assert abs(s[13] - 0.3) < 1e-7 and s[0] == 1.0 + 0.375 and s[1] == 1.0 + 0.375 and s[2] == 1.0 and phase == 0.375
    s40, _ = MR.sample(tab, 39 * 0.125 + 0.03125)
    assert s40[0] == 39.25 and abs(s40[13] - 0.2) < 1e-7               # the 40th cycle
    # the derived velocity wraps: frame 0's neighbours are frame 3 of the cycle before and frame 1
    assert abs(tab["rows"][0, 7] - 8.0) < 1e-6 and abs(tab["rows"][0, 15]) < 1e-6 and abs(tab["rows"][4, 7] - 8.0) < 1e-6
    clock = dict(t0=0.0, k=0)
    clock["k"] = 29                                                   # 29 Ts = 0.6041..: cycle 4, 0.1041.. into it
    k, u, cycles, _ = MR.map_time(tab, MR.clock_time(clock, TS))
    assert cycles == 4.0 and k == 3 and abs(u - (29 * TS - 0.5 - 0.09375) * 32) < 1e-5


def test_a_clamp_past_the_end(two):
    tab = moving_clip(two, loop=False)
    end, phase = MR.sample(tab, 10.0)
    assert (end == tab["rows"][4]).all() and phase == 1.0              # the last frame, velocities and all
    assert MR.map_time(tab, 10.0)[:3] == (3, 1.0, 0.0)
    start, phase = MR.sample(tab, -3.0)
    assert (start == tab["rows"][0]).all() and phase == 0.0 and MR.map_time(tab, float("nan"))[:2] == (0, 0.0)
    # open ends: one-sided differences
    assert abs(tab["rows"][0, 15] - 0.2 * 32) < 1e-5 and abs(tab["rows"][4, 15] + 0.2 * 32) < 1e-5


def test_done_rows_and_the_clock(two):
    tab = moving_clip(two, loop=False)
    spec = [(MR.POSE, 0, 1.0, 2.0, 0.0)]
    clock, held = MR.new_clock(), np.zeros(1)
    s = state_at(tab, 0.0)
    v, cases = MR.evaluate(two, tab, spec, s, row_of(s, done=1.0), clock, held, TS)
    assert v[0] == 0.0 and cases[0]["held"] and MR.bound(MR.POSE, cases[0]) == 0.0 and clock == dict(t0=0.0, k=0)   # no step before
    v1, _ = MR.evaluate(two, tab, spec, s, row_of(s), clock, held, TS)
    assert clock["k"] == 1 and held[0] == v1[0] and 0 < v1[0] < 1       # the reference has moved on by Ts, the state has not
    want = np.exp(-2.0 * MR.sample(tab, TS)[0][13] ** 2)
    assert abs(v1[0] - want) < 1e-12
    v2, _ = MR.evaluate(two, tab, spec, s, row_of(s, done=1.0), clock, held, TS)
    assert v2[0] == v1[0] and held[0] == 0.0 and clock == dict(t0=0.0, k=0)
    clock.update(t0=0.0625, k=0)                                      # what RSI at frame 2 leaves
    MR.evaluate(two, tab, spec, s, row_of(s), clock, held, TS)
    assert clock == dict(t0=0.0625, k=1) and abs(MR.clock_time(clock, TS) - (0.0625 + TS)) < 1e-8


def test_slerp_against_rotation_matrices(two):
    rng = np.random.default_rng(3)
    for angle in (np.radians(179.0), 1.0, np.radians(0.01), 0.0):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = rng.normal(size=4)
        a /= np.linalg.norm(a)
        b = MR.quat_mul(np.concatenate([axis * np.sin(0.5 * angle), [np.cos(0.5 * angle)]]), a)
        for u in (0.0, 0.25, 0.5, 1.0):
            want = R.axis_angle_mat(axis, u * angle) @ R.quat_to_mat(a)
            for end in (b, -b):                                       # shortest arc: the sign of an end does not matter
                got = MR.slerp(a, end, u)
                assert abs(np.linalg.norm(got) - 1) < 1e-12
                # (the normalised lerp of ends 0.01 degrees apart is off the arc by less than angle^3)
                assert np.abs(R.quat_to_mat(got) - want).max() < 1e-12 + angle ** 3 * (angle < 0.04)


def test_builder_hemisphere_and_normalisation(two):
    h = np.sqrt(0.5)
    frames = [frame(), frame(quat=(0, 0, -2 * np.sin(0.1), -2 * np.cos(0.1))), frame(quat=(0, 0, h, h))]
    tab = MR.build_table(two, np.array(frames), None, DT, False)
    quat = tab["rows"][:, 3:7]
    assert np.abs(quat[1] - [0, 0, np.sin(0.1), np.cos(0.1)]).max() < 1e-15
    assert abs(tab["rows"][1, 12] - (np.pi / 2) / (2 * DT)) < 1e-9     # yaw rate: a quarter turn over two frames
    assert MR.refusal(two, np.array([frame(q=(1.0 + 2e-6, 0.0)), frame()]), None, DT) == "outside its limits"
    assert MR.refusal(two, np.array([frame(q=(1.0 + 5e-7, 0.0)), frame()]), None, DT) is None
    prod, total = MR.compose([(0, 0, 0.5, 1, 0), (1, 0, 2.0, 1, 0)], [1.0, 0.25], -3.0, 0.5)
    assert list(prod) == [0.5, 0.5] and total == -0.5 and prod.dtype == np.float32
