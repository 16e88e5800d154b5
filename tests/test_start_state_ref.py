"""The numpy reference of the start-state randomisation (tests/start_state_ref.py) against values computed by hand, and the
properties include/trex_start_state.h promises of the draws: lo == hi is exact, a value does not depend on which other elements the
mask holds, a sharded draw is the slice of the whole, the rotation leaves |quat| = 1 and rotates the velocities with the pose.
Host-only."""
import math

import numpy as np
import pytest

import dynamics_ref as DR
import start_state_ref as SR
from sensing_ref import key_of, philox4x32, u_half_open
from start_state_ref import (BASE_ANGULAR_VELOCITY, BASE_LINEAR_VELOCITY, BASE_POSITION, BASE_RPY, FLOOR_CLEARANCE, JOINT_POSITION,
                             JOINT_VELOCITY)


@pytest.fixture(scope="module")
def slab(tmp_path_factory):
    import synthetic_models as sm
    path, props, om = sm.compile_both("slab", tmp_path_factory.mktemp("slab"))
    return om


def state_of(J, z=1.0, quat=(0, 0, 0, 1), v=(0, 0, 0), w=(0, 0, 0), q=0.0, qd=0.0):
    s = np.zeros(13 + 2 * J, np.float32)
    s[2], s[3:7], s[7:10], s[10:13], s[13:13 + J], s[13 + J:] = z, quat, v, w, q, qd
    return s


def test_hand_computed_values(slab, model):
    # lo == hi: the value is lo, whatever the draw. A quarter turn of yaw on the identity: quat (0, 0, sin 45, cos 45), v = x -> y
    terms = [(JOINT_POSITION, 0, 0, 0, 0.25, 0.25), (JOINT_VELOCITY, 0, 0, 0, -1.5, -1.5), (BASE_RPY, 0, 2, 0, math.pi / 2, math.pi / 2),
             (BASE_LINEAR_VELOCITY, 0, 2, 0, 0.5, 0.5), (BASE_POSITION, 0, 0, 0, 2.0, 2.0)]
    found = state_of(1, v=(1, 0, 0), w=(0, 0, 3), q=0.1, qd=0.5)
    for f32 in (True, False):
        a = SR.StartState(slab, 2, terms, seed=5, f32=f32).apply(np.zeros(2), np.tile(found, (2, 1)))
        assert a.first.all() and a.ep.tolist() == [1, 1]
        s = a.state[0]
        assert s[13] == (np.float32(0.1) + np.float32(0.25) if f32 else float(np.float32(0.1)) + 0.25)
        assert s[14] == 0.5 - 1.5 and s[0] == 2.0 and s[1] == 0.0 and s[2] == 1.0
        h = math.sqrt(0.5)
        assert np.abs(s[3:7] - [0, 0, h, h]).max() < 1e-6 and np.abs(s[7:10] - [0, 1, 0.5]).max() < 1e-6
        assert np.abs(s[10:13] - [0, 0, 3]).max() < 1e-6
        assert a.values[0, 0, 0] == 0.25 and a.values[0, 2, 0] == np.float32(math.pi / 2) and (a.values[:, :, 1:] == 0).all()
        assert (a.shift == 0).all() and (a.lowest == -1).all()
    # the joint limit: the slab's flap stops at 1.0
    a = SR.StartState(slab, 1, [(JOINT_POSITION, 0, 0, 0, 5.0, 5.0)], f32=True).apply([0], found[None])
    assert a.state[0, 13] == np.float32(slab["q_upper"][slab["obs_order"][0]])
    # the draw itself: counter (env_offset + e, 0, 7 << 16 | 8 t + (i >> 2), ep), output i & 3; v = lo + (hi - lo) u
    r = SR.StartState(model, 3, [(JOINT_VELOCITY, 0, 0, 0, -1.0, 3.0)], seed=2 ** 40 + 9, env_offset=100, f32=True)
    a = r.apply(np.zeros(3), np.tile(state_of(25), (3, 1)))
    for e in range(3):
        for i in (0, 3, 4, 24):
            w = philox4x32((100 + e, 0, (7 << 16) | (i >> 2), 1), key_of(2 ** 40 + 9))
            u = np.float32(u_half_open(w[i & 3]))
            assert a.values[e, 0, i] == np.float32(-1.0) + np.float32(np.float32(4.0) * u)
            assert a.state[e, 13 + 25 + i] == a.values[e, 0, i]


def test_floor_placement_by_hand(slab):
    # the slab lies flat: its lowest point ends 0.05 above the floor, whatever height it was found at
    for z in (0.3, 5.0):
        r = SR.StartState(slab, 1, [(FLOOR_CLEARANCE, 0, 0, 0, 0.05, 0.05)], floor_z=0.0)
        a = r.apply([0], state_of(1, z=z)[None])
        h = SR.point_heights(slab, a.state[0], np.float64)
        assert abs((h.min() + a.state[0, 2]) - float(np.float32(0.05))) < 1e-12 and a.lowest[0] == int(np.argmin(h))
        assert abs(a.shift[0] - (a.state[0, 2] - float(np.float32(z)))) < 1e-12 and a.gap[0] > 0


def test_lo_equal_hi_is_exact(model):
    for lo in (0.1, -3.7, 1e-30, 0.0):
        r = SR.StartState(model, 4, [(JOINT_VELOCITY, 0, 0, 0, lo, lo)], seed=3, f32=True)
        a = r.apply(np.zeros(4), np.tile(state_of(25), (4, 1)))
        assert (a.values[:, 0, :25] == np.float32(lo)).all()


def test_a_value_does_not_depend_on_the_mask(model):
    found = np.tile(state_of(25), (5, 1))
    whole = SR.StartState(model, 5, [(JOINT_POSITION, 0, 0, 0, -0.1, 0.1)], seed=8, f32=True).apply(np.zeros(5), found)
    for i in (0, 3, 4, 24):
        one = SR.StartState(model, 5, [(JOINT_POSITION, 1 << i, 0, 0, -0.1, 0.1)], seed=8, f32=True).apply(np.zeros(5), found)
        assert (one.values[:, 0, i] == whole.values[:, 0, i]).all() and (np.delete(one.values[:, 0], i, 1) == 0).all()
    shared = SR.StartState(model, 5, [(JOINT_POSITION, 0b1100, 0, 1, -0.1, 0.1)], seed=8, f32=True).apply(np.zeros(5), found)
    assert (shared.values[:, 0, 2] == whole.values[:, 0, 0]).all() and (shared.values[:, 0, 3] == whole.values[:, 0, 0]).all()


def test_a_shard_draws_the_slice_of_the_whole(model):
    terms = [(JOINT_POSITION, 0, 0, 0, -0.1, 0.1), (BASE_RPY, 0, 2, 0, -1.0, 1.0), (BASE_POSITION, 0, 1, 0, -1.0, 1.0)]
    found = np.tile(state_of(25, v=(1, 2, 3)), (12, 1))
    whole = SR.StartState(model, 12, terms, seed=4, env_offset=50, f32=True)
    part = SR.StartState(model, 5, terms, seed=4, env_offset=54, f32=True)
    for done in (np.zeros(12), (np.arange(12) % 2).astype(float)):
        a, b = whole.apply(done, found), part.apply(done[4:9], found[4:9])
        assert a.values[4:9].tobytes() == b.values.tobytes() and a.state[4:9].tobytes() == b.state.tobytes()
        assert (a.ep[4:9] == b.ep).all()


def test_the_rotation_is_rigid(model):
    terms = [(BASE_RPY, 0, 0, 0, -0.5, 0.5), (BASE_RPY, 0, 1, 0, -0.5, 0.5), (BASE_RPY, 0, 2, 0, -3.0, 3.0)]
    rng = np.random.default_rng(1)
    q0 = rng.normal(size=4)
    found = state_of(25, quat=q0 / np.linalg.norm(q0), v=(1, -2, 0.5), w=(0.3, 0.2, -1))
    a = SR.StartState(model, 9, terms, seed=6).apply(np.zeros(9), np.tile(found, (9, 1)))
    for s in a.state:
        assert abs(np.linalg.norm(s[3:7]) - 1) < 1e-12
        R = DR.quat_to_mat(s[3:7]) @ DR.quat_to_mat(found[3:7].astype(np.float64)).T       # the rotation the pose underwent
        assert np.abs(R @ found[7:10] - s[7:10]).max() < 1e-6 and np.abs(R @ found[10:13] - s[10:13]).max() < 1e-6
        assert (s[0:3] == found[0:3]).all()      # about the base origin
    # an env that does not start keeps its row; its episode count stands
    r = SR.StartState(model, 2, terms, seed=6)
    r.apply(np.zeros(2), np.tile(found, (2, 1)))
    b = r.apply([0, 1], np.tile(found, (2, 1)))
    assert b.first.tolist() == [False, True] and b.ep.tolist() == [1, 2] and (b.state[0] == found).all()
    r.reset([1, 0])
    assert r.apply([0, 0], np.tile(found, (2, 1))).ep.tolist() == [2, 2]
