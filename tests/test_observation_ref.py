"""Pins tests/observation_ref.py - the f64 restatement the composed observation rows of the GPU are compared with - without a GPU:
the gravity channel is a unit vector and, at the start pose, (0, 0, -1) turned by the start orientation; the heights there are the
start height above the floor; the point channels are link_state_ref's values in base axes; widths, scales, pass-through and the
copied channels behave as include/trex_batch.h says."""
import numpy as np
import pytest

import dynamics_ref as R
import link_state_ref as L
import observation_ref as OR
from oracle import trex_model as tm

J = 25
Z = (0.0, 0.0, 0.0)


def start_state(model):
    """get_state()'s vector of the reset pose, before any settling: start position and orientation, start angles, at rest"""
    oo = model["obs_order"]
    return np.concatenate([model["base_start_pos"], model["base_start_quat"], np.zeros(6), model["q_start"][oo], np.zeros(J)])


@pytest.fixture(scope="module")
def states(model):
    rs, _ = R.random_states(model, 6)
    return [np.asarray(s, np.float64) for s in rs]


def links_of(model):
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    toe = [l for l in range(len(names)) if "toe" in names[l]][0]
    deepest = [l for l in range(len(names)) if lb[l] == int(np.argmax(model["depth"]))][0]
    return toe, deepest


def test_gravity_is_a_unit_vector(model, states):
    """to 1e-6 on these states, whose quaternions are f32 values: |q|^2 - 1 is up to 4 x 2^-24 = 2.4e-7, and the rotation matrix
    of a quaternion that is not quite unit has rows of norm 1 + 2 (|q|^2 - 1) at most; to 1e-12 once the quaternion is normalised"""
    for s in states:
        g = OR.channels(model, s, [(OR.GRAVITY, 0, Z, 1.0)])
        assert g.shape == (3,) and abs(np.linalg.norm(g) - 1.0) <= 1e-6
        unit = s.copy()
        unit[3:7] /= np.linalg.norm(unit[3:7])
        assert abs(np.linalg.norm(OR.channels(model, unit, [(OR.GRAVITY, 0, Z, 1.0)])) - 1.0) <= 1e-12
        assert np.abs(OR.channels(model, s, [(OR.GRAVITY, 0, Z, -2.5)]) + 2.5 * g).max() <= 1e-15


def test_known_values_at_the_start_pose(model):
    s = start_state(model)
    R0 = tm.quat_to_matrix(model["base_start_quat"]) @ np.asarray(model["link_tf"], np.float64).reshape(-1, 12)[0][:9].reshape(3, 3)
    spec = [(OR.GRAVITY, 0, Z, 1.0), (OR.BASE_HEIGHT, 0, Z, 1.0), (OR.BASE_LIN, 0, Z, 1.0), (OR.BASE_ANG, 0, Z, 1.0)]
    got = OR.channels(model, s, spec)
    assert np.abs(got[:3] - R0.T @ [0.0, 0.0, -1.0]).max() <= 1e-15
    if int(model["link_body"][0]) == 0 and np.abs(np.asarray(model["link_tf"], np.float64).reshape(-1, 12)[0][9:]).max() == 0:
        assert abs(got[3] - (model["base_start_pos"][2] - tm.default_params()["floor_z"])) <= 1e-15
    assert (got[4:] == 0).all()                                  # at rest
    assert OR.FLOOR_Z == tm.default_params()["floor_z"]


def test_point_channels_are_link_state_in_base_axes(model, states):
    toe, deepest = links_of(model)
    pts = {toe: (0.1, -0.2, 0.3), deepest: (0.05, 0.0, -0.02), 0: (0.0, 0.0, 0.0)}
    for s in states:
        for link, p in pts.items():
            p32 = np.asarray(p, np.float32).astype(np.float64)
            rb = L.link_state(model, s, [link], [p32], axes="base")
            rw = L.link_state(model, s, [link], [p32], axes="world")
            got = OR.channels(model, s, [(OR.POINT_POS, link, p, 1.0), (OR.POINT_VEL, link, p, 3.0), (OR.POINT_HEIGHT, link, p, 1.0)])
            assert np.abs(got[0:3] - rb["position"][0]).max() <= 1e-15
            assert np.abs(got[3:6] - 3.0 * rb["linear_velocity"][0]).max() <= 1e-13
            assert abs(got[6] - (rw["position"][0][2] - OR.FLOOR_Z)) <= 1e-15
        # the base link's own origin: the origin of the base axes, moving with the base velocities
        base = OR.channels(model, s, [(OR.POINT_POS, 0, Z, 1.0), (OR.POINT_VEL, 0, Z, 1.0), (OR.BASE_LIN, 0, Z, 1.0)])
        assert np.abs(base[:3]).max() <= 1e-15 and np.abs(base[3:6] - base[6:9]).max() <= 1e-15


def test_base_velocities_are_the_state_in_base_axes(model, states):
    """URDF link 0 belongs to the base body: its angular velocity is the state's, turned into its axes; so is the linear
    velocity once the lever arm to the link's origin is added"""
    assert int(model["link_body"][0]) == 0
    tf0 = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)[0]
    for s in states:
        R0 = tm.quat_to_matrix(s[3:7]) @ tf0[:9].reshape(3, 3)
        d = tm.quat_to_matrix(s[3:7]) @ tf0[9:]
        got = OR.channels(model, s, [(OR.BASE_LIN, 0, Z, 1.0), (OR.BASE_ANG, 0, Z, 1.0)])
        assert np.abs(got[:3] - R0.T @ (s[7:10] + np.cross(s[10:13], d))).max() <= 1e-13
        assert np.abs(got[3:] - R0.T @ s[10:13]).max() <= 1e-13


def test_copied_channels_and_row_layout(model, states):
    toe, _ = links_of(model)
    spec = [(OR.EXTERNAL, 3, Z, 1.0), (OR.PREV_ACTION, 0, Z, 1.0), (OR.CONTACT, toe, Z, 0.5), (OR.EXTERNAL, 2, Z, -1.0)]
    assert OR.extra_dim(spec, J) == 3 + J + 1 + 2 and OR.columns(spec, J) == [(0, 3), (3, J), (3 + J, 1), (4 + J, 2)]
    rng = np.random.default_rng(0)
    act, ext, fz = rng.normal(size=J) * 5, rng.normal(size=5), rng.normal(size=model["nb"])
    row = rng.normal(size=3 * J + 5)
    for done in (0.0, 1.0):
        row[3 * J + 1] = done
        out = OR.compose(model, states[0], spec, row, 5, action=act, extern=ext, contact_fz=fz)
        assert out.shape == (3 * J + 31 + 5,)
        assert (out[:3 * J] == row[:3 * J]).all() and (out[-5:] == row[3 * J:]).all()
        ch = out[3 * J:-5]
        assert (ch[:3] == ext[:3]).all() and (ch[-2:] == -ext[3:]).all()
        assert (ch[3:3 + J] == (0 if done else act)).all()
        assert ch[3 + J] == 0.5 * fz[int(model["link_body"][toe])]
    none = OR.compose(model, states[0], spec, row, 2, action=None, extern=ext, contact_fz=fz)
    assert (none[3 * J + 3:3 * J + 3 + J] == 0).all() and len(none) == 3 * J + 31 + 2
