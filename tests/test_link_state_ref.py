"""Pins tests/link_state_ref.py - the f64 restatement the GPU link kinematics are compared with - without a GPU: its velocity to
dynamics_ref.jacobian, its acceleration to CENTRAL DIFFERENCES of its own velocity, `proper` to (0, 0, g) at rest, and the LINK
and BASE axes to rotations of the WORLD values; on the T-rex and on the depth-6 / oblique-axis / merged-link generated models.
It also checks that the library and the Python surface carry the query at all.

Central difference: the two states are advanced by +-h exactly (link_state_ref.advance), h = 1e-5 s. Tolerance
1e-6 x max(1, |a|_inf): truncation h^2 x jerk / 6 ~ 1e-8, round-off ~ 1e-16 |v| / h ~ 1e-11 on these states - a miss is a bug in
the reference, not a tolerance to widen."""
import numpy as np
import pytest

import dynamics_ref as R
import link_state_ref as L
import synthetic_models as sm
from state_sets import landing_states

G = 9.81
H = 1e-5
FD_TOL = 1e-6
POINT = (0.3, -0.2, 0.1)


def pick_links(model):
    """name -> link: the base, the head, the deepest link and - where the model has them - a toe and a link merged into its body
    across a fixed joint whose link_tf is not the identity"""
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    tf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)
    ident = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    out = dict(base=0, head=[l for l in range(len(names)) if lb[l] == int(model["head_body"])][0],
               deepest=[l for l in range(len(names)) if lb[l] == int(np.argmax(model["depth"]))][0])
    toes = [l for l in range(len(names)) if "toe" in names[l]]
    if toes:
        out["toe"] = toes[0]
    merged = [l for l in range(len(names)) if np.abs(tf[l] - ident).max() > 1e-3 and np.abs(tf[l][:9] - ident[:9]).max() > 1e-3]
    merged = merged or [l for l in range(len(names)) if np.abs(tf[l] - ident).max() > 1e-3]
    if merged:
        out["merged"] = merged[-1]
    return out


@pytest.fixture(scope="module")
def suites(oracle64, model, tmp_path_factory):
    """name -> (model dict, [state f64], {link name: link}): T-rex (landing + airborne states), deep_chain, bushy"""
    ls, _ = landing_states(oracle64, model)
    rs, _ = R.random_states(model, 4)
    out = dict(trex=(model, [s.astype(np.float64) for s in ls[:3]] + rs, pick_links(model)))
    for n in ("deep_chain", "bushy"):
        _, _, om = sm.compile_both(n, tmp_path_factory.mktemp(n))
        st, _ = R.random_states(om, 4, seed=31)
        out[n] = (om, st, pick_links(om))
    assert "toe" in out["trex"][2] and "merged" in out["trex"][2] and "merged" in out["bushy"][2]
    assert out["deep_chain"][0]["depth"].max() == 6 and out["bushy"][0]["depth"].max() == 6
    return out


def probes_of(links):
    """every picked link at its origin and at POINT"""
    ll = [l for l in links.values() for _ in range(2)]
    pts = [p for _ in links for p in ((0.0, 0.0, 0.0), POINT)]
    return ll, pts


def gen_velocity(om, s):
    J = om["nb"] - 1
    return np.concatenate([s[7:13], s[13 + J:13 + 2 * J]])


@pytest.mark.parametrize("name", ["trex", "deep_chain", "bushy"])
def test_velocity_is_the_jacobian_times_the_generalised_velocity(name, suites):
    om, states, links = suites[name]
    ll, pts = probes_of(links)
    for s in states:
        r = L.link_state(om, s, ll, pts)
        for k, (l, p) in enumerate(zip(ll, pts)):
            want = R.jacobian(om, s, l, p) @ gen_velocity(om, s)
            got = np.concatenate([r["linear_velocity"][k], r["angular_velocity"][k]])
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (name, l, p)


@pytest.mark.parametrize("with_accel", [False, True])
@pytest.mark.parametrize("name", ["trex", "deep_chain", "bushy"])
def test_acceleration_is_the_central_difference_of_the_velocity(name, with_accel, suites):
    om, states, links = suites[name]
    ll, pts = probes_of(links)
    rng = np.random.default_rng(5)
    for s in states:
        a = R.random_tau(om, s, None, rng, with_accel=True)[1] if with_accel else None
        r = L.link_state(om, s, ll, pts, accel=a)
        vp = L.velocity_array(L.link_state(om, L.advance(om, s, a, +H), ll, pts))
        vm = L.velocity_array(L.link_state(om, L.advance(om, s, a, -H), ll, pts))
        fd, got = (vp - vm) / (2 * H), L.acceleration_array(r)
        err = np.abs(got - fd).max(1)
        for k in range(len(ll)):
            assert err[k] <= FD_TOL * max(1.0, np.abs(got[k]).max()), (name, ll[k], pts[k], err[k], got[k])


def test_pose_is_the_oracles_body_pose_composed_with_link_tf(oracle64, model, suites):
    om, states, links = suites["trex"]
    ll, pts = probes_of(links)
    for s in states:
        os_ = oracle64.new_state()
        oracle64.set_state(os_, s)
        pos, rot = oracle64.body_poses(os_)
        r = L.link_state(om, s, ll, pts)
        for k, (l, p) in enumerate(zip(ll, pts)):
            bb, tf = om["link_body"][l], om["link_tf"][l]
            Rl = rot[bb] @ tf[:9].reshape(3, 3)
            pl = pos[bb] + rot[bb] @ tf[9:12] + Rl @ np.asarray(p)
            assert np.abs(r["position"][k] - pl).max() < 1e-9 and np.abs(r["rotation"][k] - Rl).max() < 1e-9
            # (the airborne states carry f32-rounded base quaternions, unit to 2^-23 only: Rl is orthonormal to a few 1e-7, and
            # that far a unit quaternion can follow it)
            assert np.abs(R.quat_to_mat(r["orientation"][k]) - Rl).max() < 1e-6 and r["orientation"][k][3] >= 0
            assert abs(np.linalg.norm(r["orientation"][k]) - 1) < 1e-6


@pytest.mark.parametrize("name", ["trex", "bushy"])
def test_proper_at_rest_is_g_up(name, suites):
    om, states, links = suites[name]
    ll, pts = probes_of(links)
    J = om["nb"] - 1
    for s in states:
        s = s.copy()
        s[7:13] = 0
        s[13 + J:] = 0
        r = L.link_state(om, s, ll, pts, proper=True)
        assert np.abs(r["linear_acceleration"] - [0, 0, G]).max() < 1e-12 and np.abs(r["angular_acceleration"]).max() == 0
        assert np.abs(L.link_state(om, s, ll, pts)["linear_acceleration"]).max() < 1e-12
        rl = L.link_state(om, s, ll, pts, proper=True, axes="link")
        want = np.einsum("kji,j->ki", r["rotation"], [0, 0, G])
        assert np.abs(rl["linear_acceleration"] - want).max() < 1e-12


@pytest.mark.parametrize("proper", [False, True])
@pytest.mark.parametrize("name", ["trex", "deep_chain", "bushy"])
def test_link_and_base_axes_are_rotations_of_world(name, proper, suites):
    om, states, links = suites[name]
    ll, pts = probes_of(links)
    rng = np.random.default_rng(6)
    keys = ("linear_velocity", "angular_velocity", "linear_acceleration", "angular_acceleration")
    for s in states:
        a = R.random_tau(om, s, None, rng, with_accel=True)[1]
        w = L.link_state(om, s, ll, pts, a, "world", proper)
        lk = L.link_state(om, s, ll, pts, a, "link", proper)
        bs = L.link_state(om, s, ll, pts, a, "base", proper)
        b0 = L.link_state(om, s, [0], None)
        R0, p0 = b0["rotation"][0], b0["position"][0]
        # (components in a frame = R^T v; the frames' rotations are orthonormal only as far as the state's base quaternion is a
        # unit one - 1e-7 for the f32-rounded airborne states - so the check applies R^T and compares lengths that far)
        for key in keys:
            tol = 1e-13 * max(1.0, np.abs(w[key]).max())
            assert np.abs(lk[key] - np.einsum("kji,kj->ki", w["rotation"], w[key])).max() < tol
            assert np.abs(bs[key] - w[key] @ R0).max() < tol
            for r in (lk, bs):
                nw = np.linalg.norm(w[key], axis=1)
                assert np.abs(np.linalg.norm(r[key], axis=1) - nw).max() < 1e-6 * max(1.0, nw.max())
        assert np.array_equal(lk["position"], w["position"]) and np.array_equal(lk["rotation"], w["rotation"])
        assert np.abs(bs["position"] - (w["position"] - p0) @ R0).max() < 1e-13
        assert np.abs(bs["rotation"] - R0.T @ w["rotation"]).max() < 1e-13
        # the base link seen from itself: the identity pose
        kb = [k for k, l in enumerate(ll) if l == 0 and pts[k] == (0.0, 0.0, 0.0)][0]
        assert np.abs(bs["position"][kb]).max() < 1e-12 and np.abs(bs["rotation"][kb] - np.eye(3)).max() < 1e-6


def test_library_and_python_surface_carry_the_query():
    from trex_gym import _capi, sensors, trex_env, vec_env
    for sym in ("trex_batch_set_link_probes", "trex_batch_link_state"):
        assert sym in _capi.SYMBOLS and hasattr(_capi.lib, sym)
    for cls in (vec_env.TrexVecEnv, trex_env.TrexBulletEnv):
        assert callable(cls.link_state) and callable(cls.bias_acceleration)
    assert callable(vec_env.TrexVecEnv.link_probes) and callable(_capi.Batch.set_link_probes) and callable(_capi.Batch.link_state)
    assert callable(sensors.Imu.read) and callable(sensors.Imu.static)
    assert vec_env.LinkState._fields == ("position", "orientation", "linear_velocity", "angular_velocity", "linear_acceleration",
                                         "angular_acceleration")
