"""Ties tests/dynamics_ref.py - the f64 restatement the GPU dynamics queries are compared with - to the frozen CPU oracle:
its M^-1, its forward dynamics, its energy / momentum and its body poses; and checks that the library and the Python surface
carry the queries at all. f64 against f64: 1e-8 relative to the largest entry compared, except the Jacobian, which is compared
with CENTRAL DIFFERENCES of the oracle's poses (step 1e-6: truncation ~ h^2 |d3x| ~ 1e-11, rounding ~ 1e-16 |x| / h ~ 1e-9 on
positions of a few metres - so 1e-7 there; the loosening the finite-difference step demands, no more)."""
import ctypes as C

import numpy as np
import pytest

import dynamics_ref as R
from state_sets import landing_states, oracle_state

TOL = 1e-8
G = 9.81


@pytest.fixture(scope="module")
def cases(oracle64, model):
    """(state f64, mass scale or None): the landing states and 8 random airborne ones, two of them with a mass scale"""
    ls, _ = landing_states(oracle64, model)
    out = [(s.astype(np.float64), None) for s in ls]
    out += list(zip(*R.random_states(model, 8)))
    return out


def test_velocity_order_against_oracle_get_state(oracle64, model):
    """the permutation of the header: oracle [w, v, joints in body order] <-> here [v, w, joints in observation order]"""
    s = oracle64.new_state()
    st = np.arange(13 + 50, dtype=np.float64) + 1.0
    oracle64.set_state(s, st)
    assert np.array_equal(oracle64.get_state(s), st)
    p = R.perm_to_oracle(model)
    assert sorted(p) == list(range(31))
    gv = st[7:13].tolist() + st[13 + 25:].tolist()          # v, w, qd (observation order)
    k = R.Kin(model, st)
    want = np.concatenate([k.w, k.v, k.qd[1:]])             # the oracle's order, from the body-order arrays
    assert np.array_equal(np.array(gv)[p], want)


def test_mass_matrix_inverts_the_oracles_minv(cases, oracle64, model):
    p = R.perm_to_oracle(model)
    inv = np.argsort(p)
    for state, scale in cases:
        Mi = oracle64.minv(oracle_state(oracle64, state, scale))[np.ix_(inv, inv)]     # into this order
        M = R.mass_matrix(model, state, scale)
        assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
        assert np.abs(M @ Mi - np.eye(31)).max() < TOL


def test_inverse_dynamics_undoes_the_oracles_forward_dynamics(cases, oracle64, model):
    rng = np.random.default_rng(1)
    for state, scale in cases:
        s = oracle_state(oracle64, state, scale)
        h = R.inverse_dynamics(model, state, None, scale, G)
        tau, a_drawn = R.random_tau(model, state, scale, rng, with_accel=True)
        qdd, ba = oracle64.forward_dynamics(s, tau, with_damping=False)
        a = np.concatenate([ba[3:6], ba[0:3], qdd])
        assert np.abs(a - a_drawn).max() < 1e-7 * np.abs(a_drawn).max()      # the oracle returns the accelerations drawn
        assert np.abs(qdd).max() <= 10.0 * (1 + 1e-6)
        want = np.concatenate([np.zeros(6), tau])
        f = R.inverse_dynamics(model, state, a, scale, G)
        # base rows over the base force that M a and h cancel to 0 from, joint rows over the largest torque
        assert R.block_dev(f, want, np.abs(h[:6]).max(), np.abs(tau).max()) < TOL
        f2 = R.mass_matrix(model, state, scale) @ a + h
        assert R.block_dev(f2, want, np.abs(h[:6]).max(), np.abs(tau).max()) < TOL


def test_centroidal_against_the_oracles_energy(cases, oracle64, model):
    for state, scale in cases:
        s = oracle_state(oracle64, state, scale)
        e = oracle64.energy(s)
        c = R.centroidal(model, state, scale, G)
        assert abs(c[12] - e["ke"]) < TOL * max(abs(e["ke"]), 1.0)
        assert abs(c[13] - e["pe"]) < TOL * abs(e["pe"])
        lin = e["momentum"][3:6]
        # the oracle's angular momentum is about the base origin: shift it to the COM
        ang = e["momentum"][0:3] - np.cross(c[0:3] - state[0:3], lin)
        big = max(np.abs(e["momentum"]).max(), 1.0)
        assert np.abs(c[6:9] - lin).max() < TOL * big
        assert np.abs(c[9:12] - ang).max() < TOL * big
        assert np.abs(c[3:6] * c[14] - lin).max() < TOL * big


def test_jacobian_against_central_differences_of_the_oracles_poses(cases, oracle64, model):
    names = model["link_names"]
    hb = int(model["head_body"])
    links = [[l for l in range(len(names)) if model["link_body"][l] == hb][0], 0,
             [l for l in range(len(names)) if "toe" in names[l]][0]]
    h = 1e-6

    def point(state, link, local):
        pos, rot = oracle64.body_poses(oracle_state(oracle64, state, None))
        b = model["link_body"][link]
        tf = model["link_tf"][link]
        Rl = rot[b] @ tf[:9].reshape(3, 3)
        return pos[b] + rot[b] @ tf[9:12] + Rl @ local, Rl

    def moved(state, k, eps):
        """the state after the generalised velocity e_k has acted for eps"""
        s = state.copy()
        if k < 3:
            s[k] += eps
        elif k < 6:
            dq = np.concatenate([np.sin(eps / 2) * np.eye(3)[k - 3], [np.cos(eps / 2)]])
            x1, y1, z1, w1 = dq
            x2, y2, z2, w2 = state[3:7]
            s[3:7] = [w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                      w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]
        else:
            s[13 + k - 6] += eps
        return s

    for state, _ in cases[::3]:
        state = state.copy()
        state[3:7] /= np.linalg.norm(state[3:7])   # (a rotation exactly: w x r IS the derivative only for an orthonormal R)
        for link in links:
            for local in (np.zeros(3), np.array([0.3, -0.2, 0.1])):
                Jm = R.jacobian(model, state, link, local)
                for k in range(31):
                    (p1, R1), (p0, R0) = point(moved(state, k, h), link, local), point(moved(state, k, -h), link, local)
                    lin = (p1 - p0) / (2 * h)
                    W = (R1 - R0) / (2 * h) @ (0.5 * (R1 + R0)).T      # [w]x
                    ang = np.array([W[2, 1], W[0, 2], W[1, 0]])
                    assert np.abs(Jm[0:3, k] - lin).max() < 1e-7 * max(np.abs(Jm).max(), 1.0), (link, k)
                    assert np.abs(Jm[3:6, k] - ang).max() < 1e-7 * max(np.abs(Jm).max(), 1.0), (link, k)


def test_library_and_python_surface_have_the_queries():
    from trex_gym import _capi
    from trex_gym.trex_env import TrexBulletEnv
    from trex_gym.vec_env import TrexVecEnv
    lib = C.CDLL(_capi.LIB_PATH)
    for name in ("trex_batch_inverse_dynamics", "trex_batch_mass_matrix", "trex_batch_jacobian", "trex_batch_centroidal"):
        assert hasattr(lib, name), name
    for name in ("inverse_dynamics", "mass_matrix", "jacobian", "centroidal", "gravity_compensation"):
        assert callable(getattr(TrexVecEnv, name, None)), name
        assert callable(getattr(TrexBulletEnv, name, None)), name
    for name in ("inverse_dynamics", "mass_matrix", "jacobian", "centroidal"):
        assert callable(getattr(_capi.Batch, name, None)), name
