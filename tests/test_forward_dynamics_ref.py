"""Ties tests/forward_dynamics_ref.py - the dense f64 reference the GPU's forward dynamics and M^-1 solves are compared with -
to the frozen CPU oracle's articulated-body algorithm (oracle_forward_dynamics, oracle_minv) on the landing states and the 8
random airborne states of the GPU dynamics tests, mass-scaled ones included; measures how far the oracle's own f32 build strays
from its f64 build in the acceleration metric (the yardstick for an f32 ABA on this tree); and checks that the library and the
Python surface carry the two calls. f64 against f64: 1e-8, as tests/test_dynamics_ref.py; the accelerations over
max(largest |a| of the block, 1)."""
import ctypes as C

import numpy as np
import pytest

import dynamics_ref as R
import forward_dynamics_ref as F
from state_sets import landing_states, oracle_state

TOL = 1e-8
G = 9.81


@pytest.fixture(scope="module")
def cases(oracle64, model):
    ls, _ = landing_states(oracle64, model)
    return [(s.astype(np.float64), None) for s in ls] + list(zip(*R.random_states(model, 8)))


def oracle_accel(orc, state, scale, tau):
    """the oracle's forward dynamics in the order of the header: [dv/dt, dw/dt, qdd in observation order]"""
    qdd, ba = orc.forward_dynamics(oracle_state(orc, state, scale), tau, with_damping=False)
    return np.concatenate([ba[3:6], ba[0:3], qdd])


def test_forward_dynamics_against_the_oracle(cases, oracle64, model):
    """zero force and [0, tau]: the two forces the oracle call takes"""
    rng = np.random.default_rng(1)
    for state, scale in cases:
        tau = R.random_tau(model, state, scale, rng)
        for t in (None, tau):
            want = oracle_accel(oracle64, state, scale, t)
            force = None if t is None else np.concatenate([np.zeros(6), t])
            assert F.accel_dev(F.forward_dynamics(model, state, force, scale, G), want) < TOL


def test_forward_dynamics_inverts_inverse_dynamics_with_a_base_force(cases, model):
    """the force the oracle call does not take: a full one, base block included, goes back through RNEA"""
    rng = np.random.default_rng(2)
    for state, scale in cases:
        h = R.inverse_dynamics(model, state, None, scale, G)
        f = h + np.concatenate([np.abs(h[:6]).max() * rng.uniform(-1, 1, 6), np.abs(h[6:]).max() * rng.uniform(-1, 1, 25)])
        a = F.forward_dynamics(model, state, f, scale, G)
        back = R.inverse_dynamics(model, state, a, scale, G)
        assert R.block_dev(back, f, np.abs(f[:6]).max(), np.abs(f[6:]).max()) < TOL


def test_minv_against_the_oracle(cases, oracle64, model):
    inv = np.argsort(R.perm_to_oracle(model))
    for state, scale in cases:
        Mi = oracle64.minv(oracle_state(oracle64, state, scale))[np.ix_(inv, inv)]
        dev, asym = F.minv_dev(R.mass_matrix(model, state, scale), Mi)
        assert dev < TOL and asym < TOL
        got = F.minv(model, state, scale)
        assert np.abs(got - Mi).max() < TOL * np.abs(Mi).max()
        rhs = np.random.default_rng(3).normal(size=(4, 31))
        assert np.abs(F.solve_mass(model, state, rhs, scale) - rhs @ Mi).max() < TOL * np.abs(rhs @ Mi).max()


def oracle32_deviation(cases, oracle64, oracle32, model):
    """(fd_accel, minv) of the f32 oracle against the f64 one: zero force and a random tau on every state"""
    rng = np.random.default_rng(1)
    inv = np.argsort(R.perm_to_oracle(model))
    acc, mi = 0.0, 0.0
    for state, scale in cases:
        tau = R.random_tau(model, state, scale, rng)
        for t in (None, tau):
            acc = max(acc, F.accel_dev(oracle_accel(oracle32, state, scale, t), oracle_accel(oracle64, state, scale, t)))
        Mi = oracle32.minv(oracle_state(oracle32, state, scale))[np.ix_(inv, inv)]
        mi = max(mi, F.minv_dev(R.mass_matrix(model, state, scale), Mi)[0])
    return acc, mi


def test_f32_oracle_strays_by(cases, oracle64, oracle32, model):
    """Prints the figures (run with -s): the yardstick the GPU's fd_accel figure is stated next to - 8.1e-4 and 9.6e-7 when
    this was written; the oracle refers every spatial quantity to one common point. Nothing is promised for it beyond what any
    usable answer must do: stay an order of magnitude inside the 1e-2 by which dropping the velocity-product terms moves the
    accelerations (test_velocity_terms_show_in_the_acceleration_metric)."""
    acc, mi = oracle32_deviation(cases, oracle64, oracle32, model)
    print("oracle32 against oracle64: fd_accel %.3g, minv %.3g" % (acc, mi))
    assert 0.0 < acc < 1e-3 and 0.0 < mi < 1e-3


def test_velocity_terms_show_in_the_acceleration_metric(cases, model):
    """dropping the velocity-product terms moves every airborne random state by far more than f32 can blur"""
    for state, scale in cases[-8:]:
        want = F.forward_dynamics(model, state, None, scale, G)
        assert F.accel_dev(F.forward_dynamics(model, state, None, scale, G, velocity_terms=False), want) > 1e-2


def test_library_and_python_surface_have_the_calls():
    from trex_gym import _capi
    from trex_gym.trex_env import TrexBulletEnv
    from trex_gym.vec_env import TrexVecEnv
    lib = C.CDLL(_capi.LIB_PATH)
    for name in ("trex_batch_forward_dynamics", "trex_batch_solve_mass"):
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS
    for name in ("forward_dynamics", "solve_mass", "inverse_mass_matrix", "operational_space_inertia"):
        assert callable(getattr(TrexVecEnv, name, None)), name
        assert callable(getattr(TrexBulletEnv, name, None)), name
    for name in ("forward_dynamics", "solve_mass"):
        assert callable(getattr(_capi.Batch, name, None)), name
