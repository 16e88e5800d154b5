"""Forward dynamics and mass-matrix solves on the GPU (trex_batch_forward_dynamics / trex_batch_solve_mass, include/trex_batch.h)
against the dense f64 reference tests/forward_dynamics_ref.py and the f64 oracle's articulated-body algorithm - the two tied
together by tests/test_forward_dynamics_ref.py - plus consistency with the other queries on the device, other trees, read-only,
refusals, stream capture, odd addresses, containment and the single-env surface. States and batches: those of
tests/test_gpu_dynamics.py (every env a state of its own).

Tolerances (TOL): min(4 x the largest deviation measured at N = 67 against the f64 references, cap); MEASURED holds the figures
that scripts/forward_dynamics_bench.py prints into profiles/r13_forward_dynamics.txt. Metrics:
  fd_force  the residual M_ref (a_gpu - a_ref) in dynamics_ref.block_dev: joint rows over the case's largest joint torque, base
            rows over the largest base component of h - the metric of id_roundtrip; cap 1e-4.
  fd_accel  |a_gpu - a_ref| per block (base linear, base angular, joints) over the block's largest |a_ref|, floored at 1 m/s^2,
            1 rad/s^2, 1 rad/s^2. No cap can be derived; the f32 oracle strays by ORACLE32_FD_ACCEL from the f64 one in the same
            metric on the base states (tests/test_forward_dynamics_ref.py prints it).
  minv      (M_ref / sqrt(M_ii M_jj)) @ (Minv_gpu * sqrt(M_ii M_jj)) - I over ||N^-1||_1, the normalisation of the minv figure of
            tests/test_gpu_dynamics.py, with M_ref the dense reference and, a second time, the inverse of oracle64.minv; cap 1e-5.
            (NOT the entrywise difference of the two inverses: ||N^-1||_1 is 700 on this tree, and an inverse rounded to f32
            entry by entry already differs by 1e-5 of that norm.)
  solve     the same residual for right-hand sides: |N (S x_gpu) - S^-1 rhs| over ||N^-1||_1 max |S^-1 rhs|, S = diag sqrt(M_ii),
            N = S^-1 M_ref S^-1 - for a unit right-hand side exactly a column of the minv figure; cap 1e-5.
  asym      the largest asymmetry of solve_mass(NULL) in the scaling of minv: recorded, bounded by 2 x TOL['minv'] (two entries,
            each within the tolerance), not promised to be zero.
  osi       operational-space inertia, each 3 x 3 block over the largest entry of the blocks it couples (linear, angular).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dynamics_ref as R
import forward_dynamics_ref as F
from conftest import ASSET_URDF
from gpu_support import DEV, dynamics_queries, loaded_vec, make_vec, random_actions
from state_sets import base_cases, case_states, oracle_state, probe_links, query_states
from tolerances import DYNAMICS_TOL

pytestmark = pytest.mark.gpu
NB, J, D = 26, 25, 31
G = 9.81

# Largest deviations measured at N = 67 on an MI355X (profiles/r13_forward_dynamics.txt). Tolerance = min(4 x measured, cap); the
# cap binds for fd_force (1e-4 < 1.8e-4). An f32 articulated-body pass of this formulation emulated in numpy on the same states
# shows the same fd_force and fd_accel (4.7e-5, 6.2e-5): the figures are the algorithm's in f32, not the kernel's.
MEASURED = dict(fd_force=4.43e-5, fd_accel=8.52e-5, minv=1.36e-7, solve=1.55e-8, asym=1.48e-7, osi=1.64e-4)
CAPS = dict(fd_force=1e-4, fd_accel=float("inf"), minv=1e-5, solve=1e-5, asym=2e-5, osi=float("inf"))
TOL = {k: min(4 * v, CAPS[k]) for k, v in MEASURED.items()}
ORACLE32_FD_ACCEL = 8.1e-4      # oracle32 against oracle64, fd_accel, base states (test_f32_oracle_strays_by)
# the generated models: fd_force, fd_accel, minv over the module's states (same file)
MEASURED_SYN = dict(deep_chain=dict(fd_force=4.44e-6, fd_accel=1.95e-5, minv=1.27e-7),
                    bushy=dict(fd_force=8.31e-7, fd_accel=1.91e-5, minv=8.04e-8))


def scaled_solve_dev(M, rhs, x_got):
    """`solve` of the module docstring for the rows rhs [K, D] -> x [K, D]"""
    dg = np.sqrt(np.diag(M))
    norm = np.abs(np.linalg.inv(M) * np.outer(dg, dg)).sum(0).max()
    return (np.abs((x_got @ M - rhs) / dg).max(1) / (norm * np.abs(rhs / dg).max(1))).max()


def osi_dev(got, want):
    ll, aa = np.abs(want[:3, :3]).max(), np.abs(want[3:, 3:]).max()
    d = np.abs(got - want)
    return max(d[:3, :3].max() / ll, d[3:, 3:].max() / aa, d[:3, 3:].max() / np.sqrt(ll * aa), d[3:, :3].max() / np.sqrt(ll * aa))


def deviations(oracle64, model, n, envs=None, batch=None):
    """{figure: largest deviation over the envs `envs` (all) of a batch of `batch` (n) envs holding the n case states in turn}"""
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases, batch)
    N = v.num_envs
    envs = range(N) if envs is None else envs
    rng = np.random.default_rng(11)
    inv = np.argsort(R.perm_to_oracle(model))
    links = probe_links(model)
    ref = {}
    tau = np.zeros((N, J), np.float32)
    full = np.zeros((N, D), np.float32)
    for e in envs:
        s, ms = cases[e % len(cases)]
        M, h = R.mass_matrix(model, s, ms), R.inverse_dynamics(model, s, None, ms, G)
        tau[e] = R.random_tau(model, s, ms, rng)
        full[e] = h + np.concatenate([np.abs(h[:6]).max() * rng.uniform(-1, 1, 6), np.abs(h[6:]).max() * rng.uniform(-1, 1, J)])
        ref[e] = (M, h)
    r1 = torch.tensor(rng.normal(size=(N, D)).astype(np.float32), device=DEV)
    r64 = torch.tensor(rng.normal(size=(N, 64, D)).astype(np.float32), device=DEV)
    Jh, Jt = v.jacobian(links["head"]), v.jacobian(links["toe"], (0.1, 0.0, -0.05))
    host = lambda t: t.cpu().numpy().astype(np.float64)
    a0, at, af = host(v.forward_dynamics()), host(v.forward_dynamics(tau=tau)), host(v.forward_dynamics(torch.tensor(full)))
    Mi = host(v.inverse_mass_matrix())
    x1, xh, xt, x64 = host(v.solve_mass(r1)), host(v.solve_mass(Jh)), host(v.solve_mass(Jt)), host(v.solve_mass(r64))
    lam = {nm: host(v.operational_space_inertia(links[nm], p)) for nm, p in (("head", None), ("toe", (0.1, 0.0, -0.05)))}
    r1, r64, Jh, Jt = host(r1), host(r64), host(Jh), host(Jt)
    dev = dict(fd_force=0.0, fd_accel=0.0, minv=0.0, solve=0.0, asym=0.0, osi=0.0)
    for e in envs:
        s, ms = cases[e % len(cases)]
        M, h = ref[e]
        os_ = oracle_state(oracle64, s, ms)
        bs = np.abs(h[:6]).max()
        t64 = tau[e].astype(np.float64)
        # (accelerations, the force they answer, joint scale, the oracle's answer where its call takes the force)
        for got, force, js, orc in ((a0[e], np.zeros(D), np.abs(h[6:]).max(), oracle64.forward_dynamics(os_, None, with_damping=False)),
                                    (at[e], np.concatenate([np.zeros(6), t64]), np.abs(t64).max(),
                                     oracle64.forward_dynamics(os_, t64, with_damping=False)),
                                    (af[e], full[e].astype(np.float64), np.abs(full[e, 6:]).max(), None)):
            wants = [np.linalg.solve(M, force - h)]
            if orc is not None:
                wants.append(np.concatenate([orc[1][3:6], orc[1][0:3], orc[0]]))
            for want in wants:
                dev["fd_accel"] = max(dev["fd_accel"], F.accel_dev(got, want))
                dev["fd_force"] = max(dev["fd_force"], R.block_dev(M @ (got - want), np.zeros(D), bs, js))
        dm, asym = F.minv_dev(M, Mi[e])
        dev["minv"] = max(dev["minv"], dm, F.minv_dev(np.linalg.inv(oracle64.minv(os_)[np.ix_(inv, inv)]), Mi[e])[0])
        dev["asym"] = max(dev["asym"], asym)
        for rhs, x in ((r1[e][None], x1[e][None]), (Jh[e], xh[e]), (Jt[e], xt[e]), (r64[e], x64[e])):
            dev["solve"] = max(dev["solve"], scaled_solve_dev(M, rhs, x))
        for nm, p in (("head", (0.0, 0.0, 0.0)), ("toe", (0.1, 0.0, -0.05))):
            Jr = R.jacobian(model, s, links[nm], p)
            dev["osi"] = max(dev["osi"], osi_dev(lam[nm][e], np.linalg.inv(Jr @ np.linalg.solve(M, Jr.T))))
    v.close()
    return dev


def check(d, where):
    print("deviations %s: %s" % (where, {k: "%.3g" % x for k, x in d.items()}))
    for k in d:
        assert d[k] <= TOL[k], (where, k, d[k])


# ---------------------------------------------------------------- 1. against the references
@pytest.fixture(scope="module")
def dev67(oracle64, model):
    d = deviations(oracle64, model, 67)
    print("deviations N=67:", {k: "%.3g" % x for k, x in d.items()})
    return d


@pytest.mark.parametrize("name", ["fd_force", "fd_accel", "minv", "solve", "asym", "osi"])
def test_against_references_n67(name, dev67):
    """every env of 67: forward dynamics of no force, of [0, tau] (dynamics_ref.random_tau) and of a full force with a base
    block, against the dense reference and - the first two - the oracle; solve_mass(NULL) against the reference and
    oracle.minv; solve_mass at K = 1, 6 (the GPU's Jacobians of the head and a toe link) and 64; the operational-space inertia of
    the head and of a toe point against inv(J M^-1 J^T) of the reference (3.). Measured maxima: MEASURED."""
    assert TOL[name] <= CAPS[name]
    assert dev67[name] <= TOL[name], (name, dev67[name])


@pytest.mark.parametrize("n", [1, 3, 5])
def test_against_references_small_batches(n, oracle64, model):
    """1: one live wave, three dead ones at the barriers; 3: a ragged workgroup; 5: a second workgroup with one env"""
    check(deviations(oracle64, model, n), "N=%d" % n)


def test_against_references_n4096(oracle64, model):
    envs = sorted(set(np.linspace(0, 4095, 64).astype(int).tolist()))
    check(deviations(oracle64, model, 67, envs=envs, batch=4096), "N=4096")


def test_the_tolerance_tells_the_velocity_terms(oracle64, model):
    """the answer with the velocity-product terms dropped, M^-1 (f - g), misses the final fd_accel tolerance on every airborne
    random state (CPU arithmetic; the tolerance is the thing under test)"""
    for s, ms in base_cases(oracle64, model)[-8:]:
        want = F.forward_dynamics(model, s, None, ms, G)
        assert F.accel_dev(F.forward_dynamics(model, s, None, ms, G, velocity_terms=False), want) > TOL["fd_accel"]


# ---------------------------------------------------------------- 2. consistency on the device
@pytest.fixture(scope="module")
def vec67(oracle64, model):
    cases = case_states(oracle64, model, 67)
    v = loaded_vec(cases)
    yield v, cases
    v.close()


def test_round_trips_with_inverse_dynamics(vec67, model):
    v, cases = vec67
    rng = np.random.default_rng(21)
    acc, frc = np.zeros((67, D), np.float32), np.zeros((67, D), np.float32)
    for e, (s, ms) in enumerate(cases):
        tau, a = R.random_tau(model, s, ms, rng, with_accel=True)
        acc[e] = a
        h = R.inverse_dynamics(model, s, None, ms, G)
        frc[e] = h + np.concatenate([np.abs(h[:6]).max() * rng.uniform(-1, 1, 6), np.abs(h[6:]).max() * rng.uniform(-1, 1, J)])
    acc_t, frc_t = torch.tensor(acc, device=DEV), torch.tensor(frc, device=DEV)
    f_of_a = v.inverse_dynamics(acc_t)
    a2 = v.forward_dynamics(f_of_a).cpu().numpy().astype(np.float64)
    f2 = v.inverse_dynamics(v.forward_dynamics(frc_t)).cpu().numpy().astype(np.float64)
    a_fd = v.forward_dynamics(frc_t).cpu().numpy().astype(np.float64)
    a_sm = v.solve_mass(frc_t - v.inverse_dynamics()).cpu().numpy().astype(np.float64)
    f_of_a = f_of_a.cpu().numpy().astype(np.float64)
    tol = TOL["fd_force"] + DYNAMICS_TOL["id_roundtrip"]          # one pass through each query, both in the same metric
    worst = [0.0, 0.0, 0.0]
    for e, (s, ms) in enumerate(cases):
        M, h = R.mass_matrix(model, s, ms), R.inverse_dynamics(model, s, None, ms, G)
        bs = np.abs(h[:6]).max()
        worst[0] = max(worst[0], R.block_dev(M @ (a2[e] - acc[e]), np.zeros(D), bs, np.abs(f_of_a[e, 6:]).max()))
        worst[1] = max(worst[1], R.block_dev(f2[e], frc[e].astype(np.float64), bs, np.abs(frc[e, 6:]).max()))
        worst[2] = max(worst[2], F.accel_dev(a_fd[e], a_sm[e]))
    print("fd(id(a)) - a: %.3g   id(fd(f)) - f: %.3g   fd(f) - solve_mass(f - h): %.3g" % tuple(worst))
    assert worst[0] <= tol and worst[1] <= tol
    assert worst[2] <= 4 * TOL["fd_accel"]                 # 2 x the tolerance of each side, both accelerations in fd_accel


def test_solve_mass_is_linear_and_columns_do_not_depend_on_their_place(vec67, model):
    v, cases = vec67
    gen = torch.Generator(device=DEV).manual_seed(4)
    x, y = torch.randn(67, D, generator=gen, device=DEV), torch.randn(67, D, generator=gen, device=DEV)
    sx, sy, sc = v.solve_mass(x), v.solve_mass(y), v.solve_mass(2.0 * x - 3.0 * y)
    rhs = (2.0 * x - 3.0 * y).cpu().numpy().astype(np.float64)
    for e, (s, ms) in enumerate(cases):
        M = R.mass_matrix(model, s, ms)
        dg = np.sqrt(np.diag(M))
        norm = np.abs(np.linalg.inv(M) * np.outer(dg, dg)).sum(0).max()
        d = (M @ (sc[e] - (2.0 * sx[e] - 3.0 * sy[e])).cpu().numpy().astype(np.float64)) / dg
        # the residuals of three solves, each within TOL['solve'] of its own right-hand side's scale (|2 x - 3 y| <= 2 |x| + 3 |y|)
        scale = norm * (np.abs(rhs[e] / dg).max() + 2 * np.abs(x[e].cpu().numpy() / dg).max() + 3 * np.abs(y[e].cpu().numpy() / dg).max())
        assert np.abs(d).max() <= TOL["solve"] * scale, e
    big = torch.randn(67, 64, D, generator=gen, device=DEV)
    for k in (0, 1, 30, 63):
        big[:, k] = x
    out = v.solve_mass(big)
    for k in (0, 1, 30, 63):                               # both lane halves, first and last pair
        assert torch.equal(out[:, k], sx), k
    assert torch.equal(v.solve_mass(x[:, None, :].contiguous())[:, 0], sx)


def test_in_place_repeat_and_batch_size_are_bitwise(vec67, oracle64, model):
    v, cases = vec67
    gen = torch.Generator(device=DEV).manual_seed(6)
    f, r = torch.randn(67, D, generator=gen, device=DEV), torch.randn(67, 7, D, generator=gen, device=DEV)
    a, x, mi = v.forward_dynamics(f), v.solve_mass(r), v.inverse_mass_matrix()
    assert torch.equal(v.forward_dynamics(f), a) and torch.equal(v.solve_mass(r), x) and torch.equal(v.inverse_mass_matrix(), mi)
    f2, r2 = f.clone(), r.clone()
    assert v.batch.forward_dynamics(f2, f2) is f2 and torch.equal(f2, a)
    assert v.batch.solve_mass(r2, r2) is r2 and torch.equal(r2, x)
    for e in (0, 5, 66):
        one = loaded_vec([cases[e]])
        assert torch.equal(one.forward_dynamics(f[e:e + 1]), a[e:e + 1]), e
        assert torch.equal(one.solve_mass(r[e:e + 1]), x[e:e + 1]), e
        assert torch.equal(one.inverse_mass_matrix(), mi[e:e + 1]), e
        one.close()


# ---------------------------------------------------------------- 4. other trees
def other_tree_deviations(name, directory):
    """{fd_force, fd_accel, minv} of the generated model `name` over six of its airborne query states"""
    import synthetic_models as sm
    from oracle import oracle as O
    from trex_gym.vec_env import TrexVecEnv
    path, props, om = sm.compile_both(name, directory)
    o64 = O.Oracle(om, params=props["params"])
    states = query_states(om)[:6]
    nj = om["nb"] - 1
    v = TrexVecEnv(len(states), urdf_path=path, device=DEV, params=props["params"])
    v.reset()
    v.set_state(torch.tensor(np.array(states, np.float32)))
    rng = np.random.default_rng(9)
    tau = np.array([R.random_tau(om, s, None, rng) for s in states], np.float32)
    a0 = v.forward_dynamics().cpu().numpy().astype(np.float64)
    at = v.forward_dynamics(tau=tau).cpu().numpy().astype(np.float64)
    Mi = v.inverse_mass_matrix().cpu().numpy().astype(np.float64)
    inv = np.argsort(R.perm_to_oracle(om))
    dev = dict(fd_force=0.0, fd_accel=0.0, minv=0.0)
    for e, s in enumerate(states):
        M, h = R.mass_matrix(om, s), R.inverse_dynamics(om, s, None, None, G)
        os_ = o64.new_state()
        o64.set_state(os_, s)
        for got, t, js in ((a0[e], None, np.abs(h[6:]).max()), (at[e], tau[e].astype(np.float64), np.abs(tau[e]).max())):
            qdd, ba = o64.forward_dynamics(os_, t, with_damping=False)
            force = np.zeros(6 + nj) if t is None else np.concatenate([np.zeros(6), t])
            for want in (np.concatenate([ba[3:6], ba[0:3], qdd]), np.linalg.solve(M, force - h)):
                dev["fd_accel"] = max(dev["fd_accel"], F.accel_dev(got, want))
                dev["fd_force"] = max(dev["fd_force"], R.block_dev(M @ (got - want), np.zeros(6 + nj), np.abs(h[:6]).max(), js))
        dev["minv"] = max(dev["minv"], F.minv_dev(M, Mi[e])[0], F.minv_dev(np.linalg.inv(o64.minv(os_)[np.ix_(inv, inv)]), Mi[e])[0])
    v.close()
    return dev


@pytest.mark.parametrize("name", ["deep_chain", "bushy"])
def test_other_trees(name, tmp_path):
    """six tree levels (deep_chain) and four children below the base (bushy): the level loops and child lists of the three
    passes, against that model's own oracle and the dense reference at the module's airborne states"""
    dev = other_tree_deviations(name, tmp_path)
    print("%s, largest deviations: %s" % (name, {k: "%.3g" % x for k, x in dev.items()}))
    for k, x in dev.items():
        assert x <= min(4 * MEASURED_SYN[name][k], CAPS[k]), (name, k, x)


# ---------------------------------------------------------------- 5. read-only
def new_queries(v):
    f = torch.ones(v.num_envs, D, device=DEV)
    return [v.forward_dynamics(), v.forward_dynamics(f), v.solve_mass(f), v.inverse_mass_matrix(), v.solve_mass(v.jacobian(5))]


@pytest.mark.parametrize("n", [2, 3])
def test_queries_are_read_only(n, oracle64, model):
    """as tests/test_gpu_dynamics.py::test_queries_are_read_only - warm start, contact sensor and an external wrench active - with
    the two new calls between every two steps: rows, state, contact wrench and episode steps bitwise those without; and the four
    existing queries return bitwise the same before and after the new calls"""
    gen = torch.Generator(device=DEV).manual_seed(5)
    w = 50 * torch.randn(n, NB, 6, generator=gen, device=DEV)
    acts = [random_actions(model, n, gen) for _ in range(10)]
    landed = torch.tensor(np.array([base_cases(oracle64, model)[k][0] for k in (20, 22, 24)[:n]], np.float32))
    pair = []
    for probe in (False, True):
        v = make_vec(n, params={"warmstart": 0.85}, max_episode_steps=50)
        v.enable_contact_sensor(True)
        v.reset_tensor()
        v.set_state(landed)
        v.set_external_wrench(w)
        rows = []
        for a in acts:
            v.step_tensor(a)
            rows.append(v.rows.clone())
            if probe:
                before = dynamics_queries(v, 5)
                out = new_queries(v)
                assert all(torch.isfinite(o).all() for o in out)
                for x, y in zip(before, dynamics_queries(v, 5)):
                    assert torch.equal(x, y)
        steps = torch.zeros(n, dtype=torch.int32, device=DEV)
        v.batch.get_episode_steps(steps)
        pair.append((torch.stack(rows), v.get_state(), v.contact_wrench().clone(), steps))
    for x, y in zip(*pair):
        assert torch.equal(x, y)
    assert pair[0][2].abs().sum() > 0


# ---------------------------------------------------------------- 6. refusals
def test_refusals(model):
    from trex_gym import _capi as capi
    n = 5
    v, ref = make_vec(n), make_vec(n)
    v.reset_tensor()
    ref.reset_tensor()
    b, lib = v.batch, capi.lib
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    SENT = 7.0
    out = torch.full((n * 64 * D,), SENT, device=DEV)
    rhs = torch.zeros(n * 64 * D, device=DEV)
    fd = lambda f, a: lib.trex_batch_forward_dynamics(b.h, f, a, s)
    sm = lambda r, k, x: lib.trex_batch_solve_mass(b.h, r, k, x, s)
    assert fd(None, ptr(out)) == 0 and sm(ptr(rhs), 64, ptr(out)) == 0 and sm(None, D, ptr(out)) == 0     # the calls work at all
    torch.cuda.synchronize()
    out.fill_(SENT)
    for k in (0, 65, -1, -64):
        assert sm(ptr(rhs), k, ptr(out)) == capi.E_INVALID, k
    for k in (1, D - 1, D + 1, 64):
        assert sm(None, k, ptr(out)) == capi.E_INVALID, k                          # NULL rhs is the identity: K = D only
    assert fd(None, None) == capi.E_INVALID and sm(ptr(rhs), 3, None) == capi.E_INVALID                   # NULL output
    host = np.zeros(n * 64 * D, np.float32)
    hp = C.c_void_p(host.ctypes.data)
    assert fd(None, hp) == capi.E_INVALID and fd(hp, ptr(out)) == capi.E_INVALID
    assert sm(ptr(rhs), 2, hp) == capi.E_INVALID and sm(hp, 2, ptr(out)) == capi.E_INVALID
    hip = C.CDLL("libamdhip64.so")
    for floats, call in ((n * D, lambda p: fd(None, p)), (n * D, lambda p: fd(p, ptr(out))), (n * 6 * D, lambda p: sm(ptr(rhs), 6, p)),
                         (n * 6 * D, lambda p: sm(p, 6, ptr(out))), (n * D * D, lambda p: sm(None, D, p))):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(4 * floats - 4)) == 0           # one float short
        try:
            assert call(p) == capi.E_INVALID
        finally:
            hip.hipFree(p)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                               # nothing was launched
    assert np.all(host == 0)
    with pytest.raises(capi.TrexError):
        b.forward_dynamics(torch.zeros(n, D))                                      # the Python layer: a host tensor
    with pytest.raises(capi.TrexError):
        b.solve_mass(torch.zeros(n, 65, D, device=DEV))
    with pytest.raises(capi.TrexError):
        b.solve_mass(torch.zeros(n, 2, D - 1, device=DEV))
    with pytest.raises(ValueError):
        v.forward_dynamics(force=torch.zeros(n, D), tau=torch.zeros(n, J))
    a = torch.zeros(n, J, device=DEV)
    v.step_tensor(a)
    ref.step_tensor(a)
    assert torch.equal(v.rows, ref.rows)


# ---------------------------------------------------------------- 7. stream capture
def test_stream_capture(vec67):
    """the SECOND call of each captured on one stream, one linear chain, replayed twice: bitwise the eager results"""
    v, _ = vec67
    n = v.num_envs
    gen = torch.Generator(device=DEV).manual_seed(8)
    f, r = torch.randn(n, D, generator=gen, device=DEV), torch.randn(n, 6, D, generator=gen, device=DEV)
    outs = [torch.zeros(n, D, device=DEV), torch.zeros(n, 6, D, device=DEV), torch.zeros(n, D, D, device=DEV)]

    def calls():
        v.batch.forward_dynamics(f, outs[0])
        v.batch.solve_mass(r, outs[1])
        v.batch.solve_mass(None, outs[2])

    calls()
    eager = [o.clone() for o in outs]
    assert all(o.abs().sum() > 0 for o in eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            calls()
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for o, want in zip(outs, eager):
            assert torch.equal(o, want)


# ---------------------------------------------------------------- 8. off the 16-byte grid
def test_buffers_off_the_16_byte_grid(oracle64, model):
    """inputs and outputs that start 4 bytes into an allocation: bitwise the aligned call, nothing written outside"""
    v = loaded_vec(case_states(oracle64, model, 67)[:7])
    n = v.num_envs
    gen = torch.Generator(device=DEV).manual_seed(9)
    for shape, call in (((D,), lambda i, o: v.batch.forward_dynamics(i, o)), ((1, D), lambda i, o: v.batch.solve_mass(i, o)),
                        ((6, D), lambda i, o: v.batch.solve_mass(i, o)), ((5, D), lambda i, o: v.batch.solve_mass(i, o))):
        numel = n * int(np.prod(shape))
        src = torch.randn(numel + 2, generator=gen, device=DEV)
        flat = torch.full((numel + 2,), 7.0, device=DEV)
        odd_in, odd_out = src[1:1 + numel].view((n,) + shape), flat[1:1 + numel].view((n,) + shape)
        assert odd_in.data_ptr() % 16 == 4 and odd_out.data_ptr() % 16 == 4
        call(odd_in, odd_out)
        assert torch.equal(odd_out, call(odd_in.clone(), None))
        assert flat[0].item() == 7.0 and flat[-1].item() == 7.0
    v.close()


# ---------------------------------------------------------------- 9. NaN containment
def test_nan_state_is_contained(oracle64, model):
    cases = case_states(oracle64, model, 67)[:9]
    clean = loaded_vec(cases)
    want = new_queries(clean)
    st = clean.get_state().clone()
    slot = list(model["obs_order"]).index(int(model["head_body"]))
    st[5, 13 + slot] = float("nan")       # the head joint's angle of env 5 (second workgroup, shared with envs 4, 6, 7)
    st[2, 11] = float("nan")              # a base angular velocity of env 2: forward dynamics only, M^-1 depends on q alone
    dirty = loaded_vec(cases)
    dirty.set_state(st)
    got = new_queries(dirty)
    keep = [0, 1, 3, 4, 6, 7, 8]
    for g_, w_ in zip(got, want):
        assert torch.equal(g_[keep], w_[keep])
    assert all(torch.isnan(g_[5]).any() for g_ in got)
    assert torch.isnan(got[0][2]).any() and torch.isnan(got[1][2]).any()
    for g_, w_ in zip(got[2:], want[2:]):
        assert torch.equal(g_[2], w_[2])
    clean.close()
    dirty.close()


# ---------------------------------------------------------------- 10. single-env surface
def test_single_env_surface(model):
    from trex_gym.trex_env import TrexBulletEnv
    env = TrexBulletEnv(urdf_path=ASSET_URDF)
    env.reset()
    a0, at = env.forward_dynamics(), env.forward_dynamics(tau=np.zeros(J))
    af = env.forward_dynamics(force=np.zeros(D))
    x1, xk, mi = env.solve_mass(np.ones(D)), env.solve_mass(np.ones((3, D))), env.inverse_mass_matrix()
    lam = env.operational_space_inertia(probe_links(model)["head"])
    for arr, shape in ((a0, (D,)), (at, (D,)), (af, (D,)), (x1, (D,)), (xk, (3, D)), (mi, (D, D)), (lam, (6, 6))):
        assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == shape
    assert np.array_equal(a0, at) and np.array_equal(a0, af) and np.array_equal(xk[1], x1)
    assert np.array_equal(env.solve_mass(), mi)
    with pytest.raises(ValueError):
        env.forward_dynamics(force=np.zeros(D), tau=np.zeros(J))
    env.close()
