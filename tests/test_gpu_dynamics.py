"""Dynamics queries on the GPU (trex_batch_inverse_dynamics / _mass_matrix / _jacobian / _centroidal, include/trex_batch.h)
against the f64 restatement tests/dynamics_ref.py - itself tied to the oracle by tests/test_dynamics_ref.py - and against the
oracle and the step kernel directly; plus read-only, refusals, stream capture, containment and the product's grid sizes.

States (state_sets.case_states): the landing states and 8 random airborne ones (two with a per-body mass scale), cycled over
the envs with an env-specific perturbation from the second lap on, so that EVERY env has a state of its own.

Tolerances (TOL): 4 x the largest deviation measured on these very states at N = 67 (scripts/dynamics_bench.py prints them;
profiles/r12_dynamics.txt records them), never above the caps 1e-4 (inverse dynamics, Jacobian, centroidal) / 1e-5 (mass
matrix). Scales: inverse dynamics - the largest |force| component of the env's case, taken per block because the blocks carry
different units: the joint rows (N m) over the largest joint torque of the case (max |tau| for the round trip, max |h_joint| for
zero accelerations), the base rows (N, N m) over the largest base component of h - the base force that M a cancels to 0 in the
round trip; mass matrix - |dM_ij| / sqrt(M_ii M_jj);
Jacobian - absolute over the largest entry; centroidal - per quantity over its magnitude, momenta floored at 1 % of
mass x 1 m/s (x 1 m for the angular one)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dynamics_ref as R
from conftest import ASSET_URDF
from dynamics_model_cases import cent_dev     # (the centroidal metric of the module docstring: one text, shared with the generated models)
from gpu_support import DEV, dynamics_queries as all_queries, loaded_vec, make_vec, random_actions
from state_sets import base_cases, case_states, oracle_state, probe_links
from tolerances import DYNAMICS_CAPS as CAPS, DYNAMICS_MEASURED as MEASURED, DYNAMICS_TOL as TOL  # noqa: F401  (MEASURED: the docstrings' pointer)

pytestmark = pytest.mark.gpu
NB, J, D = 26, 25, 31
G = 9.81

# MEASURED, CAPS, TOL: tests/tolerances.py (the link-state and forward-dynamics tests read them as well)


def deviations(oracle64, model, n, envs=None, batch=None):
    """the figures TOL is set from: {name: largest deviation over the envs `envs` (all) of a batch of `batch` (n) envs}"""
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases, batch)
    envs = range(v.num_envs) if envs is None else envs
    rng = np.random.default_rng(3)
    dev = dict(id_zero=0.0, id_roundtrip=0.0, mass=0.0, minv=0.0, jac=0.0, cent=0.0)
    inv = np.argsort(R.perm_to_oracle(model))
    h_gpu = v.inverse_dynamics().cpu().numpy().astype(np.float64)
    M_gpu = v.mass_matrix()
    assert torch.equal(M_gpu, M_gpu.transpose(1, 2).contiguous())            # exactly symmetric
    M_gpu = M_gpu.cpu().numpy().astype(np.float64)
    c_gpu = v.centroidal().data.cpu().numpy().astype(np.float64)
    links = probe_links(model)
    jac = {(nm, k): v.jacobian(l, loc).cpu().numpy().astype(np.float64)
           for nm, l in links.items() for k, loc in enumerate((None, (0.3, -0.2, 0.1)))}
    acc = np.zeros((v.num_envs, D), np.float32)
    taus = {}
    for e in envs:
        s, ms = cases[e % len(cases)]
        h = R.inverse_dynamics(model, s, None, ms, G)
        dev["id_zero"] = max(dev["id_zero"], R.block_dev(h_gpu[e], h, np.abs(h[:6]).max(), np.abs(h[6:]).max()))
        M = R.mass_matrix(model, s, ms)
        dg = np.sqrt(np.diag(M))
        dev["mass"] = max(dev["mass"], (np.abs(M_gpu[e] - M) / np.outer(dg, dg)).max())
        os_ = oracle_state(oracle64, s, ms)
        Mi = oracle64.minv(os_)[np.ix_(inv, inv)]
        # M Minv = I in the coordinates of the mass-matrix metric: with S = diag(sqrt(M_ii)), N = S^-1 M S^-1 has a unit
        # diagonal and an entrywise error dN <= the metric, so E = dN N^-1 obeys |E_ij| <= metric x ||N^-1||_1: E over that norm
        # is bounded by the same tolerance as the mass matrix itself
        Ni = Mi * np.outer(dg, dg)
        E = (M_gpu[e] / np.outer(dg, dg)) @ Ni - np.eye(D)
        dev["minv"] = max(dev["minv"], np.abs(E).max() / np.abs(Ni).sum(0).max())
        for (nm, k), Jg in jac.items():
            Jr = R.jacobian(model, s, links[nm], (0.0, 0.0, 0.0) if k == 0 else (0.3, -0.2, 0.1))
            dev["jac"] = max(dev["jac"], np.abs(Jg[e] - Jr).max() / np.abs(Jr).max())
        cr = R.centroidal(model, s, ms, G)
        dev["cent"] = max(dev["cent"], cent_dev(c_gpu[e], cr))
        # ... and with the oracle's own energy and momentum (about the base origin: shifted to the COM), the rest from cr
        en = oracle64.energy(os_)
        co = cr.copy()
        co[6:9], co[12], co[13] = en["momentum"][3:6], en["ke"], en["pe"]
        co[3:6] = co[6:9] / cr[14]
        co[9:12] = en["momentum"][0:3] - np.cross(cr[0:3] - s[0:3], co[6:9])
        dev["cent"] = max(dev["cent"], cent_dev(c_gpu[e], co))
        tau = R.random_tau(model, s, ms, rng)
        qdd, ba = oracle64.forward_dynamics(os_, tau, with_damping=False)
        acc[e] = np.concatenate([ba[3:6], ba[0:3], qdd])
        taus[e] = tau
    f = v.inverse_dynamics(torch.tensor(acc)).cpu().numpy().astype(np.float64)
    for e in envs:
        s, ms = cases[e % len(cases)]
        h = R.inverse_dynamics(model, s, None, ms, G)
        want = np.concatenate([np.zeros(6), taus[e]])
        dev["id_roundtrip"] = max(dev["id_roundtrip"], R.block_dev(f[e], want, np.abs(h[:6]).max(), np.abs(taus[e]).max()))
    v.close()
    return dev


@pytest.fixture(scope="module")
def dev67(oracle64, model):
    d = deviations(oracle64, model, 67)
    print("deviations N=67:", {k: "%.3g" % x for k, x in d.items()})
    return d


@pytest.mark.parametrize("name", ["id_roundtrip", "id_zero", "mass", "minv", "jac", "cent"])
def test_against_reference_n67(name, dev67):
    """Every env of 67 (17 workgroups, the last one short) with a state of its own.
    id_roundtrip: the f64 oracle's forward-dynamics accelerations for a random tau go back to [0, tau];
    id_zero: h against RNEA;
    mass: |dM_ij| / sqrt(M_ii M_jj), the output bitwise symmetric;
    minv: M_gpu x oracle.minv = I in the metric's coordinates, over ||N^-1||_1 (see deviations);
    jac: head, toe and base link, zero and non-zero point;
    cent: all seven quantities against the reference and against oracle.energy, mass-scaled envs included.
    Measured maxima: see MEASURED."""
    assert TOL[name] <= CAPS[name]
    assert dev67[name] <= TOL[name], (name, dev67[name])


def test_against_reference_n1(oracle64, model):
    d = deviations(oracle64, model, 1)
    for k in d:
        assert d[k] <= TOL[k], (k, d[k])


@pytest.mark.parametrize("n", [4096, 32768])
def test_bigger_batches(n, oracle64, model):
    """the grid sizes the product uses: 64 sampled envs (first, last, a spread) of a batch holding the 67 states in turn"""
    envs = sorted(set(np.linspace(0, n - 1, 64).astype(int).tolist()))
    d = deviations(oracle64, model, 67, envs=envs, batch=n)
    for k in d:
        assert d[k] <= TOL[k], (k, d[k])


def test_gravity_compensation_at_rest(oracle64, model):
    cases = case_states(oracle64, model, 67)[:5]
    rest = []
    for s, ms in cases:
        s = s.copy()
        s[7:13] = 0
        s[13 + J:] = 0
        rest.append((s, ms))
    v = loaded_vec(rest)
    f = v.inverse_dynamics()
    gc = v.gravity_compensation()
    assert tuple(gc.shape) == (5, J) and torch.equal(gc, f[:, 6:])
    for e, (s, ms) in enumerate(rest):
        h = R.inverse_dynamics(model, s, None, ms, G)
        assert R.block_dev(f[e].cpu().numpy(), h, np.abs(h[:6]).max(), np.abs(h[6:]).max()) <= TOL["id_zero"]
        assert abs(h[2] - G * (model["mass"] * (1 if ms is None else ms)).sum()) < 1e-6 * abs(h[2])   # it carries the weight


def test_jacobian_is_the_velocity_of_link_transforms(oracle64, model):
    """J qdot against the finite-difference velocity of link_transforms across one free-flight substep (dt = 2 ms, substeps 1).
    The step moves the positions with the velocities AFTER it, so qdot is the generalised velocity after the step and J the
    Jacobian before it: what is left is the O(dt) change of J along the motion. The reference itself (dynamics_ref.jacobian on
    the same states) sets the tolerance: 2 x its own deviation + the f32 resolution of the poses, 2^-23 |x| / dt."""
    prm = {"substeps": 1, "link_damping": 0.0}
    cases = [c for c in case_states(oracle64, model, 67) if c[0][2] > 3.5][:6]
    assert len(cases) >= 4
    v = loaded_vec(cases, params=prm, control_mode="torque")
    links = probe_links(model)
    dt = 0.002
    st0 = v.get_state().cpu().numpy().astype(np.float64)
    T0 = v.link_transforms().cpu().numpy().astype(np.float64)
    Jg = {nm: v.jacobian(l).cpu().numpy().astype(np.float64) for nm, l in links.items()}
    v.step_tensor(torch.zeros(len(cases), J, device=DEV))
    T1 = v.link_transforms().cpu().numpy().astype(np.float64)
    st1 = v.get_state().cpu().numpy().astype(np.float64)
    for e, (s, ms) in enumerate(cases):
        gv = np.concatenate([st1[e, 7:13], st1[e, 13 + J:]])
        for nm, l in links.items():
            fd = (T1[e, l, :3] - T0[e, l, :3]) / dt
            ref_dev = np.abs(R.jacobian(model, st0[e], l)[0:3] @ gv - fd).max()
            res = 2.0 ** -23 * np.abs(T0[e, l, :3]).max() / dt
            assert np.abs(Jg[nm][e, 0:3] @ gv - fd).max() <= 2 * ref_dev + 2 * res, (e, nm)


def test_centroidal_angular_momentum_is_conserved_in_free_flight(oracle64, oracle32, model):
    """5 env-steps in free flight, gravity on, link_damping 0: motors, joint damping and limits are internal, gravity has no moment
    about the COM. Drift of L allowed: what the f32 oracle shows over the same steps (in f64 arithmetic on its states) plus the
    resolution of the query itself, TOL['cent'] of |L|, at both ends."""
    from oracle import oracle as O
    prm = {"link_damping": 0.0}
    o32 = O.Oracle(model, params=prm, precision="f32")
    cases = []
    for s, ms in [c for c in case_states(oracle64, model, 67) if c[0][2] > 3.5][:4]:
        s = s.copy()
        s[2] += 20.0          # (the robot is 12 m long and the states are randomly oriented: well clear of the floor)
        cases.append((s, ms))
    v = loaded_vec(cases, params=prm)
    act = model["q_start"][model["obs_order"]].astype(np.float32)
    L0 = v.centroidal().angular_momentum.cpu().numpy().astype(np.float64)
    for _ in range(5):
        v.step_tensor(torch.tensor(np.tile(act, (len(cases), 1)), device=DEV))
    L1 = v.centroidal().angular_momentum.cpu().numpy().astype(np.float64)
    for e, (s, ms) in enumerate(cases):
        so = oracle_state(o32, s, ms)
        for _ in range(5):
            o32.step(so, act.astype(np.float64))
        l0, l1 = R.centroidal(model, s, ms, G)[9:12], R.centroidal(model, o32.get_state(so), ms, G)[9:12]
        floor = max(np.abs(l0).max(), 0.01 * R.centroidal(model, s, ms, G)[14])
        assert np.abs(L1[e] - L0[e]).max() <= np.abs(l1 - l0).max() + 2 * TOL["cent"] * floor, e


def step_tied_deviation(oracle64, model):
    """(largest deviation, per env: rows that tell tau - damping qd from tau) of the step-tied check below"""
    prm = {"substeps": 1, "link_damping": 0.0}
    dt = 0.002
    rng = np.random.default_rng(8)
    s0 = oracle64.new_state()
    oracle64.reset(s0)
    st = oracle64.get_state(s0)
    st[2] += 3.0
    n = 4
    states = np.tile(st, (n, 1))
    states[1:, 7:13] = 0.2 * rng.normal(size=(n - 1, 6))
    states[1:, 13 + J:] = 0.3 * rng.normal(size=(n - 1, J))
    states = states.astype(np.float32)
    damp = model["joint_damping"][model["obs_order"]]
    # the command carries the damping torque on top, so that the step accelerates every joint as drawn (within 10 rad/s^2):
    # 1 N m s x 0.3 rad/s of damping alone would turn a toe of 0.01 kg m^2 at 30 rad/s^2 and more through the coupling
    tau = np.array([R.random_tau(model, s.astype(np.float64), None, rng) + damp * s[13 + J:] for s in states]).astype(np.float32)
    assert np.abs(tau).max() < model_param(model, "motor_max_force")
    v = make_vec(n, params=prm, control_mode="torque")
    v.reset()
    v.set_state(torch.tensor(states))
    before = v.get_state().clone()
    v.step_tensor(torch.tensor(tau, device=DEV))
    after = v.get_state()
    vel = lambda t: torch.cat([t[:, 7:13], t[:, 13 + J:]], 1)
    a = (vel(after) - vel(before)) / dt
    assert a[:, 6:].abs().max() < 12.0          # (drawn within 10 rad/s^2: nothing is thrown)
    v.set_state(before)
    f = v.inverse_dynamics(a).cpu().numpy().astype(np.float64)
    v.close()
    worst, told = 0.0, []
    for e in range(n):
        s = states[e].astype(np.float64)
        want = np.concatenate([np.zeros(6), tau[e] - damp * s[13 + J:]])
        h = R.inverse_dynamics(model, s, None, None, G)
        bs, js = np.abs(h[:6]).max(), np.abs(want).max()
        worst = max(worst, R.block_dev(f[e], want, bs, js))
        told.append(int((np.abs(f[e, 6:] - tau[e]) > TOL["id_step"] * js).sum()))
    return worst, told


def test_inverse_dynamics_of_a_step_returns_the_commanded_torque(oracle64, model):
    """No oracle: one step of the step kernel in free flight, every joint in TORQUE mode, substeps 1, link_damping 0;
    a = (v_after - v_before) / dt, state restored, inverse dynamics of a = [0, tau - joint_damping qd]. tau from
    dynamics_ref.random_tau: every joint accelerates within 10 rad/s^2. Scale as for the round trip: joint rows over the largest
    joint torque of the case, max |tau - damping qd|, base rows over the base force (the largest base component of h).
    Tolerance TOL['id_step'] = 4 x the measured maximum (MEASURED), under the 1e-4 cap; it holds the differencing of the f32
    velocities and the step kernel's own f32 forward dynamics as well as the query. The tolerance must also TELL: against plain tau,
    without the damping term, at least a third of the joint rows of every moving env miss it. Env 0 starts at rest."""
    assert TOL["id_step"] <= CAPS["id_step"]
    worst, told = step_tied_deviation(oracle64, model)
    print("step-tied: deviation %.3g, rows that tell tau from tau - damping qd: %s of %d" % (worst, told, J))
    assert worst <= TOL["id_step"], worst
    assert told[0] == 0 and min(told[1:]) >= J // 3, told


def model_param(model, name):
    from oracle import trex_model
    return trex_model.default_params()[name]


@pytest.mark.parametrize("n", [2, 3])
def test_queries_are_read_only(n, oracle64, model):
    """warm start, contact sensor and an external wrench active; 10 steps with all four queries between every two steps are
    bitwise the 10 steps without: rows, state, contact wrench, episode steps. N = 2 steps in the pair form, N = 3 in the single."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    w = 50 * torch.randn(n, NB, 6, generator=gen, device=DEV)
    acts = [random_actions(model, n, gen) for _ in range(10)]
    landed = torch.tensor(np.array([base_cases(oracle64, model)[k][0] for k in (20, 22, 24)[:n]], np.float32))   # standing on the floor
    pair = []
    for probe in (False, True):
        v = make_vec(n, params={"warmstart": 0.85}, max_episode_steps=50)
        assert v.batch.launch_info()["block"] == (128 if n == 2 else 64)
        v.enable_contact_sensor(True)
        v.reset_tensor()
        v.set_state(landed)
        v.set_external_wrench(w)
        rows = []
        for a in acts:
            v.step_tensor(a)
            rows.append(v.rows.clone())
            if probe:
                out = all_queries(v, 5)
                assert all(torch.isfinite(o).all() for o in out)
        steps = torch.zeros(n, dtype=torch.int32, device=DEV)
        v.batch.get_episode_steps(steps)
        pair.append((torch.stack(rows), v.get_state(), v.contact_wrench().clone(), steps))
    for x, y in zip(*pair):
        assert torch.equal(x, y)
    assert pair[0][2].abs().sum() > 0


def test_refusals(model):
    from trex_gym import _capi as capi
    n = 5
    v = make_vec(n)
    ref = make_vec(n)
    v.reset_tensor()
    ref.reset_tensor()
    b = v.batch
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = capi.lib
    xyz = (C.c_double * 3)(0.0, 0.0, 0.0)
    nan = (C.c_double * 3)(0.0, float("nan"), 0.0)
    sizes = dict(id=n * D, mass=n * D * D, jac=n * 6 * D, cent=n * 16)
    good = {k: torch.zeros(x, device=DEV) for k, x in sizes.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    call = dict(id=lambda p: lib.trex_batch_inverse_dynamics(b.h, None, p, s),
                mass=lambda p: lib.trex_batch_mass_matrix(b.h, p, s),
                jac=lambda p: lib.trex_batch_jacobian(b.h, 3, xyz, p, s),
                cent=lambda p: lib.trex_batch_centroidal(b.h, p, s))
    hip = C.CDLL("libamdhip64.so")
    for k, f in call.items():
        assert f(ptr(good[k])) == 0
        host = np.zeros(sizes[k], np.float32)
        assert f(C.c_void_p(host.ctypes.data)) == capi.E_INVALID, k                    # a host pointer
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(4 * sizes[k] - 4)) == 0           # one float short
        try:
            assert f(p) == capi.E_INVALID, k
        finally:
            hip.hipFree(p)
    host = np.zeros(n * D, np.float32)
    assert lib.trex_batch_inverse_dynamics(b.h, C.c_void_p(host.ctypes.data), ptr(good["id"]), s) == capi.E_INVALID
    nl = len(v.model.links())
    assert lib.trex_batch_jacobian(b.h, -1, xyz, ptr(good["jac"]), s) == capi.E_INVALID
    assert lib.trex_batch_jacobian(b.h, nl, xyz, ptr(good["jac"]), s) == capi.E_INVALID
    assert lib.trex_batch_jacobian(b.h, nl - 1, xyz, ptr(good["jac"]), s) == 0
    assert lib.trex_batch_jacobian(b.h, 3, nan, ptr(good["jac"]), s) == capi.E_INVALID
    with pytest.raises(capi.TrexError):
        b.mass_matrix(torch.zeros(n, D, D))                                           # the Python layer: a host tensor
    with pytest.raises(capi.TrexError):
        b.jacobian(0, None, torch.zeros(n, 6, D - 1, device=DEV))
    with pytest.raises(KeyError):
        v.jacobian("no_such_link")
    a = torch.zeros(n, J, device=DEV)
    v.step_tensor(a)
    ref.step_tensor(a)
    assert torch.equal(v.rows, ref.rows)


def test_stream_capture(oracle64, model):
    """the SECOND call of each query captured on one stream, one linear chain; the replay's outputs are bitwise the eager ones"""
    cases = case_states(oracle64, model, 67)
    v = loaded_vec(cases)
    n = v.num_envs
    acc = torch.randn(n, D, device=DEV)
    link = probe_links(model)["head"]
    outs = [torch.zeros(n, D, device=DEV), torch.zeros(n, D, D, device=DEV), torch.zeros(n, 6, D, device=DEV),
            torch.zeros(n, 16, device=DEV)]
    v.batch.inverse_dynamics(acc, outs[0])
    v.batch.mass_matrix(outs[1])
    v.batch.jacobian(link, (0.1, 0.0, -0.2), outs[2])
    v.batch.centroidal(outs[3])
    eager = [o.clone() for o in outs]
    assert all(o.abs().sum() > 0 for o in eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            v.batch.inverse_dynamics(acc, outs[0])
            v.batch.mass_matrix(outs[1])
            v.batch.jacobian(link, (0.1, 0.0, -0.2), outs[2])
            v.batch.centroidal(outs[3])
    for o in outs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    for o, want in zip(outs, eager):
        assert torch.equal(o, want)


def test_outputs_off_the_16_byte_grid(oracle64, model):
    """an output that starts 4 bytes into an allocation takes the scalar stores: bitwise the same values"""
    v = loaded_vec(case_states(oracle64, model, 67)[:7])
    n = v.num_envs
    link = probe_links(model)["toe"]
    acc = torch.randn(n, D, device=DEV)
    for shape, call in (((D,), lambda o: v.batch.inverse_dynamics(acc, o)), ((D, D), lambda o: v.batch.mass_matrix(o)),
                        ((6, D), lambda o: v.batch.jacobian(link, (0.1, 0.2, 0.3), o)), ((16,), lambda o: v.batch.centroidal(o))):
        numel = n * int(np.prod(shape))
        flat = torch.full((numel + 2,), 7.0, device=DEV)
        odd = flat[1:1 + numel].view((n,) + shape)
        assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
        call(odd)
        assert torch.equal(odd, call(None))
        assert flat[0].item() == 7.0 and flat[-1].item() == 7.0


def test_nan_state_is_contained(oracle64, model):
    cases = case_states(oracle64, model, 67)[:9]
    clean = loaded_vec(cases)
    head = probe_links(model)["head"]
    want = all_queries(clean, head)
    st = clean.get_state().clone()
    slot = list(model["obs_order"]).index(int(model["head_body"]))
    st[5, 13 + slot] = float("nan")       # the head joint's angle of env 5 (second workgroup, shared with envs 4, 6, 7)
    st[2, 11] = float("nan")              # a base angular velocity of env 2
    dirty = loaded_vec(cases)
    dirty.set_state(st)
    got = all_queries(dirty, head)
    keep = [0, 1, 3, 4, 6, 7, 8]
    for g_, w_ in zip(got, want):
        assert torch.equal(g_[keep], w_[keep])
    assert all(torch.isnan(g_[5]).any() for g_ in got)        # inverse dynamics, mass matrix, the head's Jacobian, centroidal
    assert torch.isnan(got[0][2]).any() and torch.isnan(got[3][2]).any()


def test_single_env_surface(model):
    from trex_gym.trex_env import TrexBulletEnv
    env = TrexBulletEnv(urdf_path=ASSET_URDF)
    env.reset()
    f, gc, M = env.inverse_dynamics(), env.gravity_compensation(), env.mass_matrix()
    Jh, c = env.jacobian(probe_links(model)["head"]), env.centroidal()
    assert f.shape == (D,) and gc.shape == (J,) and M.shape == (D, D) and Jh.shape == (6, D)
    assert np.array_equal(gc, f[6:]) and np.array_equal(M, M.T)
    assert c.com.shape == (3,) and abs(float(c.mass) - model["mass"].sum()) < 1e-4 * model["mass"].sum()
    assert np.allclose(c.momentum, c.com_velocity * c.mass, rtol=1e-5, atol=1e-3)
    env.close()
