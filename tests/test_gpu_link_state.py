"""Link kinematics on the GPU (trex_batch_set_link_probes / trex_batch_link_state, include/trex_batch.h) against the f64
restatement tests/link_state_ref.py - itself pinned by tests/test_link_state_ref.py - and against what the batch already offers
(link_transforms, jacobian); the tiling's edges, read-only, refusals, stream capture, containment, the IMU of trex_gym.sensors
and the single-env facade.

States: those of state_sets.case_states - landing and airborne, two of them mass-scaled (the scale does not enter: this is
kinematics), every env with a state of its own.

Tolerances (TOL): 4 x the largest deviation measured on these very states at N = 67 on an MI355X (scripts/link_state_bench.py
prints them; profiles/r17_link_state.txt records them), never above the caps 1e-4 (velocity, accelerations) / 1e-5 (pose).
Scales: position over max(1 m, the env's largest |p| entry); quaternion absolute, up to sign; velocity over max(1, the env's
largest |v| entry); acceleration over max(g, the env's largest |a| entry) - the entries of the reference's [K, 6] block of that
env in the axes compared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dynamics_ref as R
import gpu_support
import link_state_ref as L
from conftest import ASSET_URDF
from gpu_support import DEV, guarded, guards_intact, loaded_vec, random_steps, replay_equals_eager
from state_sets import built_models, case_states, pick_links
from tolerances import DYNAMICS_TOL as DYN_TOL, LINK_CAPS as CAPS, LINK_MEASURED as MEASURED, LINK_TOL as TOL  # noqa: F401  (MEASURED: the docstrings' pointer)

pytestmark = pytest.mark.gpu
NB, J, D = 26, 25, 31
G = 9.81
AXES = ("world", "link", "base")

# MEASURED, CAPS, TOL at N = 67: tests/tolerances.py (the observation and proximity tests read them as well). The largest
# deviations on the generated models at N = 3 (test_synthetic_models), same profile:
MEASURED_SYN = dict(deep_chain=dict(pose=2.13e-7, velocity=2.83e-7, acc=3.17e-7), big_body=dict(pose=7.9e-8, velocity=1.11e-7, acc=1.43e-7),
                    bushy=dict(pose=1.58e-7, velocity=1.32e-7, acc=1.99e-7))
# mount_first (URDF link 0 in a moving body at depth 2: the base axes of axes="base") has no recorded entry: it is no deeper and no
# larger than the models above, and takes the largest entry per quantity
SYN_MODELS = list(MEASURED_SYN) + ["mount_first"]
SYN_LARGEST = {k: max(m[k] for m in MEASURED_SYN.values()) for k in ("pose", "velocity", "acc")}


def parity_probes(model):
    """the picked links, each at its origin and at an offset point"""
    ll = [l for l in pick_links(model) for _ in range(2)]
    pts = [p for _ in range(len(ll) // 2) for p in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1))]
    return ll, np.array(pts)


def spread_probes(model, K, seed=0):
    """K probes over all links (every link once K reaches their number), random points within 0.3 m"""
    nl = len(model["link_names"])
    rng = np.random.default_rng(seed + K)
    return ((np.arange(K) * 37 + 5) % nl).tolist(), rng.uniform(-0.3, 0.3, (K, 3))


def random_accels(model, cases, seed=3):
    rng = np.random.default_rng(seed)
    return np.array([R.random_tau(model, s, ms, rng, with_accel=True)[1] for s, ms in cases]).astype(np.float32)


def quat_dev(got, want):
    return np.minimum(np.abs(got - want).max(-1), np.abs(got + want).max(-1)).max()


def env_dev(got, ref, what):
    """largest scaled deviation of one env's [K, 7] pose or [K, 6] velocity / acceleration block (module docstring)"""
    got = np.asarray(got, np.float64)
    if what == "pose":
        return max(np.abs(got[:, :3] - ref[:, :3]).max() / max(1.0, np.abs(ref[:, :3]).max()), quat_dev(got[:, 3:], ref[:, 3:]))
    return np.abs(got - ref).max() / max(G if what == "acc" else 1.0, np.abs(ref).max())


def run_query(v, slot, K, axes, proper, accel, pose=True, vel=True, acc=True, guard=64):
    """trex_batch_link_state through _capi.Batch into NaN-filled buffers with `guard` floats around each output: the three
    outputs as numpy (None where not asked for); the guards must still be NaN"""
    n, nan = v.num_envs, float("nan")
    bufs = [guarded((n, K, width), guard, nan) if want else (None, None) for want, width in ((pose, 7), (vel, 6), (acc, 6))]
    a = None if accel is None else torch.as_tensor(accel, dtype=torch.float32).to(DEV).contiguous()
    v.batch.link_state(slot, AXES.index(axes), proper, a, *[o for _, o in bufs], probes=K)
    torch.cuda.synchronize()
    assert all(guards_intact(b, o.shape, guard, nan) for b, o in bufs if b is not None), "the call wrote outside an output"
    return [None if o is None else o.cpu().numpy() for _, o in bufs]


def check_against_reference(v, model, cases, links, pts, slot, combos, accel, worst=None):
    """every env of v against the reference for the (axes, proper) combos; -> the largest deviations {pose, velocity, acc}"""
    K, n = len(links), v.num_envs
    worst = dict(pose=0.0, velocity=0.0, acc=0.0) if worst is None else worst
    for axes, proper in combos:
        pose, vel, acc = run_query(v, slot, K, axes, proper, accel)
        assert np.isfinite(pose).all() and np.isfinite(vel).all() and np.isfinite(acc).all()
        for e in range(n):
            s = cases[e % len(cases)][0]
            r = L.link_state(model, s, links, pts, None if accel is None else accel[e].astype(np.float64), axes, proper, G)
            worst["pose"] = max(worst["pose"], env_dev(pose[e], L.pose_array(r), "pose"))
            worst["velocity"] = max(worst["velocity"], env_dev(vel[e], L.velocity_array(r), "vel"))
            worst["acc"] = max(worst["acc"], env_dev(acc[e], L.acceleration_array(r), "acc"))
    return worst


ALL_COMBOS = [(a, p) for a in AXES for p in (False, True)]


def deviations(oracle64, model, n=67):
    """the figures TOL is set from: {pose, velocity, bias, accel} over every env of n, the three axes, with and without proper"""
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    links, pts = parity_probes(model)
    h = v.link_probes(links, pts)
    acc = random_accels(model, cases)
    w0 = check_against_reference(v, model, cases, links, pts, h.slot, ALL_COMBOS, None)
    w1 = check_against_reference(v, model, cases, links, pts, h.slot, ALL_COMBOS, acc)
    v.close()
    return dict(pose=max(w0["pose"], w1["pose"]), velocity=max(w0["velocity"], w1["velocity"]), bias=w0["acc"], accel=w1["acc"])


@pytest.fixture(scope="module")
def dev67(oracle64, model):
    d = deviations(oracle64, model, 67)
    print("link_state deviations N=67:", {k: "%.3g" % x for k, x in d.items()})
    return d


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pose", "velocity", "bias", "accel"])
def test_against_reference_n67(name, dev67):
    """Every env of 67 with a state of its own; head, toe, base, deepest and a merged link, at the origin and at an offset point;
    WORLD, LINK and BASE axes; the accelerations with and without `proper`. Measured maxima: see MEASURED."""
    assert TOL[name] <= CAPS[name]
    assert dev67[name] <= TOL[name], (name, dev67[name])


# 2 ------------------------------------------------------------------------------------------------------------------------
SHAPE_K = (1, 3, 32, 33, 255, 256, 257, 1024)


@pytest.mark.parametrize("n", [1, 2, 7, 9, 67])
def test_tiling_edges(n, oracle64, model):
    """K on both sides of every change of the mapping (1: 8 envs per workgroup; 32 | 33: 8 | 7; 255 | 256 | 257: one env, one
    chunk | two chunks; 1024: four) at batch sizes that leave the last workgroup short, plus a set over all 133 links in link
    order, two probes on one link and a set of base-link probes only - all three outputs against the reference, NaN guards
    behind each. Axes and `proper` rotate over the sets."""
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    acc = random_accels(model, cases, seed=4)
    nl = len(model["link_names"])
    toe = [l for l in range(nl) if "toe" in model["link_names"][l]][0]
    sets = [spread_probes(model, K) for K in SHAPE_K]
    sets.append((list(range(nl)), np.zeros((nl, 3))))
    sets.append(([toe, toe], np.array([[0.1, 0.0, 0.0], [0.0, -0.2, 0.05]])))
    sets.append(([0, 0, 0], np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.5, -0.5]])))
    assert len(set(sets[-4][0])) == nl                     # (K = 1024 spans every link as well)
    for i, (links, pts) in enumerate(sets):
        slot = i % 8
        v.batch.set_link_probes(slot, links, pts)
        w = check_against_reference(v, model, cases, links, pts, slot, [(AXES[i % 3], bool(i % 2))], acc if i % 4 else None)
        print("N = %d, K = %d, %s%s: %s" % (n, len(links), AXES[i % 3], ", proper" if i % 2 else "", {k: "%.3g" % x for k, x in w.items()}))
        assert w["pose"] <= TOL["pose"] and w["velocity"] <= TOL["velocity"] and w["acc"] <= TOL["accel"], (n, len(links), w)
    v.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_consistent_with_link_transforms_and_jacobian(oracle64, model):
    """WORLD pose = link_transforms() composed with the local point; velocity = jacobian() @ v; acc(a) - acc(0) = J a. The
    Jacobian's entries carry DYN_TOL['jac'] of its largest entry each, so J x is good to that x max|J| x |x|_1; the link-state
    side adds its own tolerance. Then: the three instantiations agree bitwise on their common outputs, and so do two calls."""
    n = 9
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    links, pts = parity_probes(model)
    K = len(links)
    h = v.link_probes(links, pts)
    acc = random_accels(model, cases, seed=5)
    st = v.get_state().cpu().numpy().astype(np.float64)
    gv = np.concatenate([st[:, 7:13], st[:, 13 + J:]], 1)
    lt = v.link_transforms().cpu().numpy().astype(np.float64)
    pose, vel, a1 = run_query(v, h.slot, K, "world", False, acc)
    _, _, a0 = run_query(v, h.slot, K, "world", False, None)
    from oracle import trex_model as tm
    for k, (l, p) in enumerate(zip(links, pts)):
        Jg = v.jacobian(l, p).cpu().numpy().astype(np.float64)
        for e in range(n):
            want = lt[e, l, :3] + tm.quat_to_matrix(lt[e, l, 3:]) @ p
            assert np.abs(pose[e, k, :3] - want).max() <= 2 * TOL["pose"] * max(1.0, np.abs(want).max())
            assert quat_dev(pose[e, k, 3:], lt[e, l, 3:]) <= 2 * TOL["pose"]
            jmax = np.abs(Jg[e]).max()
            jv = Jg[e] @ gv[e]
            assert np.abs(vel[e, k] - jv).max() <= DYN_TOL["jac"] * jmax * np.abs(gv[e]).sum() + TOL["velocity"] * max(1.0, np.abs(vel[e]).max())
            ja = Jg[e] @ acc[e].astype(np.float64)
            lim = DYN_TOL["jac"] * jmax * np.abs(acc[e]).sum() + 2 * TOL["accel"] * max(G, np.abs(a1[e]).max(), np.abs(a0[e]).max())
            assert np.abs((a1[e, k].astype(np.float64) - a0[e, k]) - ja).max() <= lim
    # probes at link origins: the pose rows are those of link_transforms (reported, not required, to the bit)
    for axes in AXES:
        p3, v3, _ = run_query(v, h.slot, K, axes, True, acc)
        p2, v2, _ = run_query(v, h.slot, K, axes, True, None, acc=False)
        p1, _, _ = run_query(v, h.slot, K, axes, False, None, vel=False, acc=False)
        _, v1, _ = run_query(v, h.slot, K, axes, False, None, pose=False, acc=False)
        _, _, a_only = run_query(v, h.slot, K, axes, True, acc, pose=False, vel=False)
        again = run_query(v, h.slot, K, axes, True, acc)
        assert p3.tobytes() == p2.tobytes() == p1.tobytes() and v3.tobytes() == v2.tobytes() == v1.tobytes()
        assert a_only.tobytes() == again[2].tobytes() and p3.tobytes() == again[0].tobytes() and v3.tobytes() == again[1].tobytes()
    v.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return built_models(SYN_MODELS, tmp_path_factory)


def synthetic_deviation(m, n=3):
    from trex_gym.vec_env import TrexVecEnv
    om = m["om"]
    states, _ = R.random_states(om, n, seed=31)
    v = TrexVecEnv(n, urdf_path=m["path"], device=DEV, params=m["props"]["params"])
    v.reset()
    v.set_state(torch.tensor(np.array(states, np.float32)))
    cases = [(s, None) for s in states]
    nl = len(om["link_names"])
    links = list(range(nl)) + pick_links(om)
    pts = np.concatenate([np.zeros((nl, 3)), np.tile([[0.07, -0.02, 0.03]], (len(links) - nl, 1))])
    v.batch.set_link_probes(0, links, pts)
    acc = random_accels(om, cases, seed=6)
    w = check_against_reference(v, om, cases, links, pts, 0, ALL_COMBOS, acc)
    w = check_against_reference(v, om, cases, links, pts, 0, [("world", False), ("base", True)], None, w)
    v.close()
    return w


@pytest.mark.parametrize("name", SYN_MODELS)
def test_synthetic_models(name, built):
    """deep_chain (depth 6, oblique axes that are no unit vectors), big_body (the swept plate) and bushy (26 bodies, four children,
    six merged links) and mount_first (link 0 welded to body 2 behind a turned frame) at N = 3: every link at its origin and the
    picked ones at an offset point, all axes, against the reference.
    Tolerance: 4 x the deviations measured on these states (MEASURED_SYN; mount_first: the largest of them), under the same caps."""
    w = synthetic_deviation(built[name])
    print("%s link_state deviations: %s" % (name, {k: "%.3g" % x for k, x in w.items()}))
    ms = MEASURED_SYN.get(name, SYN_LARGEST)
    for k, cap in (("pose", CAPS["pose"]), ("velocity", CAPS["velocity"]), ("acc", CAPS["accel"])):
        assert w[k] <= min(4 * ms[k], cap), (name, k, w[k])


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_read_only(model):
    """state, warm-start record, contact sensor, episode counts and the next steps' rows are bitwise those of a batch that never
    made the call (the warm-start record is private: the next steps agree only if it was left alone)"""
    from trex_gym.vec_env import TrexVecEnv
    n = 33
    envs = [TrexVecEnv(n, device=DEV, params={"warmstart": 0.85}) for _ in range(2)]
    for e in envs:
        e.enable_contact_sensor(True)
        e.reset_tensor()
        random_steps(e, 5, seed=1)
    before = envs[0].get_state().clone()
    wrench = envs[0].contact_wrench().clone()
    links, pts = spread_probes(model, 300)
    h = envs[0].link_probes(links, pts)
    acc = torch.ones(n, D, device=DEV)
    for axes in AXES:
        envs[0].link_state(h, accel=acc, axes=axes, proper=True, acceleration=True)
    envs[0].link_state("cranium" if "cranium" in model["link_names"] else 1)
    envs[0].bias_acceleration(3, (0.1, 0.2, 0.3))
    assert envs[0].get_state().cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    assert envs[0].contact_wrench().cpu().numpy().tobytes() == wrench.cpu().numpy().tobytes()
    assert (envs[0].episode_steps == envs[1].episode_steps).all()
    rows = []
    for e in envs:
        random_steps(e, 2, seed=2)
        rows.append(e.rows.cpu().numpy())
    assert rows[0].tobytes() == rows[1].tobytes()
    assert envs[0].contact_wrench().cpu().numpy().tobytes() == envs[1].contact_wrench().cpu().numpy().tobytes()
    for e in envs:
        e.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(model):
    """every TREX_E_INVALID case of the header, nothing launched: the probe table's checks, the query's, short buffers, host
    tensors, and the ninth link_probes() handle"""
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    n = 4
    env = TrexVecEnv(n, device=DEV)
    env.reset_tensor()
    b, nl = env.batch, len(model["link_names"])
    E = _capi.E_INVALID
    refused = functools.partial(gpu_support.refused, E)
    b.set_link_probes(0, [1, 2, 3], np.zeros((3, 3)))
    K = 3
    pose, vel, acc = (torch.full((n, K, w), 7.0, device=DEV) for w in (7, 6, 6))
    # the table: link range, non-finite point, set range, size range - and nothing changed: set 0 still answers with K = 3
    refused(b.set_link_probes, 0, [nl], np.zeros((1, 3)))
    refused(b.set_link_probes, 0, [-1], np.zeros((1, 3)))
    refused(b.set_link_probes, 0, [1, 2], np.array([[0, 0, 0], [0, np.nan, 0]]))
    refused(b.set_link_probes, 0, [1], np.array([[np.inf, 0, 0]]))
    refused(b.set_link_probes, 8, [1], np.zeros((1, 3)))
    refused(b.set_link_probes, -1, [1], np.zeros((1, 3)))
    refused(b.set_link_probes, 0, [1] * 1025, np.zeros((1025, 3)))
    b.link_state(0, 0, False, None, pose, vel, acc, probes=K)
    torch.cuda.synchronize()
    assert torch.isfinite(pose).all() and not (pose == 7.0).all()
    raw = _capi.lib.trex_batch_set_link_probes
    assert raw(b.h, 0, None, None, 2) == E and raw(b.h, 0, None, None, -1) == E
    # the query: empty / never-set / out-of-range set, axes, all outputs NULL
    for o in (pose, vel, acc):
        o.fill_(7.0)
    refused(b.link_state, 1, 0, False, None, pose, vel, acc)           # never set
    b.set_link_probes(2, [1], np.zeros((1, 3)))
    b.set_link_probes(2, [])                                          # freed
    refused(b.link_state, 2, 0, False, None, pose, vel, acc)
    refused(b.link_state, 8, 0, False, None, pose, vel, acc)
    refused(b.link_state, -1, 0, False, None, pose, vel, acc)
    refused(b.link_state, 0, 3, False, None, pose, vel, acc)
    refused(b.link_state, 0, -1, False, None, pose, vel, acc)
    refused(b.link_state, 0, 0, False, None, None, None, None)
    # host tensors, wrong dtype, one element short (the binding knows K), a wrong accel
    refused(b.link_state, 0, 0, False, None, pose.cpu(), None, None, probes=K)
    refused(b.link_state, 0, 0, False, None, None, vel.cpu(), None)
    refused(b.link_state, 0, 0, False, None, None, None, acc.cpu())
    refused(b.link_state, 0, 0, False, torch.zeros(n, D), None, None, acc)
    refused(b.link_state, 0, 0, False, None, pose.double(), None, None)
    refused(b.link_state, 0, 0, False, None, torch.empty(n * K * 7 - 1, device=DEV), None, None, probes=K)
    refused(b.link_state, 0, 0, False, None, None, torch.empty(n, K, 5, device=DEV), None, probes=K)
    refused(b.link_state, 0, 0, False, None, None, None, torch.empty(n * K * 6 - 1, device=DEV), probes=K)
    refused(b.link_state, 0, 0, False, torch.zeros(n, D - 1, device=DEV), None, None, acc, probes=K)
    torch.cuda.synchronize()
    assert (pose == 7.0).all() and (vel == 7.0).all() and (acc == 7.0).all()          # nothing was launched
    # the raw C-ABI refuses short buffers by itself (the binding's check bypassed). On 4 096 envs x 1 024 probes every output is
    # 100 MB or more - more than the allocation a small tensor lives in, whatever the allocator pooled around it
    big = TrexVecEnv(4096, device=DEV)
    big.reset_tensor()
    links, pts = spread_probes(model, 1024)
    big.batch.set_link_probes(0, links, pts)
    short = torch.full((100,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    raw = _capi.lib.trex_batch_link_state
    for args in ((None, p(short), None, None), (None, None, p(short), None), (None, None, None, p(short))):
        assert raw(big.batch.h, 0, 0, 0, *args, None) == E, args
    host = np.zeros(4096 * 1024 * 7, np.float32)
    assert raw(big.batch.h, 0, 0, 0, None, C.c_void_p(host.ctypes.data), None, None, None) == E
    torch.cuda.synchronize()
    assert (short == 7.0).all()
    big.close()
    # the ninth handle; closing one frees its slot
    env2 = TrexVecEnv(2, device=DEV)
    env2.reset_tensor()
    hs = [env2.link_probes(i) for i in range(8)]
    with pytest.raises(RuntimeError, match="probe sets"):
        env2.link_probes(9)
    hs[3].close()
    h9 = env2.link_probes(["cranium"] if "cranium" in model["link_names"] else [9])
    assert h9.slot == 3
    with pytest.raises(ValueError):
        env2.link_state(hs[3])
    with pytest.raises(ValueError):
        env.link_state(h9)                                                           # another env's handle
    assert torch.isfinite(env2.link_state(h9).position).all()
    # the batch keeps answering and stepping
    env.step_tensor(torch.zeros(n, env.J, device=DEV))
    b.link_state(0, 0, False, None, pose, vel, acc, probes=K)
    torch.cuda.synchronize()
    assert torch.isfinite(pose).all() and torch.isfinite(env.obs).all()
    env.close()
    env2.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_stream_capture(oracle64, model):
    """link_state inside torch.cuda.graph on one stream after a warm-up call; after a state change the replay is bitwise the
    eager call"""
    n = 8
    cases = case_states(oracle64, model, 2 * n)
    v = loaded_vec(cases[:n])
    links, pts = spread_probes(model, 40)
    K = len(links)
    h = v.link_probes(links, pts)
    acc = torch.tensor(random_accels(model, cases[:n], seed=7), device=DEV)
    outs = [torch.empty(n, K, w, device=DEV) for w in (7, 6, 6)]
    call = lambda o: v.batch.link_state(h.slot, 2, True, acc, *o, probes=K)
    replay_equals_eager(call, outs, lambda: v.set_state(torch.tensor(np.array([c[0] for c in cases[n:]], np.float32))))
    v.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 300])
def test_containment(K, oracle64, model):
    """one env with a NaN state: NaN outputs for that env, the others bitwise unchanged (K = 5: the env shares its workgroup with
    seven others; 300: it has two of its own)"""
    n = 11
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    links, pts = spread_probes(model, K)
    v.batch.set_link_probes(0, links, pts)
    acc = random_accels(model, cases, seed=8)
    good = run_query(v, 0, K, "base", True, acc)
    st = v.get_state()
    st[4] = float("nan")
    v.set_state(st)
    bad = run_query(v, 0, K, "base", True, acc)
    keep = [e for e in range(n) if e != 4]
    for g, b in zip(good, bad):
        assert np.isnan(b[4]).all()
        assert g[keep].tobytes() == b[keep].tobytes()
    v.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_imu_static_at_rest(oracle64, model):
    """zero velocities: the accelerometer reads R_link^T (0, 0, g), the gyro zero"""
    from trex_gym.sensors import Imu
    n = 9
    cases = []
    for s, ms in case_states(oracle64, model, n):
        s = s.copy()
        s[7:13] = 0
        s[13 + J:] = 0
        cases.append((s, ms))
    v = loaded_vec(cases)
    link = pick_links(model)[1]
    imu = Imu(v, link, (0.1, 0.0, 0.05))
    f, gyro = imu.static()
    f, gyro = f.cpu().numpy().astype(np.float64), gyro.cpu().numpy()
    assert (gyro == 0).all()
    for e, (s, _) in enumerate(cases):
        Rl = L.link_state(model, s, [link])["rotation"][0]
        assert np.abs(f[e] - Rl.T @ [0, 0, G]).max() <= TOL["bias"] * G
    imu.close()
    v.close()


def test_imu_read_is_the_finite_difference_of_the_velocity(oracle64, model):
    """read() after one step() = (v1 - v0) / (substeps x dt) + g z in the link's axes after the step, v0 and v1 the probe's
    world velocities the f64 reference gives at get_state() before and after. Tolerance: the f32 resolution of the velocities
    over the interval, 2^-23 |v| / (substeps x dt), x 4 - |v| the largest velocity entry that enters: the probe's world velocity
    and the env's generalised velocity, at either end."""
    from trex_gym.sensors import Imu
    n = 12
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    link, point = pick_links(model)[3], (0.05, 0.02, -0.01)
    imu = Imu(v, link, point)
    T = v.model.get_param("substeps") * v.model.get_param("dt")
    assert imu.interval == T and T > 0
    f_first, g_first = imu.read()
    f_stat, g_stat = imu.static()
    assert torch.equal(f_first, f_stat) and torch.equal(g_first, g_stat)              # the first call: static()
    s0 = v.get_state().cpu().numpy().astype(np.float64)
    act = torch.tensor(model["q_start"][model["obs_order"]].astype(np.float32)).repeat(n, 1).to(DEV)
    v.step_tensor(act)
    done = v.done.clone()
    s1 = v.get_state().cpu().numpy().astype(np.float64)
    f, gyro = imu.read()
    f, gyro = f.cpu().numpy().astype(np.float64), gyro.cpu().numpy().astype(np.float64)
    live = [e for e in range(n) if not bool(done[e])]
    assert len(live) >= n // 2
    for e in live:
        r0 = L.link_state(model, s0[e], [link], [point])
        r1 = L.link_state(model, s1[e], [link], [point])
        a = (r1["linear_velocity"][0] - r0["linear_velocity"][0]) / T + [0, 0, G]
        want = r1["rotation"][0].T @ a
        vmax = max(np.abs(r0["linear_velocity"]).max(), np.abs(r1["linear_velocity"]).max(), np.abs(s0[e, 7:13]).max(),
                   np.abs(s1[e, 7:13]).max(), np.abs(s0[e, 13 + J:]).max(), np.abs(s1[e, 13 + J:]).max())
        tol = 4 * 2.0 ** -23 * vmax / T
        print("imu env %d: |f - want| %.3g, tolerance %.3g, |f| %.3g" % (e, np.abs(f[e] - want).max(), tol, np.abs(want).max()))
        assert np.abs(f[e] - want).max() <= tol, (e, f[e], want)
        assert np.abs(gyro[e] - r1["rotation"][0].T @ r1["angular_velocity"][0]).max() <= TOL["velocity"] * max(1.0, np.abs(r1["angular_velocity"]).max())
    imu.close()
    v.close()


def test_imu_takes_no_difference_across_an_episode_boundary(model):
    from trex_gym.sensors import Imu
    from trex_gym.vec_env import TrexVecEnv
    n = 6
    v = TrexVecEnv(n, urdf_path=ASSET_URDF, device=DEV, max_episode_steps=1)
    v.reset_tensor()
    imu = Imu(v, pick_links(model)[1])
    imu.read()
    act = torch.tensor(model["q_start"][model["obs_order"]].astype(np.float32)).repeat(n, 1).to(DEV)
    v.step_tensor(act)
    assert bool(v.done.all())                                       # the limit of 1: every env has been restarted
    f, gyro = imu.read(v.done)
    fs, gs = imu.static()
    assert torch.equal(f, fs) and torch.equal(gyro, gs)
    mixed = v.done.clone()
    mixed[::2] = False
    v.step_tensor(act)
    f2, _ = imu.read(mixed)
    fs2, _ = imu.static()
    assert torch.equal(f2[1::2], fs2[1::2]) and not torch.equal(f2[::2], fs2[::2])
    imu.close()
    v.close()


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_facade_agrees_with_a_one_env_batch(model):
    from trex_gym.trex_env import TrexBulletEnv
    from trex_gym.vec_env import TrexVecEnv
    env = TrexBulletEnv(urdf_path=ASSET_URDF)
    env.reset()
    v = TrexVecEnv(1, urdf_path=ASSET_URDF, device=DEV)
    v.reset()
    a = model["q_start"][model["obs_order"]].astype(np.float32) + 0.05
    for _ in range(3):
        env.step(a)
    v.set_state(env._vec.get_state())
    links = pick_links(model)
    acc = np.linspace(-1, 1, D).astype(np.float32)
    got = env.link_state(links, accel=acc, axes="base", proper=True, acceleration=True)
    want = v.link_state(links, accel=acc[None], axes="base", proper=True, acceleration=True)
    for g, w in zip(got, want):
        assert g.shape == tuple(w.shape[1:]) and g.tobytes() == w[0].cpu().numpy().tobytes()
    only = env.link_state(links[1], velocity=False)
    assert only.position.shape == (1, 3) and only.linear_velocity is None and only.angular_acceleration is None
    b = env.bias_acceleration(links[3], (0.1, 0.0, 0.0))
    assert b.shape == (6,) and b.tobytes() == v.bias_acceleration(links[3], (0.1, 0.0, 0.0))[0].cpu().numpy().tobytes()
    z = v.link_state(v.link_probes([links[3]], [(0.1, 0.0, 0.0)]), acceleration=True)
    assert torch.equal(torch.cat([z.linear_acceleration, z.angular_acceleration], -1)[:, 0], v.bias_acceleration(links[3], (0.1, 0.0, 0.0)))
    env.close()
    v.close()
