"""Proximity between bodies on the GPU (trex_batch_set_proximity_shapes / trex_batch_proximity, include/trex_batch.h) against the
f64 restatement tests/proximity_ref.py - itself pinned by tests/test_proximity_ref.py - on the default T-rex table, the synthetic
geometry cases of tests/proximity_cases.py and generated models; the tiling's edges, a cross-check with link_state, read-only,
refusals, stream capture, containment and the Python surface.

States: those of state_sets.case_states, every env with a state of its own. Tables: f32-exact, so the batch and the
reference hold the same capsules.

What is compared, per env and pair (check_env):
  distance   |d - d_ref| over scale = max(1 m, the env's largest |body-origin coordinate|). TOL = 4 x the largest deviation
             measured on these very states at N = 67 on an MI355X (scripts/proximity_bench.py prints them, profiles/r18_proximity.txt
             records them: MEASURED), never above the cap 1e-5 - link_state's pose cap, for the same f32 forward kinematics.
  winner     the capsule indices are the reference's wherever its runner-up is more than 1e-4 m behind; elsewhere any test of
             the pair within that gap of the reference's minimum is accepted. No pair is left out.
  certificate, on the capsules the kernel returned - so it holds where the closest points are not unique: |n| = 1 to TOL;
             point_a + rA n lies on A's segment and point_b - rB n on B's to TOL x scale; (point_a - point_b) . n = distance to
             TOL x scale.
  direction  n against the reference's where its axis distance exceeds 0.01 m and the winner is the reference's, to
             4 x TOL x scale / axis distance: the direction error is the point error over the lever."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dynamics_ref as R
import gpu_support
import proximity_cases as PC
import proximity_ref as PR
from conftest import ASSET_URDF
from gpu_support import DEV, guarded, guards_intact, loaded_vec, make_vec, random_actions, replay_equals_eager
from state_sets import base_cases, built_models, case_states, pick_links
from tolerances import LINK_TOL

pytestmark = pytest.mark.gpu
NB, J = 26, 25
GAP = 1e-4
CAP = 1e-5

# The largest distance deviation measured on an MI355X (profiles/r18_proximity.txt): the default T-rex table with all 253 pairs at
# N = 67. Tolerance = 4 x measured, never above the cap; the one tolerance holds for every check of this file. (Seen elsewhere, for
# the record: the synthetic cases 1.2e-8, deep_chain 3.3e-8, big_body 3.3e-8, bushy 2.1e-8 - all at N = 3, close to the base.)
MEASURED = dict(trex=3.73e-7)
TOL = {k: min(4 * MEASURED["trex"], CAP) for k in ("trex", "cases", "deep_chain", "big_body", "bushy")}

OUTS = ("distance", "point_a", "point_b", "normal", "capsule")
WIDTH = dict(distance=1, point_a=3, point_b=3, normal=3, capsule=2)


def run_query(batch, P, only=OUTS, guard=64):
    """trex_batch_proximity through _capi.Batch into NaN-filled (capsule: -7-filled) buffers with `guard` elements around each
    output: {name: numpy} of the outputs asked for; the guards must be intact"""
    n = batch.num_envs
    fill = {name: (-7, torch.int32) if name == "capsule" else (float("nan"), torch.float32) for name in OUTS}
    bufs = {name: guarded((n, P) if WIDTH[name] == 1 else (n, P, WIDTH[name]), guard, *fill[name]) for name in OUTS if name in only}
    batch.proximity(*[bufs[name][1] if name in bufs else None for name in OUTS], pairs=P)
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        assert guards_intact(whole, view.shape, guard, fill[name][0]), "the call wrote outside " + name
    return {name: view.cpu().numpy() for name, (_, view) in bufs.items()}


def point_to_segment(x, p0, p1):
    """[P] distances of the points x [P, 3] from the segments p0 p1"""
    d = p1 - p0
    dd = (d * d).sum(1)
    u = np.clip(np.where(dd > 0, ((x - p0) * d).sum(1) / np.where(dd > 0, dd, 1.0), 0.0), 0.0, 1.0)
    return np.linalg.norm(x - (p0 + u[:, None] * d), axis=1)


_REF = {}


def reference(key, model, state, bodies, caps, pairs):
    """PR.proximity and the world capsules, computed once per key"""
    if key not in _REF:
        _REF[key] = (PR.proximity(model, state, bodies, caps, pairs), PR.world_capsules(model, state, bodies, caps),
                     max(1.0, float(np.abs(R.Kin(model, state).p).max())))
    return _REF[key]


FIGS = {}      # the largest figures check_env has seen, per label prefix: what scripts/proximity_bench.py prints


def check_env(got, e, ref, wc, scale, tol, label):
    """env e of `got` against its reference (module docstring); -> the largest distance deviation. Every figure is finite. The
    figures are noted in FIGS[label's first word] before anything is asserted on them."""
    d, pa, pb, n, cap = (np.asarray(got[k][e], np.float64) for k in OUTS)
    assert np.isfinite(d).all() and np.isfinite(pa).all() and np.isfinite(pb).all() and np.isfinite(n).all(), label
    d_ref = np.array([r["distance"] for r in ref])
    cap = cap.astype(int)
    A0, A1, rA = (np.array([wc[c][k] for c in cap[:, 0]]) for k in range(3))
    B0, B1, rB = (np.array([wc[c][k] for c in cap[:, 1]]) for k in range(3))
    same = np.array([tuple(cap[p]) == r["capsule"] for p, r in enumerate(ref)])
    lever = np.array([r["axis"] for r in ref])
    turn = np.array([np.abs(n[p] - r["normal"]).max() for p, r in enumerate(ref)])
    told = same & (lever > 0.01)
    fig = dict(distance=np.abs(d - d_ref).max() / scale, unit=np.abs(np.linalg.norm(n, axis=1) - 1.0).max(),
               on_a=point_to_segment(pa + rA[:, None] * n, A0, A1).max() / scale,
               on_b=point_to_segment(pb - rB[:, None] * n, B0, B1).max() / scale,
               gap=np.abs(((pa - pb) * n).sum(1) - d).max() / scale,
               direction=(turn[told] * lever[told]).max() / scale if told.any() else 0.0)
    seen = FIGS.setdefault(label.split()[0], {})
    for k, x in fig.items():
        seen[k] = max(seen.get(k, 0.0), float(x))
    # the winner
    for p, r in enumerate(ref):
        if not same[p]:
            assert r["gap"] <= GAP, (label, p, tuple(cap[p]), r["capsule"], r["gap"])
            near = [(ia, ib) for ia, ib, x in r["cands"] if x <= r["distance"] + GAP]
            assert tuple(cap[p]) in near, (label, p, tuple(cap[p]), near)
    # the certificate, on the returned capsules
    assert fig["unit"] <= tol, (label, fig)
    assert fig["on_a"] <= tol and fig["on_b"] <= tol and fig["gap"] <= tol, (label, fig, tol)
    # the direction: |n - n_ref| <= 4 tol scale / axis distance
    assert fig["direction"] <= 4 * tol, (label, fig, tol)
    return fig["distance"]


def default_table(model):
    if "table" not in _REF:
        bodies, caps = PR.fitted_table(model)
        _REF["table"] = (bodies, caps, PR.all_pairs(bodies), PR.default_pairs(model, bodies, caps))
    return _REF["table"]


def trex_deviation(oracle64, model, n=67):
    """the figure TOL['trex'] is set from: the largest distance deviation over every env of n and all 253 pairs (every other
    check of check_env asserted on the way, with the tolerance in force)"""
    bodies, caps, every, _ = default_table(model)
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    v.batch.set_proximity_shapes(bodies, caps, every)
    got = run_query(v.batch, len(every))
    worst = 0.0
    for e, (s, _) in enumerate(cases):
        ref, wc, scale = reference(("trex", n, e), model, s, bodies, caps, every)
        worst = max(worst, check_env(got, e, ref, wc, scale, TOL["trex"], "trex env %d" % e))
    v.close()
    return worst


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_against_reference_n67(oracle64, model):
    """Default T-rex table (74 capsules, the fit at max_radius 0.2, 3 divisions, min_points 4), all 253 pairs, 67 envs with a state
    of their own: distance, winner, certificate and direction of every env and pair. Measured maximum: MEASURED['trex']."""
    assert TOL["trex"] <= CAP
    dev = trex_deviation(oracle64, model)
    print("proximity distance deviation N=67: %.3g (tolerance %.3g)" % (dev, TOL["trex"]))
    assert dev <= TOL["trex"], dev


# 2 ------------------------------------------------------------------------------------------------------------------------
CASES = PC.cases()


@pytest.fixture(scope="module")
def case_env(oracle64, model):
    cases = case_states(oracle64, model, 67)[:3]
    v = loaded_vec(cases)
    yield v, cases
    v.close()


def cases_deviation(v, states, model, case):
    bodies, caps, pairs = PC.table(model, states[0][0], case)
    v.batch.set_proximity_shapes(bodies, caps, pairs)
    got = run_query(v.batch, 1)
    worst = 0.0
    for e, (s, _) in enumerate(states):
        ref, wc, scale = reference(("case", case["name"], e), model, s, bodies, caps, pairs)
        worst = max(worst, check_env(got, e, ref, wc, scale, TOL["cases"], "cases %s env %d" % (case["name"], e)))
    return worst, got


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_synthetic_cases(case, case_env, model):
    """the designed geometry at env 0's state (the same two capsules in general position in envs 1 and 2): the checks of the
    parity test; the two fallback cases additionally n = (0, 0, 1) and the distance -(rA + rB)"""
    v, states = case_env
    dev, got = cases_deviation(v, states, model, case)
    print("%s: distance deviation %.3g (tolerance %.3g)" % (case["name"], dev, TOL["cases"]))
    assert dev <= TOL["cases"], dev
    if case["fallback"]:
        scale = max(1.0, float(np.abs(R.Kin(model, states[0][0]).p).max()))
        assert np.array_equal(got["normal"][0, 0], [0.0, 0.0, 1.0])
        d = float(got["distance"][0, 0])
        assert np.isfinite(d) and abs(d + case["a"][2] + case["b"][2]) <= TOL["cases"] * scale


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full67(oracle64, model):
    """the default table, all 253 pairs, at N = 67: every output, the rows the tiling tests compare with bitwise"""
    bodies, caps, every, _ = default_table(model)
    cases = case_states(oracle64, model, 67)
    v = loaded_vec(cases)
    v.batch.set_proximity_shapes(bodies, caps, every)
    got = run_query(v.batch, len(every))
    again = run_query(v.batch, len(every))
    v.close()
    for k in OUTS:
        assert got[k].tobytes() == again[k].tobytes()          # two calls on the same state
    return cases, got


@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_rows_do_not_depend_on_the_batch_size(n, full67, model):
    """the first n of the 67 states in a batch of n: every row bitwise that of the batch of 67"""
    cases, full = full67
    bodies, caps, every, _ = default_table(model)
    v = loaded_vec(cases[:n])
    v.batch.set_proximity_shapes(bodies, caps, every)
    got = run_query(v.batch, len(every))
    v.close()
    for k in OUTS:
        assert got[k].tobytes() == full[k][:n].tobytes(), k


@pytest.mark.parametrize("P", [1, 2, 255, 256, 257, 1024])
def test_rows_do_not_depend_on_the_other_pairs(P, full67, model):
    """P pairs, the 253 repeated to fill (P = 1, 2: pairs from the middle of the list, queried nearly alone), at N = 9: column j
    is bitwise the column of its pair in the full table - one block of 256 lanes, one short of it, one more, and four"""
    cases, full = full67
    bodies, caps, every, _ = default_table(model)
    n = 9
    pick = [(100 + 77 * j) % len(every) for j in range(P)] if P <= 2 else [j % len(every) for j in range(P)]
    v = loaded_vec(cases[:n])
    v.batch.set_proximity_shapes(bodies, caps, [every[j] for j in pick])
    got = run_query(v.batch, P)
    v.close()
    for k in OUTS:
        assert got[k].tobytes() == np.ascontiguousarray(full[k][:n, pick]).tobytes(), k


def generated_capsules(rng, count):
    """capsules within 0.4 m of a body's origin, one in five a sphere, f32-exact"""
    p0 = rng.uniform(-0.3, 0.3, (count, 3))
    p1 = p0 + rng.uniform(-0.25, 0.25, (count, 3))
    p1[::5] = p0[::5]
    return PR.round_table(np.concatenate([p0, p1, rng.uniform(0.0, 0.08, (count, 1))], 1))


# (capsules on A, on B): 1, 255 and 256 tests in ONE pair, and 258 - one pair cannot hold 257 tests, a prime, within 256 capsules;
# then C = 256 as 128 x 128 = 16 384 tests, 64 trips of the 256 lanes into one LDS word
ONE_PAIR = [(1, 1), (15, 17), (16, 16), (2, 129), (128, 128)]


@pytest.mark.parametrize("ca,cb", ONE_PAIR, ids=["%dx%d" % x for x in ONE_PAIR])
def test_tests_of_one_pair(ca, cb, oracle64, model):
    """generated capsules on bodies 5 and 20, every test inside the one pair, N = 2: against the reference, all checks"""
    rng = np.random.default_rng(ca * 1000 + cb)
    bodies = np.array([5] * ca + [20] * cb, np.int32)
    caps = generated_capsules(rng, ca + cb)
    cases = case_states(oracle64, model, 67)[:2]
    v = loaded_vec(cases)
    v.batch.set_proximity_shapes(bodies, caps, [(5, 20)])
    got = run_query(v.batch, 1)
    v.close()
    for e, (s, _) in enumerate(cases):
        ref, wc, scale = reference(("one", ca, cb, e), model, s, bodies, caps, [(5, 20)])
        assert len(ref[0]["cands"]) == ca * cb
        dev = check_env(got, e, ref, wc, scale, TOL["trex"], "one_pair %dx%d env %d" % (ca, cb, e))
        assert dev <= TOL["trex"], (ca, cb, e, dev)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_consistent_with_link_state(oracle64, model):
    """spheres at link-probe points: distance + rA + rB is the distance between link_state's positions of the two points, within
    the two tolerances added"""
    n = 9
    cases = case_states(oracle64, model, 67)[:n]
    v = loaded_vec(cases)
    links = pick_links(model)
    pts = np.array([(0.1, -0.05, 0.02)] * len(links))
    lb = np.asarray(model["link_body"], int)
    tf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)
    bodies, rows = [], []
    for l, x in zip(links, pts):
        c = tf[l][:9].reshape(3, 3) @ x + tf[l][9:12]
        bodies.append(lb[l])
        rows.append(np.concatenate([c, c, [0.03 + 0.01 * len(rows)]]))
    caps = PR.round_table(rows)
    # (the rounded centre, carried back to the link frame, is the probe point: both queries then see the same point)
    local = np.array([tf[l][:9].reshape(3, 3).T @ (c[0:3] - tf[l][9:12]) for l, c in zip(links, caps)])
    of_body = {}
    for k, b in enumerate(bodies):
        of_body.setdefault(int(b), k)
    first = sorted(of_body.values())            # one sphere per body, so that a pair is one test
    bodies1, caps1 = np.array([bodies[k] for k in first], np.int32), caps[first]
    pairs = [(int(bodies1[i]), int(bodies1[j])) for i in range(len(first)) for j in range(i + 1, len(first))]
    assert len(pairs) >= 3
    v.batch.set_proximity_shapes(bodies1, caps1, pairs)
    got = run_query(v.batch, len(pairs), only=("distance",))
    h = v.link_probes([links[k] for k in first], local[first])
    pos = v.link_state(h, velocity=False).position.cpu().numpy().astype(np.float64)
    rad = {int(b): c[6] for b, c in zip(bodies1, caps1)}
    idx = {int(b): k for k, b in enumerate(bodies1)}
    for e, (s, _) in enumerate(cases):
        scale = max(1.0, float(np.abs(R.Kin(model, s).p).max()))
        for p, (a, b) in enumerate(pairs):
            want = np.linalg.norm(pos[e, idx[a]] - pos[e, idx[b]])
            assert abs(got["distance"][e, p] + rad[a] + rad[b] - want) <= (TOL["trex"] + 2 * LINK_TOL["pose"]) * scale
    v.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
SYN = ("deep_chain", "big_body", "bushy")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return built_models(SYN, tmp_path_factory)


def synthetic_deviation(m, name, n=3):
    from trex_gym.vec_env import TrexVecEnv
    om = m["om"]
    states, _ = R.random_states(om, n, seed=31)
    v = TrexVecEnv(n, urdf_path=m["path"], device=DEV, params=m["props"]["params"])
    v.reset()
    v.set_state(torch.tensor(np.array(states, np.float32)))
    bodies, caps = PR.fitted_table(om)
    pairs = PR.all_pairs(bodies)
    v.batch.set_proximity_shapes(bodies, caps, pairs)
    got = run_query(v.batch, len(pairs))
    v.close()
    worst = 0.0
    for e, s in enumerate(states):
        ref, wc, scale = reference(("syn", name, e), om, s, bodies, caps, pairs)
        worst = max(worst, check_env(got, e, ref, wc, scale, TOL[name], "%s env %d" % (name, e)))
    return worst


@pytest.mark.parametrize("name", SYN)
def test_synthetic_models(name, built):
    """deep_chain (depth 6, oblique axes), big_body (32 capsules on the plate) and bushy (26 bodies, four children) at N = 3 with
    the table fitted to their hulls and every pair of bodies: all checks, with the tolerance of the parity test."""
    dev = synthetic_deviation(built[name], name)
    print("%s proximity distance deviation: %.3g (tolerance %.3g)" % (name, dev, TOL[name]))
    assert dev <= TOL[name], (name, dev)


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_read_only(n, oracle64, model):
    """warm start, contact sensor and an external wrench active; 10 steps with a proximity query (every output) between every two
    steps are bitwise the 10 steps without: rows, state, contact wrench, episode steps. N = 2 steps in the pair form, N = 3 in the
    single."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    w = 50 * torch.randn(n, NB, 6, generator=gen, device=DEV)
    acts = [random_actions(model, n, gen) for _ in range(10)]
    landed = torch.tensor(np.array([base_cases(oracle64, model)[k][0] for k in (20, 22, 24)[:n]], np.float32))   # standing on the floor
    bodies, caps, _, chosen = default_table(model)
    pair = []
    for probe in (False, True):
        v = make_vec(n, params={"warmstart": 0.85}, max_episode_steps=50)
        assert v.batch.launch_info()["block"] == (128 if n == 2 else 64)
        v.enable_contact_sensor(True)
        v.reset_tensor()
        v.set_state(landed)
        v.set_external_wrench(w)
        if probe:
            v.proximity_shapes((bodies, caps), chosen)
        rows = []
        for a in acts:
            v.step_tensor(a)
            rows.append(v.rows.clone())
            if probe:
                out = v.closest_points(points=True)
                assert all(torch.isfinite(o.float()).all() for o in out)
        steps = torch.zeros(n, dtype=torch.int32, device=DEV)
        v.batch.get_episode_steps(steps)
        pair.append((torch.stack(rows), v.get_state(), v.contact_wrench().clone(), steps))
        v.close()
    for x, y in zip(*pair):
        assert torch.equal(x, y)
    assert pair[0][2].abs().sum() > 0


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(model):
    """every TREX_E_INVALID case of the header leaves the previous table answering as before; host pointers and short buffers are
    refused before a launch; no table is refused; num_capsules 0 frees the table"""
    from trex_gym import _capi
    n = 4
    env = make_vec(n)
    env.reset_tensor()
    b = env.batch
    E = _capi.E_INVALID
    refused = functools.partial(gpu_support.refused, E)
    dist = torch.full((n, 2), 7.0, device=DEV)
    refused(b.proximity, dist)                                                        # no table yet
    ok_b = [3, 3, 7, 9]
    ok_c = np.array([[0, 0, 0, 0.1, 0, 0, 0.05], [0, 0.1, 0, 0, 0.1, 0, 0.02], [0, 0, 0, 0, 0, 0.2, 0.03], [0.1, 0, 0, 0.1, 0, 0, 0.04]])
    ok_p = [(3, 7), (9, 3)]
    b.set_proximity_shapes(ok_b, ok_c, ok_p)
    before = run_query(b, 2)
    cap = lambda i, k, x: np.concatenate([ok_c[:i], [np.concatenate([ok_c[i][:k], [x], ok_c[i][k + 1:]])], ok_c[i + 1:]])
    bad = [
        ([3] * 257, np.tile(ok_c[0], (257, 1)), [(3, 7)]),                            # C > 256
        (ok_b, ok_c, []),                                                             # P < 1
        (ok_b, ok_c, [(3, 7)] * 1025),                                                # P > 1024
        ([3, 3, 7, NB], ok_c, ok_p), ([3, -1, 7, 9], ok_c, ok_p),                     # body out of range
        (ok_b, cap(1, 2, np.nan), ok_p), (ok_b, cap(2, 4, np.inf), ok_p),             # non-finite coordinate
        (ok_b, cap(0, 6, np.nan), ok_p), (ok_b, cap(0, 6, np.inf), ok_p), (ok_b, cap(3, 6, -0.01), ok_p),   # radius
        (ok_b, ok_c, [(3, 3)]),                                                       # A == B
        (ok_b, ok_c, [(3, 8)]), (ok_b, ok_c, [(8, 3)]), (ok_b, ok_c, [(3, NB)]),      # a body without a capsule / out of range
        ([3] * 128 + [7] * 128, np.tile(ok_c[0], (256, 1)), [(3, 7)] * 5),            # 5 x 16 384 > 65 536 tests
    ]
    for args in bad:
        refused(b.set_proximity_shapes, *args)
        after = run_query(b, 2)
        for k in OUTS:
            assert after[k].tobytes() == before[k].tobytes(), (k, args[2][:2])
    b.set_proximity_shapes([3] * 128 + [7] * 128, np.tile(ok_c[0], (256, 1)), [(3, 7)] * 4)     # exactly 65 536 tests: accepted
    b.set_proximity_shapes(ok_b, ok_c, ok_p)
    raw = _capi.lib.trex_batch_set_proximity_shapes
    assert raw(b.h, None, None, 2, None, 1) == E and raw(b.h, None, None, -1, None, 1) == E
    # the query: distance NULL, host tensors, a wrong dtype, one element short (the binding knows P)
    pts = torch.full((n, 2, 3), 7.0, device=DEV)
    idx = torch.full((n, 2, 2), 7, dtype=torch.int32, device=DEV)
    refused(b.proximity, None, pts)
    refused(b.proximity, dist.cpu())
    refused(b.proximity, dist, pts.cpu())
    refused(b.proximity, dist, None, None, None, idx.cpu())
    refused(b.proximity, dist.double())
    refused(b.proximity, dist, None, None, None, idx.float())
    refused(b.proximity, torch.empty(n * 2 - 1, device=DEV), pairs=2)
    refused(b.proximity, dist, None, torch.empty(n, 2, 2, device=DEV), pairs=2)
    refused(b.proximity, dist, None, None, None, torch.empty(n * 2 * 2 - 1, dtype=torch.int32, device=DEV), pairs=2)
    torch.cuda.synchronize()
    assert (dist == 7.0).all() and (pts == 7.0).all() and (idx == 7).all()            # nothing was launched
    # the raw C-ABI refuses short buffers and host memory by itself (the binding's check bypassed). On 4 096 envs x 1 024 pairs
    # every output is 16 MB or more - more than the allocation a small tensor lives in, whatever the allocator pooled around it
    big = make_vec(4096)
    big.reset_tensor()
    big.batch.set_proximity_shapes(ok_b, ok_c, [ok_p[j % 2] for j in range(1024)])
    good = torch.empty(4096, 1024, device=DEV)
    short = torch.full((100,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    raw = _capi.lib.trex_batch_proximity
    for args in ((p(short), None, None, None, None), (p(good), p(short), None, None, None), (p(good), None, p(short), None, None),
                 (p(good), None, None, p(short), None), (p(good), None, None, None, p(short))):
        assert raw(big.batch.h, *args, None) == E, args
    host = np.zeros(4096 * 1024, np.float32)
    assert raw(big.batch.h, C.c_void_p(host.ctypes.data), None, None, None, None, None) == E
    assert raw(big.batch.h, None, None, None, None, None, None) == E
    torch.cuda.synchronize()
    assert (short == 7.0).all()
    big.close()
    # freed: refused again; set again: answers as before; the batch keeps stepping
    b.set_proximity_shapes([])
    refused(b.proximity, dist)
    b.set_proximity_shapes(ok_b, ok_c, ok_p)
    after = run_query(b, 2)
    for k in OUTS:
        assert after[k].tobytes() == before[k].tobytes()
    env.step_tensor(torch.zeros(n, env.J, device=DEV))
    assert np.isfinite(run_query(b, 2)["distance"]).all() and torch.isfinite(env.obs).all()
    env.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_stream_capture(oracle64, model):
    """proximity inside torch.cuda.graph on one stream after a warm-up call; after a state change the replay is bitwise the
    eager call"""
    n = 8
    cases = case_states(oracle64, model, 2 * n)
    v = loaded_vec(cases[:n])
    bodies, caps, _, chosen = default_table(model)
    P = len(chosen)
    v.batch.set_proximity_shapes(bodies, caps, chosen)
    outs = [torch.empty(n, P, device=DEV)] + [torch.empty(n, P, 3, device=DEV) for _ in range(3)] + [
        torch.empty(n, P, 2, dtype=torch.int32, device=DEV)]
    call = lambda o: v.batch.proximity(*o, pairs=P)
    change = lambda: v.set_state(torch.tensor(np.array([c[0] for c in cases[n:]], np.float32)))
    replay_equals_eager(call, outs, change, changed=range(4))       # (the capsule indices may well be those of the first state)
    v.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_containment(oracle64, model):
    """one env of 5 with a NaN state: the other envs bitwise unchanged, the bad env's capsule indices capsules of the pair's
    bodies; and the same with only the base position or only one joint angle NaN"""
    n = 5
    cases = case_states(oracle64, model, 67)[:n]
    bodies, caps, every, _ = default_table(model)
    v = loaded_vec(cases)
    v.batch.set_proximity_shapes(bodies, caps, every)
    good = run_query(v.batch, len(every))
    clean = v.get_state().clone()
    keep = [e for e in range(n) if e != 3]
    for what in (slice(None), slice(0, 3), slice(13 + 7, 13 + 8)):
        st = clean.clone()
        st[3, what] = float("nan")
        v.set_state(st)
        bad = run_query(v.batch, len(every))
        for k in OUTS:
            assert good[k][keep].tobytes() == bad[k][keep].tobytes(), k
        for p, (a, b) in enumerate(every):
            ia, ib = bad["capsule"][3, p]
            assert 0 <= ia < len(bodies) and 0 <= ib < len(bodies) and bodies[ia] == a and bodies[ib] == b
    v.close()


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_python_surface(oracle64, model):
    """proximity_shapes() chooses the default table - 74 capsules, 230 pairs, the reference's choice; closest_points(),
    self_collision_distance() and in_self_collision() on the case states: the flags are the reference's (no env's minimum is
    within the tolerance of 0: tests/test_proximity_cases_host.py)"""
    n = 67
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    shapes = v.proximity_shapes()
    bodies, caps, every, chosen = default_table(model)
    assert len(shapes.bodies) == 74 and len(shapes.pairs) == 230
    assert np.array_equal(shapes.bodies, bodies) and [tuple(p) for p in shapes.pairs] == chosen
    assert np.abs(shapes.capsules.astype(np.float32).astype(np.float64) - caps).max() < 1e-6   # (the library's fit, the oracle's)
    v.proximity_shapes((bodies, caps), chosen)                       # the f32-exact table for the comparison
    d = v.closest_points()
    assert tuple(d.shape) == (n, 230) and v.closest_points() is d    # a buffer of the env
    r = v.closest_points(points=True)
    assert torch.equal(r.distance, d) and tuple(r.point_a.shape) == (n, 230, 3) and r.capsule.dtype == torch.int32
    col = {p: k for k, p in enumerate(every)}
    want, scales = [], []
    for e, (s, _) in enumerate(cases):
        ref, _, scale = reference(("trex", n, e), model, s, bodies, caps, every)
        m = min(ref[col[p]]["distance"] for p in chosen)
        assert abs(m) > TOL["trex"] * scale
        want.append(m)
        scales.append(scale)
    want = np.array(want)
    scd = v.self_collision_distance().cpu().numpy()
    assert scd.shape == (n,) and (np.abs(scd - want) <= TOL["trex"] * np.array(scales)).all()
    flags = v.in_self_collision().cpu().numpy()
    assert flags.dtype == bool and np.array_equal(flags, want < 0) and flags.any() and not flags.all()
    assert np.array_equal(v.in_self_collision(margin=0.05).cpu().numpy(), scd < 0.05)
    assert v.proximity_shapes(()) is None
    with pytest.raises(Exception):
        v.batch.proximity(d)
    v.close()


def test_primitive_collision_takes_the_models_spheres(oracle64, model):
    """collision="primitives": the default table is the spheres the physics collides with, as capsules of length 0, and the
    default pairs are the reference's for that table; distances against the reference"""
    from oracle import trex_model as tm
    om = tm.use_primitive_collision(model, 0.2, 3, 4)
    n = 3
    cases = case_states(oracle64, model, 67)[:n]
    v = loaded_vec(cases, collision="primitives")
    shapes = v.proximity_shapes()
    bodies = np.repeat(np.arange(NB), np.diff(om["hull_start"])).astype(np.int32)
    caps = PR.round_table(np.concatenate([om["hull_xyz"], om["hull_xyz"], om["hull_radius"][:, None]], 1))
    assert np.array_equal(shapes.bodies, bodies) and len(bodies) > 74
    assert np.array_equal(shapes.capsules[:, 0:3], shapes.capsules[:, 3:6]) and np.abs(shapes.capsules - caps).max() < 1e-6
    chosen = PR.default_pairs(om, bodies, caps)
    assert [tuple(p) for p in shapes.pairs] == chosen
    v.proximity_shapes((bodies, caps), chosen)
    d = v.closest_points().cpu().numpy().astype(np.float64)
    for e, (s, _) in enumerate(cases):
        ref, _, scale = reference(("spheres", e), om, s, bodies, caps, chosen)
        assert np.abs(d[e] - [r["distance"] for r in ref]).max() <= TOL["trex"] * scale
    v.close()


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
    shapes = v.proximity_shapes(exclude_adjacent=False, exclude_start_overlaps=False)
    assert len(shapes.pairs) == 253
    r = v.closest_points(points=True)
    k = [tuple(p) for p in shapes.pairs].index((4, 13))
    (got,) = env.getClosestPoints(4, 13)
    assert got[0] == 0 and got[1] == got[2] == env.ROBOT_ID and len(got) == 10
    f32 = lambda x: np.asarray(x, np.float32).tobytes()
    assert f32(got[5]) == r.point_a[0, k].cpu().numpy().tobytes() and f32(got[6]) == r.point_b[0, k].cpu().numpy().tobytes()
    assert f32(got[7]) == r.normal[0, k].cpu().numpy().tobytes() and f32([got[8]]) == r.distance[0, k:k + 1].cpu().numpy().tobytes()
    (back,) = env.getClosestPoints(13, 4)
    assert back[5] == got[6] and back[6] == got[5] and back[8] == got[8] and back[3] == got[4] and back[4] == got[3]
    assert f32(back[7]) == (-r.normal[0, k]).cpu().numpy().tobytes()
    assert env.getClosestPoints(1, 13) == []                          # body 1 carries no hull
    with pytest.raises(IndexError):
        env.getClosestPoints(0, NB)
    env.close()
    v.close()
