"""The planner on the device (include/trex_planner.h, csrc/planner.hip) through its C-ABI, on every case of tests/planner_cases.py,
against the numpy reference tests/planner_ref.py: what is compared bitwise and what within which tolerance is stated there. Then
the refusals, stream capture, a run sharded over groups, and trex_gym.planner.Planner on real physics."""
import numpy as np
import pytest
import torch

import planner_cases as pc
import planner_ref as ref
from gpu_support import DEV, guarded, guards_intact, make_vec, refused, replay_equals_eager, same_bits

pytestmark = pytest.mark.gpu

CASE_IDS = dict(ids=lambda c: c.name)


def _handle(case, groups=None, env_offset=None):
    """a planner of the case's shape - or of the groups [lo, hi) of it - with its nominal and noise set"""
    from trex_gym.planner_capi import PlannerHandle
    lo_g, hi_g = (0, case.G) if groups is None else groups
    h = PlannerHandle(hi_g - lo_g, case.K, case.S, case.P, case.A, case.kind, 0)
    h.set_nominal(torch.tensor(pc.nominal_of(case)[lo_g:hi_g], device=DEV))
    sigma, lo, hi = pc.noise_of(case)
    h.set_noise(sigma, lo, hi, case.seed, case.env_offset + lo_g * case.K if env_offset is None else env_offset)
    return h


def _sample(h):
    whole, actions = guarded((h.S, h.N, h.A))
    h.sample(actions)
    torch.cuda.synchronize()
    assert guards_intact(whole, (h.S, h.N, h.A))
    return actions


def _update(case, h, inp=None, temperature=None):
    """one update on the case's inputs -> dict of the guarded outputs as numpy"""
    inp = pc.inputs_of(case) if inp is None else inp
    block = torch.tensor(inp.block, device=DEV)
    terminal = None if inp.terminal is None else torch.tensor(inp.terminal, device=DEV)
    shapes = dict(returns=((h.N,), torch.float32), weights=((h.N,), torch.float32), best=((h.G,), torch.int32), stats=((h.G, 4), torch.float32))
    bufs = {k: guarded(s, fill=7 if dt == torch.int32 else 7.0, dtype=dt) for k, (s, dt) in shapes.items()}
    h.update(block[inp.reward_offset:], inp.step_stride, inp.env_stride, block[inp.done_offset:], terminal, case.gamma,
             case.temperature if temperature is None else temperature, bufs["returns"][1], bufs["weights"][1], bufs["best"][1], bufs["stats"][1])
    torch.cuda.synchronize()
    for k, (s, _) in shapes.items():
        assert guards_intact(bufs[k][0], s, fill=7 if k == "best" else 7.0), k
    assert same_bits(block, torch.tensor(inp.block))          # the inputs are read only
    return {k: v[1].cpu().numpy() for k, v in bufs.items()}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", pc.CASES, **CASE_IDS)
def test_sample(case):
    sigma, lo, hi = pc.noise_of(case)
    nominal, table = pc.nominal_of(case), ref.tap_table(case.kind, case.S, case.P)
    h, twin = _handle(case), _handle(case)
    gau, bound = pc.gaussian(case), pc.gaussian_bound(case)
    for it in (0, 1):                                      # the second sample draws with it = 1
        assert h.info()["it"] == it
        actions = _sample(h)
        knots = h.get_samples().cpu().numpy()
        assert h.info()["it"] == it + 1
        want64 = ref.sample_knots(nominal, case.K, sigma, lo, hi, case.seed, case.env_offset, it)
        want32 = ref.sample_knots(nominal, case.K, sigma, lo, hi, case.seed, case.env_offset, it, f32=True)
        # sample 0 of every group, the zero-sigma actions: everything without a draw, bit for bit
        assert _bits(knots[~gau], want32[~gau])
        assert _bits(knots[::case.K], ref.clip(nominal, lo, hi))
        if gau.any():
            err = np.abs(knots[gau].astype(np.float64) - want64[gau])
            print("%s it %d: largest Gaussian deviation %.3g = %.2f of the tolerance %.3g" % (case.name, it, err.max(), err.max() / (4 * bound), 4 * bound))
            assert err.max() <= 4 * bound
        # the action block: the interpolation of the device's OWN knots
        assert _bits(actions.cpu().numpy(), ref.actions_of(knots, table, lo, hi, f32=True))
        assert (actions.cpu().numpy() >= lo).all() and (actions.cpu().numpy() <= hi).all()
        # two runs give the same bits
        assert same_bits(_sample(twin), actions) and same_bits(twin.get_samples(), h.get_samples())
    assert same_bits(h.get_nominal(), torch.tensor(nominal))


@pytest.mark.parametrize("case", pc.CASES, **CASE_IDS)
def test_update_shift_action(case):
    sigma, lo, hi = pc.noise_of(case)
    nominal, table, inp = pc.nominal_of(case), ref.tap_table(case.kind, case.S, case.P), pc.inputs_of(case)
    G, K = case.G, case.K
    h, twin = _handle(case), _handle(case)
    _sample(h), _sample(twin)
    knots = h.get_samples().cpu().numpy()
    out = _update(case, h)
    R = out["returns"]
    assert _bits(R, ref.returns_of(inp.reward, inp.done, inp.terminal, case.gamma, f32=True))
    u64, u32, bound, tol = pc.update_bounds(case, R, knots, nominal)
    assert np.array_equal(out["best"], u32["best"])
    st = out["stats"]
    assert _bits(st[:, 0], u32["stats"][:, 0]) and _bits(st[:, 3], R[::K]) and _bits(st[:, 1], u32["stats"][:, 1])
    ess_err = np.abs(st[:, 2].astype(np.float64) - u64["stats"][:, 2])
    assert (ess_err <= tol["ess"]).all()
    w = out["weights"]
    zero = u64["weights"] == 0
    assert (w[zero] == 0).all() and (u32["weights"][zero] == 0).all()        # exact zeros, the underflow included
    w_err = np.abs(w.astype(np.float64) - u64["weights"])
    assert (w_err <= tol["weights"]).all()
    got = h.get_nominal().cpu().numpy()
    dead = out["best"] < 0
    assert _bits(got[dead], nominal[dead])                                   # a group without a finite return keeps its nominal
    if case.temperature == 0:
        assert _bits(w, u32["weights"])
        live = np.flatnonzero(~dead)
        assert _bits(got[live], knots.reshape((G, K) + knots.shape[1:])[live, out["best"][live]])
    n_err = np.abs(got.astype(np.float64) - u64["nominal"])
    assert (n_err <= tol["nominal"]).all()
    share = lambda err, t: float((err / np.broadcast_to(t, err.shape)).max())
    print("%s: shares of the tolerances - weights %.2f, nominal %.2f, effective sample size %.2f"
          % (case.name, share(w_err, tol["weights"]), share(n_err, tol["nominal"]), share(ess_err, tol["ess"])))
    # two runs give the same bits
    out2 = _update(case, twin)
    assert all(out[k].tobytes() == out2[k].tobytes() for k in out) and same_bits(twin.get_nominal(), h.get_nominal())
    # every output is nullable: the same nominal without them
    h.update(torch.tensor(inp.block, device=DEV)[inp.reward_offset:], inp.step_stride, inp.env_stride)     # (no done, no terminal)
    # the nominal's action and the shift, from the device's own nominal
    h.set_nominal(torch.tensor(got, device=DEV))
    for step in sorted({0, case.S // 2, case.S - 1}):
        whole, act = guarded((G, case.A))
        h.action(act, step)
        assert _bits(act.cpu().numpy(), ref.action_of(got, table, step, lo, hi, f32=True)) and guards_intact(whole, (G, case.A))
    now = got
    for steps in (0, 1, 1, 3, case.S + 2):
        h.shift(steps)
        now = ref.shift_of(now, case.kind, case.S, steps, f32=True)
        assert _bits(h.get_nominal().cpu().numpy(), now), steps
    assert h.info()["it"] == 1


def test_set_nominal_mask_and_info():
    case = pc.BY_NAME["wave+1"]
    h = _handle(case)
    assert h.info() == dict(groups=3, samples=65, horizon=7, knots=2, act_dim=4, interpolation=ref.LINEAR, it=0)
    other = torch.full((case.G, case.P, case.A), 0.5, device=DEV)
    h.set_nominal(other, torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV))
    got, nominal = h.get_nominal().cpu().numpy(), pc.nominal_of(case)
    assert _bits(got[[0, 2]], nominal[[0, 2]]) and (got[1] == 0.5).all()


def test_refusals_leave_the_state_unchanged():
    from trex_gym import _capi
    from trex_gym.planner_capi import PlannerHandle
    case = pc.BY_NAME["pairs"]
    E = _capi.E_INVALID
    for bad in (dict(groups=0), dict(samples=0), dict(samples=4097), dict(horizon=0), dict(horizon=257), dict(knots=0), dict(knots=3),
                dict(horizon=40, knots=33), dict(act_dim=0), dict(act_dim=65), dict(interpolation=3), dict(interpolation=-1),
                dict(groups=2 ** 17, samples=4096, horizon=256, act_dim=64), dict(device=99)):
        kw = dict(groups=1, samples=2, horizon=2, knots=2, act_dim=4, interpolation=0, device=0)
        kw.update(bad)
        refused(E, PlannerHandle, **kw)
    fresh = PlannerHandle(case.G, case.K, case.S, case.P, case.A, case.kind, 0)
    acts = torch.zeros(case.S, case.G * case.K, case.A, device=DEV)
    inp = pc.inputs_of(case)
    block = torch.tensor(inp.block, device=DEV)
    refused(E, fresh.sample, acts)                                          # before set_noise
    refused(E, fresh.update, block, inp.step_stride, inp.env_stride)
    h = _handle(case)
    _sample(h)
    _update(case, h)
    state = lambda: (h.get_nominal().clone(), h.get_samples().clone(), h.info()["it"])
    before = state()
    sigma, lo, hi = pc.noise_of(case)
    neg, nan, inf = sigma.copy(), sigma.copy(), sigma.copy()
    neg[0], nan[1], inf[2] = -0.1, np.nan, np.inf
    flipped_lo = lo.copy()
    flipped_lo[1] = hi[1] + 1
    nan_hi = hi.copy()
    nan_hi[0] = np.nan
    for s, l, u, off in ((neg, lo, hi, 0), (nan, lo, hi, 0), (inf, lo, hi, 0), (sigma, flipped_lo, hi, 0), (sigma, lo, nan_hi, 0),
                         (sigma, lo, hi, 2 ** 32 - case.G * case.K + 1)):
        refused(E, h.set_noise, s, l, u, 0, off)
    host = torch.zeros(case.S, case.G * case.K, case.A)
    refused(E, h.sample, host)
    refused(E, h.sample, acts[1:])                                          # a short buffer
    refused(E, h.sample, acts.double())
    up = lambda **kw: h.update(**dict(dict(reward=block, step_stride=inp.step_stride, env_stride=inp.env_stride, gamma=0.9, temperature=0.5), **kw))
    for kw in (dict(step_stride=0), dict(env_stride=0), dict(env_stride=-1), dict(gamma=-0.1), dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(reward=None),
               dict(reward=torch.tensor(inp.block)), dict(step_stride=inp.block.size), dict(done=block[-2:]),
               dict(returns=torch.zeros(case.G * case.K - 1, device=DEV)), dict(best=torch.zeros(case.G, device=DEV)),
               dict(stats=torch.zeros(case.G, 3, device=DEV)), dict(terminal=torch.zeros(case.G * case.K))):
        refused(E, up, **kw)
    refused(E, h.shift, -1)
    refused(E, h.action, torch.zeros(case.G, case.A, device=DEV), -1)
    refused(E, h.action, torch.zeros(case.G, case.A, device=DEV), case.S)
    refused(E, h.action, torch.zeros(case.G, case.A - 1, device=DEV), 0)
    refused(E, h.set_nominal, torch.zeros(case.G, case.P, case.A))
    refused(E, h.set_nominal, torch.zeros(case.G, case.P, case.A, device=DEV), torch.zeros(case.G - 1, dtype=torch.uint8, device=DEV))
    refused(E, h.get_samples, torch.zeros(3, device=DEV))
    if torch.cuda.device_count() > 1:
        refused(E, h.sample, acts.to("cuda:1"))
    after = state()
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2] == after[2]
    # the raw pointer check of the C-ABI itself: a buffer shorter than its strides reach
    from trex_gym.planner_capi import lib
    import ctypes as C
    short = torch.zeros(8, device=DEV)          # (a step stride of 2^28 floats reaches a GiB: beyond any allocation this one lies in)
    code = lib.trex_planner_update(h.h, C.c_void_p(short.data_ptr()), 1 << 28, inp.env_stride, None, None, 1.0, 0.0, None, None, None,
                                   None, None)
    assert code == E and b"reward" in lib.trex_last_error()
    after = state()
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2] == after[2]


def test_capture_and_replay_equal_eager():
    case = pc.BY_NAME["wave-1"]
    h, twin = _handle(case), _handle(case)
    inp = pc.inputs_of(case)
    block = torch.tensor(inp.block, device=DEV)
    acts, acts2 = (torch.zeros(case.S, case.G * case.K, case.A, device=DEV) for _ in range(2))
    h.shift(1), twin.shift(1)                                               # (the shift table of one step exists before the capture)

    def run(handle, actions, outs):
        handle.sample(actions)
        handle.update(block[inp.reward_offset:], inp.step_stride, inp.env_stride, block[inp.done_offset:], None, case.gamma, case.temperature,
                      outs[0], outs[1], outs[2], outs[3])
        handle.shift(1)
        handle.action(outs[4], 1)

    def fresh():
        n, g = case.G * case.K, case.G
        return [torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(g, dtype=torch.int32, device=DEV),
                torch.zeros(g, 4, device=DEV), torch.zeros(g, case.A, device=DEV)]

    # h: one warm-up call, then the second call captured; twin runs the same calls eagerly
    outs = fresh()
    run(h, acts, outs)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run(h, acts, outs)
    assert h.info()["it"] == 1                                              # a capture runs nothing
    eager = fresh()
    run(twin, acts2, eager)                                                 # twin's warm-up: it = 1
    for replay in range(3):
        block[inp.reward_offset::inp.env_stride][:5] += 0.25                # the replay reads the new rewards
        for o in outs:
            o.zero_()
        graph.replay()
        run(twin, acts2, eager)
        torch.cuda.synchronize()
        assert h.info()["it"] == twin.info()["it"] == replay + 2            # `it` advances across replays, on the device
        for o, want in zip(outs, eager):
            assert same_bits(o, want)
        assert same_bits(acts, acts2) and same_bits(h.get_nominal(), twin.get_nominal()) and same_bits(h.get_samples(), twin.get_samples())
    del graph

    # the helper's form on the update alone
    def update(o):
        h.update(block[inp.reward_offset:], inp.step_stride, inp.env_stride, block[inp.done_offset:], None, case.gamma, case.temperature, *o)

    def change():
        block[inp.reward_offset::inp.env_stride][:64] -= 0.5

    replay_equals_eager(update, fresh()[:4], change, replays=2, changed=[0, 3])


def test_a_run_sharded_over_groups_equals_the_whole_run():
    case = pc.BY_NAME["cubic-257"]
    K, N = case.K, case.G * case.K
    inp = pc.inputs_of(case)
    whole = _handle(case)
    acts = _sample(whole)
    ref_out = _update(case, whole)
    pieces = []
    for lo_g, hi_g in ((0, 1), (1, 3)):
        h = _handle(case, groups=(lo_g, hi_g))
        a = _sample(h)
        assert same_bits(a, acts[:, lo_g * K:hi_g * K].contiguous()) and same_bits(h.get_samples(), whole.get_samples()[lo_g * K:hi_g * K])
        e = slice(lo_g * K, hi_g * K)
        n = (hi_g - lo_g) * K
        block = np.full(case.S * n * 2, 7.0, np.float32)
        view = block.reshape(case.S, n, 2)
        view[:, :, 0], view[:, :, 1] = inp.reward[:, e], inp.done[:, e]
        part = inp._replace(block=block, reward=inp.reward[:, e], done=inp.done[:, e], terminal=inp.terminal[e], step_stride=2 * n,
                            env_stride=2, reward_offset=0, done_offset=1)
        out = _update(case, h, part)
        assert out["returns"].tobytes() == ref_out["returns"][e].tobytes() and out["weights"].tobytes() == ref_out["weights"][e].tobytes()
        assert out["best"].tobytes() == ref_out["best"][lo_g:hi_g].tobytes() and out["stats"].tobytes() == ref_out["stats"][lo_g:hi_g].tobytes()
        pieces.append(h.get_nominal())
    assert same_bits(torch.cat(pieces), whole.get_nominal())


# ---------------------------------------------------------------- trex_gym.planner.Planner on real physics

def _plants(tmp_path, which):
    if which == "trex":
        return lambda n: make_vec(n)
    import synthetic_models as sm
    path, props = sm.deep_chain(str(tmp_path))
    return lambda n: make_vec(n, urdf=path, params=props["params"])


def _settled(make, n, steps=3):
    v = make(n)
    v.reset_tensor()
    for _ in range(steps):
        v.step_tensor(torch.zeros(n, v.A, device=DEV))
    return v


@pytest.mark.parametrize("which", ["trex", "deep_chain"])
def test_predictive_sampling_never_loses_its_best_rollout(which, tmp_path):
    """temperature 0, the plant not stepped: the best sample's knots become the nominal bit for bit, so the next plan's sample 0
    replays that rollout - R[g, 0] is the previous plan's R_max[g] bit for bit, and never decreases"""
    from trex_gym.planner import Planner
    plant = _settled(_plants(tmp_path, which), 2)
    p = Planner(plant, 64, 8, temperature=0.0, sigma=0.1, seed=3)
    assert (p.G, p.K, p.S, p.P, p.N) == (2, 64, 8, 6, 128)
    state = plant.get_state().clone()
    last_max, last_r0 = None, None
    for plan in range(5):
        st = p.plan().cpu().numpy()
        assert np.isfinite(st).all() and (st[:, 0] >= st[:, 3]).all()
        if last_max is not None:
            assert st[:, 3].tobytes() == last_max.tobytes(), plan
            assert (st[:, 3] >= last_r0).all()
        last_max, last_r0 = st[:, 0].copy(), st[:, 3].copy()
        assert p.handle.info()["it"] == plan + 1
    assert same_bits(plant.get_state(), state)                              # planning does not touch the plant
    p.close()


def test_planner_step_equals_the_capi_sequence(tmp_path):
    from trex_gym.planner import Planner
    from trex_gym.planner_capi import PlannerHandle
    make = _plants(tmp_path, "trex")
    G, K, S, P = 2, 16, 6, 3
    plant, plant2 = _settled(make, G), _settled(make, G)
    p = Planner(plant, K, S, knots=P, interpolation="linear", sigma=0.05, temperature=0.2, gamma=0.9, seed=5)
    sim = make_vec(G * K, penalties_in_rows=True)
    sim.reset_tensor()
    h = PlannerHandle(G, K, S, P, plant2.A, "linear", 0)
    h.set_noise(0.05, plant2.action_space.low, plant2.action_space.high, 5, 0)
    acts = torch.zeros(S, G * K, plant2.A, device=DEV)
    rows = torch.zeros(S, G * K, sim.rows.shape[1], device=DEV)
    W, col = rows.shape[2], 3 * sim.J
    R, act = torch.zeros(G * K, device=DEV), torch.zeros(G, plant2.A, device=DEV)
    for _ in range(3):
        out = p.step()
        sim.set_state(plant2.get_state().repeat_interleave(K, 0), motors_enabled=True)
        h.sample(acts)
        sim.step_many_tensor(acts, rows)
        h.update(rows.view(-1)[col:], G * K * W, W, rows.view(-1)[col + 1:], None, 0.9, 0.2, R)
        out2 = plant2.step_tensor(h.action(act, 0))
        h.shift(1)
        assert same_bits(p.returns, R) and same_bits(p.action(0), h.action(act, 0)) and same_bits(p.nominal, h.get_nominal())
        assert all(same_bits(a, b) for a, b in zip(out, out2)) and same_bits(plant.get_state(), plant2.get_state())
    # record(): the plant's states before each step
    states = p.record(2)
    assert tuple(states.shape) == (2, G, plant.batch.state_width) and same_bits(states[0], plant2.get_state())
    # expansions per group, and the constructor's refusals by name
    p.set_domain(friction=torch.tensor([0.5, 0.9]))
    p.set_motor_gains(kp=torch.full((G, plant.J), 0.2))
    with pytest.raises(ValueError):
        p.set_domain(friction=torch.tensor([0.5, 0.9, 1.0]))
    with pytest.raises(ValueError):
        Planner(plant, K, S, rollout="parallel")
    with pytest.raises(ValueError):
        Planner(plant, K, S, interpolation="quintic")
    from trex_gym import rewards
    with pytest.raises(ValueError):
        Planner(plant, K, S, rollout="many", sim_kwargs=dict(rewards=rewards.locomotion(plant.model)))
    p.close()


def test_graphs_equal_eager_and_steps_equal_many(tmp_path):
    from trex_gym.planner import Planner
    make = _plants(tmp_path, "trex")
    G, K, S = 2, 16, 5
    kw = dict(knots=3, sigma=0.05, temperature=0.3, seed=9, iterations=2)
    planners = [Planner(_settled(make, G), K, S, **kw), Planner(_settled(make, G), K, S, use_graphs=True, **kw),
                Planner(_settled(make, G), K, S, rollout="steps", **kw)]
    for step in range(3):
        for p in planners:
            p.step()
        eager, graphs, steps = planners
        for other in (graphs, steps):
            assert same_bits(eager.returns, other.returns) and same_bits(eager.stats, other.stats), step
            assert same_bits(eager.nominal, other.nominal) and same_bits(eager.plant.get_state(), other.plant.get_state())
    assert planners[1]._graph is not None and planners[1].handle.info()["it"] == 6
    for p in planners:
        p.close()
