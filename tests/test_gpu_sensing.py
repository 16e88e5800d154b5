"""The sensor model on the GPU (trex_batch_set_sensing / _apply_sensing / _sensing_reset / _set_action_delay / _delay_actions /
_sensing_info, include/trex_sensing.h) against the numpy restatement tests/sensing_ref.py, on the cases and with the comparison of
tests/sensing_cases.py - which tests/test_sensing_cases_host.py qualifies without a GPU: n in {1, 63, 64, 65, 257}; rows 3, 75, 93
and 512 columns wide; 1, 6 and 64 groups, one of them from column 5 over 7 columns; delays 0, 1 and 8 over 20 rows; in place and
into a padded block inside guard bytes; seeded rows with planted done flags (the kernel needs no physics). Integers - the drawn
delays, and k and ep as the delay pattern shows them - are exact; uniform noise and bias within 2 ulp of the largest operand;
Gaussian columns within 4 x the case's own bound, the reference's f32 run against its f64 run; quantised columns exact away from
the rounding boundaries, at most 1 % left out. Then: sharding (env e of a batch = env 0 of a batch at env_offset e, bitwise), seeds,
stream capture, episode restarts, the reset masks, the action delay, refusals, off is off, the env end to end, and the trainer.

The largest Gaussian deviation as a share of the allowed 4 x bound is printed (-s) and recorded in profiles/r28_sensing.txt."""
import numpy as np
import pytest
import torch

import sensing_cases as SC
import sensing_ref as SR
from gpu_support import DEV, guarded, guards_intact, make_vec, random_actions, refused, same_bits

pytestmark = pytest.mark.gpu
J = 25
INVALID = -1
G, U = SR.GAUSSIAN, SR.UNIFORM
NAN = float("nan")


def env_of(kind, n, tmp_path):
    """an env whose batch has the case's observation dimension and tail"""
    from trex_gym import _capi, observations as O
    if kind == "slab":
        import synthetic_models as sm
        path, props = sm.MODELS["slab"](tmp_path / "slab")
        return make_vec(n, urdf=path, params=props["params"])
    if kind == "locomotion":
        return make_vec(n, observations=O.locomotion(_capi.Model(), DEV))
    if kind == "external":
        return make_vec(n, observations=O.external(512 - 3 * J), external=torch.zeros(n, 512 - 3 * J, device=DEV))
    if kind == "penalties":
        return make_vec(n, penalties_in_rows=True)
    return make_vec(n)


def api_of(v):
    from trex_gym import sensing_capi
    return sensing_capi.BatchSensing(v.batch)


def run_case(api, case, steps=SC.STEPS, inputs=None, check_delays=None):
    """the case's blocks through the device -> [[n, D + tail] f32 arrays]; in place or into a padded, guarded block"""
    n, width = case.n, case.D + case.tail
    got = []
    whole, out = guarded((n, width + case.pad), fill=NAN)
    delays = torch.zeros(n, len(case.groups), dtype=torch.int32, device=DEV)
    for t in range(steps):
        rows = torch.as_tensor(SC.rows_of(case, t) if inputs is None else inputs[t], device=DEV)
        if case.in_place:
            out[:, :width].copy_(rows)
            api.apply(out)
        else:
            out.fill_(NAN)
            api.apply(rows, out)
            assert same_bits(rows, torch.as_tensor(SC.rows_of(case, t) if inputs is None else inputs[t]))   # the input is only read
        torch.cuda.synchronize()
        assert guards_intact(whole, (n, width + case.pad), fill=NAN)
        assert bool(torch.isnan(out[:, width:]).all())                 # the padding of a wider stride is not written
        got.append(out[:, :width].cpu().numpy().copy())
        if check_delays is not None:
            api.info(delays=delays)
            assert (delays.cpu().numpy() == check_delays[t]).all(), "step %d: the drawn delays differ" % t
    return got


def reference_with_delays(case, **kw):
    """the f64 reference's blocks and, per step, the delays its envs hold"""
    s = SR.Sensors(case.n, case.D, case.tail, case.groups, case.seed, case.env_offset)
    ref, delays = [], []
    for t in range(SC.STEPS):
        ref.append(s.apply(SC.rows_of(case, t)))
        delays.append(s.delay[:, :len(case.groups)].copy())
    return ref, delays


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_apply_against_the_reference(case, tmp_path):
    v = env_of(case.model, case.n, tmp_path)
    assert v.batch.observation_dim() == case.D and v.rows.shape[1] == case.D + case.tail
    api = api_of(v)
    assert api.set_sensing(case.groups, case.seed, case.env_offset) == len(case.groups)
    ref, delays = reference_with_delays(case)
    packed = sum(g[1] for g in case.groups if g[7] > 0)
    assert api.info() == dict(groups=len(case.groups), delayed_columns=packed, action_delay=(0, 0))
    got = run_case(api, case, check_delays=delays)
    r = SC.compare(case, ref, got)
    print("%s: Gaussian deviation %.3f of the allowed %.3g; soft columns %.2f ulp; %.3f %% of the quantised values left out"
          % (case.name, r["gaussian_share"], 4 * SC.gaussian_bound(case), r["ulps"], 100 * r["left_out"]))
    assert not r["failures"], r["failures"][:6]
    assert r["left_out"] <= 0.01


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_a_shard_draws_what_the_whole_batch_draws():
    """env e of 65 envs = env 0 of a one-env batch at env_offset e, bit for bit over 12 rows; one seed twice agrees, another differs"""
    case = SC.CASES[1]._replace(n=65, in_place=True, pad=0)
    whole = run_case(api_seeded(make_vec(65), case), case, steps=12)
    again = run_case(api_seeded(make_vec(65), case), case, steps=12)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
    other = run_case(api_seeded(make_vec(65), case, seed=case.seed + 1), case, steps=12)
    cov = SC.column_classes(case)[0]
    assert all((a[:, :case.D][:, cov] != b[:, :case.D][:, cov]).mean() > 0.5 for a, b in zip(whole, other))
    one = make_vec(1)
    for e in (0, 1, 37, 64):
        api = api_seeded(one, case, env_offset=e)
        shard = run_case(api, case._replace(n=1), steps=12, inputs=[SC.rows_of(case, t)[e:e + 1] for t in range(12)])
        assert all(a[e:e + 1].tobytes() == b.tobytes() for a, b in zip(whole, shard)), e


def api_seeded(v, case, seed=None, env_offset=None):
    api = api_of(v)
    api.set_sensing(case.groups, case.seed if seed is None else seed, case.env_offset if env_offset is None else env_offset)
    return api


def test_graph_replay_equals_eager():
    """The launch keeps its counters on the device, so a replay is the NEXT row, not the same one: two batches with one seed, one
    applied eagerly four times, the other once eagerly (it learns the buffers) and then captured on a side stream and replayed three
    times - with a reset of half the envs inside the graph - give the same four blocks, bit for bit. (gpu_support.replay_equals_eager
    replays one call into zeroed outputs and expects the eager result; here the second call of anything differs by design.)"""
    case = SC.CASES[1]._replace(n=65)
    n, width = 65, case.D + case.tail
    mask = (torch.arange(n, device=DEV) % 2).to(torch.uint8)
    src = [torch.as_tensor(SC.rows_of(case, t), device=DEV) for t in range(4)]

    def call(api, rows, out, acts, acts_out):
        api.reset(mask)
        api.apply(rows, out)
        api.delay_actions(acts, acts_out, mask)

    envs = [make_vec(n), make_vec(n)]
    apis = [api_seeded(v, case) for v in envs]
    for a in apis:
        a.set_action_delay(0, 3)
    acts = [torch.as_tensor(SC.action_rows(5, t, n, J), device=DEV) for t in range(4)]
    eager = []
    for t in range(4):
        out, ao = torch.zeros(n, width, device=DEV), torch.zeros(n, J, device=DEV)
        call(apis[0], src[t], out, acts[t], ao)
        eager.append((out, ao))
    rows, out, a_in, a_out = torch.zeros(n, width, device=DEV), torch.zeros(n, width, device=DEV), torch.zeros(n, J, device=DEV), torch.zeros(n, J, device=DEV)
    rows.copy_(src[0])
    a_in.copy_(acts[0])
    call(apis[1], rows, out, a_in, a_out)
    torch.cuda.synchronize()
    assert same_bits(out, eager[0][0]) and same_bits(a_out, eager[0][1])
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call(apis[1], rows, out, a_in, a_out)
    for t in range(1, 4):
        rows.copy_(src[t])
        a_in.copy_(acts[t])
        out.zero_()
        a_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager[t][0]) and same_bits(a_out, eager[t][1]), t
    del graph


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_a_done_row_restarts_that_env_and_no_other():
    """bias alone on columns 0..7, a pure delay of 3 on 8..15: after a done row on env 2 its bias is another, its delayed columns
    hold the done row's values for three rows; envs 0, 1, 3 carry on. A NaN in a row passes through, late where its column is."""
    n, D = 4, 3 * J
    groups = [(0, 8, G, 0.0, 0.25, 0.0, 0, 0), (8, 8, G, 0.0, 0.0, 0.0, 3, 3)]
    api = api_of(make_vec(n))
    api.set_sensing(groups, 21, 0)
    ref = SR.Sensors(n, D, 2, groups, 21, 0)
    outs = []
    for t in range(11):
        rows = np.full((n, D + 2), float(t), np.float32)
        rows[:, D:] = 0.0
        rows[2, D + 1] = float(t == 5)
        if t == 7:
            rows[1, 3] = rows[1, 9] = np.nan
        dev = torch.as_tensor(rows, device=DEV)
        api.apply(dev)
        want = ref.apply(rows).out.astype(np.float32)
        got = dev.cpu().numpy()
        outs.append(got)
        assert np.array_equal(got[:, 8:], want[:, 8:], equal_nan=True)
        assert np.allclose(got[:, :8], want[:, :8], rtol=0, atol=2 * np.spacing(np.float32(10.0)), equal_nan=True)
    bias = lambda t: outs[t][:, :8] - np.float32(t)
    near = lambda a, b: np.abs(a - b) < 2e-6          # (out - t carries the rounding of t + bias)
    assert (bias(0) != 0).all() and near(bias(0), bias(4)).all() and near(bias(5), bias(0))[[0, 1, 3]].all()
    assert (np.abs(bias(5)[2] - bias(0)[2]) > 1e-5).all() and near(bias(10)[2], bias(5)[2]).all()
    assert (outs[4][:, 8:16] == 1.0).all() and (outs[6][2, 8:16] == 5.0).all() and (outs[6][[0, 1, 3], 8:16] == 3.0).all()
    assert np.isnan(outs[7][1, 3]) and np.isnan(outs[7]).sum() == 1 and np.isnan(outs[10][1, 9]) and np.isnan(outs[10]).sum() == 1


@pytest.mark.parametrize("which", ["none", "all", "alternate"])
def test_sensing_reset_masks(which):
    case = SC.CASES[1]._replace(n=64, done_rate=0.0, in_place=True, pad=0)
    n = case.n
    api = api_seeded(make_vec(n), case)
    ref = SR.Sensors(n, case.D, case.tail, case.groups, case.seed, case.env_offset)
    mask = dict(none=np.zeros(n, np.uint8), all=None, alternate=(np.arange(n) % 2).astype(np.uint8))[which]
    got, want, inputs = [], [], []
    for t in range(12):
        if t in (4, 9):
            api.reset(None if mask is None else torch.as_tensor(mask, device=DEV))
            ref.reset(mask)
        rows = SC.rows_of(case, t)
        dev = torch.as_tensor(rows, device=DEV)
        api.apply(dev)
        got.append(dev.cpu().numpy())
        want.append(ref.apply(rows))
        inputs.append(rows)
    r = SC.compare(case, want, got, inputs=inputs)
    assert not r["failures"], r["failures"][:6]
    marked = np.ones(n, bool) if mask is None else mask != 0
    assert (ref.ep == np.where(marked, 3, 1)).all()
    delays = torch.zeros(n, len(case.groups), dtype=torch.int32, device=DEV)
    api.info(delays=delays)
    assert (delays.cpu().numpy() == ref.delay).all()


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, stiff, lo, hi, in_place", [(1, False, 1, 1, False), (65, False, 0, 8, True), (64, True, 2, 5, False), (257, False, 8, 8, False)])
def test_delay_actions_against_the_reference(n, stiff, lo, hi, in_place):
    v = make_vec(n, variable_stiffness=stiff)
    A = v.A
    assert A == (2 * J if stiff else J)
    api = api_of(v)
    api.set_sensing((), 77, 5)                    # (no groups: the seed and the env offset of the action stream)
    api.set_action_delay(lo, hi)
    assert api.info() == dict(groups=0, delayed_columns=0, action_delay=(lo, hi))
    ref = SR.ActionDelay(n, A, lo, hi, 77, 5)
    whole, out = guarded((n, A), fill=NAN)
    drawn = torch.zeros(n, dtype=torch.int32, device=DEV)
    seen = set()
    for t in range(SC.STEPS):
        acts = SC.action_rows(3, t, n, A)
        done = None if t == 0 else SC.done_flags(3, t, n)
        if t == 13:
            api.reset(torch.as_tensor((np.arange(n) % 3 == 0).astype(np.uint8), device=DEV))
            ref.reset(np.arange(n) % 3 == 0)
        want = ref.step(acts, done)
        a = torch.as_tensor(acts, device=DEV)
        d = None if done is None else torch.as_tensor(done, device=DEV)
        if in_place:
            out.copy_(a)
            api.delay_actions(out, out, d)
        else:
            api.delay_actions(a, out, d)
        api.info(action_delays=drawn)
        torch.cuda.synchronize()
        assert guards_intact(whole, (n, A), fill=NAN)
        assert out.cpu().numpy().tobytes() == want.tobytes(), t
        assert (drawn.cpu().numpy() == ref.delay).all()
        seen |= set(ref.delay.tolist())
    assert n < 64 or seen == set(range(lo, hi + 1))           # every delay of the range is drawn


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    n, D = 8, 3 * J
    v = make_vec(n)
    api = api_of(v)
    width = D + 2
    rows = torch.as_tensor(np.random.default_rng(0).normal(size=(n, width)).astype(np.float32), device=DEV)
    whole, out = guarded((n, width), fill=5.0)
    acts = torch.zeros(n, J, device=DEV)
    wa, ao = guarded((n, J), fill=5.0)
    intact = lambda: guards_intact(whole, (n, width), fill=5.0) and bool((out == 5.0).all()) and guards_intact(wa, (n, J), fill=5.0) and bool((ao == 5.0).all())
    refused(INVALID, api.apply, rows, out)                                   # nothing set
    refused(INVALID, api.reset, None)
    refused(INVALID, api.delay_actions, acts, ao)
    refused(INVALID, api.info, torch.zeros(n, 1, dtype=torch.int32, device=DEV))
    refused(INVALID, api.info, None, torch.zeros(n, dtype=torch.int32, device=DEV))
    ok = (10, 5, G, 0.1, 0.1, 0.01, 0, 2)
    assert api.set_sensing([ok], 1, 0) == 1
    bad = [[ok, (14, 3, G, 0.0, 0.0, 0.0, 0, 0)], [(70, 6) + ok[2:]], [(-1, 2) + ok[2:]], [(0, 0) + ok[2:]], [ok[:2] + (2,) + ok[3:]],
           [ok[:3] + (-0.1,) + ok[4:]], [ok[:4] + (NAN,) + ok[5:]], [ok[:5] + (float("inf"),) + ok[6:]], [ok[:6] + (0, 9)],
           [ok[:6] + (3, 2)], [ok[:6] + (-1, 0)], [(c, 1) + ok[2:] for c in range(65)]]
    for groups in bad:
        refused(INVALID, api.set_sensing, groups, 1, 0)
    refused(INVALID, api.set_sensing, [ok], 1, 2 ** 32 - 4)                  # env_offset + n beyond 2^32
    assert api.info()["groups"] == 1 and api.num_groups == 1                 # the groups set before are intact
    first = torch.empty_like(rows)
    api.apply(rows, first)
    cov = slice(10, 15)
    assert not torch.equal(first[:, cov], rows[:, cov]) and torch.equal(first[:, :10], rows[:, :10]) and torch.equal(first[:, 15:], rows[:, 15:])
    refused(INVALID, api.apply, rows[:, :width - 1].contiguous(), out)       # a stride below 3J + tail
    refused(INVALID, api.apply, rows, out[:, :width - 1])                    # (a view that is not contiguous: refused before the call)
    refused(INVALID, api.apply, rows, torch.zeros(n, width - 1, device=DEV))
    refused(INVALID, api.apply, rows.cpu(), out)                             # host memory
    refused(INVALID, api.apply, rows, torch.zeros(n - 1, width, device=DEV))
    flat = torch.zeros(2 * n * width, device=DEV)
    refused(INVALID, api.apply, flat[:n * width].view(n, width), flat[width:width + n * width].view(n, width))   # a partial overlap
    for lo, hi in ((0, 9), (-1, 0), (3, 2)):
        refused(INVALID, api.set_action_delay, lo, hi)
    api.set_action_delay(1, 2)
    refused(INVALID, api.delay_actions, acts, torch.zeros(n * J - 1, device=DEV))
    refused(INVALID, api.delay_actions, acts.cpu(), ao)
    refused(INVALID, api.delay_actions, flat[:n * J], flat[J:J + n * J])     # a partial overlap
    v.batch.set_stiffness_actions(True, 100.0)                               # the action rows are 2J wide now
    refused(INVALID, api.delay_actions, torch.zeros(n, 2 * J, device=DEV), torch.zeros(n, 2 * J, device=DEV))
    v.batch.set_stiffness_actions(False, 100.0)
    from trex_gym import observations as O
    v.batch.set_observation(O.resolve(O.gravity(), None, J)[0])              # the observation dimension moves: 78
    refused(INVALID, api.apply, torch.zeros(n, 80, device=DEV), torch.zeros(n, 80, device=DEV))
    refused(INVALID, api.apply, rows, out)
    v.batch.set_observation(())
    torch.cuda.synchronize()
    assert intact()
    again = torch.empty_like(rows)
    api.reset(None)
    api.apply(rows, again)                                                   # back at 75 columns: the groups apply again
    assert torch.equal(again[:, :10], rows[:, :10]) and not torch.equal(again[:, cov], rows[:, cov])
    api.set_sensing(())
    api.set_action_delay(0, 0)
    assert api.info() == dict(groups=0, delayed_columns=0, action_delay=(0, 0))
    refused(INVALID, api.apply, rows, out)
    assert intact()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(model):
    """an env that never had sensors and one whose sensors were attached and taken off: the same rows, bit for bit, over 10 steps;
    a specification without effect - every magnitude 0, every delay 0 - gives rows == clean_rows, bit for bit"""
    from trex_gym import sensing as S
    n = 17
    plain, cleared, empty = (make_vec(n, max_episode_steps=7) for _ in range(3))
    S.attach(cleared, S.typical(cleared, delay=(0, 2)), action_delay=(1, 2), seed=4)
    assert cleared.sense_api is not None and cleared.clean_rows is not None and cleared.sensing["action_delay"] == [1, 2]
    with pytest.raises(ValueError):
        cleared.step_many_tensor(torch.zeros(2, n, J, device=DEV))
    S.attach(cleared, None)
    assert cleared.sensing is None and cleared.sense_api is None and cleared.clean_rows is None and cleared.clean_obs is None
    S.attach(empty, [S.noise(S.columns(empty, "q"), std=0.0), S.bias(S.columns(empty, "qd"), 0.0), S.quantize([(50, 25)], 0.0)], action_delay=0)
    assert empty.sense_api.info() == dict(groups=3, delayed_columns=0, action_delay=(0, 0)) and empty.clean_rows is not empty.rows
    gen = torch.Generator(device=DEV).manual_seed(2)
    for v in (plain, cleared, empty):
        v.reset_tensor()
    for _ in range(10):
        act = random_actions(model, n, gen)
        for v in (plain, cleared, empty):
            v.step_tensor(act)
        assert same_bits(plain.rows, cleared.rows) and same_bits(plain.rows, empty.rows) and same_bits(empty.rows, empty.clean_rows)
    assert same_bits(plain.get_state(), cleared.get_state()) and same_bits(plain.get_state(), empty.get_state())
    assert bool(plain.rows[:, 3 * J + 1].sum() == 0) and plain.episode_steps.max() == 3       # (episodes ended on the way: 10 = 7 + 3)


def test_spec_constructors_and_columns():
    from trex_gym import _capi, observations as O, sensing as S
    v = make_vec(2, observations=O.locomotion(_capi.Model(), DEV))
    assert S.columns(v, "q") == [(0, J)] and S.columns(v, "qd") == [(J, J)] and S.columns(v, "torque") == [(2 * J, J)]
    assert S.columns(v, 0) == [(75, 3)] == S.columns(v, "projected_gravity") and S.columns(v, "base_height") == [(84, 1)]
    assert len(S.columns(v, "contact_force")) == 2
    with pytest.raises(ValueError):
        S.columns(v, "prev_action")
    q = S.columns(v, "q")
    one = S.merge(S.noise(q, std=0.1), S.bias(q, 0.2), S.quantize(q, 0.01), S.latency(q, (1, 2)), S.noise(S.columns(v, "qd"), uniform=0.3))
    assert one == [S.Group(0, J, S.GAUSSIAN, 0.1, 0.2, 0.01, 1, 2), S.Group(J, J, S.UNIFORM, 0.3, 0.0, 0.0, 0, 0)]
    assert S.from_tuples(S.as_tuples(one)) == one
    for bad in (lambda: S.merge(S.noise(q, std=0.1), S.noise(q, uniform=0.1)), lambda: S.merge(S.noise(q, std=0.1), S.bias([(3, 4)], 0.1)),
                lambda: S.noise(q), lambda: S.noise(q, std=-1.0), lambda: S.latency(q, 9), lambda: S.bias(q, float("nan"))):
        with pytest.raises(ValueError):
            bad()
    t = S.typical(v)
    covered = sorted((g.col0, g.width) for g in t)
    assert covered == [(0, J), (J, J), (75, 3), (78, 3), (81, 3), (84, 1)] and all(g.delay_max == 0 for g in t)
    assert [g.noise for g in S.typical(v, scale=2.0)] == [2.0 * g.noise for g in t]
    assert all((g.delay_min, g.delay_max) == (1, 3) for g in S.typical(v, delay=(1, 3)))


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_env_end_to_end(model):
    """64 envs, episodes of 7 steps, the locomotion channels, sensing.typical with a latency of 0..2 steps and an action delay of 1..2
    steps, 30 steps under random actions: clean_rows is what an identically driven env without sensors but with the same action
    delay composes, bit for bit, and rows is the reference applied to clean_rows"""
    from trex_gym import _capi, observations as O, sensing as S
    n, steps = 64, 30
    spec = O.locomotion(_capi.Model(), DEV)
    noisy, quiet = (make_vec(n, max_episode_steps=7, observations=spec) for _ in range(2))
    S.attach(noisy, S.typical(noisy, delay=(0, 2)), action_delay=(1, 2), seed=9)
    S.attach(quiet, [], action_delay=(1, 2), seed=9)
    assert quiet.clean_rows is quiet.rows and noisy.clean_rows is not noisy.rows and noisy.obs_dim == 93
    groups = [tuple(g) for g in noisy.sensing["groups"]]
    case = SC.Case("end_to_end", "locomotion", n, 93, 2, groups, 9, 0, True, 0, 0.0)
    ref = SR.Sensors(n, 93, 2, groups, 9, noisy.env_lo)
    gen = torch.Generator(device=DEV).manual_seed(6)
    want, got, inputs = [], [], []

    def record():
        assert same_bits(noisy.clean_rows, quiet.rows)
        clean = noisy.clean_rows.cpu().numpy().copy()
        inputs.append(clean)
        want.append(ref.apply(clean))
        got.append(noisy.rows.cpu().numpy().copy())

    for v in (noisy, quiet):
        v.reset_tensor()
    ref.reset(None)
    record()
    dones = 0
    mid = random_actions(model, n, gen)
    for _ in range(steps):
        act = mid + 0.25 * (random_actions(model, n, gen) - mid)     # (a quarter of the range around a pose: qd stays at a few rad/s,
        for v in (noisy, quiet):                                      # and the case's bound, which the largest value sets, near q's scale)
            v.step_tensor(act)
        assert same_bits(noisy.done, quiet.done)
        dones += int(noisy.done.sum())
        record()
    assert dones == 4 * n                                            # 30 steps of 7-step episodes
    assert same_bits(noisy.get_state(), quiet.get_state())           # the sensors never touch the state
    r = SC.compare(case, want, got, inputs=inputs)
    print("end to end: Gaussian deviation %.3f of the allowed bound, soft columns %.2f ulp, left out %.3f %%"
          % (r["gaussian_share"], r["ulps"], 100 * r["left_out"]))
    assert not r["failures"], r["failures"][:6]
    assert not same_bits(noisy.obs, noisy.clean_obs) and same_bits(noisy.rows[:, 93:], noisy.clean_rows[:, 93:])
    # the action delay: the envs drew 1 or 2, and an env in its first step of an episode got the action it was just given
    drawn = torch.zeros(n, dtype=torch.int32, device=DEV)
    noisy.sense_api.info(action_delays=drawn)
    assert set(drawn.cpu().tolist()) == {1, 2}


def test_trainer(tmp_path):
    """three updates at 64 envs with --sensing typical, a latency and an action delay; save, load, play: the specification comes
    back, and --no_sensing leaves it off"""
    from trex_gym import trex_train
    args = trex_train.parse_args(["--sensing", "typical", "--sense_scale", "0.5", "--obs_delay", "0", "1", "--action_delay", "1", "1"])
    env = trex_train.build_environment(64, device=DEV, max_episode_steps=20, sensing=trex_train.sensing_args(args))
    assert env.sense_api.info() == dict(groups=2, delayed_columns=2 * J, action_delay=(1, 1))
    assert env.sensing["groups"][0][3] == pytest.approx(0.5 * 0.005)
    path = str(tmp_path / "agent.pt")
    agent, hist = trex_train.train(env, 3 * 64 * 32, 0, nsteps=32, noptepochs=1, save_path=path, log=lambda *_: None)
    assert len(hist) == 3 and not same_bits(env.obs, env.clean_obs)
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    assert again.env.sensing == env.sensing and again.env.sense_api.info()["action_delay"] == (1, 1)
    _, rewards = trex_train.play(again, 5, log=lambda *_: None)
    assert len(rewards) == 5 and np.isfinite(rewards).all() and not same_bits(again.env.obs, again.env.clean_obs)
    bare = trex_train.load_agent(path, num_envs=4, device=DEV, sensing=False)
    assert bare.env.sense_api is None and bare.env.sensing is None
    for bad in (["--sense_scale", "2"], ["--obs_delay", "2", "1"], ["--action_delay", "0", "9"]):
        with pytest.raises(SystemExit):
            trex_train.parse_args(bad)
