"""Start-state randomisation on the device (include/trex_start_state.h; csrc/start_state.hip) against tests/start_state_ref.py:
 1 through the C-ABI alone, the cases of tests/start_state_cases.py - five models, n = 1, 2, 3 and 65, every mask form -, a first apply
   and a second with done flags: draws, q, qd, offsets and untouched envs bitwise, quaternion, rotated velocities and the placement
   within the case's own bound (the shares used are printed), the deciding point equal, body_clearance at the drawn clearance, the
   rows patched and nothing else, guard bytes intact. The episode counts have no accessor: they are the counter word of the draws,
   so the second apply's values are bitwise the reference's only with the reference's counts;
 2 through TrexVecEnv, 33 envs with 7-step episodes, staggered, and fall termination that the perturbed roll trips: a twin env
   without the feature that is given the reported state of the envs that started steps bitwise the same rows - episode limit, fall,
   two consecutive ends of one env, envs that never end; the draws follow the reference's episode counts;  3 the same with
   warm-start records;  4 reset_tensor with an all-zero, an all-one and a mixed mask;  5 on an RSI state;  6 refusals launch nothing;
 7 a captured step replays;  8 terms set and cleared: the rows and the launch form of an env that never had any;  9 the trainer."""
import numpy as np
import pytest
import torch

import start_state_cases as SC
import start_state_ref as SR
from gpu_support import DEV, guarded, guards_intact, make_vec, random_action_steps, refused, same_bits
from start_state_ref import (BASE_ANGULAR_VELOCITY, BASE_LINEAR_VELOCITY, BASE_POSITION, BASE_RPY, FLOOR_CLEARANCE, JOINT_POSITION,
                             JOINT_VELOCITY)

pytestmark = pytest.mark.gpu
J = 25
INVALID = -1
CASE_NAMES = ([m + s for m in SC.MODELS for s in ("_n65_full", "_n3_masks")]
              + ["trex_n1_full", "trex_n2_full", "trex_n65_plain", "slab_n2_plain", "trex_n65_masks"])


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return SC.build(tmp_path_factory.mktemp("start_state_models"))


def env_of(b, n, **kw):
    return make_vec(n, urdf=b.path, params=b.params, collision=b.collision, **kw)


def api_of(v, terms, seed=0, env_offset=0):
    from trex_gym import start_state_capi
    api = start_state_capi.BatchStartState(v.batch)
    api.set(terms, seed, env_offset)
    return api


def read(api, n):
    """-> (values, shift, lowest) as numpy, through guard-padded buffers"""
    T = max(api.num_terms, 1)
    bufs = [guarded((n, T, 32)), guarded((n,)), guarded((n,), fill=7, dtype=torch.int32)]
    assert api.info(*(b[1] for b in bufs)) == api.num_terms
    torch.cuda.synchronize()
    assert guards_intact(bufs[0][0], (n, T, 32)) and guards_intact(bufs[1][0], (n,)) and guards_intact(bufs[2][0], (n,), fill=7)
    return [b[1].cpu().numpy() for b in bufs]


def state_of(v):
    return v.get_state().cpu().numpy()


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_the_generator_s(built):
    assert [c.name for c in SC.cases(built)] == CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_against_the_reference(name, built):
    case = {c.name: c for c in SC.cases(built)}[name]
    b, n, nj = built[case.model], case.n, SC.NJ[case.model]
    v = env_of(b, n)
    assert v.J == nj and v.model.num_bodies == nj + 1
    v.reset_tensor()
    found = state_of(v)
    assert (found == found[0]).all()
    api = api_of(v, case.terms, case.seed, case.env_offset)
    vals0, shift0, low0 = read(api, n)
    assert not vals0.any() and not shift0.any() and (low0 == -1).all()      # nothing has started since the set
    whole, rows = guarded((n, 3 * nj + 4))
    width = 3 * nj + 4
    shares = {}
    done = [np.zeros(n, np.float32), SC.done_flags(case)]
    for k in range(2):
        mark = torch.arange(n * width, device=DEV, dtype=torch.float32).view(n, width) + 0.5
        rows.copy_(mark)
        rows[:, 3 * nj + 1] = torch.as_tensor(done[k], device=DEV)
        before = rows.clone()
        rows_found = state_of(v)
        api.apply(rows, rows, 3 * nj + 1)
        torch.cuda.synchronize()
        assert guards_intact(whole, (n, width))
        got = state_of(v)
        # the f32 and the f64 run, the second apply on the states the device held
        a32, a64 = (SC.reference(case, b, found[0], f32, second=rows_found)[k] for f32 in (True, False))
        values, shift, lowest = read(api, n)
        res = SC.compare(case, a32, a64, rows_found, got, values, shift, lowest)
        assert not res["failures"], (k, res["failures"])
        for q, s in res["share"].items():
            shares[q] = max(shares.get(q, 0.0), s)
        # the rows: columns [0, 3J) of the envs that started are q | qd | zeros, everything else as found
        f = torch.as_tensor(a32.first, device=DEV)
        st = torch.as_tensor(got, device=DEV)
        assert same_bits(rows[f][:, :2 * nj], st[f][:, 13:]) and not bool(rows[f][:, 2 * nj:3 * nj].any())
        assert same_bits(rows[:, 3 * nj:], before[:, 3 * nj:]) and same_bits(rows[~f], before[~f])
        # after a placement body_clearance reports the drawn clearance
        if SC.has(case, FLOOR_CLEARANCE):
            t = [x[0] for x in case.terms].index(FLOOR_CLEARANCE)
            c = torch.zeros(n, nj + 1, device=DEV)
            v.batch.body_clearance(c, None)
            least = c.cpu().numpy().astype(np.float64).min(1)
            bound = SC.bounds(a32, a64, case)["z"]
            err = np.abs(least - values[:, t, 0].astype(np.float64))[a32.first].max()
            shares["clearance"] = max(shares.get("clearance", 0.0), err / bound)
            assert err <= bound, (k, err, bound)
            if k == 0:
                assert np.array_equal(lowest, a64.lowest) and (lowest >= 0).all()
    print("%s: largest used fraction of the bounds: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(shares.items()))))
    v.close()


# 2, 3 ---------------------------------------------------------------------------------------------------------------------
TWIN_TERMS = [(JOINT_POSITION, 0, 0, 0, -0.2, 0.2), (JOINT_VELOCITY, 0, 0, 1, -1.0, 1.0), (BASE_RPY, 0, 0, 0, -0.5, 0.5),
              (BASE_RPY, 0, 2, 0, -3.0, 3.0), (BASE_LINEAR_VELOCITY, 0, 0, 0, -0.5, 0.5), (BASE_POSITION, 0, 1, 0, -1.0, 1.0),
              (FLOOR_CLEARANCE, 0, 0, 0, 0.0, 0.02)]
MAX_TILT = 0.3      # rad: about two in five of the rolls drawn in +-0.5 lie beyond it - those envs fall at their first step


@pytest.mark.parametrize("n, warmstart", [(33, 0.0), (2, 0.0), (65, 0.0), (3, 0.5)], ids=["n33", "n2", "n65", "n3_warmstart"])
def test_a_twin_given_the_reported_state_steps_the_same_rows(n, warmstart, model):
    """16 steps. a has the feature, b not; behind every step b is given a's state for the envs that started, and must then step
    the same rows. An env that does not start is never given anything: it tracks its twin bit for bit from the reset on. With
    warm-start records there is no fall criterion and no stagger, so that all envs start at one step: set_state empties every
    record of b, as the apply launch empties those of the envs that start."""
    from trex_gym import start_state as S
    limit = 7
    kw = dict(max_episode_steps=limit, terminate=None if warmstart else dict(max_tilt=MAX_TILT),
              params=dict(warmstart=warmstart) if warmstart else None)
    a, b = make_vec(n, **kw), make_vec(n, **kw)
    S.attach(a, S.from_tuples(TWIN_TERMS), seed=11)
    assert a.start_values.shape == (n, len(TWIN_TERMS), 32) and a.start_state["seed"] == 11
    b.reset_tensor()
    s0 = state_of(b)[0]
    ref = SR.StartState(model, n, TWIN_TERMS, seed=11, env_offset=0, floor_z=float(a.model.get_param("floor_z")), f32=True)
    a.reset_tensor()
    want = ref.apply(np.zeros(n), np.tile(s0, (n, 1)))
    sa = state_of(a)
    assert sa[:, 13:].tobytes() == want.state[:, 13:].astype(np.float32).tobytes()
    assert same_bits(a.obs[:, :2 * J], torch.as_tensor(sa[:, 13:], device=DEV)) and not bool(a.obs[:, 2 * J:].any())
    b.batch.set_state(a.get_state())
    if not warmstart:
        stagger = torch.arange(n, device=DEV, dtype=torch.int32) % limit
        a.set_episode_steps(stagger)
        b.set_episode_steps(stagger)
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=a.model.lower, q_upper=a.model.upper), 16, n, 3)
    ends = np.zeros(n, int)
    twice = falls = 0
    last = np.zeros(n, bool)
    for t in range(16):
        before = state_of(b)
        a.step_tensor(actions[t])
        b.step_tensor(actions[t])
        done = a.done.cpu().numpy()
        assert np.array_equal(done, b.done.cpu().numpy()), t
        d = torch.as_tensor(done, device=DEV)
        assert same_bits(a.rows[:, 3 * J:], b.rows[:, 3 * J:]) and same_bits(a.rows[~d], b.rows[~d]), t
        sa, sb = state_of(a), state_of(b)
        assert sa[~done].tobytes() == sb[~done].tobytes(), t
        if done.any():      # b holds what the reset inside the launch left: the state a's launch found
            want = ref.apply(done.astype(np.float32), sb)
            assert sa[done][:, 13:].tobytes() == want.state[done][:, 13:].astype(np.float32).tobytes(), t
            a.start_api.info(values=a.start_values)
            assert a.start_values.cpu().numpy().tobytes() == want.values.astype(np.float32).tobytes(), t
            assert same_bits(a.rows[d][:, :2 * J], torch.as_tensor(sa[done][:, 13:], device=DEV)) and not bool(a.rows[d][:, 2 * J:3 * J].any())
            assert np.abs(np.linalg.norm(sa[:, 3:7].astype(np.float64), axis=1) - 1).max() < 1e-6
            assert not warmstart or done.all()
            b.batch.set_state(torch.as_tensor(np.where(done[:, None], sa, sb), device=DEV))
        falls += 0 if warmstart else int((a.termination_reason != 0).sum())
        twice += int((done & last).sum())
        last = done
        ends += done
    assert ends.min() >= 2                   # (7-step episodes over 16 steps: every env ends at least twice)
    if n >= 33:                              # falls, and an env that ends at two consecutive steps
        assert falls > 0 and twice > 0
    a.close(); b.close()


def test_an_env_that_never_ends_tracks_a_twin_without_the_feature():
    """no limit, no termination: behind the first apply nothing starts, and the rows of 8 steps are the twin's bit for bit"""
    from trex_gym import start_state as S
    n = 3
    a, b = make_vec(n), make_vec(n)
    S.attach(a, S.from_tuples(TWIN_TERMS), seed=2)
    a.reset_tensor(); b.reset_tensor()
    b.batch.set_state(a.get_state())
    a.start_api.info(values=a.start_values)
    v0 = a.start_values.clone()
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=a.model.lower, q_upper=a.model.upper), 8, n, 5)
    for t in range(8):
        a.step_tensor(actions[t]); b.step_tensor(actions[t])
        assert same_bits(a.rows, b.rows) and same_bits(a.get_state(), b.get_state()), t
    a.start_api.info(values=a.start_values)
    assert same_bits(a.start_values, v0)
    with pytest.raises(ValueError):
        a.step_many_tensor(actions[:2])
    S.attach(a, None)
    assert a.start_api is None and a.start_state is None and a.start_values is None
    a.step_many_tensor(actions[:2])
    with pytest.raises(ValueError):
        S.attach(a, [])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_reset_tensor_with_an_all_zero_an_all_one_and_a_mixed_mask(model):
    from trex_gym import start_state as S
    n = 5
    a, b = make_vec(n), make_vec(n)
    S.attach(a, S.from_tuples(TWIN_TERMS), seed=4)
    b.reset_tensor()
    s0 = state_of(b)[0]
    ref = SR.StartState(model, n, TWIN_TERMS, seed=4, floor_z=float(a.model.get_param("floor_z")), f32=True)
    a.reset_tensor()
    want = ref.apply(np.zeros(n), np.tile(s0, (n, 1)))
    ep = np.ones(n, np.int64)
    for mask in (np.zeros(n, np.uint8), np.ones(n, np.uint8), np.array([1, 0, 0, 1, 0], np.uint8)):
        before = state_of(a)
        a.reset_tensor(torch.as_tensor(mask, device=DEV))
        ref.reset(mask)
        m = mask != 0
        want = ref.apply(np.zeros(n), np.where(m[:, None], s0, before))
        got = state_of(a)
        assert got[~m].tobytes() == before[~m].tobytes()
        assert got[m][:, 13:].tobytes() == want.state[m][:, 13:].astype(np.float32).tobytes()
        assert got[:, :2].tobytes() == want.state[:, :2].astype(np.float32).tobytes()
        a.start_api.info(values=a.start_values)
        assert a.start_values.cpu().numpy().tobytes() == want.values.astype(np.float32).tobytes()
        ep += m
        assert np.array_equal(want.ep, ep)
        assert same_bits(a.obs[:, :2 * J], torch.as_tensor(got[:, 13:], device=DEV))
    a.close(); b.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_on_an_rsi_state_the_noise_is_a_perturbation_of_the_clip_s_state(model):
    """a and b both start their episodes at instants of the clip drawn from one seed; a perturbs that state. The state a's launch
    leaves is the reference's perturbation of motion_sample at the drawn instant; and b, given that state, steps the same rows -
    the reward column holds the tracking terms, which read the clip's clock: the launch left it alone."""
    import motion_cases as MC
    from trex_gym import motion as M, start_state as S
    n = 9
    terms = [(JOINT_POSITION, 0, 0, 0, -0.05, 0.05), (JOINT_VELOCITY, SC.bits(3), 0, 0, -1.0, 1.0), (BASE_POSITION, 0, 0, 0, -1.0, 1.0),
             (BASE_ANGULAR_VELOCITY, 0, 1, 0, 0.25, 0.25)]
    a, b = make_vec(n, max_episode_steps=4), make_vec(n, max_episode_steps=4)
    for v in (a, b):
        M.attach(v, M.Clip(MC.clip_frames(model, 33, seed=8), MC.DT), rsi=True, seed=6)
    S.attach(a, S.from_tuples(terms), seed=7)
    ref = SR.StartState(model, n, terms, seed=7, floor_z=float(a.model.get_param("floor_z")), f32=True)
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=a.model.lower, q_upper=a.model.upper), 5, n, 9)
    sample = torch.zeros(n, 13 + 2 * J, device=DEV)
    starts = 0
    for t in range(6):
        if t == 0:
            a.reset_tensor(); b.reset_tensor()
            done = np.ones(n, bool)
        else:
            a.step_tensor(actions[t - 1]); b.step_tensor(actions[t - 1])
            done = a.done.cpu().numpy()
            d = torch.as_tensor(done, device=DEV)
            assert bool(done.all()) == (t == 4) and same_bits(a.done, b.done)
            assert same_bits(a.rows[:, 3 * J:], b.rows[:, 3 * J:]) and same_bits(a.rows[~d], b.rows[~d]), t
        assert same_bits(a._rsi_time, b._rsi_time)
        if not done.any():
            continue
        starts += 1
        a.motion_api.sample(a._rsi_time, state=sample)      # the clip at the instants RSI drew
        own = torch.zeros_like(sample)
        a.motion_api.sample(None, state=own)                  # ... and at each env's own clock: RSI's, as the launch found it
        assert same_bits(own[torch.as_tensor(done, device=DEV)], sample[torch.as_tensor(done, device=DEV)])
        before, sb = sample.cpu().numpy(), state_of(b)
        assert sb[done].tobytes() == before[done].tobytes()   # (b is on the clip's state: what a's launch found)
        want = ref.apply(np.zeros(n) if t == 0 else done.astype(np.float32), before)
        got = state_of(a)
        assert got[done].tobytes() == want.state[done].astype(np.float32).tobytes(), t      # (nothing rotates: all of it bitwise)
        assert not (got[done][:, 13:] == before[done][:, 13:]).all()
        b.batch.set_state(torch.as_tensor(np.where(done[:, None], got, sb), device=DEV))
    assert starts == 2 and bool((a._rsi_time > 0).any())
    a.close(); b.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_keep_the_terms(built):
    from trex_gym import start_state_capi
    n = 3
    v = make_vec(n)
    v.reset_tensor()
    bare = start_state_capi.BatchStartState(v.batch)
    rows = torch.zeros(n, 3 * J + 2, device=DEV)
    refused(INVALID, bare.apply, torch.zeros(n, device=DEV), rows)             # no terms set
    refused(INVALID, bare.reset)
    refused(INVALID, bare.info, torch.zeros(n, 1, 32, device=DEV))
    refused(INVALID, bare.set, TWIN_TERMS, 0, 2 ** 32 - n + 1)                  # env_offset + N beyond 2^32
    api = api_of(v, TWIN_TERMS, 5, 0)
    api.apply(torch.zeros(n, device=DEV), rows)
    values = read(api, n)[0]
    state = v.get_state().clone()
    jp = (JOINT_POSITION, 0, 0, 0, -0.1, 0.1)
    bad = [[(7, 0, 0, 0, 0.0, 1.0)], [(JOINT_POSITION, 0, 0, 0, 2.0, 1.0)], [(JOINT_VELOCITY, 1 << 25, 0, 0, 0.0, 1.0)],
           [(BASE_RPY, 0, 3, 0, 0.0, 1.0)], [(BASE_POSITION, 0, -1, 0, 0.0, 1.0)], [(BASE_RPY, 0, 1, 0, 0.0, 1.0)] * 2,
           [jp, (JOINT_POSITION, 1, 0, 0, 0.0, 0.0)], [(FLOOR_CLEARANCE, 0, 0, 0, 0.0, 0.1)] * 2,
           [(BASE_LINEAR_VELOCITY, 0, 0, 0, float("nan"), 1.0)], [(BASE_ANGULAR_VELOCITY, 0, 0, 0, 0.0, float("inf"))],
           [(JOINT_POSITION, 1 << i, 0, 0, 0.0, 0.1) for i in range(17)]]
    ones = torch.ones(n, device=DEV)
    for terms in bad:
        refused(INVALID, start_state_capi.BatchStartState(v.batch).set, terms, 1, 0)
    refused(INVALID, api.apply, ones.cpu(), rows)                                # host memory
    refused(INVALID, api.apply, torch.ones(n - 1, device=DEV), rows)             # a short buffer
    refused(INVALID, api.apply, ones, torch.zeros(n, 3 * J + 1, device=DEV))     # a row stride below 3J + 2
    refused(INVALID, api.apply, ones, rows.cpu())
    refused(INVALID, api.apply, ones, rows, 1)                                   # (the binding's: a column outside a 1-D done)
    refused(INVALID, api.info, torch.zeros(n, len(TWIN_TERMS), 31, device=DEV))
    torch.cuda.synchronize()
    assert same_bits(v.get_state(), state) and read(api, n)[0].tobytes() == values.tobytes()     # nothing launched, the terms intact
    v.batch.set_penalties_in_rows(True)
    refused(INVALID, api.apply, ones, torch.zeros(n, 3 * J + 4, device=DEV))     # 3J + 5 with penalties in rows
    v.batch.set_penalties_in_rows(False)
    api.apply(ones, None)                                                        # rows are nullable
    torch.cuda.synchronize()
    assert not same_bits(v.get_state(), state)
    api.set(())
    refused(INVALID, api.apply, ones, rows)                                      # cleared: no terms set
    v.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """step + apply, four times eagerly in one batch; in another with the same seed once eagerly (the calls learn the buffers), then
    captured on a side stream and replayed three times: the same rows and states, bit for bit. The counters live on the device,
    so a replay is the NEXT row (the skeleton of tests/test_gpu_randomize.py's capture test)."""
    n = 65
    actions, outs = None, []
    for captured in (False, True):
        v = make_vec(n, max_episode_steps=3)
        v.reset_tensor()
        v.set_episode_steps(torch.arange(n, device=DEV, dtype=torch.int32) % 3)
        api = api_of(v, TWIN_TERMS, seed=9, env_offset=3)
        if actions is None:
            actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=v.model.lower, q_upper=v.model.upper), 4, n, 4)
        rows, act = torch.zeros(n, 3 * J + 2, device=DEV), torch.zeros(n, J, device=DEV)

        def call():
            v.batch.step_rows(act, rows)
            api.apply(rows, rows, 3 * J + 1)

        api.apply(torch.zeros(n, device=DEV), rows)
        seen, graph = [], None
        for t in range(4):
            act.copy_(actions[t])
            if captured and t == 1:
                torch.cuda.synchronize()
                side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(graph, stream=side):
                        call()
            if graph is not None:
                graph.replay()
            else:
                call()
            torch.cuda.synchronize()
            seen.append([rows.cpu().numpy().copy(), state_of(v)] + read(api, n))
        outs.append(seen)
        del graph
        v.close()
    for t, (e, c) in enumerate(zip(*outs)):
        for x, y in zip(e, c):
            assert x.tobytes() == y.tobytes(), t
    assert all((s[0][:, 3 * J + 1] != 0).any() for s in outs[0])      # episodes ended inside the captured launches


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_nothing_attached_is_the_plain_env():
    """the rows of 20 steps of an env whose terms were set and cleared are bitwise those of an env that never had any: cleared is
    not a launch and not a byte; and the launch form is the same"""
    n = 33
    a, b = make_vec(n, max_episode_steps=7), make_vec(n, max_episode_steps=7)
    from trex_gym import start_state as S
    S.attach(a, S.typical(a, clearance=(0.0, 0.02)), seed=1)
    S.attach(a, None)
    a.reset_tensor(); b.reset_tensor()
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=a.model.lower, q_upper=a.model.upper), 20, n, 8)
    for t in range(20):
        a.step_tensor(actions[t]); b.step_tensor(actions[t])
        assert same_bits(a.rows, b.rows), t
    assert a.batch.launch_info() == b.batch.launch_info()
    a.close(); b.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
TRAIN_N, NSTEPS, TRAIN_LIMIT, TRAIN_WINDOW = 64, 8, 6, 100      # (tests/test_gpu_pipeline.py's trainer run)


def test_pipeline_env_with_the_feature_runs_the_trainer_with_every_flag(tmp_path, oracle64, model):
    """tests/pipeline_cases.build_env with start-state terms attached in front of and behind the other features; then the trainer
    with every flag plus --start_noise, with graphs: finite losses, the specification stored and restored, --no_start_noise's path"""
    import pipeline_cases as PC
    from trex_gym import start_state as S, trex_train
    env = PC.build_env(oracle64, model, "full")
    S.attach(env, S.typical(env, scale=0.5, clearance=(0.0, 0.01)), seed=3)
    env.reset_tensor()
    for a in PC.actions(model)[:2 * PC.LIMIT + 1]:
        env.step_tensor(torch.as_tensor(a, device=DEV))
    assert bool(torch.isfinite(env.rows).all()) and bool(torch.isfinite(env.critic_rows).all())
    env.start_api.info(values=env.start_values)
    assert bool((env.start_values[:, 0, :J] != 0).any())
    env.close()
    args = trex_train.parse_args(["--start_noise", "typical", "--start_scale", "0.5", "--start_clearance", "0.0", "0.02", "--graphs"])
    cfg = trex_train.start_state_args(args)
    assert cfg == dict(preset="typical", scale=0.5, clearance=[0.0, 0.02])
    from trex_gym import motion as M, observations as O
    import motion_cases as MC
    clip = str(tmp_path / "clip.npz")
    M.Clip(MC.clip_frames(model, 33, seed=8), MC.DT).save(clip)
    channels = O.as_tuples(O.gravity() + O.base_velocity() + O.base_height())
    env = trex_train.build_environment(
        TRAIN_N, device=DEV, max_episode_steps=TRAIN_LIMIT, observations=channels, rewards="locomotion", motion=dict(clip=clip, rsi=False),
        sensing=dict(preset="typical", obs_delay=(0, 2), action_delay=(1, 2)), randomize=dict(preset="typical", push=100.0, command_interval=3),
        monitor=dict(window=TRAIN_WINDOW, terms=True), critic="privileged", terminate=dict(max_tilt=1.0), start_state=cfg)
    assert [t[0] for t in env.start_state_config["terms"]] == [0, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 6]
    path = str(tmp_path / "agent.pt")
    agent, hist = trex_train.train(env, 2 * TRAIN_N * NSTEPS, 0, nsteps=NSTEPS, noptepochs=1, save_path=path, log=lambda *_: None,
                                   use_graphs=args.graphs)
    assert len(hist) == 2
    for h in hist:
        assert all(np.isfinite(h[k]) for k in ("policy_loss", "value_loss", "entropy", "mean_step_reward")), h
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    assert again.env.start_state_config == env.start_state_config is not None
    bare = trex_train.load_agent(path, num_envs=4, device=DEV, start_state=False)
    assert bare.env.start_api is None
    for bad in (["--start_scale", "2"], ["--start_clearance", "0", "0.1"], ["--start_noise", "typical", "--start_scale", "-1"],
                ["--start_noise", "typical", "--start_clearance", "0.2", "0.1"]):
        with pytest.raises(SystemExit):
            trex_train.parse_args(bad)
    env.close(); again.env.close(); bare.env.close()
