"""Episode randomisation on the device (include/trex_randomize.h; csrc/randomize.hip) against tests/randomize_ref.py:
 1 through the C-ABI alone, the cases of tests/randomize_cases.py row by row: values, push_left and commands bitwise, push forces
   within the case's own bound (the share used is printed);
 2 the effect: a twin batch that is given, before every step, what _info reports through set_domain, set_motor_gains and
   set_external_wrench steps bitwise the same rows, episode ends inside the step launch included, in the pair and the single-env form;
 3 a caller's wrench on the push body and on another body: base + push, base, and base again after the push - the same twin;
 4 two shards draw what the whole batch draws;  5 step + apply captured and replayed equal the eager run;
 6 guard-padded outputs;  7 refusals launch nothing and keep the terms;  8 clearing restores buffers and launch form;
 9 - 11 through TrexVecEnv and the trainer."""
import numpy as np
import pytest
import torch

import randomize_cases as RC
import randomize_ref as RR
from gpu_support import DEV, guarded, guards_intact, make_vec, random_action_steps, refused, same_bits

pytestmark = pytest.mark.gpu
J, NB = 25, 26
INVALID = -1
MASS, FRICTION, KP, KD, MAX_FORCE, PUSH, COMMAND = range(7)


def env_of(model, n, tmp_path, **kw):
    if model == "trex":
        return make_vec(n, **kw)
    import synthetic_models as sm
    path, props = sm.MODELS[model](tmp_path / model)
    return make_vec(n, urdf=path, params=props["params"], **kw)


def api_of(v, terms, seed=0, env_offset=0):
    from trex_gym import randomize_capi
    api = randomize_capi.BatchRandomization(v.batch)
    api.set(terms, seed, env_offset)
    return api


def read(api, n):
    """-> (values, push_force, push_left) as numpy, through guard-padded buffers"""
    T, P = max(api.num_terms, 1), max(api.num_pushes, 1)
    bufs = [guarded((n, T, 32)), guarded((n, P, 3)), guarded((n, P), fill=7, dtype=torch.int32)]
    assert api.info(*(b[1] for b in bufs)) == api.num_terms
    torch.cuda.synchronize()
    assert guards_intact(bufs[0][0], (n, T, 32)) and guards_intact(bufs[1][0], (n, P, 3)) and guards_intact(bufs[2][0], (n, P), fill=7)
    return [b[1].cpu().numpy() for b in bufs]


def run_case(api, case, n=None, first_env=0):
    n = case.n if n is None else n
    done = RC.done_flags(case)[:, first_env:first_env + n]
    whole, command = guarded((n, 3))
    command.zero_()
    got = []
    for t in range(case.rows):
        if t == RC.RESET_ROW:
            api.reset(torch.as_tensor(RC.reset_mask(case)[first_env:first_env + n], device=DEV))
        api.apply(torch.as_tensor(done[t], device=DEV), command)
        values, force, left = read(api, n)
        got.append((values, force, left, command.cpu().numpy().copy()))
    assert guards_intact(whole, (n, 3))
    return got


# 1, 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_draws_against_the_reference(case, tmp_path):
    v = env_of(case.model, case.n, tmp_path)
    assert (v.model.num_bodies, v.J) == (case.nb, case.nj)
    res = RC.compare(case, run_case(api_of(v, case.terms, case.seed, case.env_offset), case))
    print("%s: push forces use %.3f of the bound %.3g" % (case.name, res["share"], RC.force_bound(case)))
    assert not res["failures"], res["failures"][:5]


def test_done_is_read_from_a_column_of_a_row_block_and_nothing_else_is_written():
    """the done flags as column 3J + 1 of a padded row block, as step_tensor passes them: the block itself stays as it was"""
    case = RC.CASES[3]
    v = make_vec(case.n)
    api = api_of(v, case.terms, case.seed, case.env_offset)
    done = RC.done_flags(case)
    rows = torch.full((case.n, 3 * J + 7), 3.0, device=DEV)
    command, got = torch.zeros(case.n, 3, device=DEV), []
    for t in range(case.rows):
        rows[:, 3 * J + 1] = torch.as_tensor(done[t], device=DEV)
        before = rows.clone()
        if t == RC.RESET_ROW:
            api.reset(torch.as_tensor(RC.reset_mask(case), device=DEV))
        api.apply(rows, command, 3 * J + 1)
        assert same_bits(rows, before)
        got.append((*read(api, case.n), command.cpu().numpy().copy()))
    assert not RC.compare(case, got)["failures"]


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_two_shards_draw_what_the_whole_batch_draws():
    case = RC.CASES[4]
    half = case.n // 2
    whole = run_case(api_of(make_vec(case.n), case.terms, case.seed, case.env_offset), case)
    for first in (0, half):
        part = run_case(api_of(make_vec(half), case.terms, case.seed, case.env_offset + first), case, n=half, first_env=first)
        for w, p in zip(whole, part):
            for a, b in zip(w, p):
                assert a[first:first + half].tobytes() == b.tobytes()


# 2, 3 ---------------------------------------------------------------------------------------------------------------------
TWIN_TERMS = [(MASS, 0, 0, 0, 0.8, 1.25, 0, 0, 0.0), (FRICTION, 0, 0, 0, 0.5, 1.25, 0, 0, 0.0),
              (KP, RC.bits(*range(0, 25, 2)), 0, 0, 0.7, 1.3, 0, 0, 0.0), (KD, 0, 0, 1, 0.8, 1.2, 0, 0, 0.0),
              (MAX_FORCE, RC.bits(3, 4, 24), 0, 0, 0.5, 1.0, 0, 0, 0.0),
              (PUSH, 0, 0, 0, 100.0, 400.0, 3, 2, 1.0), (PUSH, 0, 9, 0, 5.0, 20.0, 1, 1, 0.5)]


def twin_inputs(v, api, base):
    """what the twin is given before a step: mass scale, friction, the three gains and the wrench, from _info and the nominal"""
    n = v.num_envs
    values, force, left = (torch.as_tensor(x, device=DEV) for x in read(api, n))
    nominal = [torch.full((n, J), v.model.get_param(k), dtype=torch.float32, device=DEV) for k in ("motor_kp", "motor_kd", "motor_max_force")]
    gains = []
    for t, nom in zip((2, 3, 4), nominal):
        mask = TWIN_TERMS[t][1] or (1 << J) - 1
        covered = torch.tensor([(mask >> j) & 1 for j in range(J)], dtype=torch.bool, device=DEV)
        gains.append(torch.where(covered[None, :], nom * values[:, t, :J], nom).contiguous())
    wrench = base.clone()
    for p, body in enumerate((0, 9)):
        on = (left[:, p] > 0)[:, None]
        wrench[:, body, :3] = torch.where(on, base[:, body, :3] + force[:, p], base[:, body, :3])
    return values[:, 0, :NB].contiguous(), values[:, 1, 0].contiguous(), gains, wrench


@pytest.mark.parametrize("n, with_base", [(130, False), (65, False), (65, True)], ids=["pair_n130", "single_n65", "caller_wrench_n65"])
def test_a_twin_given_the_reported_values_steps_the_same_rows(n, with_base):
    """20 steps with an episode limit of 6, staggered, so that episodes end inside the step launch at different steps per env. With
    a caller's wrench: on the push body 0 and on body 5, replaced in the middle of the run while pushes act, cleared later."""
    a, b = make_vec(n, max_episode_steps=6), make_vec(n, max_episode_steps=6)
    for v in (a, b):
        v.reset_tensor()
        v.set_episode_steps(torch.arange(n, device=DEV, dtype=torch.int32) % 6)
    api = api_of(a, TWIN_TERMS, seed=31, env_offset=7)
    base = torch.zeros(n, NB, 6, device=DEV)
    if with_base:
        g = torch.Generator(device=DEV).manual_seed(5)
        base[:, 0] = 30.0 * torch.randn(n, 6, device=DEV, generator=g)
        base[:, 5] = 10.0 * torch.randn(n, 6, device=DEV, generator=g)
        a.batch.set_external_wrench(base)
    from trex_gym import _capi
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=a.model.lower, q_upper=a.model.upper), 20, n, 3)
    rows_a, rows_b = torch.zeros(n, 3 * J + 2, device=DEV), torch.zeros(n, 3 * J + 2, device=DEV)
    api.apply(torch.zeros(n, device=DEV))
    ends = pushing = 0
    for t in range(20):
        if with_base and t == 9:      # a new base while pushes act: the push stays on top of it
            base = -0.5 * base
            a.batch.set_external_wrench(base)
        if with_base and t == 15:     # the caller clears its wrench: the base is zeros, the pushes go on
            base = torch.zeros_like(base)
            a.batch.set_external_wrench(None)
        mass, friction, gains, wrench = twin_inputs(a, api, base)
        b.batch.set_domain(mass, friction)
        b.batch.set_motor_gains(*gains)
        b.batch.set_external_wrench(wrench)
        pushing += int((wrench != base).flatten(1).any(1).sum())
        a.batch.step_rows(actions[t], rows_a)
        b.batch.step_rows(actions[t], rows_b)
        assert same_bits(rows_a, rows_b), t
        assert bool(torch.isfinite(rows_a).all())
        ends += int((rows_a[:, 3 * J + 1] != 0).sum())
        api.apply(rows_a, None, 3 * J + 1)
    assert ends >= 3 * n and pushing > n        # episodes ended in the launch, pushes acted
    assert a.batch.launch_info() == b.batch.launch_info()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """step + apply, four times eagerly in one batch; in another with the same seed once eagerly (the calls learn the buffers), then
    captured on a side stream and replayed three times: the same rows, values, push state and commands, bit for bit. The counters
    live on the device, so a replay is the NEXT row (gpu_support.replay_equals_eager expects the same result from a replay: not
    what a launch that advances does - the capture skeleton is the same)."""
    n, terms = 65, RC.CASES[4].terms
    actions = None
    outs = []
    for captured in (False, True):
        v = make_vec(n, max_episode_steps=3)
        v.reset_tensor()
        v.set_episode_steps(torch.arange(n, device=DEV, dtype=torch.int32) % 3)
        api = api_of(v, terms, seed=9, env_offset=3)
        if actions is None:
            actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=v.model.lower, q_upper=v.model.upper), 4, n, 4)
        rows, command, act = torch.zeros(n, 3 * J + 2, device=DEV), torch.zeros(n, 3, device=DEV), torch.zeros(n, J, device=DEV)

        def call():
            v.batch.step_rows(act, rows)
            api.apply(rows, command, 3 * J + 1)

        api.apply(torch.zeros(n, device=DEV), command)
        seen = []
        graph = None
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
            seen.append([rows.cpu().numpy().copy(), command.cpu().numpy().copy()] + read(api, n))
        outs.append(seen)
        del graph
    for t, (e, c) in enumerate(zip(*outs)):
        for x, y in zip(e, c):
            assert x.tobytes() == y.tobytes(), t
    assert any((s[0][:, 3 * J + 1] != 0).any() for s in outs[0])      # episodes ended inside the captured launches


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_keep_the_terms():
    case = RC.CASES[3]
    v = make_vec(case.n)
    from trex_gym import randomize_capi
    bare = randomize_capi.BatchRandomization(v.batch)
    command = torch.zeros(case.n, 3, device=DEV)
    refused(INVALID, bare.apply, torch.zeros(case.n, device=DEV), command)             # no terms set
    refused(INVALID, bare.reset)
    refused(INVALID, bare.info, torch.zeros(case.n, 1, 32, device=DEV))
    refused(INVALID, bare.set, case.terms, 0, 2 ** 32 - case.n + 1)                     # env_offset + N beyond 2^32
    api = api_of(v, case.terms, case.seed, case.env_offset)
    done = RC.done_flags(case)
    bad = [[(7, 0, 0, 0, 0.0, 1.0, 0, 0, 0.0)], [(MASS, 0, 0, 0, 2.0, 1.0, 0, 0, 0.0)], [(MASS, 1 << 26, 0, 0, 1.0, 1.0, 0, 0, 0.0)],
           [(PUSH, 0, 26, 0, 0.0, 1.0, 1, 1, 1.0)], [(PUSH, 0, 0, 0, 0.0, 1.0, 0, 1, 1.0)], [(COMMAND, 0, 3, 0, 0.0, 1.0, 0, 0, 0.0)],
           [(COMMAND, 0, 0, 0, 0.0, 1.0, -1, 0, 0.0)], [(FRICTION, 0, 0, 0, 0.5, 1.0, 0, 0, 1.5)],
           [(KP, 1, 0, 0, 1.0, 1.0, 0, 0, 0.0), (KP, 0, 0, 0, 1.0, 1.0, 0, 0, 0.0)], [(FRICTION, 0, 0, 0, 0.5, 1.0, 0, 0, 0.0)] * 17,
           [(PUSH, 0, b, 0, 0.0, 1.0, 1, 1, 1.0) for b in range(5)], [(MASS, 0, 0, 0, float("nan"), 1.0, 0, 0, 0.0)]]
    got = []
    for t in range(case.rows):
        if t == RC.RESET_ROW:
            api.reset(torch.as_tensor(RC.reset_mask(case), device=DEV))
        if t < len(bad):          # a refused set between two rows: the terms, the counters and the draws go on as if it had not been
            refused(INVALID, randomize_capi.BatchRandomization(v.batch).set, bad[t], 1, 0)
            refused(INVALID, api.apply, torch.as_tensor(done[t], device=DEV), None)     # a COMMAND term and no command buffer
            refused(INVALID, api.apply, torch.as_tensor(done[t]), command)              # host memory
            refused(INVALID, api.apply, torch.zeros(case.n - 1, device=DEV), command)   # a short buffer
        api.apply(torch.as_tensor(done[t], device=DEV), command)
        got.append((*read(api, case.n), command.cpu().numpy().copy()))
    assert not RC.compare(case, got)["failures"]
    v.batch.set_stiffness_actions(True, 1.0)
    refused(INVALID, randomize_capi.BatchRandomization(v.batch).set, [(KD, 0, 0, 0, 1.0, 1.0, 0, 0, 0.0)], 0, 0)     # KD with stiffness actions


# 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", [False, True], ids=["defaults", "caller_values"])
def test_clearing_restores_buffers_and_launch_form(preset):
    """x is never randomised, y is randomised for some steps and cleared; both then continue from one state under the same actions:
    the same rows bit for bit, and y reports the launch form it had before. With caller_values both had their own gains, domain
    and wrench set before."""
    n = 66
    x, y = make_vec(n), make_vec(n)
    g = torch.Generator(device=DEV).manual_seed(8)
    rnd = lambda *shape: torch.rand(*shape, device=DEV, generator=g)
    for v in (x, y):
        v.reset_tensor()
    if preset:
        kp, mass, fr = 0.004 + 0.002 * rnd(n, J), 0.9 + 0.2 * rnd(n, NB), 0.5 + 0.5 * rnd(n)
        w = torch.zeros(n, NB, 6, device=DEV)
        w[:, 0, :3] = 20.0 * (rnd(n, 3) - 0.5)
        for v in (x, y):
            v.batch.set_motor_gains(kp, None, None)
            v.batch.set_domain(mass, fr)
            v.batch.set_external_wrench(w)
    before = y.batch.launch_info()
    assert before == x.batch.launch_info()
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=x.model.lower, q_upper=x.model.upper), 8, n, 6)
    api = api_of(y, TWIN_TERMS, seed=4)
    rows_x, rows_y = torch.zeros(n, 3 * J + 2, device=DEV), torch.zeros(n, 3 * J + 2, device=DEV)
    done = torch.zeros(n, device=DEV)
    for t in range(4):
        done[:] = (torch.arange(n, device=DEV) % 4 == t).float()
        api.apply(done)
        y.batch.step_rows(actions[t], rows_y)
        x.batch.step_rows(actions[t], rows_x)
    assert not same_bits(rows_x, rows_y)            # the randomisation did something
    api.set(())
    assert y.batch.launch_info() == before
    y.set_state(x.get_state())
    for t in range(4, 8):
        y.batch.step_rows(actions[t], rows_y)
        x.batch.step_rows(actions[t], rows_x)
        assert same_bits(rows_x, rows_y), t
    refused(INVALID, api.apply, done)               # cleared: no terms set


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_env_redraws_gains_at_every_episode_end():
    """max_episode_steps = 6 and no termination: the episodes end inside the step launch - the case in which gains drawn on the host
    (perturb.RandomGains) stay what they were. Here the kp factors change at every episode end, and only there."""
    from trex_gym import perturb, randomize as Z
    n = 33
    v = make_vec(n, max_episode_steps=6)
    link = v.model.links()[3][0]             # a push term names a URDF link: attach resolves it to the link's body
    Z.attach(v, [Z.kp(0.8, 1.2), Z.friction(0.5, 1.0), Z.push(link, 10.0, 20.0, 3, 2, 1.0)], seed=2)
    assert v.randomization["terms"][2][2] == int(v.model.array("link_body")[3]) and v.random_values.shape == (n, 3, 32)
    v.reset_tensor()
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=v.model.lower, q_upper=v.model.upper), 13, n, 1)
    seen = []
    for t in range(13):
        v.random_api.info(values=v.random_values)
        seen.append(v.random_values[:, 0, :J].clone())
        _, _, done = v.step_tensor(actions[t])
        assert bool(done.all()) == (t % 6 == 5)
    for t in range(1, 13):
        changed = ~(seen[t] == seen[t - 1]).all(dim=1)
        assert bool(changed.all()) if t % 6 == 0 else not bool(changed.any()), t
    assert bool(((seen[0] >= 0.8) & (seen[0] <= 1.2)).all()) and len(torch.unique(seen[0])) > n * J // 2
    with pytest.raises(ValueError):
        v.step_many_tensor(actions[:2])
    v.gains = perturb.RandomGains(n, J, device=torch.device(DEV))
    with pytest.raises(ValueError):
        v.step_tensor(actions[0])
    v.gains = None
    Z.attach(v, None)
    assert v.random_api is None and v.randomization is None and v.random_values is None
    v.step_many_tensor(actions[:2])
    with pytest.raises(ValueError):
        Z.attach(make_vec(2, pushes=perturb.RandomPushes(2, device=torch.device(DEV))), [Z.friction(0.5, 1.0)])


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_the_new_command_shows_in_the_first_row_and_the_done_row_is_rewarded_against_the_old_one():
    from trex_gym import randomize as Z, trex_train
    n = 16
    a, b = (trex_train.build_environment(n, device=DEV, max_episode_steps=5, observations="locomotion", rewards="locomotion") for _ in range(2))
    Z.attach(a, [Z.command(0, 0.5, 2.0), Z.command(1, -0.3, 0.3, interval=2), Z.command(2, -1.0, 1.0, zero_probability=0.5)], seed=6)
    a.reset_tensor()
    b.commands.copy_(a.commands)
    b.reset_tensor()
    assert same_bits(a.obs, b.obs) and bool((a.commands[:, 0] >= 0.5).all()) and same_bits(a.obs[:, -3:], a.commands)
    actions = random_action_steps(dict(obs_order=np.arange(J), q_lower=a.model.lower, q_upper=a.model.upper), 11, n, 2)
    ends = 0
    for t in range(11):
        old = a.commands.clone()
        b.commands.copy_(old)                       # the twin tracks, for this step, the command the step started with
        _, rew_a, done = a.step_tensor(actions[t])
        _, rew_b, _ = b.step_tensor(actions[t])
        assert same_bits(rew_a, rew_b), t            # ... and that is the command the finished step was rewarded against
        assert same_bits(a.obs[:, -3:], a.commands)  # the row shows the command in force from now on
        assert same_bits(a.obs[:, :-3], b.obs[:, :-3])
        moved = (a.commands != old)
        if bool(done.all()):
            ends += 1
            assert bool(moved[:, 0].all())           # a new episode: a new vx, in the first row already
        else:
            assert not bool(moved[:, 0].any()) and not bool(moved[:, 2].any())
    assert ends == 2
    assert bool((a.commands[:, 2] == 0).any()) and bool((a.commands[:, 2] != 0).any())


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_trainer_with_graphs(tmp_path):
    """two updates at 64 envs with --randomize typical --graphs: finite losses; save, load: the specification comes back, and
    randomize=False leaves it off"""
    from trex_gym import trex_train
    args = trex_train.parse_args(["--randomize", "typical", "--graphs", "--rand_scale", "0.5", "--rand_push", "100", "--rewards", "locomotion",
                                  "--command_range", "1", "0.2", "0.5", "--command_interval", "10"])
    env = trex_train.build_environment(64, device=DEV, max_episode_steps=20, rewards=args.rewards, randomize=trex_train.randomize_args(args))
    kinds = [t[0] for t in env.randomization["terms"]]
    assert kinds == [MASS, FRICTION, KP, KD, MAX_FORCE, PUSH, COMMAND, COMMAND, COMMAND] and env.randomization["terms"][5][5] == 50.0
    path = str(tmp_path / "agent.pt")
    agent, hist = trex_train.train(env, 2 * 64 * 32, 0, nsteps=32, noptepochs=1, save_path=path, log=lambda *_: None, use_graphs=args.graphs)
    assert len(hist) == 2
    for h in hist:
        assert all(np.isfinite(h[k]) for k in ("policy_loss", "value_loss", "entropy", "mean_step_reward")), h
    env.random_api.info(values=env.random_values)
    assert bool((env.random_values[:, 1, 0] >= 0.5).all()) and bool((env.commands != 0).any())
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    assert again.env.randomization == env.randomization
    bare = trex_train.load_agent(path, num_envs=4, device=DEV, randomize=False)
    assert bare.env.random_api is None
    for bad in (["--rand_scale", "2"], ["--randomize", "typical", "--push_force", "10"], ["--randomize", "typical", "--gain_scale", "0.2"],
                ["--randomize", "typical", "--command_interval", "-1"]):
        with pytest.raises(SystemExit):
            trex_train.parse_args(bad)
