"""CPU checks that keep tests/test_gpu_pipeline.py from being vacuous. The scenario of tests/pipeline_cases.py, run on the f64
oracle, meets the conditions without which the chain of references could not tell a right launch order from a wrong one - each
with a margin, because the device's f32 physics of a randomised robot may flip a borderline event - and the chain TELLS: with each
of six single mistakes planted in its order (pipeline_cases.MISTAKES), the affected output moves by at least 100 x the bound that
output is compared with on the GPU (the factor of tests/test_dynamics_model_cases_host.py); outputs that are compared bitwise
differ outright in at least 3 env-steps."""
import numpy as np
import pytest

import pipeline_cases as PC
import reward_ref as RR
import sensing_cases as SC
import sensing_ref as SR

SEPARATION = 100.0
N, J = PC.N, PC.J
# the chains run the first CHAIN_N envs over the first CHAIN_STEPS steps - env e of a batch draws what env e of any batch at the same
# offset draws -: every env ends two episodes, and the masked reset lies inside
CHAIN_N, CHAIN_STEPS = 12, 19


@pytest.fixture(scope="module")
def sc(oracle64, model):
    return PC.scenario(oracle64, model)


@pytest.fixture(scope="module")
def run(oracle64, model, sc):
    return PC.host_run(oracle64, model)


def ends(run):
    """(env-steps that end an episode at the limit, by a fall, launches that have both)"""
    limit = sum(int(((r["done"] != 0) & (r["reason"] == 0)).sum()) for r in run[1:])
    fall = sum(int((r["reason"] != 0).sum()) for r in run[1:])
    both = sum(1 for r in run[1:] if ((r["done"] != 0) & (r["reason"] == 0)).any() and (r["reason"] != 0).any())
    return limit, fall, both


def test_the_specifications_are_the_presets_for_the_oracles_feet(sc, model):
    from trex_gym import sensing_capi
    assert len(sc.feet) == 2 and len(sc.limbs) == 14
    assert len(sc.chans) == 10 and sum(c[0] == 9 for c in sc.chans) == 1 and sc.chans[-1][0] == 8        # external(3), prev_action last
    assert any(t[0] == RR.ACTION_RATE for t in sc.reward_terms) and any(t[0] == RR.TRACK_LIN for t in sc.reward_terms)
    D = 3 * J + 18 + 3 + J
    cmd0 = 3 * J + 18
    late = [g for g in sc.groups if g[7] > 0]
    assert any(g[0] >= 3 * J and g[0] + g[1] <= cmd0 for g in late)                  # a late group on channel columns beyond 3J
    assert any(g[0] == cmd0 and g[1] == 3 for g in late)                             # ... and one on the command columns
    assert all(g[0] + g[1] <= D - J for g in sc.groups)                              # the prev_action columns stay clean
    assert [g[:2] for g in sc.groups_3j] == [(0, J), (J, J)] and len(sc.groups) <= sensing_capi.MAX_GROUPS
    assert sum(t[0] == 5 for t in sc.random_terms) == 2 and sum(t[0] == 6 for t in sc.random_terms) == 3
    assert all(t[6] == PC.COMMAND_INTERVAL < PC.LIMIT for t in sc.random_terms if t[0] == 6)


def test_conditions_of_the_run(run, sc):
    steps = run[1:]
    assert len(steps) == PC.STEPS
    drawn = np.concatenate([r["action_delay"] for r in steps])
    assert set(drawn.tolist()) == {1, 2}
    late = sum(int((r["applied"] != r["action"]).any(axis=1).sum()) for r in steps)
    print("delayed action rows that differ from the policy's: %d of %d" % (late, N * PC.STEPS))
    assert late >= N * PC.STEPS // 4
    limit, fall, both = ends(run)
    print("episode ends: %d at the limit, %d by a fall, %d launches with both" % (limit, fall, both))
    assert limit >= 3 and fall >= 3 and both >= 1
    per_env = sum((r["done"] != 0).astype(int) for r in steps)
    assert per_env.min() >= 4 and per_env.sum() + N <= PC.WINDOW                     # every env ends four episodes; the window holds all


@pytest.mark.parametrize("factor", [0.8, 1.25])
def test_the_fall_threshold_has_a_margin(factor, oracle64, model):
    """a fifth off the threshold either way - more than the randomised masses and gains move a tilt of a few hundredths of a
    radian - both end reasons still occur, three times each, and some launch has both"""
    limit, fall, both = ends(PC.host_run(oracle64, model, max_tilt=factor * PC.MAX_TILT))
    print("max_tilt x %.2f: %d at the limit, %d by a fall, %d launches with both" % (factor, limit, fall, both))
    assert limit >= 3 and fall >= 3 and both >= 1


def chain_run(model, sc, run, mistake=None):
    """the chain fed the oracle-stepped rows -> per row what it left"""
    ch = PC.Chain(model, sc, n=CHAIN_N, mistake=mistake)
    out = []
    run = [{k: (v[:CHAIN_N] if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in run[:CHAIN_STEPS + 1]]

    def keep(step):
        out.append(dict(step=step, clean=ch.clean.copy(), rows=ch.rows, critic=ch.critic.copy(), commands=ch.commands.copy(),
                        monitor=ch.monitor.state(), reward_terms=None if not step else ch.reward_terms.copy(),
                        bounds=None if not step else ch.reward_bounds.copy(), reward=None if not step else ch.reward.copy()))
    ch.reset(run[0]["row"], run[0]["state"])
    keep(False)
    for r in run[1:]:
        if r["masked"] is not None:
            # the envs that are reset: the reset state and its row (no reward, no done); the others keep row and state of the step before
            m = r["masked"][:, None] != 0
            ch.reset(np.where(m, run[0]["row"], r["prev_row"]), np.where(m, run[0]["state"], r["prev_state"]), r["masked"])
            keep(False)
        ch.step(r["row"], r["state"], r["action"], r["applied"], r["force"])
        keep(True)
    return out


@pytest.fixture(scope="module")
def right(model, sc, run):
    prev = run[0]
    for r in run[1:]:
        r["prev_state"], r["prev_row"] = prev["state"], prev["row"]
        prev = r
    return chain_run(model, sc, run)


def test_the_right_chain_changes_commands_at_episode_ends(right, run):
    """at least 10 env-steps end an episode in which some command component changes by more than 0.1"""
    stepped = [x for x in right if x["step"]]
    before = [x for x, nxt in zip(right, right[1:]) if nxt["step"]]
    moved = 0
    for r, b, a in zip([{k: (v[:CHAIN_N] if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in run[1:]], before, stepped):
        moved += int(((r["done"] != 0) & (np.abs(a["commands"] - b["commands"]).max(axis=1) > 0.1)).sum())
    print("episode ends with a command moved by more than 0.1: %d" % moved)
    assert moved >= 10


def term_column(sc, kind):
    return [t for t, s in enumerate(sc.reward_terms) if s[0] == kind]


def separation(right, wrong, columns):
    """the largest |wrong - right| / bound over the stepped rows and these reward-term columns, bounds of the right chain"""
    worst = 0.0
    for a, b in zip(right, wrong):
        if a["step"]:
            d = np.abs(a["reward_terms"][:, columns].astype(np.float64) - b["reward_terms"][:, columns])
            live = a["bounds"][:, columns] > 0
            if live.any():
                worst = max(worst, float((d[live] / a["bounds"][:, columns][live]).max()))
    return worst


def records(x):
    s = x["monitor"]
    return [(s["ring_return"][j].tobytes(), int(s["ring_length"][j]), int(s["ring_env"][j])) for j in range(s["total"])]


@pytest.mark.parametrize("mistake", PC.MISTAKES)
def test_each_single_mistake_is_told_apart(mistake, model, sc, run, right):
    wrong = chain_run(model, sc, run, mistake)
    D = right[0]["clean"].shape[1] - 2
    if mistake == "reward_gets_delayed_action":
        s = separation(right, wrong, term_column(sc, RR.ACTION_RATE))
        print("action_rate moves by %.3g x its bound" % s)
        assert s >= SEPARATION
    elif mistake == "command_before_reward":
        s = separation(right, wrong, term_column(sc, RR.TRACK_LIN) + term_column(sc, RR.TRACK_ANG))
        print("the tracking terms move by %.3g x their bound" % s)
        assert s >= SEPARATION
    elif mistake == "monitor_before_motion":
        a, b = records(right[-1]), records(wrong[-1])
        assert len(a) == len(b) and sum(x[0] != y[0] for x, y in zip(a, b)) >= 3 and [x[1:] for x in a] == [y[1:] for y in b]
    elif mistake == "sensing_before_compose":
        # the channel columns of the policy's rows stay clean: they lie further from the sensed values than 100 x what
        # sensing_cases.compare allows a Gaussian column (4 x the reference's own f32 deviation) or any other (2 ulp)
        groups = [g for g in sc.groups if g[0] >= 3 * J]
        cols = np.concatenate([np.arange(g[0], g[0] + g[1]) for g in groups])
        case = SC.Case("pipeline", "locomotion", CHAIN_N, D, 2, sc.groups, PC.SENSE_SEED, 0, True, 0, 0.0)
        inputs = [x["clean"] for x in right]
        bound = 4.0 * SC.gaussian_bound(case, inputs)
        worst = max(float(np.abs(b["rows"].out[:, cols] - a["rows"].y[:, cols]).max()) for a, b in zip(right, wrong))
        print("sensed channel columns move by %.3g, the Gaussian bound is %.3g" % (worst, bound))
        assert bound > 0 and worst >= SEPARATION * bound
        assert all(np.array_equal(b["rows"].out[:, cols].astype(np.float32), b["clean"][:, cols]) for b in wrong)
    elif mistake == "prev_action_gets_delayed_action":
        differ = sum(int((a["clean"][:, D - J:D] != b["clean"][:, D - J:D]).any(axis=1).sum()) for a, b in zip(right, wrong))
        assert differ >= 3
    else:
        differ = sum(int((a["critic"][:, :D] != b["critic"][:, :D]).any(axis=1).sum()) for a, b in zip(right, wrong))
        assert differ >= 3
