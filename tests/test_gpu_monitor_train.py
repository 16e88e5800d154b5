"""The episode monitor under the trainer (trex_gym.ppo, trex_train.py --monitor): PPO on 64 envs, nsteps 8, an episode limit of 6,
two iterations, eager and with the rollout replayed as a HIP graph - the applies inside the captured rollout, the summary outside.
info["eprewmean"] and info["eplenmean"] are those recomputed on the host from the b_rew and b_done of the rollouts, within the
bound of the summary's means (an n-term f64 sum in any order: 2^-53 * sum|x|), and the two modes agree."""
import numpy as np
import pytest
import torch

from gpu_support import DEV

pytestmark = pytest.mark.gpu
N, NSTEPS, LIMIT, WINDOW = 64, 8, 6, 100


def run(graphs):
    from trex_gym import trex_train
    from trex_gym.ppo import PPO
    env = trex_train.build_environment(N, device=DEV, max_episode_steps=LIMIT, monitor=dict(window=WINDOW))
    assert env.monitor == dict(window=WINDOW, terms=True) and env.monitor_config == env.monitor
    agent = PPO(env, nsteps=NSTEPS, nminibatches=8, noptepochs=1, seed=3, use_graphs=graphs)
    rollouts, lines = [], []

    def log(line):
        lines.append(line)
        if line.startswith("it "):
            rollouts.append((agent.b_rew.cpu().numpy().copy(), agent.b_done.cpu().numpy().copy()))
    hist = agent.learn(2 * N * NSTEPS, log=log)
    assert len(hist) == 2 and len(rollouts) == 2
    assert sum(1 for l in lines if "eprewmean" in l and "eplenmean" in l and "ended by" in l) == 2
    env.close()
    return hist, rollouts


def host_windows(rollouts):
    """per iteration: (mean return, mean length, episodes, the bound of the return mean) over the last WINDOW episodes, from the
    rollouts' rewards and done flags alone, in f64"""
    ret, length, records, out = np.zeros(N), np.zeros(N, np.int64), [], []
    for rew, done in rollouts:
        for t in range(NSTEPS):
            ret += rew[t].astype(np.float64)
            length += 1
            for e in np.flatnonzero(done[t]):
                records.append((np.float64(np.float32(ret[e])), int(length[e])))
                ret[e], length[e] = 0.0, 0
        last = records[-WINDOW:]
        r = np.array([x[0] for x in last])
        out.append((r.sum() / len(last), np.mean([x[1] for x in last]), len(records), 2.0 ** -53 * np.abs(r).sum()))
    return out


def test_eprewmean_and_eplenmean_are_the_host_s_eager_and_with_graphs():
    got = {}
    for graphs in (False, True):
        hist, rollouts = run(graphs)
        want = host_windows(rollouts)
        assert [w[2] for w in want] == [N, 2 * N]            # every env finishes one episode per rollout: the window wraps in the second
        for h, (ret, length, episodes, bound) in zip(hist, want):
            print("graphs %s: eprewmean %.17g, host %.17g, bound %.3g; eplenmean %.17g" % (graphs, h["eprewmean"], ret, bound, h["eplenmean"]))
            assert abs(h["eprewmean"] - ret) <= bound
            assert h["eplenmean"] == length == LIMIT and h["episodes"] == episodes
            assert h["end_reasons"] == dict(limit=1.0, head=0.0, tilt=0.0, clearance=0.0)
        got[graphs] = hist
    # the two modes agree: the counts exactly; the returns as closely as this project holds an eager and a replayed first
    # rollout to each other (tests/test_gpu_termination.py test_trainer_flags_with_graphs: 2e-3 of the value)
    a, b = got[True][0], got[False][0]
    print("first iteration: eprewmean with graphs %.9g, eager %.9g" % (a["eprewmean"], b["eprewmean"]))
    assert (a["episodes"], a["eplenmean"]) == (b["episodes"], b["eplenmean"])
    assert abs(a["eprewmean"] - b["eprewmean"]) <= 2e-3 * abs(b["eprewmean"])


def test_the_flag_the_checkpoint_and_play(tmp_path):
    from trex_gym import trex_train
    args = trex_train.parse_args(["--monitor", "50", "--graphs", "--terminate_tilt", "1.0", "--num_envs", "64", "--max_episode_steps", "6"])
    assert trex_train.monitor_args(args) == dict(window=50, terms=True) and trex_train.monitor_args(trex_train.parse_args([])) is None
    for bad in (["--monitor", "0"], ["--monitor", "65537"]):
        with pytest.raises(SystemExit):
            trex_train.parse_args(bad)
    env = trex_train.environment_from_args(args)
    assert env.monitor == dict(window=50, terms=True) and env._term_on
    path, lines = str(tmp_path / "agent.pt"), []
    agent, hist = trex_train.train(env, 2 * 64 * 8, 0, nsteps=8, noptepochs=1, save_path=path, log=lines.append, use_graphs=args.graphs)
    assert len(hist) == 2 and all(k in hist[-1] for k in ("eprewmean", "eplenmean", "episodes", "end_reasons"))
    assert hist[-1]["episodes"] >= 64 and sum(1 for l in lines if "eprewmean" in l) == 2
    again = trex_train.load_agent(path, num_envs=2, device=DEV, max_episode_steps=4)
    assert again.env.monitor == env.monitor
    said = []
    trex_train.play(again, 9, log=said.append)
    assert any(l.startswith("Last finished episode: return") and "length 4" in l for l in said), said
