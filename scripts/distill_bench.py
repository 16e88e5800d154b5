#!/usr/bin/env python
"""Cost of K19 (policy distillation: trex_policy_distill_minibatch_step) on the GPU beside the PPO step it shares its kernel text
with, and the driver's rate.

At 4 096 samples per minibatch of a 16 384-sample rollout, obs_dim D = 93 (the locomotion channels), 25 actions, in ONE process,
hipEvents around `iters` back-to-back calls after a warm-up, the median (min .. max) of `repeats` groups, the variants taking turns
group by group:
  (a) trex_policy_minibatch_step beside trex_policy_distill_minibatch_step, both kinds (lr 0: the parameters stay), and trex_policy_act;
  (b) the autograd behaviour-cloning step a trainer without the native learner would run: MlpPolicy forward, the KL or the squared
      error, backward, trex_policy_adam - eager, the ~90-small-kernel path;
  (c) env-steps/s of Distill (rollout with two act launches + update) beside symmetric PPO over `--updates` updates of 32 steps x
      4 096 envs, throughput preset, --observations locomotion --sensing typical --randomize typical, eager and from graphs; the
      teacher is a fresh policy on the clean row (rates do not depend on what it knows).
--parent-lib LIB adds (d): the plain act launch and the plain PPO minibatch step of that library - the parent commit's build - and
of this one in processes of their own, taking turns, two each; the plain paths must be where the parent's are, within the spread of
the alternation itself. The expectation checked in (a): the distillation step costs no more than the PPO step plus that run's own
spread (its head does less arithmetic: no expf per sample, no ratio, no clip). No gate hangs on the timings, and no training benefit is claimed.
Writes profiles/r34_distill.txt (--out); --append FILE adds the lines of FILE (the disassembly record, taken where the compiler is)."""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from observations_bench import groups_us  # noqa: E402

DEV = "cuda:0"
D, A = 93, 25
SAMPLES = 4


def kernels(n, distill=True):
    """{name: call} on random data: the PPO step and the act launch, and (distill) the distillation steps and the autograd steps"""
    from trex_gym import _capi
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    kern = _capi.Policy(n, D, A, 64, 0)
    count = kern.param_count
    theta, grad, m, v = 0.1 * rnd(count), torch.zeros(count, device=DEV), torch.zeros(count, device=DEV), torch.zeros(count, device=DEV)
    rows, noise = rnd(n, D + 2), rnd(n, A)
    rows[:, D + 1] = 0.0
    actions, obs_o, act_o, logp_o, val_o = rnd(n, A), rnd(n, D), rnd(n, A), rnd(n), rnd(n)
    N = SAMPLES * n
    obs, act, logp, val, adv, ret = rnd(N, D), rnd(N, A), -30.0 + rnd(N), rnd(N), rnd(N), rnd(N)
    perm = torch.randperm(N, device=DEV)
    stats = torch.tensor([0.0, 1.0], device=DEV)
    sums = torch.zeros(2, device=DEV)
    fns = {
        "act": lambda: kern.act(theta, rows, noise, actions, obs_o, act_o, logp_o, val_o),
        "PPO minibatch step": lambda: kern.minibatch_step(theta, grad, m, v, obs, act, logp, val, adv, ret, perm, 0, n, stats, lr=0.0, loss_sums=sums),
    }
    if not distill:
        return fns
    from trex_gym import distill_capi
    from trex_gym.ppo import MlpPolicy
    dist = distill_capi.PolicyDistill(kern)
    tlog = -0.5 + 0.3 * rnd(A)
    for name in ("kl", "mse"):
        fns["distillation step, %s" % name] = lambda name=name: dist.minibatch_step(
            theta, grad, m, v, obs, act, ret, tlog if name == "kl" else None, perm, 0, n, name, 0.5, lr=0.0, loss_sums=sums)
    pol = MlpPolicy(kern.layout, count, torch.device(DEV))
    am, av = torch.zeros(count, device=DEV), torch.zeros(count, device=DEV)

    def autograd(name):
        idx = perm[:n]
        o, tm, tv = obs.index_select(0, idx), act.index_select(0, idx), ret.index_select(0, idx)
        d = pol.mean(o) - tm
        if name == "kl":
            ls = pol.logstd
            l_pi = (ls - tlog + (torch.exp(2 * tlog) + d * d) / (2 * torch.exp(2 * ls)) - 0.5).sum(-1).mean()
        else:
            l_pi = 0.5 * (d * d).sum(-1).mean()
        loss = l_pi + 0.5 * 0.5 * ((pol.value(o) - tv) ** 2).mean()
        loss.backward()
        kern.adam(pol.theta, pol.grad, am, av, lr=0.0)

    for name in ("kl", "mse"):
        fns["autograd behaviour-cloning step, %s" % name] = lambda name=name: autograd(name)
    return fns


def rate(n, distill, graphs, updates):
    from trex_gym import trex_train
    from trex_gym.ppo import PPO
    args = trex_train.parse_args(["--observations", "locomotion", "--sensing", "typical", "--randomize", "typical"])
    env = trex_train.build_environment(n, device=DEV, observations=args.observations, sensing=trex_train.sensing_args(args),
                                       randomize=trex_train.randomize_args(args))
    hp = dict(trex_train.PRESETS["throughput"])
    if distill:
        from trex_gym.distill import Distill, Teacher
        donor = PPO(env, nsteps=1, nminibatches=1, noptepochs=1, seed=1)            # a fresh policy of the env's shape as the teacher
        teacher = Teacher(env, (donor.policy.theta.detach().clone(), donor.kern.get_stats()), rows="clean")
        agent = Distill(env, teacher, nsteps=32, nminibatches=hp["nminibatches"], noptepochs=hp["noptepochs"], lr=hp["lr"], loss="kl",
                        beta=0.5, beta_decay=1.0, use_graphs=graphs)
    else:
        agent = PPO(env, nsteps=32, use_graphs=graphs, **hp)
    for _ in range(updates):                        # (the first updates carry the captures and the workspace: timed are `updates` more)
        agent.update(agent.collect())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        agent.update(agent.collect())
    torch.cuda.synchronize()
    r = updates * 32 * n / (time.perf_counter() - t0)
    od = env.obs_dim
    env.close()
    return r, od


def plain_child(args):
    us = groups_us(kernels(args.envs, False), args.iters, args.repeats)
    for name, key in (("ACT", "act"), ("STEP", "PPO minibatch step")):
        print("%s %.2f %.2f %.2f" % ((name,) + us[key]))


def parent_lines(args):
    runs = {k: {"parent": [], "this": []} for k in ("ACT", "STEP")}
    lines = []
    for k in range(2):
        for name, lib in (("parent", args.parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("TREX_LIB", None)
            if lib:
                env["TREX_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--envs", str(args.envs), "--iters",
                                str(args.iters), "--repeats", str(args.repeats)], capture_output=True, text=True, env=env)
            for what in runs:
                mt = re.search(r"%s (\S+) (\S+) (\S+)" % what, r.stdout)
                if not mt:
                    lines.append("  %s commit, run %d, %s: not measured (exit %d)" % (name, k + 1, what, r.returncode))
                    continue
                med, lo, hi = (float(x) for x in mt.groups())
                runs[what][name].append((med, lo, hi))
                lines.append("  %-44s %8.2f  (%.2f .. %.2f)" % ("%s commit, run %d, %s" % (name, k + 1, "act" if what == "ACT" else "PPO minibatch step"),
                                                               med, lo, hi))
    for what, rr in runs.items():
        if rr["parent"] and rr["this"]:
            width = max(hi - lo for v in rr.values() for _, lo, hi in v)
            pm, tm = [r[0] for r in rr["parent"]], [r[0] for r in rr["this"]]
            inside = all(min(pm) - width <= x <= max(pm) + width for x in tm)
            lines.append("  %s: spread of the alternation itself %.2f us within a run, the parent's medians %.2f .. %.2f; this commit's "
                         "medians %.2f .. %.2f: it %s" % ("act" if what == "ACT" else "PPO minibatch step", width, min(pm), max(pm), min(tm), max(tm),
                                                          "did not move beyond that spread" if inside else "MOVED beyond that spread"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--updates", type=int, default=3, help="timed updates per variant (0: leave the drivers out)")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libtrex_hip.so: its plain calls, in alternating processes")
    ap.add_argument("--append", default=None, help="a text file whose lines are added at the end")
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_distill.txt"))
    args = ap.parse_args()
    if args.plain_child:
        return plain_child(args)
    n = args.envs
    us = groups_us(kernels(n), args.iters, args.repeats)
    lines = ["K19, policy distillation: cost at %d samples per minibatch of %d, D = %d, %d actions (us per call: median, min .. max of %d "
             "groups of %d calls)" % (n, SAMPLES * n, D, A, args.repeats, args.iters)]
    ppo = us["PPO minibatch step"]
    for k, (med, lo, hi) in us.items():
        lines.append("  %-44s %8.2f  (%.2f .. %.2f)%s" % (k, med, lo, hi, "   %+.2f against the PPO step" % (med - ppo[0]) if k.startswith("distillation") else ""))
    spread = max(hi - lo for k, (_, lo, hi) in us.items() if k == "PPO minibatch step" or k.startswith("distillation"))
    worst = max(us[k][0] for k in us if k.startswith("distillation"))
    lines.append("  expectation, the distillation step costs no more than the PPO step plus this run's own spread (%.2f us): %s" % (
        spread, "met" if worst <= ppo[0] + spread else "NOT MET (%.2f > %.2f + %.2f)" % (worst, ppo[0], spread)))
    if args.updates > 0:
        lines += ["", "env-steps/s, %d timed updates of 32 steps x %d envs behind as many untimed ones (throughput preset; --observations "
                  "locomotion --sensing typical --randomize typical):" % (args.updates, n)]
        for graphs in (False, True):
            sym, od = rate(n, False, graphs, args.updates)
            dis, _ = rate(n, True, graphs, args.updates)
            lines.append("  %-24s %10.0f  symmetric PPO (D = %d)   %10.0f  Distill (kl, teacher on the clean row, beta 0.5)   %+.1f %%" % (
                "replayed from graphs" if graphs else "eager", sym, od, dis, 100.0 * (dis / sym - 1.0)))
        lines.append("  (rates only - a distillation rollout has a second act launch and a select per step and no GAE: whether the student "
                     "it gives is any good takes long runs nobody has made)")
    if args.parent_lib and os.path.exists(args.parent_lib):
        lines += ["", "the plain act launch and the plain PPO minibatch step of the parent commit and of this one, alternating processes of "
                  "one session (us per call: median, min .. max):"] + parent_lines(args)
    else:
        lines += ["", "the parent commit's plain calls: not measured (no --parent-lib)"]
    if args.append and os.path.exists(args.append):
        lines += [""] + [ln.rstrip("\n") for ln in open(args.append)]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
