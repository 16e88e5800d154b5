#!/usr/bin/env python
"""Cost of K16 (the privileged critic: trex_policy_critic_act / _critic_observe / _critic_minibatch_step) on the GPU beside the plain
calls, and the trainer's rate with and without a critic.

At 4 096 envs, obs_dim D = 93 (the locomotion channels), critic width Dv = 96, 25 actions, in ONE process, hipEvents around
`iters` back-to-back calls after a warm-up, the median (min .. max) of `repeats` groups, the variants taking turns group by group:
  (a) the act launch: trex_policy_act on a Policy(D), trex_policy_critic_act on the same shapes with a critic row;
  (b) the minibatch step (4 096 samples of a 16 384-sample rollout): trex_policy_minibatch_step, trex_policy_critic_minibatch_step;
  (c) trex_policy_critic_observe beside trex_policy_observe (with the reward side);
  (d) PPO env-steps/s over `--updates` updates of 32 steps x 4 096 envs, throughput preset, --observations locomotion --sensing
      typical --randomize typical: symmetric against --critic privileged, eager and replayed from graphs.
--parent-lib LIB adds (e): the plain act launch and the plain minibatch step of that library - the parent commit's build - and of
this one in processes of their own, taking turns, two each; the plain paths must be where the parent's are, within the spread of the
alternation itself. No gate hangs on the timings, and no training benefit is claimed: that takes long runs nobody has made.
Writes profiles/r31_critic.txt (--out); --append FILE adds the lines of FILE (the disassembly record and the resource usage of the
new instantiations, taken where the compiler is)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from observations_bench import groups_us  # noqa: E402

DEV = "cuda:0"
D, DV, A = 93, 96, 25
SAMPLES = 4


def kernels(n, critic):
    """{name: call} of the act launch, the minibatch step and the statistics launches on random data, plain or with a critic"""
    from trex_gym import _capi, critic_capi
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    kern = _capi.Policy(n, D, A, 64, 0)
    crit = None
    count = kern.param_count
    if critic:
        crit = critic_capi.PolicyCritic(kern)
        crit.set(DV)
        count = crit.param_count
    theta, grad, m, v = 0.1 * rnd(count), torch.zeros(count, device=DEV), torch.zeros(count, device=DEV), torch.zeros(count, device=DEV)
    rows, rows_v, noise = rnd(n, D + 2), rnd(n, DV), rnd(n, A)
    rows[:, D + 1] = 0.0
    actions, obs_o, obs_vo, act_o, logp_o, val_o = rnd(n, A), rnd(n, D), rnd(n, DV), rnd(n, A), rnd(n), rnd(n)
    N = SAMPLES * n
    obs, obs_v, act, logp, val, adv, ret = rnd(N, D), rnd(N, DV), rnd(N, A), -30.0 + rnd(N), rnd(N), rnd(N), rnd(N)
    perm = torch.randperm(N, device=DEV)
    stats = torch.tensor([0.0, 1.0], device=DEV)
    sums = torch.zeros(2, device=DEV)
    if critic:
        return {
            "act with a critic row": lambda: crit.act(theta, rows, rows_v, noise, actions, obs_o, obs_vo, act_o, logp_o, val_o),
            "minibatch step with a critic buffer": lambda: crit.minibatch_step(theta, grad, m, v, obs, obs_v, act, logp, val, adv, ret, perm, 0, n,
                                                                               stats, lr=0.0, loss_sums=sums),
            "critic observe (Dv = %d)" % DV: lambda: crit.observe(rows_v),
        }
    return {
        "act": lambda: kern.act(theta, rows, noise, actions, obs_o, act_o, logp_o, val_o),
        "minibatch step": lambda: kern.minibatch_step(theta, grad, m, v, obs, act, logp, val, adv, ret, perm, 0, n, stats, lr=0.0, loss_sums=sums),
        "observe (D = %d, with the reward side)" % D: lambda: kern.observe(rows, True, 0.99),
    }


def ppo_rate(n, critic, graphs, updates):
    from trex_gym import trex_train
    args = trex_train.parse_args(["--observations", "locomotion", "--sensing", "typical", "--randomize", "typical"])
    env = trex_train.build_environment(n, device=DEV, observations=args.observations, sensing=trex_train.sensing_args(args),
                                       randomize=trex_train.randomize_args(args), critic="privileged" if critic else None)
    agent, hist = trex_train.train(env, updates * 32 * n, 0, nsteps=32, log=lambda s: None, use_graphs=graphs, preset="throughput")
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()                        # (the first updates carry the captures and the workspace: timed are `updates` more)
    for _ in range(updates):
        agent.update(agent.collect())
    torch.cuda.synchronize()
    rate = updates * 32 * n / (time.perf_counter() - t0)
    spec = getattr(env, "critic_spec", None)
    env.close()
    return rate, env.obs_dim, (spec["dim"], [s[0] for s in spec["sources"]], spec["left_out"]) if spec else None


def plain_child(args):
    us = groups_us(kernels(args.envs, False), args.iters, args.repeats)
    for name, key in (("ACT", "act"), ("STEP", "minibatch step")):
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
                lines.append("  %-44s %8.2f  (%.2f .. %.2f)" % ("%s commit, run %d, plain %s" % (name, k + 1, "act" if what == "ACT" else "minibatch step"),
                                                               med, lo, hi))
    for what, rr in runs.items():
        if rr["parent"] and rr["this"]:
            width = max(hi - lo for v in rr.values() for _, lo, hi in v)
            pm, tm = [r[0] for r in rr["parent"]], [r[0] for r in rr["this"]]
            inside = all(min(pm) - width <= x <= max(pm) + width for x in tm)
            lines.append("  plain %s: spread of the alternation itself %.2f us within a run, the parent's medians %.2f .. %.2f; this commit's "
                         "medians %.2f .. %.2f: it %s" % ("act" if what == "ACT" else "minibatch step", width, min(pm), max(pm), min(tm), max(tm),
                                                          "did not move beyond that spread" if inside else "MOVED beyond that spread"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--updates", type=int, default=3, help="timed PPO updates per variant (0: leave the trainer out)")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libtrex_hip.so: its plain calls, in alternating processes")
    ap.add_argument("--append", default=None, help="a text file whose lines are added at the end")
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_critic.txt"))
    args = ap.parse_args()
    if args.plain_child:
        return plain_child(args)
    n = args.envs
    fns = kernels(n, False)
    fns.update(kernels(n, True))
    us = groups_us(fns, args.iters, args.repeats)
    lines = ["K16, privileged critic: cost at %d envs, D = %d, Dv = %d, %d actions (us per call: median, min .. max of %d groups of %d "
             "calls)" % (n, D, DV, A, args.repeats, args.iters)]
    order = ["act", "act with a critic row", "minibatch step", "minibatch step with a critic buffer",
             "observe (D = %d, with the reward side)" % D, "critic observe (Dv = %d)" % DV]
    for k in order:
        med, lo, hi = us[k]
        base = us[order[order.index(k) - 1]][0] if order.index(k) % 2 else None
        lines.append("  %-44s %8.2f  (%.2f .. %.2f)%s" % (k, med, lo, hi, "" if base is None else "   %+.2f" % (med - base)))
    lines.append("  the act and learner launches keep their shape - one workgroup per (tile of 32, net) - and the vf workgroups read their own "
                 "row; the critic observe is the statistics' two launches on a second block")
    if args.updates > 0:
        lines += ["", "PPO env-steps/s, %d timed updates of 32 steps x %d envs behind as many untimed ones (throughput preset; --observations "
                  "locomotion --sensing typical --randomize typical):" % (args.updates, n)]
        for graphs in (False, True):
            sym, od, _ = ppo_rate(n, False, graphs, args.updates)
            asy, _, spec = ppo_rate(n, True, graphs, args.updates)
            lines.append("  %-44s %10.0f  symmetric (D = %d)   %10.0f  --critic privileged (Dv = %d: %s; left out: %s)   %+.1f %%" % (
                "replayed from graphs" if graphs else "eager", sym, od, asy, spec[0], ", ".join(spec[1]), ", ".join(spec[2]) or "none",
                100.0 * (asy / sym - 1.0)))
        lines.append("  (rates only: whether a privileged critic trains a better policy takes long runs nobody has made)")
    if args.parent_lib and os.path.exists(args.parent_lib):
        lines += ["", "the plain act launch and the plain minibatch step of the parent commit and of this one, alternating processes of one "
                  "session (us per call: median, min .. max):"] + parent_lines(args)
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
