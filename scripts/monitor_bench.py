#!/usr/bin/env python
"""Cost of kernel K15 (the episode monitor: trex_batch_monitor_apply) on the GPU, against the same statistics from torch ops, and its
resource lines.

Cost at 4 096 envs in ONE process, with the locomotion channels and reward preset, on bench.py's stationary episode mix (1000-step
episodes with staggered phases, uniform random actions from a pool, a pre-roll of one episode length), hipEvents around `iters`
back-to-back calls after a warm-up, the median (min .. max) of `repeats` groups, the variants taking turns group by group:
  (a) step_tensor alone: no monitor - what the parent commit runs;
  (b) step_tensor with the monitor attached at W = 100 and the preset's term columns: two more launches behind the step call;
  (c) the same statistics from torch ops behind the plain env's step, without a host read-back: the f64 accumulates, the `where`
      on done, the records scattered into a ring at slots from a `cumsum` of done, the reason copy.
--parent-lib LIB adds (d): the plain step of that library - the parent commit's build - and of this one in processes of their own,
taking turns, two each; the plain step must be where the parent's is, within the spread of the alternation itself.
No gate hangs on the timings. Writes profiles/r30_monitor.txt (--out); --accuracy FILE appends the lines tests/test_gpu_monitor.py
printed (pytest -s) that it finds in FILE."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from observations_bench import EPISODE_STEPS, POOL, groups_us  # noqa: E402

WINDOW = 100


def make_env(n, preset=True, monitor=False):
    """an env on the stationary mix (observations_bench.make_env), with the locomotion channels and reward preset"""
    from trex_gym import monitor as monitoring, trex_train
    kw = dict(observations="locomotion", rewards="locomotion") if preset else {}
    v = trex_train.build_environment(n, device="cuda:0", max_episode_steps=EPISODE_STEPS, **kw)
    if monitor:
        monitoring.attach(v, window=WINDOW)
    v.reset_tensor()
    v.set_episode_steps(((torch.arange(n) * EPISODE_STEPS) // n).to(torch.int32))
    gen = torch.Generator().manual_seed(0)
    lo, hi = torch.tensor(v.model.lower, dtype=torch.float32), torch.tensor(v.model.upper, dtype=torch.float32)
    pool = [(lo + (hi - lo) * torch.rand(n, v.J, generator=gen)).to(v.device) for _ in range(POOL)]
    state = dict(t=0)

    def step():
        v.step_tensor(pool[state["t"] % POOL])
        state["t"] += 1
    for _ in range(EPISODE_STEPS):
        step()
    torch.cuda.synchronize()
    return v, step


def torch_path(v, step):
    """the monitor's statistics from torch ops behind the env's own step; nothing is read back"""
    n, dev, C = v.num_envs, v.device, v.reward_terms.shape[1]
    ret, col = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, C, dtype=torch.float64, device=dev)
    length, episodes = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    reason, reason_src = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    ring_ret, ring_len = torch.zeros(WINDOW + 1, device=dev), torch.zeros(WINDOW + 1, dtype=torch.int32, device=dev)
    ring_reason, ring_cols = torch.zeros(WINDOW + 1, dtype=torch.int32, device=dev), torch.zeros(WINDOW + 1, C, device=dev)
    total = torch.zeros((), dtype=torch.int64, device=dev)
    dump = torch.full((n,), WINDOW, dtype=torch.int64, device=dev)      # the slot of an env that did not finish: one past the ring
    zero64, zero32 = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.int32, device=dev)

    def call():
        step()
        done = v.done
        ret.add_(v.rew)
        length.add_(1)
        col.add_(v.reward_terms)
        reason.copy_(reason_src)
        rank = torch.cumsum(done, 0) - 1
        slot = torch.where(done, (total + rank) % WINDOW, dump)
        ring_ret.index_copy_(0, slot, ret.float())
        ring_len.index_copy_(0, slot, length)
        ring_reason.index_copy_(0, slot, reason)
        ring_cols.index_copy_(0, slot, col.float())
        total.add_(done.sum())
        episodes.add_(done)
        ret.copy_(torch.where(done, zero64, ret))
        length.copy_(torch.where(done, zero32, length))
        col.copy_(torch.where(done[:, None], zero64, col))
    return call


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "monitor.hip")
    if not os.path.exists(hipcc):
        return ["  not recorded: no hipcc here"]
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "-fno-slp-vectorize", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True)
    keep = [ln.split("remark:")[1].split("[-Rpass")[0].strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    out, at = [], 0
    for k, item in enumerate(keep):                                 # one line per kernel
        if item.startswith("Function Name") and k:
            out.append("  " + "; ".join(keep[at:k]))
            at = k
    return out + ["  " + "; ".join(keep[at:])] if keep else ["  not recorded: hipcc exit %d" % r.returncode]


def plain_child(args):
    v, step = make_env(args.envs, preset=False)
    med, lo, hi = groups_us(dict(plain=step), args.iters, args.repeats)["plain"]
    print("PLAIN %.2f %.2f %.2f" % (med, lo, hi))


def parent_lines(args):
    """the plain step (77-column rows, nothing attached) of the parent's library and of this one, processes taking turns"""
    runs = {"parent": [], "this": []}
    lines = []
    for k in range(2):
        for name, lib in (("parent", args.parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("TREX_LIB", None)
            if lib:
                env["TREX_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--envs", str(args.envs), "--iters",
                                str(args.iters), "--repeats", str(args.repeats)], capture_output=True, text=True, env=env)
            m = re.search(r"PLAIN (\S+) (\S+) (\S+)", r.stdout)
            if not m:
                lines.append("  %s commit, run %d: not measured (exit %d)" % (name, k + 1, r.returncode))
                continue
            med, lo, hi = (float(x) for x in m.groups())
            runs[name].append((med, lo, hi))
            lines.append("  %-28s %8.1f  (%.1f .. %.1f)" % ("%s commit, run %d" % (name, k + 1), med, lo, hi))
    if runs["parent"] and runs["this"]:
        width = max(hi - lo for v in runs.values() for _, lo, hi in v)
        pm, tm = [r[0] for r in runs["parent"]], [r[0] for r in runs["this"]]
        inside = all(min(pm) - width <= x <= max(pm) + width for x in tm)
        lines.append("  spread of the alternation itself: %.1f us within a run, the parent's medians %.1f .. %.1f; this commit's medians "
                     "%.1f .. %.1f: the plain step %s" % (width, min(pm), max(pm), min(tm), max(tm),
                                                          "did not move beyond that spread" if inside else "MOVED beyond that spread"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--accuracy", default=None, help="a file with the output of pytest -s tests/test_gpu_monitor.py")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libtrex_hip.so: its plain step, in alternating processes")
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_monitor.txt"))
    args = ap.parse_args()
    if args.plain_child:
        return plain_child(args)
    n = args.envs
    plain, step_plain = make_env(n)
    native, step_native = make_env(n, monitor=True)
    eager, step_eager = make_env(n)
    step_torch = torch_path(eager, step_eager)
    names = ("step_tensor alone", "step + K15 (W = %d, %d term columns)" % (WINDOW, native.monitor_api.cols), "step + the same from torch ops")
    us = groups_us(dict(zip(names, (step_plain, step_native, step_torch))), args.iters, args.repeats)
    lines = ["K15, episode monitor: cost at %d envs, locomotion channels and reward preset (us per call: median, min .. max of %d groups "
             "of %d calls)" % (n, args.repeats, args.iters)]
    base = us[names[0]][0]
    for k, (med, lo_, hi_) in us.items():
        lines.append("  %-42s %8.1f  (%.1f .. %.1f)%s" % (k, med, lo_, hi_, "" if k.endswith("alone") else "   %+.1f" % (med - base)))
    a, b = us[names[1]][0] - base, us[names[2]][0] - base
    lines.append("  the device path is %s than the torch path: %+.1f us against %+.1f us per step" % ("CHEAPER" if a < b else "NOT cheaper", a, b))
    from trex_gym import monitor as monitoring
    stats = monitoring.episode_stats(native)
    team = 1
    while team < native.monitor_api.cols:
        team *= 2
    lines.append("  form (a): two launches per apply - accumulate (a team of %d lanes per env), commit (one workgroup); form (b), one launch "
                 "with a last-arriving committer, was not built" % team)
    lines.append("  the monitor after the run: %d episodes, eprewmean %.4g, eplenmean %.1f over the last %d" % (stats["episodes"], stats["eprewmean"],
                                                                                                         stats["eplenmean"], stats["window_episodes"]))
    lines += ["resource usage (hipcc -Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if args.parent_lib and os.path.exists(args.parent_lib):
        lines += ["", "the plain step of the parent commit and of this one, alternating processes of one session (77-column rows; us per call: "
                  "median, min .. max):"] + parent_lines(args)
    else:
        lines += ["", "the parent commit's plain step: not measured (no --parent-lib)"]
    if args.accuracy and os.path.exists(args.accuracy):
        found = [ln.rstrip() for ln in open(args.accuracy) if "summary |device - reference|" in ln]
        lines += ["", "accuracy, tests/test_gpu_monitor.py (ring, running episodes, last records and counters are bitwise the reference's; the "
                  "summary's largest deviation from the reference's f64 summary beside the derived bound of the return mean):"]
        lines += ["  " + ln.lstrip(". ") for ln in found]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
