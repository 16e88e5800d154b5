#!/usr/bin/env python
"""Cost of kernel K14 (episode randomisation: trex_batch_apply_randomization) on the GPU, against the same effect from the host
path, and its resource lines.

Cost at 4 096 envs in ONE process, on bench.py's stationary episode mix (1000-step episodes with staggered phases, uniform random
actions from a pool, a pre-roll of one episode length), hipEvents around `iters` back-to-back calls after a warm-up, the median
(min .. max) of `repeats` groups, the variants taking turns group by group:
  (a) step_tensor alone: no randomisation - what the parent commit runs;
  (b) step_tensor with randomize.typical and three command terms attached: one more launch behind the step call;
  (c) the same effect from the host path around the plain env's step: perturb.RandomPushes.wrench with set_external_wrench,
      perturb.RandomGains.draw(done) with set_motor_gains, mass scale and friction redrawn by `where` on done with set_domain,
      the command resampled by `where` on done and on the interval.
No gate hangs on the timings. Writes profiles/r29_randomize.txt (--out); --accuracy FILE appends the lines
tests/test_gpu_randomize.py printed (pytest -s) that it finds in FILE; --parent FILE the lines of a file that holds the plain step
time of the parent commit and of this one, measured in the same session by alternating processes."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from observations_bench import groups_us, make_env  # noqa: E402


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "randomize.hip")
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


def spread_line(path):
    """the plain-step medians of the parent commit and of this one in the file --parent names, and whether this commit's lie
    within the spread of the session: the parent's own range widened by the largest (max - min) of a single run"""
    import re
    runs = {"parent": [], "this": []}
    width = 0.0
    for ln in open(path):
        m = re.match(r"\s*(parent|this) commit.*?(\d+\.\d+)\s+\((\d+\.\d+) \.\. (\d+\.\d+)\)", ln)
        if m:
            runs[m.group(1)].append(float(m.group(2)))
            width = max(width, float(m.group(4)) - float(m.group(3)))
    if not runs["parent"] or not runs["this"]:
        return "  (no runs found)"
    lo, hi = min(runs["parent"]) - width, max(runs["parent"]) + width
    inside = all(lo <= x <= hi for x in runs["this"])
    return ("  run-to-run spread of the session: %.1f us within a run, the parent's medians %.1f .. %.1f; this commit's medians %.1f .. %.1f: "
            "the plain step %s" % (width, min(runs["parent"]), max(runs["parent"]), min(runs["this"]), max(runs["this"]),
                                   "did not move beyond that spread" if inside else "MOVED beyond that spread"))


def spec_of(env):
    from trex_gym import randomize as Z
    return Z.merge(Z.typical(env), [Z.command(c, -h, h, 250, 0.1) for c, h in enumerate((1.0, 0.3, 0.5))])


def host_path(v, step_pool):
    """the effect of spec_of() from torch ops and the existing setters around the env's own step"""
    from trex_gym import perturb
    n, dev, nb = v.num_envs, v.device, v.model.num_bodies
    gen = torch.Generator(device=dev).manual_seed(0)
    pushes = perturb.RandomPushes(n, body=0, interval=200, probability=1.0, max_force=300.0, duration=5, generator=gen, device=dev)
    gains = perturb.RandomGains(n, v.J, kp_scale=(0.8, 1.2), kd_scale=(0.8, 1.2), max_force_scale=(0.9, 1.1), generator=gen, device=dev)
    mass, friction = torch.ones(n, nb, device=dev), torch.full((n,), 0.8, device=dev)
    commands, count = torch.zeros(n, 3, device=dev), torch.zeros(n, dtype=torch.long, device=dev)
    half = torch.tensor([1.0, 0.3, 0.5], device=dev)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    state = dict(t=0)

    def step():
        act = step_pool[state["t"] % len(step_pool)]
        state["t"] += 1
        done = v.done
        v.set_external_wrench(pushes.wrench(nb, done))
        v.set_motor_gains(**gains.draw(done))
        mass.copy_(torch.where(done[:, None], 0.9 + 0.2 * rand(n, nb), mass))
        friction.copy_(torch.where(done, 0.5 + 0.75 * rand(n), friction))
        v.set_domain(mass, friction)
        count.mul_(~done).add_(1)
        again = done | (count % 250 == 0)
        fresh = torch.where(rand(n, 3) < 0.1, torch.zeros_like(commands), (2.0 * rand(n, 3) - 1.0) * half)
        commands.copy_(torch.where(again[:, None], fresh, commands))
        v.step_tensor(act)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--accuracy", default=None, help="a file with the output of pytest -s tests/test_gpu_randomize.py")
    ap.add_argument("--parent", default=None, help="a file with the plain step times of the parent commit and this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_randomize.txt"))
    args = ap.parse_args()
    from trex_gym import randomize as Z
    n = args.envs
    plain, step_plain = make_env(n)
    native, step_native = make_env(n, preroll=0)
    Z.attach(native, spec_of(native), seed=0)
    native.reset_tensor()
    native.set_episode_steps(((torch.arange(n) * 1000) // n).to(torch.int32))      # (make_env's stagger, again after the reset)
    for _ in range(1000):
        step_native()
    eager, _ = make_env(n)
    lo, hi = torch.tensor(eager.model.lower, dtype=torch.float32), torch.tensor(eager.model.upper, dtype=torch.float32)
    pool = [(lo + (hi - lo) * torch.rand(n, eager.J, generator=torch.Generator().manual_seed(k))).to(eager.device) for k in range(16)]
    step_host = host_path(eager, pool)
    names = ("step_tensor alone", "step + K14 (typical + commands)", "step + the same from the host path")
    us = groups_us(dict(zip(names, (step_plain, step_native, step_host))), args.iters, args.repeats)
    lines = ["K14, episode randomisation: cost at %d envs, 77-column rows (us per call: median, min .. max of %d groups of %d calls)"
             % (n, args.repeats, args.iters)]
    base = us[names[0]][0]
    for k, (med, lo_, hi_) in us.items():
        lines.append("  %-38s %8.1f  (%.1f .. %.1f)%s" % (k, med, lo_, hi_, "" if k.endswith("alone") else "   %+.1f" % (med - base)))
    a, b = us[names[1]][0] - base, us[names[2]][0] - base
    lines.append("  the device path is %s than the host path: %+.1f us against %+.1f us per step" % ("CHEAPER" if a < b else "NOT cheaper", a, b))
    lines.append("  (in both, the step launch runs the wrench, actuator and per-env domain variants of the step kernel: their cost is in both "
                 "differences, beside the launch of K14 or the host's ops)")
    kinds = [Z.KIND_NAMES[t[0]] for t in native.randomization["terms"]]
    lines += ["terms: %d (%s)" % (len(kinds), ", ".join(kinds)),
              "resource usage (hipcc -Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if args.parent and os.path.exists(args.parent):
        lines += ["", "the plain step of the parent commit and of this one, alternating processes of one session (us per call: median, "
                  "min .. max):"] + ["  " + ln.rstrip() for ln in open(args.parent) if ln.strip()] + [spread_line(args.parent)]
    if args.accuracy and os.path.exists(args.accuracy):
        found = [ln.rstrip() for ln in open(args.accuracy) if "of the bound" in ln]
        lines += ["", "accuracy, tests/test_gpu_randomize.py (the largest push-force deviation as a share of the allowed bound: 4 x the "
                  "reference's own f32 run against its f64 run, floored at 2 ulp of hi; values, counters and commands are bitwise):"]
        lines += ["  " + ln.lstrip(". ") for ln in found]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
