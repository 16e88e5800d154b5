#!/usr/bin/env python
"""Cost of kernel K13 (the sensor model: trex_batch_apply_sensing, trex_batch_delay_actions) on the GPU, against the same effect from
torch ops, and its resource lines.

Cost at 4 096 envs in ONE process, on bench.py's stationary episode mix (1000-step episodes with staggered phases, uniform random
actions from a pool, a pre-roll of one episode length), with the channels of observations.locomotion (93 columns), hipEvents
around `iters` back-to-back calls after a warm-up, the median (min .. max) of `repeats` groups, the variants taking turns group by
group:
  (a) step_tensor alone: no sensors - what the parent commit runs;
  (b) step_tensor with sensing.typical and a one-step action delay: two more launches (delay_actions before the step call,
      apply_sensing behind the compose);
  (c) the same effect from torch ops around the plain env's step: the action delay as a ring of two slots indexed per env and
      restarted by `where` on done; white noise by `randn` times a row of sigmas; the bias redrawn by `where` on done; the encoder's
      resolution by round(). It reads `done` after the fact, so it restarts one row late - what the device launch does not.
No gate hangs on the timings. Writes profiles/r28_sensing.txt (--out); --accuracy FILE appends the lines tests/test_gpu_sensing.py
printed (pytest -s) that it finds in FILE."""
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
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "sensing.hip")
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


def torch_sensors(v, step_pool, groups):
    """the effect of `groups` and a one-step action delay from torch ops around the env's own step"""
    n, D, dev = v.num_envs, v.obs_dim, v.device
    sigma, half, quantum = (torch.zeros(D, device=dev) for _ in range(3))
    for c0, w, _, noise, bias, q, _, _ in groups:
        sigma[c0:c0 + w], half[c0:c0 + w], quantum[c0:c0 + w] = noise, bias, q
    has_q = quantum > 0
    safe_q = torch.where(has_q, quantum, torch.ones_like(quantum))
    gen = torch.Generator(device=dev).manual_seed(0)
    bias = (torch.rand(n, D, device=dev, generator=gen) * 2 - 1) * half
    ring = torch.zeros(2, n, v.A, device=dev)
    count = torch.zeros(n, dtype=torch.long, device=dev)       # actions of the episode so far
    env_ids = torch.arange(n, device=dev)
    noisy = torch.zeros(n, D, device=dev)
    state = dict(t=0)

    def step():
        act = step_pool[state["t"] % len(step_pool)]
        state["t"] += 1
        count.mul_(~v.done)                                     # `where` on done: the history starts afresh
        ring[count % 2, env_ids] = act
        delayed = ring[(count - 1).clamp_(min=0) % 2, env_ids]
        count.add_(1)
        v.step_tensor(delayed)
        fresh = (torch.rand(n, D, device=dev, generator=gen) * 2 - 1) * half
        bias.copy_(torch.where(v.done[:, None], fresh, bias))
        y = v.obs + bias + torch.randn(n, D, device=dev, generator=gen) * sigma
        noisy.copy_(torch.where(has_q, torch.round(y / safe_q) * safe_q, y))
    return step, noisy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--accuracy", default=None, help="a file with the output of pytest -s tests/test_gpu_sensing.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_sensing.txt"))
    args = ap.parse_args()
    from trex_gym import _capi, observations as O, sensing as S
    n = args.envs
    spec = O.locomotion(_capi.Model(), "cuda:0")
    plain, step_plain = make_env(n, observations=spec)
    native, step_native = make_env(n, preroll=0, observations=spec)
    S.attach(native, S.typical(native), action_delay=1, seed=0)
    native.reset_tensor()
    native.set_episode_steps(((torch.arange(n) * 1000) // n).to(torch.int32))      # (make_env's stagger, again after the reset)
    for _ in range(1000):
        step_native()
    eager, _ = make_env(n, observations=spec)
    lo, hi = torch.tensor(eager.model.lower, dtype=torch.float32), torch.tensor(eager.model.upper, dtype=torch.float32)
    pool = [(lo + (hi - lo) * torch.rand(n, eager.J, generator=torch.Generator().manual_seed(k))).to(eager.device) for k in range(16)]
    step_torch, _ = torch_sensors(eager, pool, native.sensing["groups"])
    fns = {"step_tensor alone": step_plain, "step + K13 (typical, action delay 1)": step_native,
           "step + the same from torch ops": step_torch}
    us = groups_us(fns, args.iters, args.repeats)
    lines = ["K13, the sensor model: cost at %d envs, 93-column rows (us per call: median, min .. max of %d groups of %d calls)"
             % (n, args.repeats, args.iters)]
    base = us["step_tensor alone"][0]
    for k, (med, lo_, hi_) in us.items():
        lines.append("  %-38s %8.1f  (%.1f .. %.1f)%s" % (k, med, lo_, hi_, "" if k.endswith("alone") else "   %+.1f" % (med - base)))
    a, b = us["step + K13 (typical, action delay 1)"][0] - base, us["step + the same from torch ops"][0] - base
    lines.append("  the native path is %s than the torch path: %+.1f us against %+.1f us per step" % ("FASTER" if a < b else "NOT faster", a, b))
    lines += ["groups: %d over %d of 93 columns (%s); action delay 1 step" % (len(native.sensing["groups"]), sum(g[1] for g in native.sensing["groups"]),
                                                                              ", ".join("[%d, %d)" % (g[0], g[0] + g[1]) for g in native.sensing["groups"])),
              "resource usage (hipcc -Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if args.accuracy and os.path.exists(args.accuracy):
        found = [ln.rstrip() for ln in open(args.accuracy) if "Gaussian deviation" in ln]
        lines += ["", "accuracy, tests/test_gpu_sensing.py (the Gaussian deviation as a share of the allowed 4 x bound, the bound being the "
                  "reference's own f32 run against its f64 run; 1 = at the limit):"] + ["  " + ln.lstrip(". ") for ln in found]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
