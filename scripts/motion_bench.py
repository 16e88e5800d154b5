#!/usr/bin/env python
"""Cost of kernel K12 (the motion clip: trex_batch_compose_motion_reward, trex_batch_motion_reset, trex_batch_motion_sample) on the
GPU, and its resource lines.

Cost at 4 096 envs in ONE process, on bench.py's stationary episode mix (1000-step episodes with staggered phases, uniform random
actions from a pool, a pre-roll of one episode length), hipEvents around `iters` back-to-back calls after a warm-up, the median
(min .. max) of `repeats` groups, the variants taking turns group by group:
  (a) step_rows alone: TrexVecEnv without a clip - what the parent commit runs;
  (b) step_rows + compose_motion_reward: the preset imitation(model) - pose, velocity, end effector (4 points), root pose - against a
      looping clip of 64 frames;
  (c) the same with rsi: one more launch (motion_reset) and one in-place draw of the instants per step;
  (d) motion_sample alone, state and points.
The accuracy figures are what tests/test_gpu_motion.py prints (pytest -s). No gate hangs on the timings. Writes
profiles/r24_motion.txt (--out)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from observations_bench import groups_us, make_env  # noqa: E402


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "motion.hip")
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


def looping_clip(model, frames=64, frame_dt=1.0 / 30.0):
    """sinusoids of one period inside the middle half of every joint's range; the base walks along x at its start height"""
    from trex_gym.motion import Clip
    lo, hi = np.asarray(model.lower, np.float64), np.asarray(model.upper, np.float64)
    s = np.arange(frames) / (frames - 1.0)
    rng = np.random.default_rng(0)
    q = 0.5 * (lo + hi) + 0.25 * (hi - lo) * np.sin(2 * np.pi * s[:, None] + rng.uniform(0, 2 * np.pi, len(lo)))
    base = np.zeros((frames, 7))
    base[:, 0], base[:, 2], base[:, 6] = 1.0 * s * (frames - 1) * frame_dt, 3.0, 1.0
    return Clip(np.concatenate([base, q], 1), frame_dt, loop=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_motion.txt"))
    args = ap.parse_args()
    from trex_gym import motion as M
    from trex_gym.termination import foot_links
    n = args.envs
    plain, step_plain = make_env(n)
    feet = [(l, (0.0, 0.0, 0.0)) for l in foot_links(plain)][:4]
    fns = {"step_rows alone": step_plain}
    envs = {}
    for name, rsi in (("step + compose_motion_reward", False), ("step + compose + rsi", True)):
        v, step = make_env(n, preroll=0)
        M.attach(v, looping_clip(v.model), end_effectors=feet, rsi=rsi)
        v.reset_tensor()
        v.set_episode_steps(((torch.arange(n) * 1000) // n).to(torch.int32))      # (make_env's stagger, again after the reset)
        for _ in range(1000):
            step()
        envs[name], fns[name] = v, step
    v = envs["step + compose_motion_reward"]
    state = torch.zeros(n, v.batch.state_width, device=v.device)
    points = torch.zeros(n, len(feet), 3, device=v.device)
    fns["motion_sample (state, points)"] = lambda: v.motion_api.sample(None, state, points)
    us = groups_us(fns, args.iters, args.repeats)
    lines = ["K12, the motion clip: cost at %d envs (us per call: median, min .. max of %d groups of %d calls)" % (n, args.repeats, args.iters)]
    base = us["step_rows alone"][0]
    for k, (med, lo, hi) in us.items():
        lines.append("  %-34s %8.1f  (%.1f .. %.1f)%s" % (k, med, lo, hi, "" if k.startswith(("step_rows", "motion_sample")) else "   %+.1f" % (med - base)))
    lines += ["terms: " + ", ".join(v.motion_names) + "; %d end effectors; clip of %d frames, looping" % (len(feet), v.motion.num_frames),
              "resource usage (hipcc -Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
