#!/usr/bin/env python
"""Cost of kernel K21 (the sampling-based planner, include/trex_planner.h) on the GPU, against the same plan written with torch ops -
the path the API allowed before - and its resource lines.

Shapes: G = 1 / K = 4096 and G = 16 / K = 256, S = 16 steps, P = 6 cubic knots, A = 25 - 4096 sample envs either way. In ONE
process, hipEvents around `iters` back-to-back calls after a warm-up, the median (min .. max) of `repeats` groups, the variants
taking turns group by group:
  (a) the sample, update and shift launches alone, on a synthetic [S, N, 3J + 5] row block;
  (b) a whole Planner.plan() - state copy, sample, one step_many launch of S steps, update - eager and replayed from a graph;
  (c) the same plan from torch ops around the same step_many launch: randn, a basis matmul, clamps, a masked discounted sum, a
      softmax, an einsum - kept here as torch_plan(); and those ops alone, without the rollout.
Then the return of a 100-step closed loop (G = 16, K = 256) beside the same loop with sigma = 0 - a recorded figure, nothing more.
No gate hangs on a timing or on control quality. Writes profiles/r37_planner.txt (--out); --accuracy FILE appends the lines
tests/test_gpu_planner.py printed (pytest -s) that it finds in FILE; --parent FILE the lines of a file that holds the plain step time
of the parent commit and of this one, measured in the same session by alternating processes: each such line is what
`planner_bench.py --plain LABEL` prints - the plain step on bench.py's stationary mix of whatever library TREX_LIB names."""
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
from randomize_bench import spread_line  # noqa: E402

S, P, SIGMA, TEMPERATURE, GAMMA = 16, 6, 0.1, 0.1, 0.99
SHAPES = ((1, 4096), (16, 256))
DEV = "cuda:0"


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "planner.hip")
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


def plant_of(G):
    from trex_gym.vec_env import TrexVecEnv
    v = TrexVecEnv(G, device=DEV)
    v.reset_tensor()
    for _ in range(5):
        v.step_tensor(torch.zeros(G, v.A, device=DEV))
    return v


def launches(G, K):
    """(a): the three launches alone on a synthetic row block"""
    from trex_gym.planner_capi import PlannerHandle
    N, A, W = G * K, 25, 80
    h = PlannerHandle(G, K, S, P, A, "cubic", 0)
    h.set_noise(SIGMA, -1.0, 1.0, 0, 0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    rows = torch.rand(S, N, W, device=DEV, generator=gen)
    rows[:, :, 76] = (rows[:, :, 76] > 0.98).float()
    acts = torch.zeros(S, N, A, device=DEV)
    flat = rows.view(-1)
    R, w, best, stats = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), torch.zeros(G, dtype=torch.int32, device=DEV), torch.zeros(G, 4, device=DEV)
    return {"sample (knots + [S, N, A] actions)": lambda: h.sample(acts),
            "update (returns, weights, nominal: 3 launches)": lambda: h.update(flat[75:], N * W, W, flat[76:], None, GAMMA, TEMPERATURE, R, w, best, stats),
            "update at temperature 0 (the best sample's knots copied)": lambda: h.update(flat[75:], N * W, W, flat[76:], None, GAMMA, 0.0, R, w, best, stats),
            "shift by one step": lambda: h.shift(1)}, h


def torch_plan(plant, sim, K, state):
    """(c): one planning iteration from torch ops; `state` carries the nominal knots [G, P, A], the basis [S, P], the limits"""
    G, A = plant.num_envs, plant.A
    sim.set_state(plant.get_state().repeat_interleave(K, 0), motors_enabled=True)
    rows = sim.step_many_tensor(torch_sample(state, G, K, A), state["rows"])
    state["nominal"] = torch_update(state, rows, G, K)


def torch_sample(state, G, K, A):
    noise = torch.randn(G, K, P, A, device=DEV) * SIGMA
    noise[:, 0] = 0
    knots = torch.minimum(torch.maximum(state["nominal"][:, None] + noise, state["lo"]), state["hi"])
    state["knots"] = knots
    acts = torch.einsum("sp,gkpa->sgka", state["basis"], knots)
    return torch.minimum(torch.maximum(acts, state["lo"]), state["hi"]).reshape(S, G * K, A)


def torch_update(state, rows, G, K):
    rew, done = rows[:, :, 75], rows[:, :, 76]
    alive = torch.cat([torch.ones_like(done[:1]), (done[:-1] == 0).float().cumprod(0)], 0)
    R = (state["disc"][:, None] * rew * alive).sum(0).reshape(G, K)
    w = torch.softmax(R / TEMPERATURE, 1)
    return torch.einsum("gk,gkpa->gpa", w, state["knots"])


def torch_state(plant, K, rows_width):
    import numpy as np
    import planner_ref as ref
    idx, w = ref.tap_table(ref.CUBIC, S, P)
    basis = np.zeros((S, P), np.float32)
    for s in range(S):
        for c in range(4):
            basis[s, idx[s, c]] += w[s, c]
    G, A = plant.num_envs, plant.A
    return dict(nominal=torch.zeros(G, P, A, device=DEV), basis=torch.tensor(basis, device=DEV),
                lo=torch.tensor(plant.action_space.low, device=DEV), hi=torch.tensor(plant.action_space.high, device=DEV),
                disc=torch.tensor([GAMMA ** s for s in range(S)], device=DEV), rows=torch.zeros(S, G * K, rows_width, device=DEV))


def closed_loop(sigma, steps=100, G=16, K=256):
    from trex_gym.planner import Planner
    plant = plant_of(G)
    p = Planner(plant, K, S, knots=P, sigma=sigma, temperature=TEMPERATURE, gamma=GAMMA, seed=0)
    total = torch.zeros(G, device=DEV)
    for _ in range(steps):
        total += p.step()[1]
    out = float(total.mean()), float(total.min()), float(total.max())
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--accuracy", default=None, help="a file with the output of pytest -s tests/test_gpu_planner.py")
    ap.add_argument("--parent", default=None, help="a file with the plain step times of the parent commit and this one")
    ap.add_argument("--plain", default=None, metavar="LABEL", help="print the plain step's time under this label and nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r37_planner.txt"))
    args = ap.parse_args()
    if args.plain is not None:
        from observations_bench import make_env as stationary_env
        _, step = stationary_env(4096)
        med, lo_, hi_ = groups_us({"plain": step}, 100, 7)["plain"]
        print("%-30s %8.1f  (%.1f .. %.1f)" % (args.plain, med, lo_, hi_))
        return 0
    from trex_gym.planner import Planner
    lines = ["K21, the sampling-based planner: S = %d, P = %d cubic knots, A = 25, sigma %.2f, temperature %.2f, gamma %.2f (us per call: "
             "median, min .. max of %d groups of %d calls)" % (S, P, SIGMA, TEMPERATURE, GAMMA, args.repeats, args.iters)]
    for G, K in SHAPES:
        lines.append("G = %d, K = %d (N = %d sample envs):" % (G, K, G * K))
        fns, h = launches(G, K)
        for k, (med, lo_, hi_) in groups_us(fns, 5 * args.iters, args.repeats).items():
            lines.append("  %-52s %9.1f  (%.1f .. %.1f)" % (k, med, lo_, hi_))
        h.close()
        eager = Planner(plant_of(G), K, S, knots=P, sigma=SIGMA, temperature=TEMPERATURE, gamma=GAMMA)
        graph = Planner(plant_of(G), K, S, knots=P, sigma=SIGMA, temperature=TEMPERATURE, gamma=GAMMA, use_graphs=True)
        plant = plant_of(G)
        state = torch_state(plant, K, eager.sim.rows.shape[1])
        sim = eager.sim                                              # (the torch plan rolls out on the eager planner's sim env)
        rows = torch.rand(S, G * K, eager.sim.rows.shape[1], device=DEV)

        def torch_ops_alone():
            torch_sample(state, G, K, plant.A)
            state["nominal"] = torch_update(state, rows, G, K)
        fns = {"plan(), eager": eager.plan, "plan(), one graph replay": graph.plan,
               "the same plan from torch ops": lambda: torch_plan(plant, sim, K, state),
               "the planner's launches in plan(): sample + update": None, "the torch ops alone (no rollout, no state copy)": torch_ops_alone}
        acts = eager.actions
        fns["the planner's launches in plan(): sample + update"] = lambda: (eager.handle.sample(acts), eager.handle.update(
            eager._reward, eager._strides[0], eager._strides[1], eager._done, None, GAMMA, TEMPERATURE, eager.returns, eager.weights, eager.best, eager.stats))
        us = groups_us(fns, args.iters, args.repeats, warmup=3)
        for k, (med, lo_, hi_) in us.items():
            lines.append("  %-52s %9.1f  (%.1f .. %.1f)" % (k, med, lo_, hi_))
        a, b = us["the planner's launches in plan(): sample + update"][0], us["the torch ops alone (no rollout, no state copy)"][0]
        lines.append("  around the rollout the device path costs %.1f us against %.1f us of torch ops: %s" % (a, b, "CHEAPER" if a < b else "NOT cheaper"))
        eager.close(), graph.close()
    lines.append("closed loop, 100 control steps, G = 16, K = 256 (the sum of the step's own reward per robot: mean, min .. max; a recorded "
                 "figure - nothing is claimed about control quality):")
    for sigma in (SIGMA, 0.0):
        lines.append("  sigma = %.2f: %10.3f  (%.3f .. %.3f)" % ((sigma,) + closed_loop(sigma)))
    lines += ["resource usage (hipcc -Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if args.parent and os.path.exists(args.parent):
        lines += ["", "the plain step of the parent commit and of this one, alternating processes of one session (us per call: median, "
                  "min .. max):"] + ["  " + ln.rstrip() for ln in open(args.parent) if ln.strip()] + [spread_line(args.parent)]
    if args.accuracy and os.path.exists(args.accuracy):
        found = [re.sub(r"^[.\s]+", "", ln.rstrip()) for ln in open(args.accuracy) if "of the tolerance" in ln or "shares of the tolerances" in ln]
        lines += ["", "accuracy, tests/test_gpu_planner.py (the largest deviation as a share of its tolerance: 4 x the reference's own f32 run "
                  "against its f64 run, for the update + 2 ulp of the largest operand; everything else is bitwise):"]
        lines += ["  " + ln for ln in found]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
