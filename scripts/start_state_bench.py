#!/usr/bin/env python
"""Cost of kernel K20 (start-state randomisation: trex_batch_apply_start_state) on the GPU, against the same effect from the host
path, the apply launch alone at three shares of starting envs, and its resource lines.

Cost at 4 096 envs in ONE process, 32-step episodes with staggered phases (3 % of the envs start at every step), uniform random
actions from a pool, a pre-roll of one episode length, hipEvents around `iters` back-to-back calls after a warm-up, the median
(min .. max) of `repeats` groups, the variants taking turns group by group:
  (a) step_tensor alone: no start-state terms - what the parent commit runs;
  (b) step_tensor with start_state.typical and a clearance term attached: one more launch behind the step call;
  (c) the same effect from the host path around the plain env's step: `where` on done over a torch draw of the joint, velocity and
      attitude noise, set_state, a body_clearance query, and a second set_state that puts the lowest point on the floor;
  (d) the apply launch alone on a done column with 0 %, 3 % and 100 % of the envs starting.
No gate hangs on the timings. Writes profiles/r36_start_state.txt (--out); --accuracy FILE appends the lines
tests/test_gpu_start_state.py printed (pytest -s) that it finds in FILE; --parent FILE the lines of a file that holds the plain step
time of the parent commit and of this one, measured in the same session by alternating processes: each such line is what
`start_state_bench.py --plain LABEL` prints - the plain step on bench.py's stationary mix (1000-step episodes, as
scripts/randomize_bench.py's (a)) of whatever library TREX_LIB names."""
import argparse
import math
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from observations_bench import POOL, groups_us  # noqa: E402
from randomize_bench import spread_line  # noqa: E402

EPISODE = 32
CLEARANCE = (0.0, 0.02)


def resource_lines():
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "start_state.hip")
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


def make_env(n, attach=None):
    """an env on 32-step episodes with staggered phases, a pre-roll of one episode taken; attach(env) before the reset"""
    from trex_gym.vec_env import TrexVecEnv
    v = TrexVecEnv(n, device="cuda:0", max_episode_steps=EPISODE)
    if attach is not None:
        attach(v)
    v.reset_tensor()
    v.set_episode_steps(((torch.arange(n) * EPISODE) // n).to(torch.int32))
    gen = torch.Generator().manual_seed(0)
    lo, hi = torch.tensor(v.model.lower, dtype=torch.float32), torch.tensor(v.model.upper, dtype=torch.float32)
    pool = [(lo + (hi - lo) * torch.rand(n, v.J, generator=gen)).to(v.device) for _ in range(POOL)]
    state = dict(t=0)

    def step():
        v.step_tensor(pool[state["t"] % POOL])
        state["t"] += 1
    for _ in range(EPISODE):
        step()
    torch.cuda.synchronize()
    return v, step, pool


def host_path(v, pool):
    """the effect of the preset with a clearance term from torch ops and the existing calls around the env's own step: it cannot
    patch the row of the new episode, and it synchronises nothing but costs a round of launches per step"""
    n, dev, J, nb = v.num_envs, v.device, v.J, v.model.num_bodies
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: 2.0 * torch.rand(*shape, device=dev, generator=gen) - 1.0
    lo, hi = torch.tensor(v.model.lower, dtype=torch.float32, device=dev), torch.tensor(v.model.upper, dtype=torch.float32, device=dev)
    clear, floor_z = torch.zeros(n, nb, device=dev), float(v.model.get_param("floor_z"))
    state = dict(t=0)

    def step():
        v.step_tensor(pool[state["t"] % POOL])
        state["t"] += 1
        done = v.done[:, None]
        s = v.get_state()
        new = s.clone()
        new[:, 13:13 + J] = torch.minimum(torch.maximum(s[:, 13:13 + J] + 0.1 * rand(n, J), lo), hi)
        new[:, 13 + J:] = s[:, 13 + J:] + 0.5 * rand(n, J)
        half = 0.5 * rand(n, 3) * torch.tensor([0.05, 0.05, math.pi], device=dev)
        (cr, cp, cy), (sr, sp, sy) = torch.cos(half).unbind(1), torch.sin(half).unbind(1)
        r = torch.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], 1)
        ax, ay, az, aw = r.unbind(1)
        bx, by, bz, bw = s[:, 3:7].unbind(1)
        q = torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                         aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], 1)
        new[:, 3:7] = q / q.norm(dim=1, keepdim=True)
        new[:, 7:10] = s[:, 7:10] + rand(n, 3) * torch.tensor([0.3, 0.3, 0.1], device=dev)      # (the rotation of the velocities left out)
        new[:, 10:13] = s[:, 10:13] + 0.3 * rand(n, 3)
        new = torch.where(done, new, s)
        v.set_state(new)
        v.batch.body_clearance(clear, None)
        least = clear.min(dim=1).values
        want = 0.5 * (CLEARANCE[0] + CLEARANCE[1]) + 0.5 * (CLEARANCE[1] - CLEARANCE[0]) * rand(n)
        new[:, 2] = torch.where(done[:, 0], new[:, 2] + (want - least), new[:, 2])
        v.set_state(new)
    return step, floor_z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--accuracy", default=None, help="a file with the output of pytest -s tests/test_gpu_start_state.py")
    ap.add_argument("--parent", default=None, help="a file with the plain step times of the parent commit and this one")
    ap.add_argument("--plain", default=None, metavar="LABEL", help="print the plain step's time under this label and nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r36_start_state.txt"))
    args = ap.parse_args()
    n = args.envs
    if args.plain is not None:
        from observations_bench import make_env as stationary_env
        _, step = stationary_env(n)
        med, lo_, hi_ = groups_us({"plain": step}, args.iters, args.repeats)["plain"]
        print("%-30s %8.1f  (%.1f .. %.1f)" % (args.plain, med, lo_, hi_))
        return 0
    from trex_gym import start_state as S
    spec = S.typical(None, clearance=CLEARANCE)
    plain, step_plain, _ = make_env(n)
    native, step_native, _ = make_env(n, lambda v: S.attach(v, spec, seed=0))
    eager, _, pool = make_env(n)
    step_host, _ = host_path(eager, pool)
    names = ("step_tensor alone", "step + K20 (typical + clearance)", "step + the same from the host path")
    fns = dict(zip(names, (step_plain, step_native, step_host)))
    # the apply launch alone: its own batch, so that the envs above keep their episodes
    alone, _, _ = make_env(n, lambda v: S.attach(v, spec, seed=1))
    for share in (0.0, 1.0 / EPISODE, 1.0):
        done = (torch.arange(n, device=alone.device) < round(share * n)).float()
        done = done[torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(alone.device)].contiguous()
        fns["apply alone, %3.0f %% of the envs starting" % (100 * share)] = (lambda d: lambda: alone.start_api.apply(d, alone.rows))(done)
    us = groups_us(fns, args.iters, args.repeats)
    lines = ["K20, start-state randomisation: cost at %d envs, %d-step episodes, staggered, 77-column rows (us per call: median, "
             "min .. max of %d groups of %d calls)" % (n, EPISODE, args.repeats, args.iters)]
    base = us[names[0]][0]
    for k, (med, lo_, hi_) in us.items():
        lines.append("  %-44s %8.1f  (%.1f .. %.1f)%s" % (k, med, lo_, hi_, "   %+.1f" % (med - base) if k in names[1:] else ""))
    a, b = us[names[1]][0] - base, us[names[2]][0] - base
    lines.append("  the device path is %s than the host path: %+.1f us against %+.1f us per step" % ("CHEAPER" if a < b else "NOT cheaper", a, b))
    lines.append("  (the host path leaves the row of the new episode unpatched and the velocities unrotated: it does less)")
    kinds = [S.KIND_NAMES[t[0]] for t in native.start_state["terms"]]
    lines += ["terms: %d (%s)" % (len(kinds), ", ".join(kinds)),
              "resource usage (hipcc -Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if args.parent and os.path.exists(args.parent):
        lines += ["", "the plain step of the parent commit and of this one, alternating processes of one session (us per call: median, "
                  "min .. max):"] + ["  " + ln.rstrip() for ln in open(args.parent) if ln.strip()] + [spread_line(args.parent)]
    if args.accuracy and os.path.exists(args.accuracy):
        found = [ln.rstrip() for ln in open(args.accuracy) if "largest used fraction of the bounds" in ln]
        lines += ["", "accuracy, tests/test_gpu_start_state.py (the largest deviation of each bounded quantity as a fraction of its bound: 4 x the "
                  "reference's own f32 run against its f64 run, floored at 2 ulp of the scale; draws, q, qd and offsets are bitwise):"]
        lines += ["  " + ln.lstrip(". ") for ln in found]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
