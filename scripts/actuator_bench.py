#!/usr/bin/env python3
"""Cost of the actuator model (trex_batch_set_control_mode / _set_motor_gains / _set_stiffness_actions): env-steps/s of
trex_batch_time_steps at 4 096 envs (pair form) and 32 768 for five configurations - default (the kernels without ACT), gains
set (to the model parameters: bitwise the default's trajectories, so the difference is the ACT kernels' own cost),
all-VELOCITY (target 0), all-TORQUE (torque 0) and stiffness actions (kp 5e-3) - against the PARENT commit's library on its
default configuration, A/B interleaved: the driver starts one fresh worker process per run, parent and this build in turn,
each worker times its configurations alternating after a 50-step landing and a warm-up sample. The velocity / torque
configurations move differently from the default (other contact counts), so their figures are the cost of that workload,
not of the kernel alone. Writes the table to --out (appended to profiles/r10_actuators.txt by hand).

Build the parent's library from the same tree first, e.g.
    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/trex-gym_amd/csrc && \\
        cp /tmp/parent/trex-gym_amd/trex_gym/libtrex_hip.so trex-gym_amd/trex_gym/libtrex_hip_parent.so
    python scripts/actuator_bench.py [--parent-lib PATH] [--sizes 4096,32768] [--runs 3] [--steps 20] [--reps 9]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "trex-gym_amd"))
CONFIGS = ("default", "gains", "velocity", "torque", "stiffness")


def worker(args):
    import torch
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    has_act = hasattr(_capi.lib, "trex_batch_set_control_mode") and not args.default_only
    configs = CONFIGS if has_act else ("default",)
    out = {"build": _capi.build_id(), "ms": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        envs = {}
        for c in configs:
            kw = {}
            if c in ("velocity", "torque"):
                kw["control_mode"] = c
            if c == "stiffness":
                kw["variable_stiffness"] = True
            v = TrexVecEnv(n, device="cuda:0", **kw)
            v.reset_tensor()
            J = v.J
            a = torch.tensor(v.model.array("q_start")[v.model.array("obs_order").astype(int)], dtype=torch.float32,
                             device=v.device).repeat(n, 1)
            if c in ("velocity", "torque"):
                a = torch.zeros(n, J, device=v.device)
            if c == "stiffness":
                a = torch.cat([a, torch.full((n, J), 5e-3, device=v.device)], 1).contiguous()
            if c == "gains":
                v.set_motor_gains(kp=5e-3, kd=0.1, max_force=3e5)
            for _ in range(50):
                v.step_tensor(a)
            envs[c] = (v, (a, torch.zeros(n, 3 * J, device=v.device), torch.zeros(n, device=v.device),
                           torch.zeros(n, dtype=torch.uint8, device=v.device)))
        t = {c: [] for c in configs}
        for r in range(args.reps + 1):
            for c in configs:
                v, bufs = envs[c]
                ms = v.batch.time_steps(*bufs, args.steps)
                if r:
                    t[c].append(ms)
        for c in configs:
            out["ms"]["%d/%s" % (n, c)] = statistics.median(t[c])
            envs[c][0].close()
        del envs
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,32768")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "trex-gym_amd", "trex_gym", "libtrex_hip_parent.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_actuators_cost.txt"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--default-only", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not os.path.exists(args.parent_lib):
        sys.exit("parent library not found: %s (see the header of this script)" % args.parent_lib)
    runs = {"parent": [], "this": []}
    for r in range(args.runs):
        for who in ("parent", "this"):
            env = dict(os.environ)
            if who == "parent":
                env["TREX_LIB"] = args.parent_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--sizes", args.sizes, "--steps", str(args.steps),
                                "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("worker (%s) failed with %d:\n%s" % (who, p.returncode, p.stderr[-2000:]))
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs[who].append(res)
            print(who, r, res, flush=True)
    lines = ["scripts/actuator_bench.py on one MI355X: parent library build %s, this build %s; %d runs each (fresh processes, "
             "parent and this build in turn), per run the median of %d samples of %d launches per configuration."
             % (runs["parent"][0]["build"], runs["this"][0]["build"], args.runs, args.reps, args.steps), "",
             "%-7s %-16s %12s %12s %12s %10s" % ("envs", "configuration", "M steps/s", "min", "max", "vs parent")]
    for n in (int(s) for s in args.sizes.split(",")):
        def rate(who, c):
            return [n / (r["ms"]["%d/%s" % (n, c)] * 1e3) for r in runs[who]]     # M env-steps/s
        pr = rate("parent", "default")
        pm = statistics.median(pr)
        lines.append("%-7d %-16s %12.3f %12.3f %12.3f %10s   spread of the parent's runs %.2f %%"
                     % (n, "parent default", pm, min(pr), max(pr), "", 100 * (max(pr) - min(pr)) / pm))
        for c in CONFIGS:
            x = rate("this", c)
            lines.append("%-7d %-16s %12.3f %12.3f %12.3f %+9.2f%%" % (n, c, statistics.median(x), min(x), max(x),
                                                                        100 * (statistics.median(x) / pm - 1)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
