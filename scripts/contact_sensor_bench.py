#!/usr/bin/env python3
"""Cost of the contact sensor (trex_batch_set_contact_sensor): times trex_batch_time_steps at 4 096 envs (pair form),
4 097 (single-env form) and 32 768 with the sensor off (the default kernels) and on (the SENS kernels), each cold and with
warm start 0.85 - one batch per configuration, the configurations alternating in one process after a 50-step landing and a
warm-up, minimum and median over the repeats. Writes profiles/r08_contact_sensor.txt with the kernels' resource usage
(make resource-usage) appended. Standalone: bench.py is not involved.

    python scripts/contact_sensor_bench.py [--sizes 4096,4097,32768] [--steps 20] [--reps 15] [--no-resources]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "trex-gym_amd"))

import torch  # noqa: E402

from trex_gym import _capi  # noqa: E402
from trex_gym.vec_env import TrexVecEnv  # noqa: E402

CONFIGS = ("off", "on", "warm_off", "warm_on")


def make(n, cfg):
    v = TrexVecEnv(n, device="cuda:0", params={"warmstart": 0.85} if cfg.startswith("warm") else None)
    v.reset_tensor()
    a = torch.tensor(v.model.array("q_start")[v.model.array("obs_order").astype(int)], dtype=torch.float32,
                     device=v.device).repeat(n, 1)
    if cfg.endswith("_on") or cfg == "on":
        v.enable_contact_sensor()
    for _ in range(50):
        v.step_tensor(a)
    bufs = (a, torch.zeros(n, 3 * v.J, device=v.device), torch.zeros(n, device=v.device),
            torch.zeros(n, dtype=torch.uint8, device=v.device))
    return v, bufs


def resource_lines():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "trex-gym_amd", "csrc"), "resource-usage"], capture_output=True,
                         text=True, timeout=900).stderr
    rows, name = [], None
    keep = ("VGPRs:", "TotalSGPRs:", "SGPRs Spill:", "VGPRs Spill:", "ScratchSize", "Occupancy", "LDS Size")
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            if ("step" in name or "reset" in name) and "Kernel" in name:
                rows.append([name])
            continue
        if rows and rows[-1][0] == name and any(k in line for k in keep):
            rows[-1].append(re.sub(r"\s*\[-Rpass.*", "", line.split("remark:")[1]).strip())
    return ["%s  %s" % (r[0], "; ".join(r[1:])) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,4097,32768")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_contact_sensor.txt"))
    args = ap.parse_args()
    lines = ["trex_batch_time_steps on one MI355X, kernel build %s, scripts/contact_sensor_bench.py: %d launches per sample, %d"
             " samples per configuration, the four configurations alternating; 50-step landing (start-pose targets) + 1 warm-up"
             " sample first. ms per launch; 'vs off' against the sensor-off batch of the same warm start." % (_capi.build_id(),
                                                                                                   args.steps, args.reps), "",
             "%-7s %-9s %10s %10s %10s" % ("envs", "config", "min", "median", "vs off")]
    for n in (int(s) for s in args.sizes.split(",")):
        envs = {c: make(n, c) for c in CONFIGS}
        form = "pair" if envs["off"][0].batch.launch_info()["block"] == 128 else "single"
        t = {c: [] for c in CONFIGS}
        for r in range(args.reps + 1):
            for c in CONFIGS:
                v, bufs = envs[c]
                ms = v.batch.time_steps(*bufs, args.steps)
                if r:
                    t[c].append(ms)
        for c in CONFIGS:
            base = statistics.median(t["warm_off" if c.startswith("warm") else "off"])
            med = statistics.median(t[c])
            lines.append("%-7s %-9s %10.4f %10.4f %+9.2f%%   (%s form)" % (n, c, min(t[c]), med, 100 * (med / base - 1), form))
            print(lines[-1], flush=True)
        for c in CONFIGS:
            envs[c][0].close()
        del envs
        torch.cuda.empty_cache()
    if not args.no_resources:
        lines += ["", "make resource-usage (step kernels; *_sens_* = with the contact sensor):"] + resource_lines()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-20:]))


if __name__ == "__main__":
    main()
