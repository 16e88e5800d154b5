#!/usr/bin/env python3
"""Times trex_batch_render (include/trex_batch.h) with hipEvents on 4 096 envs after a 50-step landing (zero action): one
960 x 720 view, 4 096 views at 64 x 64 and at 84 x 84, each rgb only and rgb + depth + seg; next to one step launch.
Prints one line per case (us per call, M rays/s) and a JSON summary. Standalone: bench.py is not involved.

    python scripts/render_bench.py [--envs 4096] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "trex-gym_amd"))

import torch  # noqa: E402

from trex_gym import _capi  # noqa: E402
from trex_gym.render import Camera  # noqa: E402
from trex_gym.vec_env import TrexVecEnv  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n = args.envs
    env = TrexVecEnv(n, device="cuda:0")
    env.reset_tensor()
    zero = torch.zeros(n, env.J, device=env.device)
    for _ in range(50):
        env.step_tensor(zero)
    torch.cuda.synchronize()
    step_us = timed(lambda: env.step_tensor(zero), args.reps)
    cam = Camera()
    out = {"envs": n, "build_id": _capi.build_id(), "step_launch_us": round(step_us, 1), "cases": []}
    print("step launch: %.1f us" % step_us)
    for views, W, H in ((1, 960, 720), (n, 64, 64), (n, 84, 84)):
        ids = [0] if views == 1 else None
        rgb = torch.empty(views, H, W, 3, dtype=torch.uint8, device=env.device)
        dep = torch.empty(views, H, W, device=env.device)
        seg = torch.empty(views, H, W, dtype=torch.int32, device=env.device)
        for outputs in ("rgb", "rgb+depth+seg"):
            full = outputs != "rgb"
            us = timed(lambda: env.batch.render(cam, W, H, ids, rgb, dep if full else None, seg if full else None), args.reps)
            rays = views * W * H
            row = {"views": views, "width": W, "height": H, "outputs": outputs, "us_per_call": round(us, 1),
                   "mrays_per_s": round(rays / us, 1), "step_launches": round(us / step_us, 2)}
            out["cases"].append(row)
            print("%5d x %4d x %4d  %-14s %9.1f us  %8.1f M rays/s  %.2f step launches" % (views, W, H, outputs, us, rays / us,
                                                                                           us / step_us))
    # phase split: the same 4 096 x 64 x 64 launch with the camera turned to the sky (no primitive survives the tile cull):
    # what remains is the per-workgroup pose pass, the cull and the writes; the difference is the rays' hull loop
    rgb = torch.empty(n, 64, 64, 3, dtype=torch.uint8, device=env.device)
    sky = Camera(pitch=40.0)
    us_sky = timed(lambda: env.batch.render(sky, 64, 64, None, rgb), args.reps)
    us_64 = timed(lambda: env.batch.render(cam, 64, 64, None, rgb), args.reps)
    out["phase_split_64x64"] = {"sky_only_us": round(us_sky, 1), "scene_us": round(us_64, 1)}
    print("4096 x 64 x 64 rgb: sky-only camera %.1f us (pose pass + cull + writes), scene %.1f us (repeated)" % (us_sky, us_64))
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
