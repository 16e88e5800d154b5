#!/usr/bin/env python3
"""Times trex_batch_ray_test (include/trex_batch.h) with hipEvents on 4 096 envs after a 50-step landing (zero action), as
scripts/render_bench.py does: R = 4 downward rays from a foot link, a shared R = 64 fan on the head link, R = 1 024 per-env
world segments - each with every body and the floor, with body_mask = 0 (floor only), and in primitive-collision mode - next
to one step launch and to trex_batch_render of 4 096 views at 8 x 8, depth only (the other way to 64 distances per env).
Prints one line per case (us per call, M rays/s) and a JSON summary. Standalone: bench.py is not involved.

    python scripts/ray_test_bench.py [--envs 4096] [--reps 20]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "trex-gym_amd"))

import torch  # noqa: E402

from trex_gym import _capi, sensors  # noqa: E402
from trex_gym.render import Camera  # noqa: E402
from trex_gym.vec_env import TrexVecEnv  # noqa: E402

FOOT, HEAD = "link_tarsometatarsus_right", "link_cranium"


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
    out = {"envs": n, "build_id": _capi.build_id(), "cases": []}
    for collision in ("hulls", "primitives"):
        env = TrexVecEnv(n, device="cuda:0", collision=collision)
        env.reset_tensor()
        zero = torch.zeros(n, env.J, device=env.device)
        for _ in range(50):
            env.step_tensor(zero)
        torch.cuda.synchronize()
        step_us = timed(lambda: env.step_tensor(zero), args.reps)
        print("%s: step launch %.1f us" % (collision, step_us))
        out["step_launch_us_" + collision] = round(step_us, 1)
        base = env.get_state()[:, :3]
        g = torch.Generator().manual_seed(0)
        lo, hi = torch.tensor([-3.0, -3.0, 0.05]), torch.tensor([3.0, 3.0, 4.0])
        ends = lo + (hi - lo) * torch.rand(n, 1024, 2, 3, generator=g)
        world = (ends.to(env.device) + (base * torch.tensor([1.0, 1.0, 0.0], device=env.device)).view(n, 1, 1, 3)).reshape(n, 1024, 6)
        patterns = (("R=4 foot, down", FOOT, sensors.grid_down((-0.1, 0.1), (-0.1, 0.1), 2, 2, top=0.3, length=2.0)),
                    ("R=64 head fan, shared", HEAD, sensors.fan((0, 0, 0), (-math.pi / 2, math.pi / 2), (-1.0, 0.3), 16, 4, 6.0)),
                    ("R=1024 per-env, world", None, world.contiguous()))
        for name, link, rays in patterns:
            for what, bodies in (("all bodies + floor", None), ("floor only", [])):
                fn = lambda: env.ray_test(rays, link, bodies=bodies)   # noqa: E731
                frac, body = fn()
                us = timed(fn, args.reps)
                count = n * int(rays.shape[-2])
                row = {"collision": collision, "case": name, "mask": what, "us_per_call": round(us, 1), "mrays_per_s": round(count / us, 1),
                       "hit_share": round(float((body != -2).float().mean()), 3), "step_launches": round(us / step_us, 3)}
                out["cases"].append(row)
                print("%-10s %-24s %-18s %9.1f us  %9.1f M rays/s  hits %.3f  %.3f step launches" %
                      (collision, name, what, us, count / us, row["hit_share"], us / step_us))
        if collision == "hulls":   # 64 distances per env the other way: a depth image through a camera that follows the base
            dep = torch.empty(n, 8, 8, device=env.device)
            us = timed(lambda: env.batch.render(Camera(), 8, 8, None, None, dep, None), args.reps)
            out["render_8x8_depth_us"] = round(us, 1)
            print("trex_batch_render %d x 8 x 8, depth only: %.1f us  %.1f M rays/s" % (n, us, n * 64 / us))
        env.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
