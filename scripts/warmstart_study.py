"""PGS warm start (model parameter `warmstart`): accuracy against sweeps and speed of the step launch, cold against warm.

Accuracy: the 50 landing / rest states of tests/test_gpu_parity.py::test_one_step_parity_in_contact_and_at_rest. For each, the
batch starts from the oracle's state one env-step earlier and takes that step (which populates the warm-start record), then one
more env-step from where it is; the error of that step's qd block is measured against the f64 oracle at 6000 sweeps from the
same state. Cold and warm (0.85, 1.0) at iterations 15 / 30 / 60 / 120: median and max per cell.
Speed: env-steps/s through trex_batch_time_steps at 4096 envs (pair launch) and 4097 (single-env launch), after a 50-step
landing under random actions, for cold/60, warm/60, warm/30, warm/15.

  python scripts/warmstart_study.py [--out DIR] [--quick]      (needs the GPU; --out DIR also writes DIR/warmstart_study.json)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "trex-gym_amd")]
from oracle import oracle as O, trex_model as tm      # noqa: E402
from trex_gym.vec_env import TrexVecEnv               # noqa: E402

J = 25
DEV = "cuda:0"


def landing(model):
    orc = O.Oracle(model, precision="f64")
    q0 = model["q_start"][model["obs_order"]]
    lo, hi = model["q_lower"][model["obs_order"]], model["q_upper"][model["obs_order"]]
    rng = np.random.default_rng(5)
    s = orc.new_state()
    orc.reset(s)
    prev, a_prev, nxt = [], [], []
    for t in range(300):
        a = np.clip(q0 + 0.15 * rng.normal(size=25), lo, hi)
        before = orc.get_state(s).astype(np.float32)
        orc.step(s, a)
        if t % 6 == 0:
            prev.append(before)
            a_prev.append(a.astype(np.float32))
            nxt.append(np.clip(q0 + 0.15 * rng.normal(size=25), lo, hi).astype(np.float32))
    return np.array(prev), np.array(a_prev), np.array(nxt)


def accuracy(model, iters_list, warms):
    prev, a_prev, nxt = landing(model)
    ref = O.Oracle(model, params=dict(iterations=6000), precision="f64")
    n = len(prev)
    cells = {}
    for it in iters_list:
        for w in warms:
            v = TrexVecEnv(n, device=DEV, params=dict(iterations=it, **({"warmstart": w} if w else {})))
            v.reset()
            v.set_state(torch.tensor(prev))
            v.step_tensor(torch.tensor(a_prev, device=DEV))      # populates the record (warm)
            G = v.get_state().cpu().numpy()
            v.step_tensor(torch.tensor(nxt, device=DEV))
            g = v.obs.cpu().numpy()
            errs, rel = [], []
            for e in range(n):
                s = ref.new_state()
                ref.set_state(s, G[e].astype(np.float64))
                o, _, _ = ref.step(s, nxt[e].astype(np.float64))
                err = np.abs(g[e, J:2 * J].astype(np.float64) - o[J:2 * J]).max()
                errs.append(err)
                rel.append(err / max(1.0, np.abs(o[J:2 * J]).max()))
            v.close()
            cells[(it, w)] = (np.array(errs), np.array(rel))
            print("iterations %4d  warm %-4s  qd err median %.3e  max %.3e  (rel. to max(1,|qd|): median %.3e max %.3e)"
                  % (it, w or "cold", np.median(errs), np.max(errs), np.median(rel), np.max(rel)), flush=True)
    return cells


def speed(n, it, w, steps):
    v = TrexVecEnv(n, device=DEV, params=dict(iterations=it, **({"warmstart": w} if w else {})))
    v.reset_tensor()
    lo = torch.tensor(v.model.lower, dtype=torch.float32, device=DEV)
    hi = torch.tensor(v.model.upper, dtype=torch.float32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(50):
        v.step_tensor(lo + (hi - lo) * torch.rand(n, J, device=DEV, generator=g))
    a = (lo + (hi - lo) * torch.rand(n, J, device=DEV, generator=g)).contiguous()
    obs = torch.zeros(n, 3 * J, device=DEV)
    rew = torch.zeros(n, device=DEV)
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    v.batch.time_steps(a, obs, rew, done, 20)       # warm-up of the timed shape
    ms = v.batch.time_steps(a, obs, rew, done, steps)
    info = v.batch.launch_info()
    v.close()
    return n / (ms * 1e-3), ms, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for warmstart_study.json (the tables are printed either way)")
    ap.add_argument("--quick", action="store_true", help="fewer timed steps")
    ap.add_argument("--skip-accuracy", action="store_true")
    args = ap.parse_args()
    model = tm.compile_model(O.default_asset_urdf())
    res = {"accuracy": [], "speed": []}
    if not args.skip_accuracy:
        for (it, w), (errs, rel) in accuracy(model, [15, 30, 60, 120], [None, 0.85, 1.0]).items():
            res["accuracy"].append(dict(iterations=it, warmstart=w or 0.0, median=float(np.median(errs)), max=float(np.max(errs)),
                                        rel_median=float(np.median(rel)), rel_max=float(np.max(rel)), errs=errs.tolist()))
    steps = 100 if args.quick else 300
    for n in (4096, 4097):
        for it, w in ((60, None), (60, 0.85), (30, 0.85), (15, 0.85)):
            rate, ms, info = speed(n, it, w, steps)
            res["speed"].append(dict(envs=n, iterations=it, warmstart=w or 0.0, env_steps_per_s=rate, ms_per_launch=ms,
                                     launch=info))
            print("envs %d  iterations %3d  warm %-4s  %.3f M env-steps/s  (%.4f ms per launch, %s)"
                  % (n, it, w or "cold", rate / 1e6, ms, info), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "warmstart_study.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
