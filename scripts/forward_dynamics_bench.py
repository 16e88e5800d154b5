#!/usr/bin/env python
"""Cost and accuracy of trex_batch_forward_dynamics / trex_batch_solve_mass on the GPU: the largest deviations from the f64
references on the states of tests/test_gpu_forward_dynamics.py at N = 67 - the figures its tolerances are set from - and on the
two generated models; us per launch of both calls (K = 1, 6, 31) at 4 096 envs next to what they replace, mass_matrix() +
torch.linalg.solve for the same answers (timed as scripts/dynamics_bench.py does). Writes profiles/r13_forward_dynamics.txt
(--out). No gate hangs on the timings."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from dynamics_bench import time_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_forward_dynamics.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--envs", type=int, default=4096)
    args = ap.parse_args()
    import test_forward_dynamics_ref as TR        # (for oracle32_deviation alone)
    import test_gpu_forward_dynamics as T         # (for its deviations alone)
    from conftest import ASSET_URDF
    from oracle import oracle as O, trex_model
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    model = trex_model.compile_model(ASSET_URDF)
    o64, o32 = O.Oracle(model, precision="f64"), O.Oracle(model, precision="f32")
    lines = ["forward dynamics and mass-matrix solves: deviation from the f64 references and cost per launch",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), "",
             "largest deviation (metrics: docstring of tests/test_gpu_forward_dynamics.py):"]
    for n in (1, 67):
        d = T.deviations(o64, model, n)
        lines.append("  N = %-3d " % n + "  ".join("%s %.3g" % kv for kv in sorted(d.items())))
        print(lines[-1], flush=True)
    from state_sets import landing_states
    ls, _ = landing_states(o64, model)
    import numpy as np
    import dynamics_ref as R
    cases = [(s.astype(np.float64), None) for s in ls] + list(zip(*R.random_states(model, 8)))
    acc, mi = TR.oracle32_deviation(cases, o64, o32, model)
    lines.append("  the f32 build of the CPU oracle against its f64 build, base states: fd_accel %.3g  minv %.3g" % (acc, mi))
    print(lines[-1], flush=True)
    for name in ("deep_chain", "bushy"):
        with tempfile.TemporaryDirectory() as tmp:
            from pathlib import Path
            d = T.other_tree_deviations(name, Path(tmp))
        lines.append("  %-10s " % name + "  ".join("%s %.3g" % kv for kv in sorted(d.items())))
        print(lines[-1], flush=True)
    n = args.envs
    lines += ["", "timing: hipEvents around %d back-to-back launches, warm-up 20, median (min .. max) of %d groups, us per launch, %d envs"
              % (args.iters, args.repeats, n), "%-44s %10s" % ("launch", "us")]
    v = TrexVecEnv(n, device="cuda:0")
    v.reset_tensor()
    b, D = v.batch, 6 + v.J
    f = torch.randn(n, D, device=v.device)
    rhs = {k: torch.randn(n, k, D, device=v.device) for k in (1, 6, 31, 64)}
    out = {k: torch.empty(n, k, D, device=v.device) for k in (1, 6, 31, 64)}
    fo, M = torch.empty(n, D, device=v.device), torch.empty(n, D, D, device=v.device)
    runs = [("forward_dynamics", lambda: b.forward_dynamics(f, fo)),
            ("inverse_dynamics (for scale)", lambda: b.inverse_dynamics(f, fo)),
            ("mass_matrix (for scale)", lambda: b.mass_matrix(M))]
    runs += [("solve_mass K = %d" % k, lambda k=k: b.solve_mass(rhs[k], out[k])) for k in (1, 6, 31, 64)]
    runs += [("solve_mass NULL (M^-1, K = 31)", lambda: b.solve_mass(None, out[31]))]
    runs += [("mass_matrix + torch.linalg.solve K = %d" % k,
              lambda k=k: torch.linalg.solve(b.mass_matrix(M), rhs[k].transpose(1, 2))) for k in (1, 6, 31)]
    for name, fn in runs:
        med, lo, hi = time_us(fn, args.iters, args.repeats)
        lines.append("%-44s %10.1f   (%.1f .. %.1f)" % (name, med, lo, hi))
        print(lines[-1], flush=True)
    v.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
