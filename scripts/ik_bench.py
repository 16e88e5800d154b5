#!/usr/bin/env python
"""Accuracy and cost of the inverse kinematics query (trex_batch_inverse_kinematics) on the GPU.

Deviations: the figures the tolerances of tests/test_gpu_inverse_kinematics.py (MEASURED) are set from - q after one iteration
against tests/ik_ref.py, the residuals of `info` against the f64 evaluation of q_out, the final error norm of the unreachable
cases against the reference's, and one iteration on the generated models.

Cost at 256, 4 096 and 32 768 envs, us per call, for K = 2 position targets with 10 iterations and K = 4, M = 18 (two of the four
with their orientation) with 30: hipEvents around `iters` back-to-back launches after a warm-up, the median (min .. max) of
`repeats` such groups. Beside it the same solve composed from what the batch offered before - per iteration K jacobian() launches,
one link_state() launch and a torch.linalg.solve of the damped normal equations; jacobian() evaluates at the env's CURRENT state
only, so that loop is the real thing for its first iteration and repeats that iteration's work for the others (it cannot move
the iterate): its time is what such a solver would cost at least, its answer is not a solve - and one plain step launch, for
scale. Writes profiles/r20_inverse_kinematics.txt (--out). No gate hangs on the timings."""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def time_us(fn, iters, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def composed_solver(v, probes, modes, target, iterations, damping=0.01, gain=0.1):
    """the torch loop a user of the earlier API would write (module docstring)"""
    n, J, K = v.num_envs, v.J, len(probes.links)
    Jb = torch.empty(K, n, 6, 6 + J, device=v.device)
    rows = [r for k, m in enumerate(modes) for r in ([(k, 0)] if m & 1 else []) + ([(k, 3)] if m & 2 else [])]
    eye = torch.eye(3 * len(rows), device=v.device)

    def run():
        q = None
        for _ in range(iterations):
            for k in range(K):
                v.batch.jacobian(probes.links[k], probes.positions[k], Jb[k])
            s = v.link_state(probes, velocity=False)
            A = torch.cat([Jb[k][:, r:r + 3, 6:] for k, r in rows], 1)
            e = torch.cat([(target[:, k, :3] - s.position[:, k]) if r == 0 else
                           2 * (target[:, k, 3:6] * s.orientation[:, k, 3:] - s.orientation[:, k, :3] * target[:, k, 6:]) for k, r in rows], 1)
            lam = damping * damping + gain * (e * e).sum(1)
            x = torch.linalg.solve(A @ A.transpose(1, 2) + lam[:, None, None] * eye, e.unsqueeze(-1))
            q = (A.transpose(1, 2) @ x).squeeze(-1).clamp_(-0.2, 0.2)
        return q
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_inverse_kinematics.txt"))
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 4096, 32768])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-deviations", action="store_true")
    args = ap.parse_args()
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    lines = ["inverse kinematics (trex_batch_inverse_kinematics): deviation from the f64 reference and cost per call",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), ""]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not args.no_deviations:
        import ik_cases as IC
        import synthetic_models as sm
        import test_gpu_inverse_kinematics as T       # (for its deviations alone)
        from conftest import ASSET_URDF
        from gpu_support import case_env
        from oracle import trex_model
        model = trex_model.compile_model(ASSET_URDF)
        say("largest deviations on the cases of tests/ik_cases.py (tests/test_gpu_inverse_kinematics.py: MEASURED):")
        d = T.deviations(model)
        say("  one iteration, damping 0.05, N = 67, every form / frame / q_init / mask: |q - q_ref|      %.3g rad" % d["one_iter"])
        say("  30 iterations: info's residuals against the f64 evaluation of q_out                     %.3g m / rad" % d["info"])
        say("  unreachable targets, 30 iterations: |e| against the reference's, relative               %.3g" % d["unreachable"])
        with tempfile.TemporaryDirectory() as tmp:
            for name in ("deep_chain", "bushy"):
                path, props, om = sm.compile_both(name, os.path.join(tmp, name))
                make = lambda cs, q=None: case_env(om, cs, q, path, props["params"])
                w = max(T.one_iteration_deviation(om, IC.form_of(om, f), 3, name, make) for f in ("pos4", "head_ori", "same_body", "one_leg"))
                say("  %-10s N = 3, one iteration: |q - q_ref|                                           %.3g rad" % (name, w))
        say("")
        flush()

    say("timing: hipEvents around %d back-to-back calls, warm-up 5, median (min .. max) of %d groups, us per call"
        % (args.iters, args.repeats))
    for n in args.envs:
        v = TrexVecEnv(n, device="cuda:0")
        v.reset_tensor()
        names = [nm for nm, _ in v.model.links()]
        toes = [i for i, nm in enumerate(names) if "toe_01_a" in nm][:2]
        head = [i for i, nm in enumerate(names) if "atlas" in nm][:1] or [1]
        deep = [i for i, nm in enumerate(names) if "toe_02_b" in nm][:1] or [2]
        act = torch.zeros(n, v.A, device=v.device)
        med, lo_, hi_ = time_us(lambda: v.step_tensor(act), args.iters, args.repeats)
        say("  N = %-6d %-58s %9.1f   (%.1f .. %.1f)" % (n, "one step launch (for scale)", med, lo_, hi_))
        for label, links, modes, its in (("K = 2 positions, 10 iterations", toes, [1, 1], 10),
                                         ("K = 4, M = 18, 30 iterations", head + toes + deep, [3, 1, 3, 1], 30)):
            h = v.link_probes(links)
            s = v.link_state(h, velocity=False)
            target = torch.cat([s.position + 0.05, s.orientation], -1).contiguous()
            q, info = torch.empty(n, v.J, device=v.device), torch.empty(n, 4, device=v.device)
            fn = lambda: v.batch.inverse_kinematics(h.slot, modes, target, q, 0, None, None, info, iterations=its)
            one = time_us(fn, args.iters, args.repeats)
            say("  N = %-6d %-58s %9.1f   (%.1f .. %.1f)" % (n, "inverse_kinematics, " + label, *one))
            many = time_us(composed_solver(v, h, modes, target, its), max(1, args.iters // 5), args.repeats, warmup=2)
            say("  N = %-6d %-58s %9.1f   (%.1f .. %.1f)" % (n, "composed torch loop, " + label, *many))
            say("  N = %-6d   the single launch takes %.3g of the composed loop's time (%s)" % (
                n, one[0] / many[0], "faster" if one[0] < many[0] else "NOT faster"))
            h.close()
            flush()
        v.close()
    flush()


if __name__ == "__main__":
    main()
