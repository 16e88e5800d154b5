#!/usr/bin/env python
"""Accuracy and cost of the link kinematics query (trex_batch_link_state) on the GPU.

Deviations: the largest deviations from the f64 reference tests/link_state_ref.py on the states of tests/test_gpu_link_state.py at
N = 67 and on its generated models - the figures its tolerances (MEASURED) are set from.

Cost at 4 096 envs: us per call for K = 1, 4, 133 and 1 024 probes, pose only and all three outputs - hipEvents around `iters`
back-to-back launches after a warm-up, the median (min .. max) of `repeats` such groups - next to what the batch offered for the
same answer before: link_transforms() for poses (all 133 link frames, whatever K), and K jacobian() launches plus a batched
matrix-vector product for velocities, as torch.matmul and as a multiply and a row sum (K = 1 and 4 only: nobody would launch
133 of them). Writes profiles/r17_link_state.txt
(--out). No gate hangs on the timings."""
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


def time_us(fn, iters, repeats, warmup=20):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_link_state.txt"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-deviations", action="store_true")
    args = ap.parse_args()
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    lines = ["link kinematics (trex_batch_link_state): deviation from the f64 reference and cost per call",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), ""]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    if not args.no_deviations:
        import synthetic_models as sm
        import test_gpu_link_state as T
        from conftest import ASSET_URDF
        from oracle import oracle as O, trex_model
        model = trex_model.compile_model(ASSET_URDF)
        o64 = O.Oracle(model, precision="f64")
        say("largest deviation from the f64 reference (tests/link_state_ref.py), scales as in tests/test_gpu_link_state.py:")
        for n in (1, 67):
            d = T.deviations(o64, model, n)
            say("  N = %-3d " % n + "  ".join("%s %.3g" % (k, d[k]) for k in ("pose", "velocity", "bias", "accel")))
        with tempfile.TemporaryDirectory() as tmp:
            for name in T.MEASURED_SYN:
                path, props, om = sm.compile_both(name, os.path.join(tmp, name))
                w = T.synthetic_deviation(dict(path=path, props=props, om=om))
                say("  %-10s N = 3  " % name + "  ".join("%s %.3g" % (k, w[k]) for k in ("pose", "velocity", "acc")))
        say("")

    n = args.envs
    say("timing at %d envs: hipEvents around %d back-to-back launches, warm-up 20, median (min .. max) of %d groups, us per call"
        % (n, args.iters, args.repeats))
    v = TrexVecEnv(n, device="cuda:0")
    v.reset_tensor()
    gen = torch.Generator().manual_seed(0)
    lo, hi = torch.tensor(v.model.lower, dtype=torch.float32), torch.tensor(v.model.upper, dtype=torch.float32)
    for _ in range(5):       # (a moving state: velocities are not zero)
        v.step_tensor((lo + (hi - lo) * torch.rand(n, v.J, generator=gen)).to(v.device))
    b, dev, D = v.batch, v.device, 6 + v.J
    nl = len(v.model.links())
    acc = torch.zeros(n, D, device=dev)
    lt = torch.empty(n, nl, 7, device=dev)
    med, lo_, hi_ = time_us(lambda: b.link_transforms(lt), args.iters, args.repeats)
    say("  %-46s %8.1f   (%.1f .. %.1f)" % ("link_transforms (133 link poses, no velocities)", med, lo_, hi_))
    results = {}
    for K in (1, 4, 133, 1024):
        links = ((np.arange(K) * 37 + 5) % nl).tolist()
        pts = np.random.default_rng(K).uniform(-0.3, 0.3, (K, 3))
        b.set_link_probes(0, links, pts)
        pose, vel, ac = (torch.empty(n, K, w, device=dev) for w in (7, 6, 6))
        for name, fn in (("pose", lambda: b.link_state(0, 0, False, None, pose, None, None, probes=K)),
                         ("pose + velocity", lambda: b.link_state(0, 0, False, None, pose, vel, None, probes=K)),
                         ("all three", lambda: b.link_state(0, 0, True, acc, pose, vel, ac, probes=K))):
            med, lo_, hi_ = time_us(fn, args.iters, args.repeats)
            results[(K, name)] = med
            say("  %-46s %8.1f   (%.1f .. %.1f)" % ("link_state K = %-4d %s" % (K, name), med, lo_, hi_))
        if K <= 4:
            Jb = torch.empty(K, n, 6, D, device=dev)
            gv = torch.zeros(n, D, device=dev)

            def composed():
                for k in range(K):
                    b.jacobian(links[k], pts[k], Jb[k])
                return torch.matmul(Jb, gv.unsqueeze(-1))

            def composed_sum():      # (the same product as a multiply and a row sum: no batched GEMM of 6 x 31 matrices)
                for k in range(K):
                    b.jacobian(links[k], pts[k], Jb[k])
                return (Jb * gv[None, :, None, :]).sum(-1)
            for label, fn in (("matmul", composed), ("multiply + sum", composed_sum)):
                med, lo_, hi_ = time_us(fn, args.iters, args.repeats)
                results[(K, "composed")] = min(med, results.get((K, "composed"), med))
                say("  %-46s %8.1f   (%.1f .. %.1f)" % ("%d x jacobian + %s (velocities only)" % (K, label), med, lo_, hi_))
    v.close()
    for K in (1, 4):
        one, many = results[(K, "pose + velocity")], results[(K, "composed")]
        say("K = %d: the single launch (pose + velocity) takes %.1f us, the faster composition %.1f us: %s" % (
            K, one, many, "the single launch is faster" if one < many else "the single launch is NOT faster"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
