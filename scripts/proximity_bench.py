#!/usr/bin/env python
"""Accuracy and cost of the proximity query (trex_batch_proximity) on the GPU.

Deviations: the largest figures of tests/test_gpu_proximity.py's checks against the f64 reference tests/proximity_ref.py - the
default T-rex table with all 253 pairs at N = 67, the synthetic cases and the generated models at N = 3 - of which the distance
deviations are what its tolerances (MEASURED) are set from. They are measured with the cap (1e-5) in force, so that a figure above
4 x MEASURED is printed and not raised.

Cost at 4 096 envs: us per launch for the default table (230 pairs, 1 572 tests), a feet-only table (the bodies of one leg below
the knee against the other's) and the extreme the C-ABI admits (256 capsules, 65 536 tests in 4 pairs), distance only and every
output, next to a step launch and a link_state launch (133 link origins, pose + velocity) of the same batch - hipEvents around
`iters` back-to-back launches after a warm-up, the median (min .. max) of `repeats` such groups. Then the kernel's registers, LDS
and scratch as the compiler reports them. Writes profiles/r18_proximity.txt (--out). No gate hangs on the timings."""
import argparse
import os
import re
import statistics
import subprocess
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


def kernel_resources():
    """what hipcc reports for proximity.hip (the flags of csrc/Makefile's resource-usage target)"""
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "proximity.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "-fno-slp-vectorize", "-c",
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired) as e:
        return "not available (%s)" % e
    keep = ("VGPRs:", "AGPRs:", "TotalSGPRs:", "ScratchSize", "Occupancy", "LDS Size", "VGPRs Spill")
    found = [m.group(1).strip() for m in re.finditer(r"remark:\s+(.*?)\s+\[-Rpass-analysis", r.stderr) if any(k in m.group(1) for k in keep)]
    return "; ".join(found) or "not available (no remarks)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_proximity.txt"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-deviations", action="store_true")
    args = ap.parse_args()
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    lines = ["proximity between bodies (trex_batch_proximity): deviation from the f64 reference and cost per launch",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), ""]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not args.no_deviations:
        import proximity_cases as PC
        import synthetic_models as sm
        import test_gpu_proximity as T                # (for its deviations and FIGS alone)
        from conftest import ASSET_URDF
        from gpu_support import loaded_vec
        from oracle import oracle as O, trex_model
        from state_sets import case_states
        model = trex_model.compile_model(ASSET_URDF)
        o64 = O.Oracle(model, precision="f64")
        T.TOL = {k: T.CAP for k in T.TOL}          # measure: the cap in force, not 4 x the figures this run is to find
        say("largest figures against the f64 reference (tests/proximity_ref.py), each over the env's scale max(1 m, largest |body-origin")
        say("coordinate|) but `unit`: distance |d - d_ref|; unit ||n| - 1|; on_a, on_b: point +- r n off its capsule's segment; gap:")
        say("|(point_a - point_b) . n - d|; direction: |n - n_ref| x axis distance. MEASURED of tests/test_gpu_proximity.py quotes `distance`.")
        fmt = lambda f: "  ".join("%s %.3g" % (k, f[k]) for k in ("distance", "unit", "on_a", "on_b", "gap", "direction"))
        T.trex_deviation(o64, model, 67)
        say("  %-28s %s" % ("trex, 253 pairs, N = 67", fmt(T.FIGS["trex"])))
        states = case_states(o64, model, 67)[:3]
        v = loaded_vec(states)
        per_case = {}
        for case in PC.cases():
            per_case[case["name"]] = T.cases_deviation(v, states, model, case)[0]
        v.close()
        say("  %-28s %s" % ("synthetic cases, N = 3", fmt(T.FIGS["cases"])))
        worst = sorted(per_case, key=per_case.get)[-3:]
        say("  %-28s %s" % ("  their largest distances", "  ".join("%s %.3g" % (k, per_case[k]) for k in worst)))
        with tempfile.TemporaryDirectory() as tmp:
            for name in T.SYN:
                path, props, om = sm.compile_both(name, os.path.join(tmp, name))
                T.synthetic_deviation(dict(path=path, props=props, om=om), name)
                say("  %-28s %s" % (name + ", N = 3", fmt(T.FIGS[name])))
        say("")
        save()

    n = args.envs
    say("timing at %d envs: hipEvents around %d back-to-back launches, warm-up 20, median (min .. max) of %d groups, us per launch"
        % (n, args.iters, args.repeats))
    v = TrexVecEnv(n, device="cuda:0")
    v.reset_tensor()
    gen = torch.Generator().manual_seed(0)
    lo, hi = torch.tensor(v.model.lower, dtype=torch.float32), torch.tensor(v.model.upper, dtype=torch.float32)
    acts = (lo + (hi - lo) * torch.rand(n, v.J, generator=gen)).to(v.device)
    for _ in range(5):       # (a moving state)
        v.step_tensor(acts)
    b, dev = v.batch, v.device
    row = lambda name, t: say("  %-58s %8.1f   (%.1f .. %.1f)" % ((name,) + t))
    row("step launch (step_tensor)", time_us(lambda: v.step_tensor(acts), args.iters, args.repeats))
    nl = len(v.model.links())
    b.set_link_probes(0, list(range(nl)), np.zeros((nl, 3)))
    pose, vel = torch.empty(n, nl, 7, device=dev), torch.empty(n, nl, 6, device=dev)
    row("link_state, %d link origins, pose + velocity" % nl, time_us(lambda: b.link_state(0, 0, False, None, pose, vel, None, probes=nl),
                                                                      args.iters, args.repeats))
    shapes = v.proximity_shapes()
    count = np.bincount(shapes.bodies, minlength=v.model.num_bodies)
    tests = lambda pairs: int(sum(count[a] * count[c] for a, c in pairs))
    names = {}
    for name, body in v.model.links():
        names.setdefault(body, name)
    leg = lambda side: [x for x in range(v.model.num_bodies) if count[x] and re.search(r"(toe|tarsometatarsus|tibia).*_%s$" % side, names[x])]
    feet = [(a, c) for a in leg("left") for c in leg("right")]
    rng = np.random.default_rng(0)
    p0 = rng.uniform(-0.3, 0.3, (256, 3))
    extreme = (np.array([3] * 128 + [15] * 128, np.int32), np.concatenate([p0, p0 + rng.uniform(-0.2, 0.2, (256, 3)), rng.uniform(0.01, 0.08, (256, 1))], 1))
    tables = [("default table", None, [tuple(p) for p in shapes.pairs], tests(shapes.pairs)),
              ("feet only", None, feet, tests(feet)),
              ("extreme: 256 capsules", extreme, [(3, 15)] * 4, 4 * 128 * 128)]
    for name, caps, pairs, nt in tables:
        if not pairs:
            say("  %s: no such bodies in this model" % name)
            continue
        v.proximity_shapes(caps if caps is not None else (shapes.bodies, shapes.capsules), pairs)
        P = len(pairs)
        d = torch.empty(n, P, device=dev)
        pts = [torch.empty(n, P, 3, device=dev) for _ in range(3)]
        idx = torch.empty(n, P, 2, dtype=torch.int32, device=dev)
        label = "proximity, %s (%d pairs, %d tests)" % (name, P, nt)
        row(label + ", distance", time_us(lambda: b.proximity(d, pairs=P), args.iters, args.repeats))
        row(label + ", all outputs", time_us(lambda: b.proximity(d, *pts, idx, pairs=P), args.iters, args.repeats))
    v.close()
    say("")
    say("trex_proximity_kernel, as compiled: " + kernel_resources())
    save()


if __name__ == "__main__":
    main()
