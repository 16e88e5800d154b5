#!/usr/bin/env python
"""Cost and accuracy of the dynamics queries (trex_batch_inverse_dynamics / _mass_matrix / _jacobian / _centroidal) on the GPU:
us per launch of each query at 256, 4 096 and 32 768 envs (hipEvents around `iters` back-to-back launches after a warm-up, the
median of `repeats` such groups) next to the step launch of the same batch, and the largest deviations from the f64 reference
on the states of tests/test_gpu_dynamics.py - the figures its tolerances are set from. Writes profiles/r12_dynamics.txt
(--out). No gate hangs on the timings: they are recorded so that the next reader knows the cost.

--models: no timings; per generated model of tests/dynamics_model_cases.py the deviation d32 of the reference's f32 run, the bound
it sets and the GPU's deviation, for every metric and every identity of tests/test_gpu_dynamics_models.py. Writes
profiles/r27_dynamics_models.txt (--out)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

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


class _TmpDirs:
    """what state_sets.built_models asks of pytest's tmp_path_factory"""

    def mktemp(self, name):
        import tempfile
        return tempfile.mkdtemp(prefix=name + "_")


def models_report(out_path):
    import dynamics_model_cases as DC
    import test_gpu_dynamics_models as T
    from state_sets import built_models
    from trex_gym import _capi
    lines = ["dynamics queries on the generated models: the reference's f32 run, the bound it sets, the GPU",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()),
             "%d states per model (dynamics_ref.random_states, seed 31; the last two with a per-body mass scale); the Jacobian at every"
             % DC.N, "URDF link, at its origin and at (0.3, -0.2, 0.1). d32: the largest deviation of the reference run in float32 from the same",
             "reference in float64, in the metric. bound = min(cap, max(T-rex tolerance, 4 x d32)): from the reference alone, no GPU",
             "figure enters it. Identities: the residual of the f32 run's own outputs takes the place of d32.", ""]
    built = built_models(DC.MODELS, _TmpDirs())
    worst = 0.0
    for name in DC.MODELS:
        c = DC.case(name, built[name])
        v = T.env_of(built[name], c["cases"])
        got = T.as_numpy(T.device_outputs(v, c["om"], c["acc"]))
        v.close()
        dev, res = DC.metric_devs(c["taus"], got, c["ref"]), DC.identity_devs(c["om"], c["cases"], c["acc"], got)
        lines.append("%s   (D = %d, %d links)" % (name, 6 + c["om"]["nb"] - 1, len(c["om"]["link_names"])))
        lines.append("  %-13s %10s %10s %10s %8s" % ("", "d32", "bound", "GPU", "GPU/bound"))
        rows = [(k, c["d32"][k], c["bound"][k], dev[k]) for k in DC.METRICS] + [(k, c["res32"][k], c["id_bound"][k], res[k]) for k in DC.IDENTITIES]
        for k, d, b, g in rows:
            lines.append("  %-13s %10.3g %10.3g %10.3g %8.2f" % (k, d, b, g, g / b))
            worst = max(worst, g / b)
        lines.append("")
        print("\n".join(lines[-len(rows) - 3:]), flush=True)
    lines.append("largest GPU deviation over its bound: %.2f" % worst)
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-deviations", action="store_true")
    args = ap.parse_args()
    if args.models:
        return models_report(args.out or os.path.join(ROOT, "profiles", "r27_dynamics_models.txt"))
    args.out = args.out or os.path.join(ROOT, "profiles", "r12_dynamics.txt")
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    lines = ["dynamics queries: cost per launch and deviation from the f64 reference",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()),
             "timing: hipEvents around %d back-to-back launches, warm-up 20, median (min .. max) of %d groups, us per launch"
             % (args.iters, args.repeats), ""]
    lines.append("%8s  %-18s %10s" % ("envs", "launch", "us"))
    for n in (256, 4096, 32768):
        v = TrexVecEnv(n, device="cuda:0")
        v.reset_tensor()
        b = v.batch
        D = 6 + v.J
        acc = torch.zeros(n, D, device=v.device)
        outs = dict(id=torch.empty(n, D, device=v.device), M=torch.empty(n, D, D, device=v.device),
                    jac=torch.empty(n, 6, D, device=v.device), cent=torch.empty(n, 16, device=v.device))
        act = torch.zeros(n, v.J, device=v.device)      # (clipped to the joint limits by the step)
        runs = [("step", lambda: v.step_tensor(act)),
                ("inverse_dynamics", lambda: b.inverse_dynamics(acc, outs["id"])),
                ("mass_matrix", lambda: b.mass_matrix(outs["M"])),
                ("jacobian", lambda: b.jacobian(5, (0.1, 0.2, 0.3), outs["jac"])),
                ("centroidal", lambda: b.centroidal(outs["cent"]))]
        for name, fn in runs:
            med, lo, hi = time_us(fn, args.iters, args.repeats)
            lines.append("%8d  %-18s %10.1f   (%.1f .. %.1f)" % (n, name, med, lo, hi))
            print(lines[-1], flush=True)
        v.close()
    if not args.no_deviations:
        import test_gpu_dynamics as T
        from conftest import ASSET_URDF
        from oracle import oracle as O, trex_model
        model = trex_model.compile_model(ASSET_URDF)
        o64 = O.Oracle(model, precision="f64")
        lines += ["", "largest deviation from the f64 reference (tests/dynamics_ref.py), scales as in tests/test_gpu_dynamics.py:"]
        for n in (1, 67):
            d = T.deviations(o64, model, n)
            lines.append("  N = %-3d " % n + "  ".join("%s %.3g" % kv for kv in sorted(d.items())))
            print(lines[-1], flush=True)
        worst, told = T.step_tied_deviation(o64, model)
        lines.append("  step-tied (inverse dynamics of one step's acceleration against tau - joint_damping qd, 4 envs): id_step %.3g; "
                     "joint rows that tell it from plain tau: %s of %d" % (worst, told, model["nb"] - 1))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
