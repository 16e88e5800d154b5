#!/usr/bin/env python
"""Cost and accuracy of kernel K17 (the joint force/torque sensor: trex_batch_joint_wrench, trex_batch_generalized_velocity) on the
GPU, and its resource lines. No figure was claimed in advance; no gate hangs on the timings.

Cost at 4 096 envs in ONE process, hipEvents around `iters` back-to-back calls after a warm-up, the median (min .. max) of
`repeats` groups, the variants taking turns group by group:
  (a) the query's launch beside trex_batch_inverse_dynamics on the same batch and the same accelerations: without a wrench in world
      axes, with both wrenches in link axes and the base row, and the generalised-velocity launch;
  (b) step_tensor on bench.py's stationary episode mix (scripts/observations_bench.make_env): plain, with the contact sensor alone,
      with the joint sensor attached (the contact sensor, its read-out and the two launches of K17).
--parent-lib LIB adds (c): the plain step of that library - the parent commit's build - and of this one in processes of their own,
taking turns, two each; the plain step must be where the parent's is, within the spread of the alternation itself.
Accuracy: the largest deviation of the device from the f64 reference over every model and variant of tests/joint_wrench_cases.py, as
a share of the bound the reference's f32 run sets. The step-mean approximation: the median over envs and steps of
|joint_base_residual| over the robot's weight on a 200-step random-action rollout - the wrench a free base would still need from
outside, zero for an exact reading; reported, not asserted. Writes profiles/r32_joint_wrench.txt (--out)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from observations_bench import groups_us, make_env  # noqa: E402

DEV = "cuda:0"


def query_lines(args):
    from trex_gym.joint_wrench_capi import BatchJointWrench
    n = args.envs
    v, _ = make_env(n, preroll=50)
    api = BatchJointWrench(v.batch)
    D, nb = 6 + v.J, v.model.num_bodies
    gen = torch.Generator(device=DEV).manual_seed(1)
    acc = torch.randn(n, D, generator=gen, device=DEV)
    wa, wb = torch.randn(n, nb, 6, generator=gen, device=DEV), torch.randn(n, nb, 6, generator=gen, device=DEV)
    out, base, force = torch.zeros(n, v.J, 6, device=DEV), torch.zeros(n, 6, device=DEV), torch.zeros(n, D, device=DEV)
    latch, dv = torch.zeros(n, D, device=DEV), torch.zeros(n, D, device=DEV)
    fns = {
        "inverse_dynamics(accel)": lambda: v.batch.inverse_dynamics(acc, force),
        "joint_wrench(accel), world axes": lambda: api.joint_wrench(acc, None, None, "world", out),
        "joint_wrench(accel, a, b), link axes, base row": lambda: api.joint_wrench(acc, wa, wb, "link", out, base),
        "generalized_velocity (latch, difference)": lambda: api.generalized_velocity(latch, latch, 50.0, v.rows, 3 * v.J + 1, dv),
    }
    us = groups_us(fns, args.iters, args.repeats)
    lines = ["(a) the query at %d envs beside inverse_dynamics on the same batch (us per call: median, min .. max of %d groups of %d calls; "
             "back-to-back launches, so a figure is the larger of launch cost and kernel time)" % (n, args.repeats, args.iters)]
    lines += ["  %-52s %8.2f  (%.2f .. %.2f)" % (k, *x) for k, x in us.items()]
    v.close()
    return lines


def step_lines(args):
    from trex_gym import joint_sensor
    n = args.envs
    plain, step_plain = make_env(n)
    contact, step_contact = make_env(n)
    contact.enable_contact_sensor(True)
    sensed, step_sensed = make_env(n)
    joint_sensor.attach(sensed)
    names = ("step_tensor alone", "step + the contact sensor", "step + the joint sensor attached")
    us = groups_us(dict(zip(names, (step_plain, step_contact, step_sensed))), args.iters, args.repeats)
    lines = ["(b) step_tensor at %d envs on the stationary episode mix (us per call: median, min .. max of %d groups of %d calls)"
             % (n, args.repeats, args.iters)]
    base = us[names[0]][0]
    for k, (med, lo, hi) in us.items():
        lines.append("  %-42s %8.1f  (%.1f .. %.1f)%s" % (k, med, lo, hi, "" if k.endswith("alone") else "   %+.1f" % (med - base)))
    for e in (plain, contact, sensed):
        e.close()
    return lines


def plain_child(args):
    v, step = make_env(args.envs)
    med, lo, hi = groups_us(dict(plain=step), args.iters, args.repeats)["plain"]
    print("PLAIN %.2f %.2f %.2f" % (med, lo, hi))


def parent_lines(args):
    """the plain step (nothing attached) of the parent's library and of this one, processes taking turns"""
    runs = {"parent": [], "this": []}
    lines = []
    for k in range(2):
        for name, lib in (("parent", args.parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("TREX_LIB", None)
            if lib:
                env["TREX_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--envs", str(args.envs), "--iters",
                                str(args.iters), "--repeats", str(args.repeats)], capture_output=True, text=True, env=env)
            m = re.search(r"PLAIN (\S+) (\S+) (\S+)", r.stdout)
            if not m:
                lines.append("  %s commit, run %d: not measured (exit %d)" % (name, k + 1, r.returncode))
                continue
            med, lo, hi = (float(x) for x in m.groups())
            runs[name].append((med, lo, hi))
            lines.append("  %-28s %8.1f  (%.1f .. %.1f)" % ("%s commit, run %d" % (name, k + 1), med, lo, hi))
    if runs["parent"] and runs["this"]:
        width = max(hi - lo for v in runs.values() for _, lo, hi in v)
        pm, tm = [r[0] for r in runs["parent"]], [r[0] for r in runs["this"]]
        inside = all(min(pm) - width <= x <= max(pm) + width for x in tm)
        lines.append("  spread of the alternation itself: %.1f us within a run, the parent's medians %.1f .. %.1f; this commit's medians "
                     "%.1f .. %.1f: the plain step %s" % (width, min(pm), max(pm), min(tm), max(tm),
                                                          "did not move beyond that spread" if inside else "MOVED beyond that spread"))
    return lines


class _TmpFactory:
    """what state_sets.built_models asks of pytest's tmp_path_factory"""

    def __init__(self, root):
        self.root = root

    def mktemp(self, name):
        import pathlib
        p = pathlib.Path(self.root) / name
        p.mkdir()
        return p


def accuracy_lines():
    import joint_wrench_cases as JC
    from conftest import ASSET_URDF
    from oracle import trex_model
    from test_gpu_joint_wrench import as_numpy, device_outputs, env_of
    lines = ["accuracy: the largest deviation of the device from the f64 reference over every variant (accel / wrench_a / wrench_b NULL and "
             "given, world and link axes, joint rows and base row) of 12 states, beside the reference's own f32 run and the bound"]
    with tempfile.TemporaryDirectory() as tmp:
        built = JC.built(_TmpFactory(tmp), trex_model.compile_model(ASSET_URDF))
        for name in JC.MODELS:
            c = JC.case(name, built[name]["om"])
            v = env_of(built[name], c["inp"]["cases"])
            dev = JC.largest_deviation(as_numpy(device_outputs(v, c["inp"])), c["ref"], c["inp"]["weight"])
            v.close()
            lines.append("  %-12s device %.3g   f32 run %.3g   bound %.3g   share of the bound %.0f %%"
                         % (name, dev, c["d32"], c["bound"], 100 * dev / c["bound"]))
    return lines


def residual_lines(steps=200, n=256):
    """two rollouts from the start pose: uniform random actions - the joints are thrown about within every env-step, the hardest case
    for a step-mean reading - and the start pose held, where the robot lands and stands"""
    from trex_gym import joint_sensor
    from trex_gym.vec_env import TrexVecEnv
    q = lambda x: "median %.3g, 90th percentile %.3g" % (np.median(x), np.percentile(x, 90))
    lines = []
    for what in ("uniform random actions", "the start pose held"):
        v = joint_sensor.attach(TrexVecEnv(n, device=DEV))
        hold = v.reset_tensor()[:, :v.J].clone()
        weight = float(v.model.total_mass(include_base_link=True)) * float(v.model.get_param("gravity"))
        gen = torch.Generator().manual_seed(0)
        lo, hi = torch.tensor(v.model.lower, dtype=torch.float32), torch.tensor(v.model.upper, dtype=torch.float32)
        force, moment, contact = [], [], []
        for _ in range(steps):
            v.step_tensor(hold if what.endswith("held") else (lo + (hi - lo) * torch.rand(n, v.J, generator=gen)).to(DEV))
            r = v.joint_base_residual
            force.append(r[:, :3].norm(dim=1) / weight)
            moment.append(r[:, 3:].norm(dim=1) / weight)
            contact.append(v.contact_wrench()[:, :, 2].sum(1) / weight)
        f, m, c = (torch.stack(x).cpu().numpy() for x in (force, moment, contact))
        v.close()
        lines += ["  %s, all %d steps:" % (what, steps),
                  "    force part / weight:             %s" % q(f), "    moment part / (weight x 1 m):    %s" % q(m),
                  "    for scale, the contact sensor's summed normal force / weight: %s" % q(c),
                  "  %s, the last 50 steps:  force part %s; moment part %s; normal force %s" % (what, q(f[-50:]), q(m[-50:]), q(c[-50:]))]
    return ["the step-mean approximation on %d-step rollouts of %d envs from the start pose (weight %.0f N): |joint_base_residual| over "
            "the weight - the wrench a free base would still need from outside, zero for an exact reading; reported, not asserted"
            % (steps, n, weight)] + lines


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "joint_wrench.hip")
    if not os.path.exists(hipcc):
        return ["  not recorded: no hipcc here"]
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "-fno-slp-vectorize", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True)
    keep = [ln.split("remark:")[1].split("[-Rpass")[0].strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    out, at = [], 0
    for k, item in enumerate(keep):                                 # one line per kernel
        if item.startswith("Function Name") and k:
            out.append("  " + "; ".join(keep[at:k]))
            at = k
    return out + ["  " + "; ".join(keep[at:])] if keep else ["  not recorded: hipcc exit %d" % r.returncode]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libtrex_hip.so: its plain step, in alternating processes")
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_joint_wrench.txt"))
    args = ap.parse_args()
    if args.plain_child:
        return plain_child(args)
    from trex_gym import _capi
    lines = ["K17, joint force/torque sensor (trex_batch_joint_wrench, trex_batch_generalized_velocity): cost and accuracy",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), ""]
    lines += query_lines(args) + [""] + step_lines(args) + [""]
    if args.parent_lib and os.path.exists(args.parent_lib):
        lines += ["(c) the plain step of the parent commit and of this one, alternating processes of one session (us per call: median, "
                  "min .. max):"] + parent_lines(args)
    else:
        lines += ["(c) the parent commit's plain step: not measured (no --parent-lib)"]
    lines += [""] + accuracy_lines() + [""] + residual_lines()
    lines += ["", "resource usage (hipcc -Rpass-analysis=kernel-resource-usage; dynamic LDS 4 x (512 + 6 J + 6) floats per workgroup: 10.6 KB "
              "at J = 25):"] + resource_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
