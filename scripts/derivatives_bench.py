#!/usr/bin/env python
"""Cost and accuracy of kernel K18 (the derivatives of the inverse dynamics: trex_batch_inverse_dynamics_derivatives) on the GPU, and
its resource lines. No figure was claimed in advance; no gate hangs on the timings.

Cost at 256 and 4 096 T-rex envs in ONE process, hipEvents around `iters` back-to-back calls after a warm-up, the median
(min .. max) of `repeats` groups, the variants taking turns group by group: the launch for dfdq alone, dfdv alone, both, both by
direction; beside them inverse_dynamics, solve_mass with K = 31 rows in place, and the whole of forward_dynamics_derivatives into
given tensors.

The path the API allowed before: central differences from the host, 2 x 56 set_state + inverse_dynamics launch pairs per
linearisation (the perturbed states made on the device by the retraction), timed at the same sizes, and its accuracy on the twelve
T-rex states of tests/derivatives_cases.py in the same per-row metric, for two steps.

Accuracy: the largest deviation of the device from the f64 reference over both variants, both layouts and both matrices of every
model of tests/derivatives_cases.py, as a share of the bound the reference's f32 run sets; likewise forward_dynamics_derivatives in
its residual metric. Writes profiles/r33_derivatives.txt (--out)."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from joint_wrench_bench import _TmpFactory  # noqa: E402
from observations_bench import groups_us, make_env  # noqa: E402

DEV = "cuda:0"


def retract(state, J, j, h, velocity):
    """[n, 13 + 2J] states moved by h along direction j of the configuration tangent (velocity: of the generalised velocity)"""
    s = state.clone()
    if velocity:
        s[:, (7 + j) if j < 6 else (13 + J + j - 6)] += h
    elif j < 3:
        s[:, j] += h
    elif j < 6:
        x, y, z, w = s[:, 3], s[:, 4], s[:, 5], s[:, 6]
        a = [0.0, 0.0, 0.0]
        a[j - 3] = float(np.sin(h / 2))
        ax, ay, az, aw = a[0], a[1], a[2], float(np.cos(h / 2))
        s[:, 3:7] = torch.stack([aw * x + ax * w + ay * z - az * y, aw * y - ax * z + ay * w + az * x,
                                 aw * z + ax * y - ay * x + az * w, aw * w - ax * x - ay * y - az * z], 1)
    else:
        s[:, 13 + j - 6] += h
    return s


def host_differences(v, state, acc, h):
    """(dfdq, dfdv) [n, D, D] by central differences through set_state + inverse_dynamics: the 2 x 2 (D - 3) launch pairs the API
    allowed before (the translation columns stay zero); the env is left at `state`"""
    n, J = v.num_envs, v.J
    D = 6 + J
    out = [torch.zeros(n, D, D, device=DEV), torch.zeros(n, D, D, device=DEV)]
    f = [torch.zeros(n, D, device=DEV), torch.zeros(n, D, device=DEV)]
    for velocity in (False, True):
        for j in range(3, D):
            for k, sign in enumerate((1.0, -1.0)):
                v.set_state(retract(state, J, j, sign * h, velocity))
                v.batch.inverse_dynamics(acc, f[k])
            out[int(velocity)][:, :, j] = (f[0] - f[1]) / (2 * h)
    v.set_state(state)
    return out


def cost_lines(args, n):
    from trex_gym import derivatives
    from trex_gym.derivatives_capi import BY_DIRECTION, BatchDerivatives
    v, _ = make_env(n, preroll=50)
    api = BatchDerivatives(v.batch)
    D = 6 + v.J
    gen = torch.Generator(device=DEV).manual_seed(1)
    acc = torch.randn(n, D, generator=gen, device=DEV)
    dq, dv = torch.zeros(n, D, D, device=DEV), torch.zeros(n, D, D, device=DEV)
    force, rhs = torch.zeros(n, D, device=DEV), torch.randn(n, D, D, generator=gen, device=DEV)
    outs = [torch.zeros(n, D, device=DEV)] + [torch.zeros(n, D, D, device=DEV) for _ in range(3)]
    fns = {
        "inverse_dynamics(accel)": lambda: v.batch.inverse_dynamics(acc, force),
        "solve_mass, K = %d rows, in place" % D: lambda: v.batch.solve_mass(rhs, rhs),
        "derivatives: dfdq alone": lambda: api.inverse_dynamics_derivatives(acc, dq, None),
        "derivatives: dfdv alone": lambda: api.inverse_dynamics_derivatives(acc, None, dv),
        "derivatives: both": lambda: api.inverse_dynamics_derivatives(acc, dq, dv),
        "derivatives: both, by direction": lambda: api.inverse_dynamics_derivatives(acc, dq, dv, BY_DIRECTION),
        "forward_dynamics_derivatives, into given tensors": lambda: derivatives.forward_dynamics_derivatives(v, force, out=outs),
    }
    us = groups_us(fns, args.iters, args.repeats)
    lines = ["%d envs (us per call: median, min .. max of %d groups of %d back-to-back calls)" % (n, args.repeats, args.iters)]
    lines += ["  %-52s %9.2f  (%.2f .. %.2f)" % (k, *x) for k, x in us.items()]
    state = v.get_state()
    host = groups_us({"host": lambda: host_differences(v, state, acc, 1e-3)}, 2, 3, warmup=1)["host"]
    lines.append("  %-52s %9.1f  (%.1f .. %.1f)   %.0f x the launch for both"
                 % ("central differences from the host, %d launch pairs" % (4 * (D - 3)), *host, host[0] / us["derivatives: both"][0]))
    v.close()
    return lines


def accuracy_lines():
    import derivatives_cases as DC
    from conftest import ASSET_URDF
    from oracle import trex_model
    from test_gpu_derivatives import dev_accel, device_outputs, env_of
    from trex_gym import derivatives
    lines = ["accuracy, per row of a matrix (max_j |got - ref| / max_j |ref|), the largest over 12 states, accel given and NULL, both "
             "layouts and both matrices, beside the reference's own f32 run and the bound; then forward_dynamics_derivatives in its "
             "residual metric"]
    host = []
    with tempfile.TemporaryDirectory() as tmp:
        built = DC.built(_TmpFactory(tmp), trex_model.compile_model(ASSET_URDF))
        for name in DC.MODELS:
            c = DC.case(name, built[name]["om"])
            v = env_of(built[name], c["inp"]["cases"])
            out = device_outputs(v, c["inp"])
            jac = lambda key, m: (out[key][m].transpose(1, 2) if key[1] == "dir" else out[key][m]).cpu().numpy()
            dev = max(DC.row_deviation(jac(key, m), c["ref"][key[0]][1 + m]) for key in out for m in (0, 1))
            force = torch.tensor(c["ref"]["accel"][0].astype(np.float32)).to(DEV)
            _, dadq, dadv, _ = derivatives.forward_dynamics_derivatives(v, force)
            fwd = DC.forward_deviation(dadq.cpu().numpy(), dadv.cpu().numpy(), c["fwd"], c["ref"])
            lines.append("  %-12s device %.3g   f32 run %.3g   bound %.3g   share of the bound %.0f %%;   forward: device %.3g   f32 run %.3g   "
                         "bound %.3g   share %.0f %%" % (name, dev, c["d32"], c["bound"], 100 * dev / c["bound"], fwd, c["fwd_d32"],
                                                        c["fwd_bound"], 100 * fwd / c["fwd_bound"]))
            if name == "trex":
                acc, state = dev_accel(c["inp"], DC.N), v.get_state()
                for h in (1e-3, 1e-2):
                    fq, fv = host_differences(v, state, acc, h)
                    host.append("  central differences from the host on the T-rex cases, step %g: dfdq %.3g, dfdv %.3g (the device's launch: %.3g; "
                                "the bound %.3g)" % (h, DC.row_deviation(fq.cpu().numpy(), c["ref"]["accel"][1]),
                                                     DC.row_deviation(fv.cpu().numpy(), c["ref"]["accel"][2]), dev, c["bound"]))
            v.close()
    return lines + host


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "dynamics_derivatives.hip")
    if not os.path.exists(hipcc):
        return ["  not recorded: no hipcc here"]
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "-fno-slp-vectorize", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True)
    keep = [ln.split("remark:")[1].split("[-Rpass")[0].strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    return ["  " + "; ".join(keep)] if keep else ["  not recorded: hipcc exit %d" % r.returncode]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_derivatives.txt"))
    args = ap.parse_args()
    from trex_gym import _capi
    lines = ["K18, derivatives of the inverse dynamics (trex_batch_inverse_dynamics_derivatives): cost and accuracy",
             "command: python scripts/derivatives_bench.py --iters %d --repeats %d" % (args.iters, args.repeats),
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), "",
             "cost on the T-rex (D = 31: 28 directions per matrix, 14 passes each), beside inverse_dynamics and solve_mass on the same batch; "
             "back-to-back launches, so a figure is the larger of launch cost and kernel time"]
    for n in (256, 4096):
        lines += cost_lines(args, n)
    lines += [""] + accuracy_lines()
    lines += ["", "resource usage (hipcc -Rpass-analysis=kernel-resource-usage; dynamic LDS 4 x (32 x 39 + outputs x D x D) floats per "
              "workgroup: 50.7 KB at D = 31 with both outputs, 35.3 KB with one):"] + resource_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
