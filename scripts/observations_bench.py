#!/usr/bin/env python
"""Accuracy and cost of kernel K10 (trex_batch_compose_rows: the observation channels) on the GPU.

Deviations: what tests/test_gpu_observations.py prints before it asserts - the computed channels against the f64 reference
tests/observation_ref.py at N = 1 .. 67 and on 64 envs of 4 096, over the scales of tests/test_gpu_link_state.py, whose tolerances
the test takes. The tests run in a process of their own (pytest -s); a figure above the tolerance shows as a failure there and is
still printed.

Cost at 4 096 envs in ONE process, on bench.py's stationary episode mix (1000-step episodes with staggered phases, uniform random
actions from a pool, a pre-roll of one episode length), hipEvents around `iters` back-to-back calls after a warm-up, the median
(min .. max) of `repeats` groups, the three variants taking turns group by group:
  (a) step_rows alone: TrexVecEnv without observations;
  (b) step_rows + compose_rows: TrexVecEnv(observations=locomotion(model)) - 18 columns: gravity, base velocities, base height,
      contact force and base-frame position of the two feet - the contact sensor on, as the preset needs it;
  (c) the same 18 columns as the parent commit allows them: step_rows with the contact sensor on, link_state(axes="base") for the
      base link and the two feet (pose + velocity), link_state(axes="world", pose only) of the base link for its height and
      orientation, the gravity vector from that quaternion in torch, contact_wrench, and one torch.cat into a fresh [n, 93] tensor.
The claim to establish: (b) - (a) < (c) - (a). The file says so either way. It also records the compose kernel's resource line
(hipcc -Rpass-analysis=kernel-resource-usage, where hipcc is at hand). Writes profiles/r21_observations.txt (--out). No gate hangs
on the timings."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

EPISODE_STEPS = 1000
POOL = 16


def groups_us(fns, iters, repeats, warmup=20):
    """{name: (median, min, max) us per call}; the callables take turns, group by group"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def make_env(n, preroll=EPISODE_STEPS, **kw):
    """an env on the stationary mix: staggered 1000-step episodes, uniform random actions from a pool, `preroll` steps taken"""
    from trex_gym.vec_env import TrexVecEnv
    v = TrexVecEnv(n, device="cuda:0", max_episode_steps=EPISODE_STEPS, **kw)
    v.reset_tensor()
    v.set_episode_steps(((torch.arange(n) * EPISODE_STEPS) // n).to(torch.int32))
    gen = torch.Generator().manual_seed(0)
    lo, hi = torch.tensor(v.model.lower, dtype=torch.float32), torch.tensor(v.model.upper, dtype=torch.float32)
    pool = [(lo + (hi - lo) * torch.rand(n, v.J, generator=gen)).to(v.device) for _ in range(POOL)]
    state = dict(t=0)

    def step():
        v.step_tensor(pool[state["t"] % POOL])
        state["t"] += 1
    for _ in range(preroll):
        step()
    torch.cuda.synchronize()
    return v, step


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "observation.hip")
    if not os.path.exists(hipcc):
        return ["  not recorded: no hipcc here"]
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "-fno-slp-vectorize", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True)
    keep = [ln.split("remark:")[1].split("[-Rpass")[0].strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    return ["  " + "; ".join(keep)] if keep else ["  not recorded: hipcc exit %d" % r.returncode]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_observations.txt"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-deviations", action="store_true")
    args = ap.parse_args()
    from trex_gym import _capi, observations as O
    from trex_gym.sensors import quat_rotate_inverse
    lines = ["kernel K10 - observation channels (trex_batch_compose_rows): deviation from the f64 reference and cost",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), ""]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("trex_observation_kernel, hipcc -Rpass-analysis=kernel-resource-usage (the link-state kernels: LDS 24704 bytes, no scratch):")
    for ln in resource_lines():
        say(ln)
    say("")
    if not args.no_deviations:
        say("figures printed by tests/test_gpu_observations.py (pytest -s): the largest deviation of the computed channels over")
        say("max(1, the channel's largest |entry|) x |scale|; tolerances in force: tests/test_gpu_link_state.py TOL (pose 8.24e-7, velocity 1.73e-6)")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_observations.py"), "-s", "-q", "-p",
                            "no:cacheprovider", "-k", "values_against_reference or many_workgroups"], capture_output=True, text=True, cwd=ROOT)
        for ln in r.stdout.splitlines():
            if "observation deviations" in ln:
                say("  " + re.sub(r"np\.float64\(([^)]*)\)", r"\1", ln.strip().lstrip(".")))
        tail = [ln for ln in r.stdout.splitlines() if re.search(r"\d+ (passed|failed)", ln)]
        say("  pytest: " + (tail[-1].strip("= ") if tail else "no summary (exit %d)" % r.returncode))
        say("")
        save()

    n = args.envs
    say("timing at %d envs on the stationary episode mix: hipEvents around %d back-to-back calls, warm-up 20, median (min .. max) of"
        % (n, args.iters))
    say("%d groups taking turns, us per call" % args.repeats)
    row = lambda name, t: say("  %-86s %8.1f   (%.1f .. %.1f)" % ((name,) + t))
    model = _capi.Model()
    spec = O.locomotion(model, "cuda:0")
    va, step_a = make_env(n)
    vb, step_b = make_env(n, observations=spec)
    vc, step_c0 = make_env(n)
    vc.enable_contact_sensor(True)
    feet = [c.link for c in spec if c.kind == "contact_force"]
    foot_bodies = [int(b) for b in vc._link_bodies(feet)]
    probes = vc.link_probes([0] + feet)
    base = vc.link_probes([0])
    floor_z = vc.model.get_param("floor_z")
    down = torch.tensor([0.0, 0.0, -1.0], device=vc.device).expand(n, 3)
    wrench = torch.empty(n, vc.model.num_bodies, 6, device=vc.device)
    made = {}

    def step_c():
        step_c0()
        ls = vc.link_state(probes, axes="base")
        lw = vc.link_state(base, axes="world", velocity=False)
        w = vc.contact_wrench(wrench)
        made["obs"] = torch.cat([vc.obs, quat_rotate_inverse(lw.orientation[:, 0], down), ls.linear_velocity[:, 0], ls.angular_velocity[:, 0],
                                 lw.position[:, 0, 2:3] - floor_z, w[:, foot_bodies[0], 2:3], ls.position[:, 1], w[:, foot_bodies[1], 2:3],
                                 ls.position[:, 2]], 1)

    t = groups_us(dict(a=step_a, b=step_b, c=step_c), args.iters, args.repeats)
    assert made["obs"].shape == vb.obs.shape == (n, 93)
    row("(a) step_rows", t["a"])
    row("(b) step_rows + compose_rows, locomotion preset (18 columns, D' = 93; contact sensor on)", t["b"])
    row("(c) step_rows (sensor on) + 2 x link_state + contact_wrench + gravity in torch + torch.cat", t["c"])
    db, dc = t["b"][0] - t["a"][0], t["c"][0] - t["a"][0]
    say("  -> (b) - (a) = %.1f us, (c) - (a) = %.1f us: the compose launch costs %s the separate queries"
        % (db, dc, "less than" if db < dc else "NOT less than"))
    # the same columns, two ways, on envs that took the same actions from the same start
    dev = ((made["obs"] - vb.obs).abs() / made["obs"].abs().clamp(min=1.0)).max().item()
    say("  largest difference between the rows of (c) and of (b) after the same steps, over max(1, |value|): %.3g" % dev)
    for v in (va, vb, vc):
        v.close()
    say("")
    save()


if __name__ == "__main__":
    main()
