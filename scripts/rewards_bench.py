#!/usr/bin/env python
"""Accuracy and cost of kernel K11 (trex_batch_compose_reward: the reward terms) on the GPU.

Deviations: what tests/test_gpu_rewards.py prints before it asserts - for every kind the largest |GPU - f64 reference| over the
bound tests/reward_ref.py derives for that value (1 = at the bound), over N = 1, 8, 9, 17, the drop from the start pose and the
episode-end runs. The tests run in a process of their own (pytest -s); a figure above 1 shows as a failure there and is still
printed.

Cost at 4 096 envs in ONE process, on bench.py's stationary episode mix (1000-step episodes with staggered phases, uniform random
actions from a pool, a pre-roll of one episode length), hipEvents around `iters` back-to-back calls after a warm-up, the median
(min .. max) of `repeats` groups, the three variants taking turns group by group:
  (a) step_rows alone: TrexVecEnv without rewards - what the parent commit runs;
  (b) step_rows + compose_reward: TrexVecEnv(rewards=locomotion(model)) - 14 terms: the step's reward at weight 0, velocity
      tracking, vertical and tilting velocity, orientation, torque, joint acceleration, action rate, air time and slip of two feet,
      a contact count over the other bodies - the contact sensor on, as the preset needs it;
  (c) the same 14 terms as the parent commit allows them: step_rows with the contact sensor on, link_state(axes="base") of the base
      link, link_state(axes="world") of the base link and the two feet, contact_wrench, and torch ops for the terms, their history
      (previous actions, previous qd, timers, held values on done rows) and the weighted sum written into the reward column.
The file states what was measured; no gate hangs on the timings. It also records the kernel's resource line (hipcc
-Rpass-analysis=kernel-resource-usage, where hipcc is at hand). Writes profiles/r23_rewards.txt (--out)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from observations_bench import groups_us, make_env  # noqa: E402


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "reward.hip")
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


def torch_terms(v, spec, names):
    """the preset's terms from the queries the parent commit has, as a closure over its own history -> fn(actions) -> terms [n, T]"""
    from trex_gym.sensors import quat_rotate_inverse
    n, J, dev = v.num_envs, v.J, v.device
    Ts = float(v.model.get_param("dt") * v.model.get_param("substeps"))
    feet = [c.link for c in spec if c.kind == "foot_air_time"]
    foot_bodies = [int(b) for b in v._link_bodies(feet)]
    others = [int(b) for b in v._link_bodies([l for c in spec if c.kind == "contact_count" for l in c.mask])]
    base_b, world = v.link_probes([0]), v.link_probes([0] + feet)
    down = torch.tensor([0.0, 0.0, -1.0], device=dev).expand(n, 3)
    wrench = torch.empty(n, v.model.num_bodies, 6, device=dev)
    w = torch.tensor([c.weight for c in spec], device=dev)
    par = {c.kind: c for c in spec}
    h = dict(valid=torch.zeros(n, dtype=torch.bool, device=dev), act=torch.zeros(n, J, device=dev), qd=torch.zeros(n, J, device=dev),
             timer=torch.zeros(n, len(feet), device=dev), held=torch.zeros(n, len(spec), device=dev))
    zero = torch.zeros(n, device=dev)

    def fn(actions):
        rows = v.rows
        qd, tau, done = rows[:, J:2 * J], rows[:, 2 * J:3 * J], rows[:, 3 * J + 1] != 0
        lb = v.link_state(base_b, axes="base")
        lw = v.link_state(world, axes="world")
        f = v.contact_wrench(wrench)
        lin, ang = lb.linear_velocity[:, 0], lb.angular_velocity[:, 0]
        g = quat_rotate_inverse(lw.orientation[:, 0], down)
        c = v.commands
        cols = {"step": rows[:, 3 * J],
                "track_lin_vel": torch.exp(-((lin[:, :2] - c[:, :2]) ** 2).sum(1) / par["track_lin_vel"].p0),
                "track_ang_vel": torch.exp(-(ang[:, 2] - c[:, 2]) ** 2 / par["track_ang_vel"].p0),
                "lin_vel_z": lin[:, 2] ** 2, "ang_vel_xy": (ang[:, :2] ** 2).sum(1), "orientation": (g[:, :2] ** 2).sum(1),
                "torque": (tau ** 2).sum(1),
                "joint_acc": torch.where(h["valid"], (((qd - h["qd"]) / Ts) ** 2).sum(1), zero),
                "action_rate": torch.where(h["valid"], ((actions - h["act"]) ** 2).sum(1), zero),
                "contact_count": (f[:, others, :3].norm(dim=2) > par["contact_count"].p0).sum(1).to(torch.float32)}
        out, k = [], 0
        for name, cspec in zip(names, spec):
            if cspec.kind == "foot_air_time":
                contact = f[:, foot_bodies[k], 2] > cspec.p0
                t = h["timer"][:, k]
                out.append(torch.where(contact & (t > 0), t - cspec.p1, zero))
                h["timer"][:, k] = torch.where(contact | done, zero, t + Ts)
            elif cspec.kind == "foot_slip":
                contact = f[:, foot_bodies[k], 2] > cspec.p0
                out.append(torch.where(contact, (lw.linear_velocity[:, 1 + k, :2] ** 2).sum(1), zero))
                k += 1
            else:
                out.append(cols[cspec.kind])
        vals = torch.stack(out, 1)
        vals = torch.where(done[:, None], h["held"], vals)
        vals[:, 0] = rows[:, 3 * J]
        keep = ~done
        h["held"] = torch.where(keep[:, None], vals, h["held"])
        h["act"] = torch.where(keep[:, None], actions, h["act"])
        h["qd"] = torch.where(keep[:, None], qd, h["qd"])
        h["valid"] = keep
        terms = vals * w
        rows[:, 3 * J] = terms.sum(1)
        return terms
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_rewards.txt"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-deviations", action="store_true")
    args = ap.parse_args()
    from trex_gym import _capi, rewards as R
    lines = ["kernel K11 - reward terms (trex_batch_compose_reward): deviation from the f64 reference and cost",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), ""]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("reward.hip, hipcc -Rpass-analysis=kernel-resource-usage (the observation kernel: 70 VGPRs, LDS 20224 bytes, 7 waves/SIMD, no scratch):")
    for ln in resource_lines():
        say(ln)
    say("")
    if not args.no_deviations:
        say("figures printed by tests/test_gpu_rewards.py (pytest -s): per kind the largest |GPU - reference| / bound, the bound being")
        say("reward_ref.bound(kind, case) x |weight| (1.000 = at the bound; CONTACT_COUNT, STEP, ALIVE and held values are compared exactly)")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_rewards.py"), "-s", "-q", "-p",
                            "no:cacheprovider", "-k", "against_reference or history or done_rows_episode"], capture_output=True, text=True, cwd=ROOT)
        found = [ln for ln in r.stdout.splitlines() if "reward deviation / bound" in ln]
        if found:                                                   # (the figures accumulate over the process: the last line holds the largest)
            for item in found[-1].split(": ", 1)[1].split("  "):
                say("  " + item.strip())
        tail = [ln for ln in r.stdout.splitlines() if re.search(r"\d+ (passed|failed)", ln)]
        say("  pytest: " + (tail[-1].strip("= ") if tail else "no summary (exit %d)" % r.returncode))
        say("")
        save()

    n = args.envs
    say("timing at %d envs on the stationary episode mix: hipEvents around %d back-to-back calls, warm-up 20, median (min .. max) of"
        % (n, args.iters))
    say("%d groups taking turns, us per call" % args.repeats)
    row = lambda name, t: say("  %-94s %8.1f   (%.1f .. %.1f)" % ((name,) + t))
    model = _capi.Model()
    spec = R.locomotion(model, "cuda:0")
    names = R.names(spec)
    cmd = torch.tensor([0.5, 0.0, 0.1], device="cuda:0")
    va, step_a = make_env(n)
    vb, step_b = make_env(n, rewards=spec)
    vb.commands[:] = cmd
    vc, step_c0 = make_env(n)
    vc.enable_contact_sensor(True)
    vc.commands = cmd.expand(n, 3).contiguous()          # (a plain env has no commands: the torch variant keeps its own)
    terms_c = torch_terms(vc, spec, names)
    made = {}

    def step_c():
        step_c0()
        made["terms"] = terms_c(vc._last_actions)

    # (make_env's step keeps no handle on the actions it passed: remember them where step_tensor takes them)
    plain_step = vc.step_tensor

    def remember(actions):
        vc._last_actions = actions
        return plain_step(actions)
    vc.step_tensor = remember
    step_c0()
    t = groups_us(dict(a=step_a, b=step_b, c=step_c), args.iters, args.repeats)
    assert made["terms"].shape == vb.reward_terms.shape == (n, len(spec))
    row("(a) step_rows", t["a"])
    row("(b) step_rows + compose_reward, locomotion preset (%d terms; contact sensor on)" % len(spec), t["b"])
    row("(c) step_rows (sensor on) + 2 x link_state + contact_wrench + the terms, history and sum in torch", t["c"])
    db, dc = t["b"][0] - t["a"][0], t["c"][0] - t["a"][0]
    say("  -> (b) - (a) = %.1f us, (c) - (a) = %.1f us: the reward launch costs %s the separate queries and torch ops"
        % (db, dc, "less than" if db < dc else "NOT less than"))
    say("  mean reward per step of (b) over the last call: %.4f; per term: %s"
        % (vb.rew.mean().item(), "  ".join("%s %.4g" % (k, x) for k, x in zip(names, vb.reward_terms.mean(0).tolist()))))
    for v in (va, vb, vc):
        v.close()
    say("")
    save()


if __name__ == "__main__":
    main()
