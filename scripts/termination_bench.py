#!/usr/bin/env python
"""Accuracy and cost of kernel K8 (trex_batch_body_clearance, trex_batch_set_termination) on the GPU.

Deviations: what tests/test_gpu_termination.py prints before it asserts - clearance, lowest point, head height, cos tilt and
clearance margin against the f64 reference tests/termination_ref.py, at N = 67 on both collision models, on the judged states of
the decision tests and on the generated models - of which the largest are what its tolerances (MEASURED) are set from. The tests
run in a process of their own (pytest -s); a figure above the tolerance in force shows as a failure there and is still printed.

Cost at 4 096 envs on bench.py's stationary episode mix (1000-step episodes with staggered phases, uniform random actions, a
pre-roll of one episode length), hipEvents around `iters` back-to-back calls after a warm-up, the median (min .. max) of `repeats`
groups, the variants of a table taking turns group by group:
  body_clearance per launch, with and without the lowest point;
  step_rows plain (termination never enabled);
  step_rows with termination on and thresholds that never fire;
  step_rows with thresholds that fire on that mix (after a pre-roll of its own with them on; the share of envs that fall per step);
  the host-driven equivalent of the never-firing step: step_rows, clearance query, head position, state read-out, a torch mask,
  reset_rows with it, reward and done patched;
  the plain step_rows of another build of the library (--parent-lib: the parent commit's), in processes of its own that take turns
  with processes of this build.
Writes profiles/r19_termination.txt (--out). No gate hangs on the timings."""
import argparse
import math
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


def make_env(n, terminate=None, preroll=EPISODE_STEPS):
    """an env on the stationary mix: staggered 1000-step episodes, uniform random actions from a pool, `preroll` steps taken"""
    from trex_gym.vec_env import TrexVecEnv
    v = TrexVecEnv(n, device="cuda:0", max_episode_steps=EPISODE_STEPS, terminate=terminate)
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


def plain_child(args):
    v, step = make_env(args.envs)
    t = groups_us(dict(plain=step), args.iters, args.repeats)["plain"]
    print("PLAIN %.3f %.3f %.3f" % t, flush=True)
    v.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_termination.txt"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-deviations", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="a libtrex_hip.so built from the parent commit: its plain step_rows is timed too")
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.plain_child:
        return plain_child(args)
    from trex_gym import _capi, termination
    lines = ["kernel K8 - floor clearance and fall termination: deviation from the f64 reference and cost",
             "device: %s   kernel build id: %s" % (torch.cuda.get_device_name(0), _capi.build_id()), ""]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not args.no_deviations:
        say("figures printed by tests/test_gpu_termination.py (pytest -s), each over the env's scale max(1 m, largest |position entry|)")
        say("but cos tilt; MEASURED of the test quotes the largest of each kind:")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_termination.py"), "-s", "-q", "-p", "no:cacheprovider",
                            "-k", "values or decisions or generated"], capture_output=True, text=True, cwd=ROOT)
        for ln in r.stdout.splitlines():
            if "deviation" in ln or "judged states" in ln:
                say("  " + ln.strip().lstrip("."))
        tail = [ln for ln in r.stdout.splitlines() if re.search(r"\d+ (passed|failed)", ln)]
        say("  pytest: " + (tail[-1].strip("= ") if tail else "no summary (exit %d)" % r.returncode))
        say("")
        save()

    n = args.envs
    say("timing at %d envs on the stationary episode mix: hipEvents around %d back-to-back calls, warm-up 20, median (min .. max) of"
        % (n, args.iters))
    say("%d groups taking turns, us per call" % args.repeats)
    row = lambda name, t: say("  %-72s %8.1f   (%.1f .. %.1f)" % ((name,) + t))
    v, step = make_env(n)
    nb = v.model.num_bodies
    clr, low = torch.empty(n, nb, device=v.device), torch.empty(n, nb, 3, device=v.device)
    q = groups_us(dict(c=lambda: v.batch.body_clearance(clr), cl=lambda: v.batch.body_clearance(clr, low)), args.iters, args.repeats)
    row("body_clearance, %d bodies, %d collision points" % (nb, len(v.model.array("hull_radius"))), q["c"])
    row("body_clearance with the lowest point", q["cl"])
    fall = termination.fall_bodies(v)
    margin = v.model.get_param("contact_margin")
    floor_z = v.model.get_param("floor_z")
    never = dict(head_height=-1.0e3, max_tilt=math.pi, keep_clear={l: -1.0e3 for l in fall})
    fire = dict(head_height=0.5, max_tilt=1.2, keep_clear=fall, penalty=1.0)
    vn, step_never = make_env(n, never)
    # the host-driven equivalent, with the same never-firing thresholds: every launch and torch op a user would need per step
    vh, step_plain_h = make_env(n)
    watched = torch.as_tensor(vh._link_bodies(fall), device=vh.device)
    head = torch.empty(n, 3, device=vh.device)
    hclr = torch.empty(n, nb, device=vh.device)
    qs = torch.tensor(vh.model.array("base_start_quat"), dtype=torch.float32, device=vh.device)
    up_s = torch.stack([2 * (qs[0] * qs[2] - qs[1] * qs[3]), 2 * (qs[1] * qs[2] + qs[0] * qs[3]), 1 - 2 * (qs[0] ** 2 + qs[1] ** 2)])
    cos_never, pen = math.cos(math.pi), 0.0

    def step_host():
        step_plain_h()
        vh.batch.body_clearance(hclr)
        vh.batch.head_position(head)
        qb = vh.get_state()[:, 3:7]
        x, y, z, w = qb[:, 0], qb[:, 1], qb[:, 2], qb[:, 3]
        up = torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)
        mask = (head[:, 2] - floor_z < -1.0e3) | ((up * up_s).sum(1) < cos_never) | ((hclr[:, watched] + 1.0e3).min(1).values < 0)
        mask &= ~vh.done
        rew, done_f = vh.rew.clone(), vh.done_f.clone()
        vh.batch.reset_rows(vh.rows, mask.to(torch.uint8))
        vh.rew.copy_(torch.where(mask, rew - pen, rew))
        vh.done_f.copy_(torch.where(mask, torch.ones_like(done_f), done_f))
        vh.done.logical_or_(mask)

    t = groups_us(dict(plain=step, never=step_never, host=step_host), args.iters, args.repeats)
    row("step_rows, termination never enabled", t["plain"])
    row("step_rows, termination on, thresholds that never fire (%d bodies watched)" % len(fall), t["never"])
    row("host-driven equivalent: step_rows + clearance + head + state + torch mask + reset_rows + patch", t["host"])
    verdict = "below" if t["never"][0] < t["host"][0] else "NOT below"
    say("  -> the never-firing termination step costs %.1f us more than the plain step, %s the host-driven equivalent (+%.1f us)"
        % (t["never"][0] - t["plain"][0], verdict, t["host"][0] - t["plain"][0]))
    vn.close()
    vh.close()
    vf, step_fire = make_env(n, fire)
    fell = 0
    for _ in range(100):
        step_fire()
        fell += int((vf.termination_reason != 0).sum())
    t2 = groups_us(dict(plain=step, fire=step_fire), args.iters, args.repeats)
    row("step_rows, termination never enabled (again)", t2["plain"])
    row("step_rows, head < 0.5 m | tilt > 1.2 rad | a body but the feet within %.3g m of the floor" % margin, t2["fire"])
    say("  (that mix: %.2f %% of the envs fall per step; a fallen env's step is one settle substep on top, a light env otherwise)"
        % (100.0 * fell / (100 * n)))
    vf.close()
    v.close()
    if args.parent_lib:
        res = {"this build": [], "parent build": []}
        for _ in range(2):
            for name, lib in (("parent build", args.parent_lib), ("this build", None)):
                env = dict(os.environ)
                env.pop("TREX_LIB", None)
                if lib:
                    env["TREX_LIB"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--envs", str(n), "--iters", str(args.iters),
                                    "--repeats", str(args.repeats)], capture_output=True, text=True, env=env)
                m = re.search(r"PLAIN (\S+) (\S+) (\S+)", r.stdout)
                if m:
                    res[name].append(tuple(float(x) for x in m.groups()))
        say("")
        say("plain step_rows in processes of their own, taking turns (two each):")
        for name, runs in res.items():
            say("  %-72s %s" % (name, "   ".join("%.1f (%.1f .. %.1f)" % r for r in runs) or "not measured"))
    else:
        say("the parent commit's plain step_rows: not measured (no --parent-lib)")
    say("")
    save()


if __name__ == "__main__":
    main()
