#!/usr/bin/env python
"""Cost of kernel K22 (the mirror maps, include/trex_symmetry.h) on the GPU and what training on the mirrored samples costs.

At 4096 envs, T = 32, the locomotion preset (D = 93, A = 25), in ONE process, hipEvents around `iters` back-to-back calls after a
warm-up, the median (min .. max) of `repeats` groups, the calls taking turns group by group:
  (a) the augment launch on the [2 T n, ..] rollout buffers, with the bytes it must move (every sample's D + A + 4 words read once
      and written once) over its time; mirror_rows on the env's row block [n, D + 2], in place and out of place, and on the T n
      stored observations; symmetrize_stats (the moments and their f32 image: two launches);
  (b) PPO env-steps/s of whole iterations (collect + update, eager, a host clock around work that ends in a synchronise) for plain
      PPO, MirrorPPO(symmetry=None) - which must be the same launches - and MirrorPPO(symmetry="augment"), taking turns;
  (c) the T-rex model's residuals, and the mean |mu(s) - M_a mu(M_o s)| over the last rollout's observations after a short run with
      and without the option - recorded figures, nothing more. (Without the option the stored observations are normalised by moments
      that are not symmetric, so M_o is applied to rows whose normalisation does not commute with it: the figure mixes both effects.)
  (d) f64 on the CPU: the equivariance defects of M, h and the channels of the T-rex under its own tables, measured.
No training benefit is claimed and no gate hangs on a timing. Writes profiles/r38_symmetry.txt (--out); --tests FILE appends the
lines tests/test_gpu_symmetry.py printed (pytest -s) that it finds in FILE; --parent FILE the lines of a file that holds the plain
step time and the plain PPO rate of the parent commit and of this one, measured in the same session by alternating processes:
each such line is what `symmetry_bench.py --plain LABEL [--package DIR]` prints - the plain step and plain PPO (4096 envs, T = 32,
D = 75) of the trex_gym package under DIR (default: this tree's), whose library it loads."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "trex-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from observations_bench import groups_us  # noqa: E402

DEV = "cuda:0"
if "--package" in sys.argv:         # (behind the helpers' own path entries, before trex_gym is imported: the package - Python and
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--package") + 1]))      # library - of another build)


def resource_lines():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "trex-gym_amd", "csrc", "symmetry.hip")
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


def fmt(name, v, extra=""):
    return "  %-62s %8.1f  (%.1f .. %.1f)%s" % (name, v[0], v[1], v[2], extra)


def kernel_lines(env, mirror, T, iters, repeats):
    from trex_gym import _capi, symmetry_capi as S
    n, D, A = env.num_envs, mirror.obs_dim, mirror.act_table.width
    N = T * n
    bufs = [torch.randn(2 * N, D, device=DEV), torch.randn(2 * N, A, device=DEV)] + [torch.randn(2 * N, device=DEV) for _ in range(4)]
    rows = torch.randn(n, mirror.width, device=DEV)
    rows_out = torch.empty_like(rows)
    obs, obs_out = bufs[0][:N], torch.empty(N, D, device=DEV)
    pol = _capi.Policy(n, D, A, 64, 0)
    fns = {
        "augment": lambda: S.augment(mirror.obs_table, mirror.act_table, *bufs, N),
        "rows_block": lambda: mirror.rows(rows, rows_out),
        "rows_block_in_place": lambda: mirror.rows(rows, rows),
        "rows_obs": lambda: mirror.rows(obs, obs_out),
        "stats": lambda: S.symmetrize_stats(pol, mirror.obs_table),
    }
    us = groups_us(fns, iters, repeats)
    moved = 2 * N * (D + A + 4) * 4
    return [
        "n = %d envs, T = %d, D = %d, A = %d (us per call: median, min .. max of %d groups of %d calls)" % (n, T, D, A, repeats, iters),
        fmt("augment launch, %d samples -> %d" % (N, 2 * N), us["augment"],
            "   %.1f MB to move, %.2f TB/s achieved" % (moved / 1e6, moved / us["augment"][0] / 1e6)),
        fmt("mirror_rows on the row block [%d, %d], out of place" % (n, mirror.width), us["rows_block"]),
        fmt("mirror_rows on the row block, in place", us["rows_block_in_place"]),
        fmt("mirror_rows on the stored observations [%d, %d]" % (N, D), us["rows_obs"],
            "   %.2f TB/s" % (2 * N * D * 4 / us["rows_obs"][0] / 1e6)),
        fmt("symmetrize_stats (moments + their f32 image: 2 launches)", us["stats"]),
    ]


def asymmetry(agent, mirror):
    """mean |mu(s) - M_a mu(M_o s)| over the last rollout's stored observations"""
    T, n = agent.nsteps, agent.env.num_envs
    obs = agent.b_obs[:T].reshape(T * n, -1)
    with torch.no_grad():
        mu = agent.policy.mean(obs)
        mu_m = mirror.actions(agent.policy.mean(mirror.rows(obs)).contiguous())
    return (mu - mu_m).abs().mean().item()


def trainer_lines(n, T, iterations, short):
    from trex_gym import trex_train
    from trex_gym.ppo import PPO
    from trex_gym.symmetry import Mirror, MirrorPPO
    kinds = ("plain PPO", "MirrorPPO(symmetry=None)", 'MirrorPPO(symmetry="augment")', 'MirrorPPO(symmetry="loss")',
             'MirrorPPO(symmetry="both")')
    modes = dict(zip(kinds, (None, None, "augment", "loss", "both")))
    agents, mirrors = {}, {}
    for kind in kinds:
        env = trex_train.build_environment(n, device=DEV, observations="locomotion")
        mirrors[kind] = Mirror(env, log=None)
        kw = dict(nsteps=T, seed=0)
        agents[kind] = PPO(env, **kw) if kind == kinds[0] else MirrorPPO(env, mirrors[kind], symmetry=modes[kind], **kw)
    rates = {k: [] for k in kinds}
    for a in agents.values():
        a.update(a.collect())                      # warm-up: workspaces, code objects
    for _ in range(iterations):
        for kind, a in agents.items():             # taking turns
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.update(a.collect())
            torch.cuda.synchronize()
            rates[kind].append(n * T / (time.perf_counter() - t0))
    out = ["PPO env-steps/s of whole iterations (collect + update, eager), %d envs x T = %d, locomotion preset (D = %d): median (min .. max) of %d iterations"
           % (n, T, mirrors[kinds[0]].obs_dim, iterations)]
    for kind in kinds:
        v = rates[kind]
        out.append("  %-34s %10.0f  (%.0f .. %.0f)" % (kind, statistics.median(v), min(v), max(v)))
    base = statistics.median(rates[kinds[0]])
    out.append("  of the plain rate: augment -%.1f %%, loss -%.1f %%, both -%.1f %%; symmetry=None is %+.2f %% off it; its own spread is %.2f %%"
               % (tuple(100 * (1 - statistics.median(rates[k]) / base) for k in kinds[2:]) +
                  (100 * (statistics.median(rates[kinds[1]]) / base - 1), 100 * (max(rates[kinds[0]]) - min(rates[kinds[0]])) / base)))
    for a in agents.values():
        for _ in range(short):
            a.update(a.collect())
    out.append("mean |mu(s) - M_a mu(M_o s)| over the last rollout after %d iterations (a recorded figure; nothing is claimed):" % (short + iterations + 1))
    for kind in (kinds[0],) + kinds[2:]:
        out.append("  %-34s %.4f" % (kind, asymmetry(agents[kind], mirrors[kind])))
    res = mirrors[kinds[0]].residual
    out.append("the T-rex asset is not symmetric by (lateral axis %d of link 0): " % mirrors[kinds[0]].lateral +
               "; ".join("%s %.4g" % kv for kv in res.items()))
    env0 = agents[kinds[2]].env
    return out, env0, mirrors[kinds[2]]


def reference_lines():
    """f64, CPU: what of the T-rex is NOT equivariant under its own tables - the mass matrix, the bias forces and the kinematic
    channels of six random states (tests/symmetry_ref.py on tests/dynamics_ref.py and tests/observation_ref.py) - measured, beside
    the same figures of the generated exactly symmetric biped"""
    import tempfile

    import numpy as np

    import dynamics_ref as D
    import observation_ref as OBS
    import symmetry_models as SM
    import symmetry_ref as R
    from oracle import oracle as O, trex_model as tm

    def defects(model, chans):
        mm = R.model_table(model)
        nj = model["nb"] - 1
        src = np.concatenate([np.arange(6), 6 + mm["pair"]])
        P = np.zeros((6 + nj, 6 + nj))
        P[np.arange(6 + nj), src] = np.concatenate([[-1, 1, 1], [1, -1, -1], mm["sign"]])
        rs, rg = R.row_table(model, mm, chans, nj, 2)
        dM = dh = dc = 0.0
        for s in SM.random_states(model, 6, seed=4):
            s2 = R.mirror_state(model, mm, s)
            M, h = D.mass_matrix(model, s), D.inverse_dynamics(model, s)
            dM = max(dM, np.abs(D.mass_matrix(model, s2) - P @ M @ P.T).max() / np.abs(M).max())
            dh = max(dh, np.abs(D.inverse_dynamics(model, s2) - P @ h).max() / np.abs(h).max())
            row = np.concatenate([s[13:], np.zeros(nj + 2)])
            row2 = np.concatenate([s2[13:], np.zeros(nj + 2)])
            a, b = OBS.compose(model, s, chans, row, 2), OBS.compose(model, s2, chans, row2, 2)
            dc = max(dc, (np.abs(b - R.mirror_rows_f64(rs, rg, a)) / np.maximum(1.0, np.abs(b))).max())
        return dM, dh, dc

    trex = tm.compile_model(O.default_asset_urdf())
    feet = [trex["link_names"].index(n) for n in trex["link_names"] if "toe_03_c" in n]
    base = [(R.PROJECTED_GRAVITY, 0, (0, 0, 0), 1.0), (R.BASE_LINEAR_VELOCITY, 0, (0, 0, 0), 1.0), (R.BASE_ANGULAR_VELOCITY, 0, (0, 0, 0), 1.0),
            (R.BASE_HEIGHT, 0, (0, 0, 0), 1.0)]
    chans = base + [(k, l, (0, 0, 0), 1.0) for l in feet for k in (R.POINT_POSITION, R.POINT_VELOCITY, R.POINT_HEIGHT)]
    out = ["equivariance defects under the model's own tables, f64 on the CPU, six random states (largest relative |difference|): M, h, channels"]
    out.append("  the T-rex asset (measured, not asserted)      %.3g  %.3g  %.3g" % defects(trex, chans))
    _, _, biped = SM.compile_biped(tempfile.mkdtemp(), 0)
    bch = [c for c in SM.locomotion_channels(biped, 0) if c[0] != R.CONTACT_FORCE]
    out.append("  the generated exactly symmetric biped        %.3g  %.3g  %.3g" % defects(biped, bch))
    return out


def plain_line(label, n=4096, T=32):
    """the plain step (hipEvents, 5 groups of 100 steps behind 200 warm-up steps, uniform random actions) and plain PPO (6 whole
    iterations behind one, eager) of whatever trex_gym package is first on the path"""
    import trex_gym
    from trex_gym.ppo import PPO
    from trex_gym.vec_env import TrexVecEnv
    if "--package" in sys.argv:
        want = os.path.abspath(sys.argv[sys.argv.index("--package") + 1])
        assert os.path.abspath(trex_gym.__file__).startswith(want), (trex_gym.__file__, want)
    env = TrexVecEnv(n, device=DEV, max_episode_steps=1000)
    env.reset_tensor()
    lo = torch.tensor(env.model.lower, dtype=torch.float32, device=DEV)
    hi = torch.tensor(env.model.upper, dtype=torch.float32, device=DEV)
    pool = [lo + (hi - lo) * torch.rand(n, env.J, device=DEV) for _ in range(16)]
    for k in range(200):
        env.step_tensor(pool[k % 16])
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(100):
            env.step_tensor(pool[k % 16])
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 10.0)
    agent = PPO(TrexVecEnv(n, device=DEV), nsteps=T, seed=0)
    agent.update(agent.collect())
    rates = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.update(agent.collect())
        torch.cuda.synchronize()
        rates.append(n * T / (time.perf_counter() - t0))
    return ("  %-6s commit: plain step %7.1f us  (%.1f .. %.1f)   plain PPO %9.0f env-steps/s  (%.0f .. %.0f)   [%s]"
            % (label, statistics.median(us), min(us), max(us), statistics.median(rates), min(rates), max(rates),
               os.path.relpath(os.path.dirname(trex_gym.__file__), ROOT)))


def parent_lines(path):
    """the lines of --parent FILE and whether this commit's medians lie within the session's spread: the parent's own range of
    medians widened by the largest (max - min) of a single run"""
    import re
    runs = {"parent": [], "this": []}
    keep, width = [], [0.0, 0.0]
    for ln in open(path):
        m = re.match(r"\s*(parent|this)\s+commit: plain step\s+([\d.]+) us\s+\(([\d.]+) \.\. ([\d.]+)\)\s+plain PPO\s+(\d+) env-steps/s\s+\((\d+) \.\. (\d+)\)", ln)
        if m:
            v = [float(x) for x in m.groups()[1:]]
            runs[m.group(1)].append((v[0], v[3]))
            width = [max(width[0], v[2] - v[1]), max(width[1], v[5] - v[4])]
            keep.append(ln.rstrip())
    out = ["the plain step and plain PPO against a build of the PARENT commit, alternating processes in this session:"] + keep
    if runs["parent"] and runs["this"]:
        for k, what in ((0, "plain step"), (1, "plain PPO")):
            pv, tv = [r[k] for r in runs["parent"]], [r[k] for r in runs["this"]]
            lo, hi = min(pv) - width[k], max(pv) + width[k]
            inside = all(lo <= x <= hi for x in tv)
            out.append("  %s: this commit's medians %s lie %s the parent's %s widened by the largest spread of a run (%.4g): [%.6g, %.6g]"
                       % (what, ["%.6g" % x for x in tv], "WITHIN" if inside else "OUTSIDE", ["%.6g" % x for x in pv], width[k], lo, hi))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", default=None, metavar="LABEL")
    ap.add_argument("--package", default=None, metavar="DIR")
    ap.add_argument("--parent", default=None, metavar="FILE")
    ap.add_argument("--tests", default=None, metavar="FILE")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nsteps", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--short", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r38_symmetry.txt"))
    args = ap.parse_args()
    if args.plain is not None:
        print(plain_line(args.plain), flush=True)
        return
    lines = ["K22, the mirror maps (include/trex_symmetry.h)"]
    trainer, env, mirror = trainer_lines(args.envs, args.nsteps, args.iterations, args.short)
    lines += kernel_lines(env, mirror, args.nsteps, args.iters, args.repeats)
    lines += trainer
    lines += reference_lines()
    lines += ["note: the bytes of the augment launch are fewer than the 256 MB Infinity Cache holds and the calls run back to back on the same",
              "  buffers: its TB/s is a rate through the cache hierarchy, not an HBM figure."]
    if args.parent:
        lines += parent_lines(args.parent)
    else:
        lines += ["the plain step and plain PPO against a build of the parent commit: NOT measured in this run (--parent)"]
    if args.tests:
        found = [ln.strip().lstrip(".") for ln in open(args.tests) if "of its tolerance" in ln]
        lines += ["accuracy (tests/test_gpu_symmetry.py, pytest -s; rows, augment and moments are compared bit for bit):"] + ["  " + ln for ln in found]
    lines += ["resource usage (hipcc -Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
