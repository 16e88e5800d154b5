"""The clip table and the term list of the motion clip, on the CPU and under the sanitizers: build_motion_table and
build_motion_terms of csrc/host_tables.cpp - what trex_batch_set_motion and trex_batch_set_motion_reward hand the kernels - built
with csrc/model.cpp into tests/host/motion_harness.cpp by g++ -fsanitize=address,undefined (the flags of
tests/test_reward_tables_host.py; no HIP, nothing loaded into Python) and run as a child process, one run per case. The table is
compared with the numpy restatement motion_ref.build_table: integers exactly, f32 values to one unit in the last place (the
restatement forms its f64 differences in the builder's order). No sanitizer report may appear."""
import os
import subprocess

import numpy as np
import pytest

import layout_cases as LC
import motion_cases as MC
import motion_ref as MR
from conftest import ASSET_URDF, ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID
J = 25
COLS = 13 + 2 * J
STRIDE = (COLS + 3) // 4 * 4


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("motion_tables") / "motion_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "motion_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def run_numbers(exe, tmp_path, numbers, urdf=ASSET_URDF):
    path = os.path.join(str(tmp_path), "numbers.txt")
    with open(path, "w") as f:
        f.write(" ".join(repr(float(x)) for x in numbers))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, urdf, path], env=env, capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    if r.stdout.startswith("REFUSED "):
        _, code, msg = r.stdout.rstrip("\n").split(" ", 2)
        return ("REFUSED", int(code), msg)
    return {line.split(" ", 1)[0]: np.array(line.split()[1:], np.float64) for line in r.stdout.splitlines()}


def table(exe, tmp_path, frames, frame_dt=MC.DT, loop=False, velocities=None, F=None, urdf=ASSET_URDF):
    frames = np.asarray(frames, np.float64)
    n = [0, len(frames) if F is None else F, frame_dt, int(loop), int(velocities is not None)] + list(frames.reshape(-1))
    return run_numbers(exe, tmp_path, n + ([] if velocities is None else list(np.asarray(velocities, np.float64).reshape(-1))), urdf)


def terms(exe, tmp_path, spec, has_probes=True, step_weight=1.0):
    return run_numbers(exe, tmp_path, [1, int(has_probes), step_weight, len(spec)] + [x for s in spec for x in s])


def refused(out, text):
    assert isinstance(out, tuple) and out[0] == "REFUSED", out
    assert out[1] == INVALID and text in out[2], out


def check_table(t, model, frames, frame_dt, loop, velocities=None, J=J):
    COLS = 13 + 2 * J
    STRIDE = (COLS + 3) // 4 * 4
    w = MR.build_table(model, frames, velocities, frame_dt, loop)
    F = len(frames)
    assert t["scalars"].astype(np.int64).tolist() == [F, J, STRIDE, int(loop), F * STRIDE]
    want = np.array([w["frame_dt"], w["inv_dt"], w["duration"], w["inv_duration"], w["disp"][0], w["disp"][1]])
    assert (t["constants"].astype(np.float32) == want.astype(np.float32)).all()
    rows = t["rows"].astype(np.float32).astype(np.float64).reshape(F, STRIDE)     # (9 digits name an f32; rounding gives it back)
    assert (rows[:, COLS:] == 0).all()                                    # the padding
    got, ref = rows[:, :COLS], w["rows"]
    want32 = ref.astype(np.float32)
    err = np.abs(got - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
    assert err.max() <= 1.0, (err.max(), np.unravel_index(err.argmax(), err.shape))
    return rows, w


def test_two_frames_and_the_largest_clip(harness, tmp_path, model):
    f2 = MC.two_frame_clip(model, 60.0)
    check_table(table(harness, tmp_path, f2), model, f2, MC.DT, False)
    check_table(table(harness, tmp_path, f2, loop=True), model, f2, MC.DT, True)
    big = MC.clip_frames(model, 4096, seed=1)
    rows, _ = check_table(table(harness, tmp_path, big, 0.01), model, big, 0.01, False)
    assert rows.shape == (4096, STRIDE)


def test_quaternions_are_normalised_into_one_hemisphere(harness, tmp_path, model):
    f = MC.clip_frames(model, 9, seed=2)
    g = f.copy()
    g[3, 3:7] *= -1.0                  # q, then -q of a nearby rotation ...
    g[4, 3:7] *= -3.5                  # ... and one that is neither unit nor on the same side
    g[7, 3:7] *= 0.25
    rows, _ = check_table(table(harness, tmp_path, g), model, g, MC.DT, False)
    plain = table(harness, tmp_path, f)["rows"].astype(np.float32).astype(np.float64).reshape(9, STRIDE)
    assert np.abs(rows - plain).max() <= 2.0 ** -22          # the same clip: signs and lengths do not reach the table
    quat = rows[:, 3:7]
    assert np.abs(np.linalg.norm(quat, axis=1) - 1).max() < 1e-6
    assert ((quat[1:] * quat[:-1]).sum(1) > 0).all()


def test_derived_against_supplied_velocities(harness, tmp_path, model):
    f = MC.clip_frames(model, 33, seed=3)
    rng = np.random.default_rng(0)
    vel = rng.normal(size=(33, 6 + J))
    rows, _ = check_table(table(harness, tmp_path, f, velocities=vel), model, f, MC.DT, False, vel)
    assert (rows[:, 7:13] == vel[:, :6].astype(np.float32)).all() and (rows[:, 13 + J:COLS] == vel[:, 6:].astype(np.float32)).all()
    derived, _ = check_table(table(harness, tmp_path, f), model, f, MC.DT, False)
    # the clip is smooth: central differences are its analytic rates to second order in frame_dt
    assert np.abs(derived[1:-1, 13 + J:COLS] - (f[2:, 7:] - f[:-2, 7:]) / (2 * MC.DT)).max() < 1e-4
    assert np.abs(derived[:, 7] - 0.8).max() < 1e-4          # the base walks along x at 0.8 m/s


def test_loop_and_open_ends_differ(harness, tmp_path, model):
    f = MC.clip_frames(model, 17, seed=4, cyclic=True)
    open_rows, _ = check_table(table(harness, tmp_path, f), model, f, MC.DT, False)
    loop_rows, w = check_table(table(harness, tmp_path, f, loop=True), model, f, MC.DT, True)
    assert (open_rows[1:-1] == loop_rows[1:-1]).all()
    assert not (open_rows[0, 13 + J:COLS] == loop_rows[0, 13 + J:COLS]).all()
    assert (loop_rows[0, 7:] == loop_rows[-1, 7:]).all()                 # frame F-1 is frame 0 of the next cycle
    assert abs(loop_rows[0, 7] - 0.8) < 1e-4 and abs(open_rows[0, 7] - 0.8) < 1e-4   # the displacement is carried over the wrap
    assert w["disp"][0] == np.float32(f[-1, 0] - f[0, 0])


def test_refusals(harness, tmp_path, model):
    f = MC.clip_frames(model, 5, seed=5)
    go = lambda frames, **kw: table(harness, tmp_path, frames, **kw)
    refused(go(f[:1]), "num_frames 1 outside [2, 4096]")
    refused(go(f[:0], F=4097), "num_frames 4097 outside [2, 4096]")
    refused(go(f[:0], F=-1), "num_frames -1 outside")
    for bad in (np.nan, np.inf):
        g = f.copy()
        g[2, 9] = bad
        refused(go(g), "frame 2: a value is not finite")
        v = np.zeros((5, 6 + J))
        v[4, 0] = bad
        refused(go(f, velocities=v), "frame 4: a velocity is not finite")
    g = f.copy()
    g[1, 3:7] = 0.0
    refused(go(g), "frame 1: a quaternion of norm 0")
    for dt in (0.0, -0.01, np.nan, np.inf, 1e-60):
        refused(go(f, frame_dt=dt), "frame_dt must be positive and finite")
    oo = model["obs_order"]
    g = f.copy()
    g[3, 7 + 6] = model["q_upper"][oo][6] + 2e-6
    refused(go(g), "frame 3: joint 6 outside its limits")
    g[3, 7 + 6] = model["q_upper"][oo][6] + 5e-7           # within the 1e-6 allowance
    assert not isinstance(go(g), tuple)
    g[0, 7 + J - 1] = model["q_lower"][oo][J - 1] - 2e-6
    refused(go(g), "frame 0: joint %d outside its limits" % (J - 1))
    assert go(f[:0])["scalars"].astype(int).tolist() == [0, 0, 0, 0, 0]      # 0 frames: the empty table


def test_terms(harness, tmp_path):
    spec = [(MR.POSE, 0, 0.65, 2.0, 0.0), (MR.VELOCITY, 1, 0.1, 0.1, 0.0), (MR.POSE, 1 << (J - 1), -1.0, 1e-3, 0.0),
            (MR.END_EFFECTOR, 0, 0.15, 40.0, 0.0), (MR.ROOT_POSE, 0, 0.1, 10.0, 0.0), (MR.ROOT_VELOCITY, 0, 0.0, 1.0, 2.5),
            (MR.POSE, 0x155, 1.0, 1.0, 0.0), (MR.VELOCITY, 0, 1.0, 1.0, 0.0)]                           # 8 terms
    t = terms(harness, tmp_path, spec)
    assert t["kind"].astype(int).tolist() == [s[0] for s in spec]
    assert t["mask"].astype(np.int64).tolist() == [s[1] if s[1] else (1 << J) - 1 for s in spec]      # 0 = all joints
    for k, col in (("weight", 2), ("scale", 3), ("aux", 4)):
        assert (t[k].astype(np.float32) == np.array([s[col] for s in spec], np.float32)).all()
    assert terms(harness, tmp_path, [])["kind"].size == 0
    go = lambda spec, **kw: terms(harness, tmp_path, spec, **kw)
    refused(go([spec[0]] * 9), "num_terms 9 outside [0, 8]")
    refused(go([spec[0], (MR.KINDS, 0, 1.0, 1.0, 0.0)]), "term 1: unknown kind 5")
    refused(go([(-1, 0, 1.0, 1.0, 0.0)]), "term 0: unknown kind -1")
    for scale in (0.0, -2.0):
        refused(go([(MR.POSE, 0, 1.0, scale, 0.0)]), "term 0: scale must be positive")
    refused(go([(MR.ROOT_POSE, 0, 1.0, 1.0, -0.5)]), "term 0: aux must not be negative")
    for bad in (np.nan, np.inf):
        refused(go([(MR.POSE, 0, bad, 1.0, 0.0)]), "term 0: weight, scale or aux is not finite")
        refused(go([(MR.POSE, 0, 1.0, bad, 0.0)]), "term 0: weight, scale or aux is not finite")
        refused(go([(MR.ROOT_POSE, 0, 1.0, 1.0, bad)]), "term 0: weight, scale or aux is not finite")
        refused(go([spec[0]], step_weight=bad), "step_weight is not finite")
    refused(go([(MR.VELOCITY, 1 << J, 1.0, 1.0, 0.0)]), "term 0: a mask bit at or beyond J = %d" % J)
    refused(go([spec[3]], has_probes=False), "term 0: END_EFFECTOR needs a clip set with a probe set")


@pytest.mark.parametrize("name", ["mount_first", "deep_chain"])
def test_table_on_generated_models(name, harness, tmp_path):
    """the recorded clip of tests/row_kernel_cases.py, with its velocities, on models of J = 4 and J = 6 whose joints sort differently
    from their bodies; on mount_first every joint has limits of its own, and a frame is refused by the limits of ITS joint"""
    import row_kernel_cases as RK
    import synthetic_models as sm
    path, props, om = sm.compile_both(name, tmp_path / "model")
    nj = om["nb"] - 1
    frames, vel = RK.clip(om, RK.oracle_of(name, om, RK.params_of(props)))
    go = lambda f, **kw: table(harness, tmp_path, f, frame_dt=RK.DT, urdf=path, **kw)
    rows, _ = check_table(go(frames, velocities=vel), om, frames, RK.DT, False, vel, J=nj)
    assert rows.shape == (RK.FRAMES, (13 + 2 * nj + 3) // 4 * 4)
    check_table(go(frames), om, frames, RK.DT, False, J=nj)
    if name == "mount_first":
        oo = om["obs_order"]
        lo, hi = om["q_lower"][oo], om["q_upper"][oo]
        wide, narrow = int(np.argmax(hi)), int(np.argmin(hi))
        g = frames.copy()
        g[2, 7 + wide] = hi[wide]                       # inside its own limits, outside every other joint's
        assert hi[wide] > np.delete(hi, wide).max() + 1e-3 and not isinstance(go(g), tuple)
        g = frames.copy()
        g[2, 7 + narrow] = hi[narrow] + 2e-6            # outside its own, inside every other joint's
        refused(go(g), "frame 2: joint %d outside its limits" % narrow)
        g[2, 7 + narrow] = lo[narrow]
        assert not isinstance(go(g), tuple)


@pytest.mark.parametrize("case", LC.MOTION, ids=lambda c: "n%d-T%d" % c)
def test_the_layouts_of_clocks_and_held_values(case, harness, tmp_path):
    n, T = case
    got = LC.run_layout(harness, tmp_path, n, T)
    LC.sound(got["clock"], n * 8)
    LC.sound(got["held"], n * T * 4)


def test_the_empty_held_values(harness, tmp_path):
    LC.sound(LC.run_layout(harness, tmp_path, 3, 0)["held"], 0)
