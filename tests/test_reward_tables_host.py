"""The term table of the reward terms, on the CPU and under the sanitizers: build_reward_table of csrc/host_tables.cpp - what
trex_batch_set_reward hands the reward kernel - built with csrc/model.cpp into tests/host/reward_harness.cpp by
g++ -fsanitize=address,undefined (the flags of tests/test_observation_tables_host.py; no HIP, nothing loaded into Python) and run
as a child process, one run per case. The table is compared with the numpy restatement reward_ref.reward_table: integers exactly,
f32 values to one unit in the last place (the f64 sums may be ordered differently). No sanitizer report may appear."""
import os
import subprocess

import numpy as np
import pytest

import layout_cases as LC
import reward_ref as RR
from conftest import ASSET_URDF, ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID
J, NB = 25, 26
Z = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reward_tables") / "reward_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "reward_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def run(exe, tmp_path, spec, action_cols=J, urdf=ASSET_URDF):
    """-> {part: float64 array} of one harness run, or ('REFUSED', code, message)"""
    path = os.path.join(str(tmp_path), "numbers.txt")
    numbers = [action_cols, len(spec)] + [x for k, l, m, xyz, w, p0, p1 in spec for x in [k, l, m] + list(xyz) + [w, p0, p1]]
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


def refused(out, text):
    assert isinstance(out, tuple) and out[0] == "REFUSED", out
    assert out[1] == INVALID and text in out[2], out


def ulps(got, want64):
    want = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def term(kind, weight=1.0, link=0, mask=0, xyz=Z, p0=0.0, p1=0.0):
    return (kind, link, mask, xyz, weight, p0, p1)


def full_spec(model):
    """every kind; two terms on one body; a point on a merged link with a turned frame; masks of one joint, the last joint, all"""
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    tf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)
    toe = [l for l in range(len(names)) if "toe" in names[l]][0]
    turned = [l for l in range(len(names)) if np.abs(tf[l][:9] - np.eye(3).reshape(-1)).max() > 1e-3][-1]
    return [term(RR.STEP, 0.5), term(RR.ALIVE, 2.0), term(RR.TRACK_LIN, p0=0.25), term(RR.TRACK_ANG, 0.5, p0=1e-3), term(RR.LIN_VEL_Z, -2.0),
            term(RR.ANG_VEL_XY, -0.05), term(RR.ORIENTATION, -1.0), term(RR.BASE_HEIGHT, -1.0, p0=0.6),
            term(RR.POINT_HEIGHT, 1.0, link=turned, xyz=(1.5, 0.25, -0.75), p0=0.1), term(RR.TORQUE, -1e-4), term(RR.JOINT_VEL, -1e-3, mask=1),
            term(RR.JOINT_ACC, -2.5e-7, mask=1 << (J - 1)), term(RR.ACTION_RATE, -0.01), term(RR.JOINT_LIMIT, -1.0, p0=1.0),
            term(RR.POWER, -1e-3, mask=0x155), term(RR.JOINT_POSE, -0.1), term(RR.CONTACT_COUNT, -1.0, mask=(1 << NB) - 2, p0=1.0),
            term(RR.FOOT_AIR_TIME, 1.0, link=toe, p0=1.0, p1=0.3), term(RR.FOOT_SLIP, -0.1, link=toe, xyz=(0.1, -0.2, 0.3), p0=-1.0)]


def check_table(t, model, spec, action_cols):
    w = RR.reward_table(model, spec)
    T = len(spec)
    for k in ("kind", "body", "mask", "joint_body"):
        assert t[k].astype(np.int64).tolist() == w[k].tolist(), k
    up = lambda x: (x + 15) // 16 * 16
    assert t["scalars"].astype(np.int64).tolist() == [T, action_cols, int(w["contact"]), int(w["actions"]), int(w["command"]),
                                                      w["body_mask"], up(96 * T), up(96 * T) + 128]
    for k in ("weight", "p0", "p1"):
        assert (t[k].astype(np.float32) == w[k].astype(np.float32)).all(), k
    assert (t["tf"].reshape(T, 12).astype(np.float32) == w["tf"].astype(np.float32)).all()     # the link frames: exactly
    assert ulps(t["point"].reshape(T, 3), w["point"]).max() <= 1.0                       # R x + t in f64, rounded: the last bit may differ


def test_table_of_every_kind(harness, tmp_path, model):
    spec = full_spec(model)
    assert sorted(s[0] for s in spec) == list(range(RR.KINDS))
    t = run(harness, tmp_path, spec)
    check_table(t, model, spec, J)
    body = t["body"].astype(int)
    assert body[17] == body[18] > 0 and body[8] > 0 and (body[:8] == 0).all()
    assert int(t["scalars"][5]) == (1 << body[8]) | (1 << body[18])                      # FOOT_AIR_TIME walks no chain
    assert t["mask"].astype(np.int64)[9] == (1 << J) - 1                                 # 0 = all joints


def test_flags_and_action_width(harness, tmp_path, model):
    spec = [term(RR.ACTION_RATE), term(RR.TORQUE)]
    t = run(harness, tmp_path, spec, action_cols=2 * J)
    check_table(t, model, spec, 2 * J)
    assert t["scalars"].astype(int).tolist()[1:5] == [2 * J, 0, 1, 0]
    t = run(harness, tmp_path, [term(RR.ALIVE)])
    assert t["scalars"].astype(int).tolist()[2:6] == [0, 0, 0, 0]


def test_limits_are_reached_exactly(harness, tmp_path, model):
    spec = [term(RR.JOINT_VEL, mask=1 << (k % J)) for k in range(32)]                    # 32 terms
    check_table(run(harness, tmp_path, spec), model, spec, J)
    spec = [term(RR.JOINT_LIMIT, p0=1.0, mask=1 << (J - 1)), term(RR.CONTACT_COUNT, mask=1 << (NB - 1)), term(RR.JOINT_LIMIT, p0=1e-6)]
    check_table(run(harness, tmp_path, spec), model, spec, J)
    assert int(run(harness, tmp_path, [])["scalars"][0]) == 0                           # none: the empty table


def test_refusals(harness, tmp_path, model):
    nl = len(model["link_names"])
    go = lambda spec: run(harness, tmp_path, spec)
    refused(go([term(RR.ALIVE), term(RR.KINDS)]), "term 1: unknown kind 19")
    refused(go([term(-1)]), "term 0: unknown kind -1")
    for kind in (RR.POINT_HEIGHT, RR.FOOT_AIR_TIME, RR.FOOT_SLIP):
        refused(go([term(kind, link=nl)]), "term 0: link %d out of range [0, %d)" % (nl, nl))
        refused(go([term(kind, link=-1)]), "term 0: link -1 out of range")
    refused(go([term(RR.ALIVE, np.nan)]), "term 0: weight, p0 or p1 is not finite")
    refused(go([term(RR.ALIVE, np.inf)]), "term 0: weight, p0 or p1 is not finite")
    refused(go([term(RR.BASE_HEIGHT, p0=np.nan)]), "term 0: weight, p0 or p1 is not finite")
    refused(go([term(RR.FOOT_AIR_TIME, link=1, p1=-np.inf)]), "term 0: weight, p0 or p1 is not finite")
    refused(go([term(RR.FOOT_SLIP, link=1, xyz=(0, np.nan, 0))]), "term 0: local_xyz is not finite")
    refused(go([term(RR.STEP, xyz=(np.inf, 0, 0))]), "term 0: local_xyz is not finite")
    for kind in (RR.TRACK_LIN, RR.TRACK_ANG):
        refused(go([term(kind, p0=0.0)]), "term 0: a tracking term needs p0 > 0")
        refused(go([term(kind, p0=-0.25)]), "term 0: a tracking term needs p0 > 0")
    for p0 in (0.0, -0.5, 1.0 + 2.0 ** -20):
        refused(go([term(RR.JOINT_LIMIT, p0=p0)]), "term 0: JOINT_LIMIT needs 0 < p0 <= 1")
    for kind in RR.JOINT_SUMS:
        refused(go([term(kind, mask=1 << J, p0=0.5)]), "term 0: a mask bit at or beyond J = %d" % J)
    refused(go([term(RR.TORQUE, mask=1 << 31)]), "a mask bit at or beyond J")
    refused(go([term(RR.CONTACT_COUNT, mask=1 << NB)]), "term 0: a mask bit at or beyond the body count %d" % NB)
    refused(go([term(RR.ALIVE)] * 33), "num_terms 33 outside [0, 32]")


@pytest.mark.parametrize("name", ["mount_first", "deep_chain"])
def test_table_on_generated_models(name, harness, tmp_path):
    """the 32 terms of tests/row_kernel_cases.py on a model whose URDF link 0 lies in body 2 and whose joints sort differently from
    its bodies, and on one of J = 6: body, body-frame point, masks, and joint_body = the observation order, zero past J"""
    import row_kernel_cases as RK
    import synthetic_models as sm
    path, props, om = sm.compile_both(name, tmp_path / "model")
    nj = om["nb"] - 1
    spec = RK.reward_spec(om, RK.link_of_body(om, om["nb"] - 1))
    t = run(harness, tmp_path, spec, action_cols=nj, urdf=path)
    check_table(t, om, spec, nj)
    jb = t["joint_body"].astype(int)
    assert jb[:nj].tolist() == list(om["obs_order"]) != sorted(om["obs_order"]) and (jb[nj:] == 0).all()
    assert t["mask"].astype(np.int64)[9] == (1 << nj) - 1


@pytest.mark.parametrize("case", LC.REWARD, ids=lambda c: "n%d-A%d-J%d-T%d" % c)
def test_the_layout_of_the_history(case, harness, tmp_path):
    LC.sound(LC.run_layout(harness, tmp_path, *case)["layout"], LC.reward_bytes(*case))


def test_the_empty_history(harness, tmp_path):
    LC.sound(LC.run_layout(harness, tmp_path, 3, 25, 25, 0)["layout"], 0)
