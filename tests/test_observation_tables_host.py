"""The channel table of the observation channels, on the CPU and under the sanitizers: build_obs_table of csrc/host_tables.cpp -
what trex_batch_set_observation hands the compose kernel - built with csrc/model.cpp into tests/host/observation_harness.cpp by
g++ -fsanitize=address,undefined (the flags of tests/test_host_tables.py; no HIP, nothing loaded into Python) and run as a child
process, one run per case. The table is compared with the numpy restatement observation_ref.obs_table: integers exactly, f32
values to one unit in the last place (the f64 sums may be ordered differently). No sanitizer report may appear."""
import os
import subprocess

import numpy as np
import pytest

import observation_ref as OR
from conftest import ASSET_URDF, ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID
J = 25


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("observation_tables") / "observation_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "observation_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def run(exe, tmp_path, spec, action_cols=J, urdf=ASSET_URDF):
    """-> {part: float64 array} of one harness run, or ('REFUSED', code, message)"""
    path = os.path.join(str(tmp_path), "numbers.txt")
    numbers = [action_cols, len(spec)] + [x for k, l, xyz, s in spec for x in [k, l] + list(xyz) + [s]]
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


def full_spec(model):
    """every kind; two channels on one body; a point on the deepest link; a merged link with a turned frame"""
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    tf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)
    toe = [l for l in range(len(names)) if "toe" in names[l]][0]
    deepest = [l for l in range(len(names)) if lb[l] == int(np.argmax(model["depth"]))][0]
    turned = [l for l in range(len(names)) if np.abs(tf[l][:9] - np.eye(3).reshape(-1)).max() > 1e-3][-1]
    z = (0.0, 0.0, 0.0)
    return [(OR.GRAVITY, 0, z, 1.0), (OR.BASE_LIN, 0, z, 0.5), (OR.BASE_ANG, 0, z, 0.25), (OR.BASE_HEIGHT, 0, z, 1.0),
            (OR.POINT_POS, toe, (0.1, -0.2, 0.3), 1.0), (OR.POINT_VEL, toe, (0.1, -0.2, 0.3), 2.0), (OR.POINT_HEIGHT, deepest, (0.05, 0.0, -0.02), 1.0),
            (OR.CONTACT, toe, z, 1e-3), (OR.PREV_ACTION, 0, z, 1.0), (OR.EXTERNAL, 5, z, 1.0), (OR.POINT_POS, turned, (1.5, 0.25, -0.75), -1.0),
            (OR.EXTERNAL, 2, z, 3.0)]


def check_table(t, model, spec, action_cols):
    w = OR.obs_table(model, spec, action_cols)
    C, E = len(spec), len(w["col_chan"])
    for k in ("kind", "body", "col0", "width"):
        assert t[k].astype(np.int64).tolist() == w[k].tolist(), k
    assert t["col_chan"].astype(np.int64).tolist() == w["col_chan"].tolist()
    up = lambda x: (x + 15) // 16 * 16
    kinds = [s[0] for s in spec]
    assert t["scalars"].astype(np.int64).tolist() == [C, E, w["extern_cols"], action_cols, int(OR.CONTACT in kinds), int(OR.PREV_ACTION in kinds),
                                                      w["body_mask"], up(80 * C), up(80 * C) + up(E)]
    assert (t["scale"].astype(np.float32) == w["scale"].astype(np.float32)).all()
    tf = t["tf"].reshape(C, 12)
    assert (tf.astype(np.float32) == w["tf"].astype(np.float32)).all()                 # the link frames: exactly
    assert ulps(t["point"].reshape(C, 3), w["point"]).max() <= 1.0                     # R x + t in f64, rounded: the last bit may differ


def test_table_of_every_kind(harness, tmp_path, model):
    spec = full_spec(model)
    t = run(harness, tmp_path, spec)
    check_table(t, model, spec, J)
    assert int(t["scalars"][1]) == 3 + 3 + 3 + 1 + 3 + 3 + 1 + 1 + J + 5 + 3 + 2
    assert t["body"].astype(int)[4] == t["body"].astype(int)[5] == t["body"].astype(int)[7] > 0     # three channels, one body
    assert t["body"].astype(int).tolist()[9] == 0 and t["body"].astype(int).tolist()[11] == 5          # the EXTERNAL source columns


def test_table_with_stiffness_actions(harness, tmp_path, model):
    """PREV_ACTION is as wide as the batch's action rows: 2J with stiffness actions"""
    spec = [(OR.PREV_ACTION, 0, (0, 0, 0), 1.0), (OR.GRAVITY, 0, (0, 0, 0), 1.0)]
    t = run(harness, tmp_path, spec, action_cols=2 * J)
    check_table(t, model, spec, 2 * J)
    assert t["col0"].astype(int).tolist() == [0, 2 * J]


def test_limits_are_reached_exactly(harness, tmp_path, model):
    z = (0, 0, 0)
    t = run(harness, tmp_path, [(OR.EXTERNAL, 512 - 3 * J, z, 1.0)])                  # 3J + E = 512
    assert int(t["scalars"][1]) == 512 - 3 * J
    spec = [(OR.BASE_HEIGHT, 0, z, 1.0)] * 64                                        # 64 channels
    check_table(run(harness, tmp_path, spec), model, spec, J)
    assert int(run(harness, tmp_path, [])["scalars"][0]) == 0                       # none: the empty table


def test_refusals(harness, tmp_path, model):
    z, nl = (0, 0, 0), len(model["link_names"])
    go = lambda spec: run(harness, tmp_path, spec)
    refused(go([(OR.GRAVITY, 0, z, 1.0), (OR.KINDS, 0, z, 1.0)]), "channel 1: unknown kind 10")
    refused(go([(-1, 0, z, 1.0)]), "channel 0: unknown kind -1")
    refused(go([(OR.POINT_POS, nl, z, 1.0)]), "channel 0: link %d out of range [0, %d)" % (nl, nl))
    refused(go([(OR.CONTACT, -1, z, 1.0)]), "channel 0: link -1 out of range")
    refused(go([(OR.POINT_VEL, 1, (0, np.nan, 0), 1.0)]), "channel 0: local_xyz is not finite")
    refused(go([(OR.POINT_HEIGHT, 1, (np.inf, 0, 0), 1.0)]), "channel 0: local_xyz is not finite")
    refused(go([(OR.GRAVITY, 0, z, np.nan)]), "channel 0: scale is not finite")
    refused(go([(OR.BASE_HEIGHT, 0, z, 1.0)] * 65), "num_channels 65 outside [0, 64]")
    refused(go([(OR.EXTERNAL, 513 - 3 * J, z, 1.0)]), "3J + E = 513 observation columns with channel 0, at most 512")
    refused(go([(OR.EXTERNAL, 512 - 3 * J, z, 1.0), (OR.BASE_HEIGHT, 0, z, 1.0)]), "3J + E = 513 observation columns with channel 1")
    refused(go([(OR.EXTERNAL, 2 ** 31 - 1, z, 1.0)]), "at most 512")
    refused(go([(OR.EXTERNAL, 0, z, 1.0)]), "channel 0: an EXTERNAL channel needs link = k >= 1 columns, got 0")


@pytest.mark.parametrize("name", ["mount_first", "deep_chain"])
def test_table_on_generated_models(name, harness, tmp_path):
    """the channels of tests/row_kernel_cases.py on a model whose URDF link 0 lies in body 2 behind a turned frame, and on one of
    J = 6: body, body-frame point and link frame of every channel, the body mask"""
    import row_kernel_cases as RK
    import synthetic_models as sm
    path, props, om = sm.compile_both(name, tmp_path / "model")
    nj = om["nb"] - 1
    spec = RK.obs_spec(om, RK.link_of_body(om, om["nb"] - 1))
    t = run(harness, tmp_path, spec, action_cols=nj, urdf=path)
    check_table(t, om, spec, nj)
    body = t["body"].astype(int)
    assert body[5] == body[6] == body[7] == int(om["link_body"][0]) == props.get("link0_body", 0)     # the channels on URDF link 0
    if name == "mount_first":
        assert np.abs(t["tf"].reshape(len(spec), 12)[5][:9] - np.eye(3).reshape(-1)).max() > 1e-2 and np.abs(t["point"].reshape(-1, 3)[5]).max() > 1e-2
