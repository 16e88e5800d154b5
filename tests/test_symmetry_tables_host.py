"""The mirror tables on the CPU and under the sanitizers: build_model_mirror, build_mirror_row_table, the action and command tables,
build_mirror_words and the checks of the two row launches (csrc/host_tables.cpp) - built with csrc/model.cpp into
tests/host/symmetry_harness.cpp by g++ -fsanitize=address,undefined (the flags of tests/test_host_tables.py; no HIP, nothing loaded
into Python) and run as a child process, one run per case. The tables are compared with the numpy restatement tests/symmetry_ref.py:
integers and signs exactly, on the T-rex and on the generated bipeds; every refusal of include/trex_symmetry.h that is decided on the
host is hit. No sanitizer report may appear."""
import os
import subprocess

import numpy as np
import pytest

import symmetry_models as SM
import symmetry_ref as R
from conftest import ASSET_URDF, ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("symmetry_tables") / "symmetry_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "symmetry_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def run(exe, tmp_path, mode, numbers, urdf=None):
    """-> ({part: float64 array}, refusal): refusal None or (code, message); the parts printed before a refusal are kept"""
    path = os.path.join(str(tmp_path), "numbers.txt")
    with open(path, "w") as f:
        f.write(" ".join(repr(float(x)) for x in numbers))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, mode, path] + ([urdf] if urdf else []), env=env, capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    parts, refusal = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("REFUSED "):
            _, code, msg = line.split(" ", 2)
            refusal = (int(code), msg)
        else:
            parts[line.split(" ", 1)[0]] = np.array(line.split()[1:], np.float64)
    return parts, refusal


def refused(out, text):
    assert out[1] is not None and out[1][0] == INVALID and text in out[1][1], out


def model_numbers(lateral, tol, action_cols, tail, chans, es=(), eg=()):
    return [lateral, tol, action_cols, tail, len(chans)] + [x for k, l, xyz, s in chans for x in [k, l] + list(xyz) + [s]] + \
        [len(es)] + list(es) + list(eg)


def same_tables(parts, model, mm, chans, action_cols, tail, es=None, eg=None):
    assert int(parts["lateral"][0]) == mm["lateral"]
    for name in ("pair", "sign", "body_pair"):
        assert parts[name].tolist() == mm[name].tolist(), name
    assert np.abs(parts["residual"] - np.array(list(mm["residual"].values()))).max() < 1e-12
    for stiff, tag in ((False, "action"), (True, "action2")):
        src, sign = R.action_table(mm["pair"], mm["sign"], stiff)
        assert parts[tag + "_src"].tolist() == src.tolist() and parts[tag + "_sign"].tolist() == sign.tolist()
    src, sign = R.command_table(mm["lateral"])
    assert parts["command_src"].tolist() == src.tolist() and parts["command_sign"].tolist() == sign.tolist()
    src, sign = R.row_table(model, mm, chans, action_cols, tail, extern_src=es, extern_sign=eg)
    assert parts["row_src"].tolist() == src.tolist() and parts["row_sign"].tolist() == sign.tolist()
    assert R.check_table(src, sign)


@pytest.fixture(scope="module")
def bipeds(tmp_path_factory):
    return {lat: SM.compile_biped(tmp_path_factory.mktemp("biped%d" % lat), lat) for lat in (0, 1)}


@pytest.mark.parametrize("lateral", [0, 1])
def test_the_tables_of_the_generated_bipeds(harness, tmp_path, bipeds, lateral):
    path, props, model = bipeds[lateral]
    mm = R.model_table(model)
    chans = SM.locomotion_channels(model, lateral) + [(R.PREV_ACTION, 0, (0, 0, 0), 1.0), (R.EXTERNAL, 2, (0, 0, 0), 1.0), (R.EXTERNAL, 1, (0, 0, 0), 1.0)]
    es, eg = [2, 1, 0], [1, -1, 1]
    for search in (-1, lateral):
        for A, tail in ((SM.NJ, 2), (2 * SM.NJ, 5)):
            parts, refusal = run(harness, tmp_path, "model", model_numbers(search, 5e-3, A, tail, chans, es, eg), path)
            assert refusal is None, refusal
            same_tables(parts, model, mm, chans, A, tail, es, eg)
    assert parts["pair"].tolist() == SM.PAIR and parts["sign"].tolist() == SM.SIGN and (parts["residual"] == 0).all()


def trex_feet(model):
    names = model["link_names"]
    return [names.index(n) for n in names if "toe_03_c" in n]


def test_the_tables_of_the_trex(harness, tmp_path):
    from oracle import trex_model as tm
    model = tm.compile_model(ASSET_URDF)
    mm = R.model_table(model)
    left, right = trex_feet(model)
    chans = [(R.PROJECTED_GRAVITY, 0, (0, 0, 0), 1.0), (R.BASE_LINEAR_VELOCITY, 0, (0, 0, 0), 1.0), (R.BASE_ANGULAR_VELOCITY, 0, (0, 0, 0), 1.0),
             (R.BASE_HEIGHT, 0, (0, 0, 0), 1.0), (R.CONTACT_FORCE, left, (0, 0, 0), 1.0), (R.POINT_POSITION, left, (0, 0, 0), 1.0),
             (R.CONTACT_FORCE, right, (0, 0, 0), 1.0), (R.POINT_POSITION, right, (0, 0, 0), 1.0)]
    parts, refusal = run(harness, tmp_path, "model", model_numbers(-1, 5e-3, 25, 2, chans), ASSET_URDF)
    assert refusal is None, refusal
    same_tables(parts, model, mm, chans, 25, 2)
    assert len(parts["row_src"]) == 75 + 18 + 2
    # (the asset's asymmetry is reported, not refused: the residuals were compared with the reference's above)
    assert (parts["residual"] > 0).all()


def test_the_model_refusals(harness, tmp_path, bipeds):
    path, props, model = bipeds[0]
    chans = SM.locomotion_channels(model, 0)
    ok = lambda **kw: model_numbers(kw.get("lateral", 0), kw.get("tol", 5e-3), kw.get("A", SM.NJ), kw.get("tail", 2), kw.get("chans", chans),
                                    kw.get("es", ()), kw.get("eg", ()))
    refused(run(harness, tmp_path, "model", ok(lateral=1), path), "has no partner within tol_pos")
    refused(run(harness, tmp_path, "model", ok(lateral=3), path), "is none of -1, 0, 1, 2")
    refused(run(harness, tmp_path, "model", ok(tol=-1.0), path), "tol_pos is negative or not finite")
    refused(run(harness, tmp_path, "model", ok(tol=float("nan")), path), "tol_pos is negative or not finite")
    refused(run(harness, tmp_path, "model", ok(A=SM.NJ + 1), path), "is neither J nor 2 J")
    refused(run(harness, tmp_path, "model", ok(tail=3), path), "is neither 2 nor 5")
    # a probe whose partner is not its image; a contact channel without the other foot's; an unknown kind; a link out of range
    moved = [(k, l, (xyz[0] + 0.05, xyz[1], xyz[2]) if k == R.POINT_POSITION and j > 6 else xyz, s) for j, (k, l, xyz, s) in enumerate(chans)]
    out = run(harness, tmp_path, "model", ok(chans=moved), path)
    refused(out, "has no mirrored channel in the specification")
    assert "channel 5 " in out[1][1] and "pair" in out[0]          # (the model table was built; the row table names the channel)
    refused(run(harness, tmp_path, "model", ok(chans=chans[:8]), path), "channel 4 has no mirrored channel")
    refused(run(harness, tmp_path, "model", ok(chans=chans + [(10, 0, (0, 0, 0), 1.0)]), path), "unknown kind 10")
    refused(run(harness, tmp_path, "model", ok(chans=chans + [(R.POINT_HEIGHT, 99, (0, 0, 0), 1.0)]), path), "link 99 out of range")
    ext = chans + [(R.EXTERNAL, 2, (0, 0, 0), 1.0)]
    refused(run(harness, tmp_path, "model", ok(chans=ext), path), "needs extern_src and extern_sign")
    refused(run(harness, tmp_path, "model", ok(chans=ext, es=(0, 0), eg=(1, 1)), path), "extern_src is no permutation")
    refused(run(harness, tmp_path, "model", ok(chans=ext, es=(1, 0), eg=(1, 0)), path), "a sign is neither +1 nor -1")
    refused(run(harness, tmp_path, "model", ok(chans=chans + [(R.EXTERNAL, 600, (0, 0, 0), 1.0)], es=range(600), eg=[1] * 600), path), "the row is wider than 517")
    # limits that are not mirrored: the same biped with one limit moved, written next to the good one
    text = open(path).read().replace("lower='-0.9' upper='0.7'", "lower='-0.9' upper='0.75'", 1)
    bad = os.path.join(os.path.dirname(path), "bad_limits.urdf")
    open(bad, "w").write(text)
    refused(run(harness, tmp_path, "model", ok(), bad), "differ by more than tol_pos")
    # a joint moved off its image by more than tol_pos
    text = open(path).read().replace("xyz='0.13 0.02 -0.07'", "xyz='0.13 0.03 -0.07'", 1)
    assert text != open(path).read()
    open(bad, "w").write(text)
    refused(run(harness, tmp_path, "model", ok(), bad), "has no partner within tol_pos")
    refused(run(harness, tmp_path, "model", ok(lateral=-1), bad), "no axis of link 0 is normal to a mirror plane")


def test_table_words_and_their_refusals(harness, tmp_path):
    rng = np.random.default_rng(1)
    for W in (1, 2, 93, 517):
        src = rng.permutation(W)
        sign = rng.choice([-1, 1], W)
        parts, refusal = run(harness, tmp_path, "words", [W] + src.tolist() + sign.tolist())
        assert refusal is None
        assert parts["word"].tolist() == (src + (sign < 0) * 2 ** 31).tolist()
        assert int(parts["involution"][0]) == int(R.check_table(src, sign))
    parts, _ = run(harness, tmp_path, "words", [4, 1, 0, 3, 2, -1, -1, 1, 1])
    assert int(parts["involution"][0]) == 1
    parts, _ = run(harness, tmp_path, "words", [4, 1, 0, 3, 2, -1, 1, 1, 1])       # a pair with two signs: no involution
    assert int(parts["involution"][0]) == 0
    refused(run(harness, tmp_path, "words", [0]), "width 0 outside [1, 517]")
    refused(run(harness, tmp_path, "words", [518] + list(range(518)) + [1] * 518), "width 518 outside [1, 517]")
    refused(run(harness, tmp_path, "words", [3, 0, 1, 1, 1, 1, 1]), "column 2: src 1 is named twice")
    refused(run(harness, tmp_path, "words", [3, 0, 1, 3, 1, 1, 1]), "column 2: src 3 outside [0, width)")
    refused(run(harness, tmp_path, "words", [3, 0, 1, -1, 1, 1, 1]), "column 2: src -1 outside [0, width)")
    refused(run(harness, tmp_path, "words", [3, 0, 1, 2, 1, 0, 1]), "column 1: sign 0 is neither +1 nor -1")


def test_the_checks_of_the_row_launches(harness, tmp_path):
    rows = lambda *a: run(harness, tmp_path, "rows", a)
    # table_width in_offset in_stride out_offset out_stride n width
    assert rows(93, 0, 93, 20000, 93, 64, 93)[1] is None
    assert rows(93, 0, 96, 0, 96, 64, 93)[1] is None                      # in place
    assert rows(93, 0, 96, 64 * 96, 93, 64, 93)[1] is None                # back to back: the last in row ends at its width
    refused(rows(93, -1, 93, 0, 93, 4, 93), "null argument")
    refused(rows(93, 0, 93, -1, 93, 4, 93), "null argument")
    refused(rows(93, 0, 93, 20000, 93, 0, 93), "n 0 below 1")
    refused(rows(93, 0, 93, 20000, 93, 4, 75), "width 75 is not the table's 93")
    refused(rows(93, 0, 92, 20000, 93, 4, 93), "a stride below the width")
    refused(rows(93, 0, 93, 20000, 92, 4, 93), "a stride below the width")
    refused(rows(93, 0, 96, 0, 93, 4, 93), "in and out overlap")          # the same base with other strides
    refused(rows(93, 0, 96, 3, 96, 4, 93), "in and out overlap")
    refused(rows(93, 0, 96, 63 * 96 + 92, 96, 64, 93), "in and out overlap")
    refused(rows(2, 0, 2 ** 20, 1, 2 ** 20, 2 ** 11, 2), "n x stride is beyond 2^31")
    aug = lambda *a: run(harness, tmp_path, "augment", a)
    # obs_width act_width critic_width has_critic_table buffers obs_v num_samples D A Dv
    assert aug(93, 25, 0, 0, 1, 0, 5120, 93, 25, 0)[1] is None
    assert aug(93, 25, 96, 1, 1, 1, 5120, 93, 25, 96)[1] is None
    refused(aug(93, 25, 0, 0, 0, 0, 5120, 93, 25, 0), "null argument")
    refused(aug(93, 25, 96, 1, 1, 0, 5120, 93, 25, 96), "go together")
    refused(aug(93, 25, 0, 0, 1, 1, 5120, 93, 25, 0), "go together")
    refused(aug(93, 25, 0, 0, 1, 0, 5120, 93, 25, 96), "go together")
    refused(aug(93, 25, 0, 0, 1, 0, 0, 93, 25, 0), "num_samples 0 below 1")
    refused(aug(93, 25, 0, 0, 1, 0, 5120, 75, 25, 0), "D 75 is not the obs table's width 93")
    refused(aug(93, 25, 0, 0, 1, 0, 5120, 93, 50, 0), "A 50 is not the act table's width 25")
    refused(aug(93, 25, 96, 1, 1, 1, 5120, 93, 25, 95), "Dv 95 is not the critic table's width 96")
    refused(aug(93, 25, 0, 0, 1, 0, 2 ** 30 // 93, 93, 25, 0), "beyond 2^31")
    assert aug(93, 25, 0, 0, 1, 0, 2 ** 30 // 93 - 1, 93, 25, 0)[1] is None
