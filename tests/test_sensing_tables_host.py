"""The group table of the sensor model, on the CPU and under the sanitizers: build_sense_table and check_sense_delay of
csrc/host_tables.cpp - what trex_batch_set_sensing hands the kernel - built with csrc/model.cpp into tests/host/sensing_harness.cpp
by g++ -fsanitize=address,undefined (the flags of tests/test_motion_tables_host.py; no HIP, nothing loaded into Python) and run as
a child process, one run per case: every refusal include/trex_sensing.h lists, the column -> group map, the packing of the delayed
columns, the f32 inverse of the resolution. No sanitizer report may appear."""
import os
import subprocess

import numpy as np
import pytest

import layout_cases as LC
import sensing_cases as SC
from conftest import ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID
G, U = 0, 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sensing_tables") / "sensing_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "sensing_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def run_numbers(exe, tmp_path, numbers):
    path = os.path.join(str(tmp_path), "numbers.txt")
    with open(path, "w") as f:
        f.write(" ".join(repr(float(x)) for x in numbers))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    if r.stdout.startswith("REFUSED "):
        _, code, msg = r.stdout.rstrip("\n").split(" ", 2)
        return ("REFUSED", int(code), msg)
    return {line.split(" ", 1)[0]: np.array(line.split()[1:], np.float64) for line in r.stdout.splitlines()}


def table(exe, tmp_path, D, groups, count=None):
    return run_numbers(exe, tmp_path, [0, D, len(groups) if count is None else count] + [x for g in groups for x in g])


def refused(out, text):
    assert isinstance(out, tuple) and out[0] == "REFUSED", out
    assert out[1] == INVALID and text in out[2], out


def check(t, D, groups):
    n = len(groups)
    want_group, want_hist, packed = np.full(D, -1), np.full(D, -1), 0
    for g, (c0, w, *_rest) in enumerate(groups):
        want_group[c0:c0 + w] = g
    for c in range(D):
        if want_group[c] >= 0 and groups[want_group[c]][7] > 0:
            want_hist[c] = packed
            packed += 1
    assert t["scalars"].astype(int).tolist() == [n, D, packed, 40 * n, 40 * n + 2 * D, 40 * n + 4 * D]
    assert (t["col_group"] == want_group).all() and (t["col_hist"] == want_hist).all()
    for k, col in (("col0", 0), ("width", 1), ("kind", 2), ("delay_min", 6), ("delay_max", 7)):
        assert t[k].astype(int).tolist() == [g[col] for g in groups]
    for k, col in (("noise", 3), ("bias", 4), ("quantum", 5)):
        assert (t[k].astype(np.float32) == np.array([g[col] for g in groups], np.float32)).all()
    q = np.array([g[5] for g in groups], np.float32)
    inv = np.where(q > 0, (1.0 / np.where(q > 0, q, 1).astype(np.float64)).astype(np.float32), np.float32(0))
    assert (t["inv_quantum"].astype(np.float32) == inv).all()
    assert t["blob_is_parts"].tolist() == [1]
    return packed


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_the_tables_of_the_cases(case, harness, tmp_path):
    check(table(harness, tmp_path, case.D, case.groups), case.D, case.groups)


def test_map_and_packing(harness, tmp_path):
    """groups given out of column order, one straddling Philox blocks, delayed and undelayed ones interleaved: the history's
    columns are the delayed columns in COLUMN order, whatever the groups' order"""
    groups = [(40, 10, G, 0.1, 0.0, 0.0, 0, 3), (5, 7, U, 0.1, 0.2, 0.05, 0, 0), (12, 1, G, 0.0, 0.0, 0.0, 8, 8), (0, 5, G, 1.0, 0.0, 0.0, 1, 1),
              (74, 1, G, 0.0, 0.0, 0.0, 0, 1)]
    assert check(table(harness, tmp_path, 75, groups), 75, groups) == 10 + 1 + 5 + 1
    one = [(0, 512, G, 0.0, 0.0, 0.0, 0, 8)]
    assert check(table(harness, tmp_path, 512, one), 512, one) == 512
    empty = table(harness, tmp_path, 75, [])
    assert empty["scalars"].astype(int).tolist() == [0, 0, 0, 0, 0, 0] and empty["col_group"].size == 0      # 0 groups: the empty table


def test_refusals(harness, tmp_path):
    ok = (10, 5, G, 0.1, 0.1, 0.01, 0, 2)
    go = lambda groups, D=75, **kw: table(harness, tmp_path, D, groups, **kw)
    change = lambda **kw: tuple(kw.get(k, v) for k, v in zip("col0 width kind noise bias quantum dmin dmax".split(), ok))
    assert not isinstance(go([ok]), tuple)
    refused(go([], count=65), "num_groups 65 outside [0, 64]")
    refused(go([], count=-1), "num_groups -1 outside [0, 64]")
    refused(go([ok, (14, 3, G, 0.0, 0.0, 0.0, 0, 0)]), "group 1: column 14 is in group 0 already")          # overlap
    refused(go([ok, ok]), "group 1: column 10 is in group 0 already")
    refused(go([(12, 1, G, 0.0, 0.0, 0.0, 0, 0), ok]), "group 1: column 12 is in group 0 already")
    for c0, w in ((-1, 5), (75, 1), (70, 6), (0, 76), (0, 0), (3, -2), (2 ** 31 - 1, 2 ** 31 - 1)):
        refused(go([change(col0=c0, width=w)]), "group 0: columns [%d, %d) outside [0, 75)" % (c0, c0 + w))
    assert not isinstance(go([change(col0=70, width=5)]), tuple) and not isinstance(go([change(col0=0, width=75)]), tuple)
    for kind in (-1, 2):
        refused(go([change(kind=kind)]), "group 0: unknown noise_kind %d" % kind)
    for name in ("noise", "bias", "quantum"):
        for bad in (np.nan, np.inf, -np.inf):
            refused(go([change(**{name: bad})]), "group 0: noise, bias or quantum is not finite")
        refused(go([change(**{name: -1e-3})]), "group 0: noise, bias or quantum is negative")
    refused(go([change(quantum=1e-40)]), "group 0: the inverse of quantum is not finite in f32")
    for lo, hi in ((-1, 0), (0, 9), (3, 2), (9, 9)):
        refused(go([change(dmin=lo, dmax=hi)]), "group 0: delays [%d, %d] outside 0 <= delay_min <= delay_max <= 8" % (lo, hi))
    assert not isinstance(go([change(dmin=8, dmax=8)]), tuple)
    refused(go([ok], D=0), "the observation dimension 0 is outside [1, 512]")
    refused(go([ok], D=513), "the observation dimension 513 is outside [1, 512]")
    for lo, hi in ((-1, 0), (0, 9), (3, 2)):
        refused(run_numbers(harness, tmp_path, [1, lo, hi]), "trex_batch_set_action_delay: delays [%d, %d] outside" % (lo, hi))
    assert run_numbers(harness, tmp_path, [1, 0, 8])["ok"].tolist() == [1]


@pytest.mark.parametrize("case", LC.SENSING, ids=lambda c: "n%d-G%d-delayed%d-act%d-cols%d" % c)
def test_the_layouts_of_counters_and_histories(case, harness, tmp_path):
    got = LC.run_layout(harness, tmp_path, *case)
    for line, size in LC.sensing_bytes(*case).items():
        LC.sound(got[line], size)


def test_the_empty_counters(harness, tmp_path):
    got = LC.run_layout(harness, tmp_path, 3, 0, 0, 0, 25)
    for line in ("counters", "hist", "act_counters", "act_hist"):
        LC.sound(got[line], 0)
