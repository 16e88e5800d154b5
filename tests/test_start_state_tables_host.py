"""The term table of the start-state randomisation, on the CPU and under the sanitizers: build_start_table, check_start_apply and
start_state_layout of csrc/host_tables.cpp - what trex_batch_set_start_state and trex_batch_apply_start_state check and hand the
kernel - built with csrc/model.cpp into tests/host/start_state_harness.cpp by g++ -fsanitize=address,undefined (the flags of
tests/test_randomize_tables_host.py; no HIP, nothing loaded into Python) and run as a child process, one run per case: every
refusal include/trex_start_state.h lists, the table's layout - joint masks of 0 expanded to the model's joints, the single-element
kinds, the rotation flag and the clearance term - and set, replace, clear. No sanitizer report may appear."""
import os
import subprocess

import numpy as np
import pytest

import layout_cases as LC
from conftest import ROOT
from start_state_ref import (BASE_ANGULAR_VELOCITY, BASE_LINEAR_VELOCITY, BASE_POSITION, BASE_RPY, FLOOR_CLEARANCE, JOINT_POSITION,
                             JOINT_VELOCITY)

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("start_state_tables") / "start_state_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "start_state_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def run(exe, tmp_path, numbers, mode=None):
    path = os.path.join(str(tmp_path), "numbers.txt")
    with open(path, "w") as f:
        f.write(" ".join(repr(float(x)) for x in numbers))
    r = subprocess.run([exe] + ([mode] if mode else []) + [path], env=ENV, capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    if r.stdout.startswith("REFUSED "):
        _, code, msg = r.stdout.rstrip("\n").split(" ", 2)
        return ("REFUSED", int(code), msg)
    return {line.split(" ", 1)[0]: np.array(line.split()[1:], np.float64) for line in r.stdout.splitlines()}


def table(exe, tmp_path, nj, terms, count=None, n=4, env_offset=0):
    return run(exe, tmp_path, [nj, n, env_offset, len(terms) if count is None else count] + [x for t in terms for x in t])


def refused(out, text):
    assert isinstance(out, tuple) and out[0] == "REFUSED", out
    assert out[1] == INVALID and text in out[2], out


def check(t, nj, terms):
    kinds = [x[0] for x in terms]
    clearance = kinds.index(FLOOR_CLEARANCE) if FLOOR_CLEARANCE in kinds else -1
    assert t["scalars"].astype(int).tolist() == [len(terms), int(BASE_RPY in kinds), clearance, 24, 16 * 24 + 16]
    want_mask, want_shared, want_index = [], [], []
    for kind, mask, index, shared, *_ in terms:
        joint = kind in (JOINT_POSITION, JOINT_VELOCITY)
        want_mask.append((mask or (1 << nj) - 1) if joint else 1)
        want_shared.append(int(shared != 0) if joint else 1)
        want_index.append(0 if joint or kind == FLOOR_CLEARANCE else index)
    assert t["kind"].astype(int).tolist() == kinds and t["mask"].astype(np.int64).tolist() == want_mask
    assert t["shared"].astype(int).tolist() == want_shared and t["index"].astype(int).tolist() == want_index
    for k, col in (("lo", 4), ("hi", 5)):
        assert (t[k].astype(np.float32) == np.array([x[col] for x in terms], np.float32)).all()


FULL = [(JOINT_POSITION, 0, 9, 7, -0.2, 0.2), (JOINT_VELOCITY, 0b110, 0, 0, -1.0, 1.0), (JOINT_VELOCITY, 1 << 24, 0, 1, 0.5, 0.5),
        (BASE_RPY, 5, 0, 0, -0.1, 0.1), (BASE_RPY, 0, 2, 0, -3.0, 3.0), (BASE_LINEAR_VELOCITY, 0, 1, 0, -0.5, 0.5),
        (BASE_ANGULAR_VELOCITY, 0, 2, 3, -0.5, 0.5), (BASE_POSITION, 0, 0, 0, -1.0, 1.0), (FLOOR_CLEARANCE, 9, 5, 0, 0.01, 0.05)]


def test_layout_of_the_table(harness, tmp_path):
    check(table(harness, tmp_path, 25, FULL), 25, FULL)
    no_rotation = [t for t in FULL if t[0] not in (BASE_RPY, FLOOR_CLEARANCE)]
    check(table(harness, tmp_path, 25, no_rotation), 25, no_rotation)
    one = [(JOINT_POSITION, 0, 0, 0, 0.0, 0.0)]
    check(table(harness, tmp_path, 1, one), 1, one)
    sixteen = [(JOINT_POSITION, 1 << i, 0, 0, -0.1, 0.1) for i in range(16)]
    check(table(harness, tmp_path, 25, sixteen), 25, sixteen)


def test_set_replace_clear(harness, tmp_path):
    """what a set builds does not depend on what was set before: a table, another one, the empty one"""
    check(table(harness, tmp_path, 25, FULL), 25, FULL)
    check(table(harness, tmp_path, 25, FULL[:2]), 25, FULL[:2])
    empty = table(harness, tmp_path, 25, [])
    assert empty["scalars"].astype(int).tolist()[:3] == [0, 0, -1] and empty["kind"].size == 0


def test_refusals(harness, tmp_path):
    go = lambda terms, nj=25, **kw: table(harness, tmp_path, nj, terms, **kw)
    jp = (JOINT_POSITION, 0b1111, 0, 0, -0.1, 0.1)
    rpy = (BASE_RPY, 0, 1, 0, -0.1, 0.1)
    fc = (FLOOR_CLEARANCE, 0, 0, 0, 0.0, 0.1)
    names = "kind mask index shared lo hi".split()
    change = lambda base, **kw: tuple(kw.get(k, v) for k, v in zip(names, base))
    assert not isinstance(go([jp, rpy, fc]), tuple)
    refused(go([], count=17), "num_terms 17 outside [0, 16]")                                   # more than 16 terms
    refused(go([], count=-1), "num_terms -1 outside [0, 16]")
    for kind in (-1, 7):
        refused(go([change(jp, kind=kind)]), "term 0: unknown kind %d" % kind)                  # an unknown kind
    for base in (jp, rpy, fc):
        refused(go([change(base, lo=1.2)]), "term 0: lo > hi")                                  # lo > hi
        for name in ("lo", "hi"):
            for bad in (np.nan, np.inf, -np.inf):
                refused(go([change(base, **{name: bad})]), "term 0: lo or hi is not finite")    # a non-finite bound
    for kind in (JOINT_POSITION, JOINT_VELOCITY):
        refused(go([change(jp, kind=kind, mask=1 << 25)]), "term 0: a mask bit beyond the model's 25 joints")    # a mask bit beyond the joints
        assert not isinstance(go([change(jp, kind=kind, mask=1 << 24)]), tuple)
    refused(go([change(jp, mask=0b10)], nj=1), "a mask bit beyond the model's 1 joints")
    refused(go([jp, change(jp, mask=0b1000)]), "term 1: overlaps an earlier term of its kind")  # overlapping masks of one kind
    refused(go([jp, change(jp, mask=0)]), "term 1: overlaps an earlier term of its kind")       # (0 is all)
    assert not isinstance(go([jp, change(jp, mask=0b10000)]), tuple)
    assert not isinstance(go([jp, change(jp, kind=JOINT_VELOCITY)]), tuple)                     # (another kind: no overlap)
    for kind in (BASE_RPY, BASE_LINEAR_VELOCITY, BASE_ANGULAR_VELOCITY, BASE_POSITION):
        refused(go([change(rpy, kind=kind), change(rpy, kind=kind)]), "term 1: overlaps an earlier term of its kind")   # the same index twice
        assert not isinstance(go([change(rpy, kind=kind, index=i) for i in range(3)]), tuple)
        for index in (-1, 3):
            refused(go([change(rpy, kind=kind, index=index)]), "term 0: index %d outside [0, 2]" % index)   # an index out of range
    refused(go([fc, jp, fc]), "term 2: a second FLOOR_CLEARANCE term")                          # two FLOOR_CLEARANCE terms
    refused(go([jp], n=4, env_offset=2 ** 32 - 3), "env_offset + N is beyond 2^32")             # env_offset + N beyond 2^32
    assert not isinstance(go([jp], n=4, env_offset=2 ** 32 - 4), tuple)


def test_apply_refusals(harness, tmp_path):
    go = lambda *numbers: run(harness, tmp_path, numbers, "apply")     # num_terms done done_stride rows row_stride nj pen_in_rows
    assert "OK" in go(3, 1, 1, 0, 0, 25, 0) and "OK" in go(3, 1, 77, 1, 77, 25, 0) and "OK" in go(1, 1, 80, 1, 80, 25, 1)
    refused(go(0, 1, 1, 0, 0, 25, 0), "no terms are set")
    refused(go(3, 0, 1, 0, 0, 25, 0), "done is null")
    refused(go(3, 1, 0, 0, 0, 25, 0), "done_stride below 1")
    refused(go(3, 1, 1, 1, 76, 25, 0), "row_stride < 3J + 2")
    refused(go(3, 1, 1, 1, 79, 25, 1), "row_stride < 3J + 2 (3J + 5 with penalties in rows)")
    assert "OK" in go(3, 1, 1, 0, 5, 25, 0)            # (rows NULL: the stride is not looked at)


@pytest.mark.parametrize("case", [(n, T) for n in LC.NS for T in (1, 16)], ids=lambda c: "n%d-T%d" % c)
def test_the_layout_of_the_state(case, harness, tmp_path):
    n, T = case
    LC.sound(LC.run_layout(harness, tmp_path, n, T)["layout"], n * (4 + T * 32) * 4)


def test_the_empty_state(harness, tmp_path):
    LC.sound(LC.run_layout(harness, tmp_path, 3, 0)["layout"], 0)
