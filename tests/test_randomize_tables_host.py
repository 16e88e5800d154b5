"""The term table of the episode randomisation, on the CPU and under the sanitizers: build_random_table of csrc/host_tables.cpp -
what trex_batch_set_randomization checks and hands the kernel - built with csrc/model.cpp into tests/host/randomize_harness.cpp by
g++ -fsanitize=address,undefined (the flags of tests/test_sensing_tables_host.py; no HIP, nothing loaded into Python) and run as a
child process, one run per case: every refusal include/trex_randomize.h lists, and the table's layout - masks of 0 expanded to the
model's bodies or joints, the single-element kinds, the numbering of the push terms. No sanitizer report may appear."""
import os
import subprocess

import numpy as np
import pytest

import layout_cases as LC
import randomize_cases as RC
from conftest import ROOT
from randomize_ref import COMMAND, FRICTION, KD, KP, MASS, MAX_FORCE, PUSH

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("randomize_tables") / "randomize_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "randomize_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def table(exe, tmp_path, nb, nj, terms, count=None, stiffness=0):
    path = os.path.join(str(tmp_path), "numbers.txt")
    numbers = [nb, nj, stiffness, len(terms) if count is None else count] + [x for t in terms for x in t]
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


def refused(out, text):
    assert isinstance(out, tuple) and out[0] == "REFUSED", out
    assert out[1] == INVALID and text in out[2], out


def check(t, nb, nj, terms):
    kinds = [x[0] for x in terms]
    pushes = [i for i, k in enumerate(kinds) if k == PUSH]
    gains = any(k in (KP, KD, MAX_FORCE) for k in kinds)
    assert t["scalars"].astype(int).tolist() == [len(terms), len(pushes), MASS in kinds, FRICTION in kinds, gains, COMMAND in kinds, 36]
    want_mask, want_shared = [], []
    for kind, mask, index, shared, *_ in terms:
        if kind in (MASS, KP, KD, MAX_FORCE):
            want_mask.append(mask or (1 << (nb if kind == MASS else nj)) - 1)
            want_shared.append(int(shared != 0))
        else:
            want_mask.append(0 if kind == PUSH else 1)
            want_shared.append(int(shared != 0) if kind == PUSH else 1)
    assert t["kind"].astype(int).tolist() == kinds and t["mask"].astype(np.int64).tolist() == want_mask
    assert t["shared"].astype(int).tolist() == want_shared
    for k, col in (("index", 2), ("interval", 6), ("duration", 7)):
        assert t[k].astype(int).tolist() == [x[col] for x in terms]
    for k, col in (("lo", 4), ("hi", 5), ("probability", 8)):
        assert (t[k].astype(np.float32) == np.array([x[col] for x in terms], np.float32)).all()
    slot = [-1] * 16
    for p, i in enumerate(pushes):
        slot[i] = p
    assert t["push_slot"].astype(int).tolist() == slot


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_the_tables_of_the_cases(case, harness, tmp_path):
    check(table(harness, tmp_path, case.nb, case.nj, case.terms), case.nb, case.nj, case.terms)


def test_layout(harness, tmp_path):
    empty = table(harness, tmp_path, 26, 25, [])
    assert empty["scalars"].astype(int).tolist()[:6] == [0, 0, 0, 0, 0, 0] and empty["kind"].size == 0
    assert empty["push_slot"].astype(int).tolist() == [-1] * 16
    terms = [(PUSH, 0, 3, 0, 1.0, 2.0, 5, 2, 0.5), (MASS, 0, 0, 5, 0.5, 1.5, 0, 0, 0.0), (PUSH, 0, 0, 0, 0.0, 0.0, 1, 1, 1.0),
             (KP, 1 << 24, 0, 0, 1.0, 1.0, 0, 0, 0.0)]
    check(table(harness, tmp_path, 26, 25, terms), 26, 25, terms)
    check(table(harness, tmp_path, 2, 1, [(MASS, 0, 0, 0, 1, 1, 0, 0, 0), (KD, 0, 0, 0, 1, 1, 0, 0, 0)]), 2, 1,
          [(MASS, 0, 0, 0, 1, 1, 0, 0, 0), (KD, 0, 0, 0, 1, 1, 0, 0, 0)])


def test_refusals(harness, tmp_path):
    go = lambda terms, nb=26, nj=25, **kw: table(harness, tmp_path, nb, nj, terms, **kw)
    mass = (MASS, 0b1111, 0, 0, 0.9, 1.1, 0, 0, 0.0)
    push = (PUSH, 0, 0, 0, 0.0, 10.0, 3, 2, 0.5)
    cmd = (COMMAND, 0, 1, 0, -1.0, 1.0, 4, 0, 0.1)
    names = "kind mask index shared lo hi interval duration probability".split()
    change = lambda base, **kw: tuple(kw.get(k, v) for k, v in zip(names, base))
    assert not isinstance(go([mass, push, cmd]), tuple)
    refused(go([], count=17), "num_terms 17 outside [0, 16]")                                  # more than 16 terms
    refused(go([], count=-1), "num_terms -1 outside [0, 16]")
    for kind in (-1, 7):
        refused(go([change(mass, kind=kind)]), "term 0: unknown kind %d" % kind)                # an unknown kind
    refused(go([change(mass, lo=1.2)]), "term 0: lo > hi")                                      # lo > hi
    for name in ("lo", "hi"):
        for bad in (np.nan, np.inf, -np.inf):
            refused(go([change(mass, **{name: bad})]), "term 0: lo or hi is not finite")        # a non-finite bound
    refused(go([change(mass, mask=1 << 26)]), "term 0: a mask bit beyond the model's 26 bodies")       # a mask bit beyond the model
    assert not isinstance(go([change(mass, mask=1 << 25)]), tuple)
    for kind in (KP, KD, MAX_FORCE):
        refused(go([change(mass, kind=kind, mask=1 << 25)]), "term 0: a mask bit beyond the model's 25 joints")
        assert not isinstance(go([change(mass, kind=kind, mask=1 << 24)]), tuple)
    refused(go([change(mass, mask=0b100)], nb=2, nj=1), "a mask bit beyond the model's 2 bodies")
    refused(go([mass, change(mass, mask=0b1000)]), "term 1: overlaps an earlier term of its kind")      # overlapping masks of one kind
    refused(go([mass, change(mass, mask=0)]), "term 1: overlaps an earlier term of its kind")           # (0 is all)
    assert not isinstance(go([mass, change(mass, mask=0b10000)]), tuple)
    assert not isinstance(go([mass, change(mass, kind=KP)]), tuple)                                     # (another kind: no overlap)
    refused(go([(FRICTION, 0, 0, 0, 0.5, 1.0, 0, 0, 0.0)] * 2), "term 1: overlaps an earlier term of its kind")
    refused(go([cmd, cmd]), "term 1: overlaps an earlier term of its kind")
    refused(go([change(push, index=b) for b in range(5)]), "term 4: more than 4 PUSH terms")            # more than 4 pushes
    assert not isinstance(go([change(push, index=b) for b in range(4)]), tuple)
    refused(go([push, push]), "term 1: overlaps an earlier term of its kind")                           # two on one body
    for body in (-1, 26):
        refused(go([change(push, index=body)]), "term 0: body %d outside [0, 26)" % body)               # a body out of range
    for comp in (-1, 3):
        refused(go([change(cmd, index=comp)]), "term 0: command component %d outside [0, 2]" % comp)    # a command index out of range
    for interval, duration in ((0, 1), (1, 0), (-3, 2)):
        refused(go([change(push, interval=interval, duration=duration)]), "term 0: a PUSH term needs interval >= 1 and duration >= 1")
    refused(go([change(cmd, interval=-1)]), "term 0: a COMMAND term needs interval >= 0")
    assert not isinstance(go([change(cmd, interval=0)]), tuple)
    for p in (-0.01, 1.01, np.nan):
        refused(go([change(push, probability=p)]), "term 0: probability outside [0, 1]")                # a probability outside [0, 1]
        refused(go([change(cmd, probability=p)]), "term 0: probability outside [0, 1]")
    for kind in (KP, KD):                                                                               # KP, KD with stiffness actions
        refused(go([change(mass, kind=kind)], stiffness=1), "KP and KD terms are refused while stiffness actions are on")
    assert not isinstance(go([change(mass, kind=MAX_FORCE)], stiffness=1), tuple)
    # (env_offset + N beyond 2^32 is the C entry's own check: tests/test_gpu_randomize.py)


@pytest.mark.parametrize("case", LC.RANDOM, ids=lambda c: "n%d-T%d-P%d" % c)
def test_the_layout_of_the_state(case, harness, tmp_path):
    LC.sound(LC.run_layout(harness, tmp_path, *case)["layout"], LC.random_bytes(*case))


def test_the_empty_state(harness, tmp_path):
    LC.sound(LC.run_layout(harness, tmp_path, 3, 0, 0)["layout"], 0)
