"""The HIP-free part of the episode monitor, on the CPU and under the sanitizers: monitor_layout and check_monitor_apply of
csrc/host_tables.cpp - what trex_batch_set_monitor and trex_batch_monitor_apply check before any HIP call, and where every member of
the monitor's state lies - built with csrc/model.cpp into tests/host/monitor_harness.cpp by g++ -fsanitize=address,undefined (the
flags of tests/test_randomize_tables_host.py; no HIP, nothing loaded into Python) and run as a child process, one run per case: the
refusals include/trex_monitor.h lists for the set and the strides of the apply, the team and the workgroup count of the
accumulate launch, and a layout whose members neither overlap nor leave the allocation. No sanitizer report may appear."""
import os
import subprocess

import pytest

import monitor_cases as MC
from conftest import ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID = -1          # TREX_E_INVALID
BLOCK = 256           # TREX_MON_BLOCK


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("monitor_tables") / "monitor_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "monitor_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def ask(exe, tmp_path, *numbers):
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
    return {line.split(" ", 1)[0]: [int(x) for x in line.split()[1:]] for line in r.stdout.splitlines()}


def refused(out, text):
    assert isinstance(out, tuple) and out[0] == "REFUSED", out
    assert out[1] == INVALID and text in out[2], out


def team_of(cols):
    team = 1
    while team < cols:
        team *= 2
    return team


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c.name)
def test_the_layouts_of_the_cases(case, harness, tmp_path):
    out = ask(harness, tmp_path, case.n, case.window, case.cols_a, case.cols_b, case.env_offset, BLOCK)
    C = case.cols_a + case.cols_b
    per = BLOCK // team_of(C)
    assert out["shape"] == [case.window, case.cols_a, case.cols_b, C, team_of(C), -(-case.n // per)]
    size, clashes, misaligned, unused = out["layout"]
    assert clashes == 0 and misaligned == 0 and unused == 0
    assert size == case.n * (8 + 8 * C + 28 + 4 * C) + 40 + 4 + case.window * (20 + 4 * C) + 4 * (-(-case.n // per))


def test_the_team_and_the_empty_layout(harness, tmp_path):
    for cols, team in ((0, 1), (1, 1), (2, 2), (3, 4), (33, 64), (64, 64)):
        out = ask(harness, tmp_path, 4096, 100, cols, 0, 0, BLOCK)
        assert out["shape"][4:] == [team, 4096 * team // BLOCK] and out["layout"][1:] == [0, 0, 0]
    assert ask(harness, tmp_path, 7, 0, 99, -5, 2 ** 32 - 1, BLOCK) == {"shape": [0, 0, 0, 0, 1, 0], "layout": [0, 0, 0, 0]}   # (a clear looks at nothing else)
    assert ask(harness, tmp_path, 1, 65536, 32, 32, 2 ** 32 - 1, BLOCK)["layout"][1:] == [0, 0, 0]


def test_refusals_of_the_set(harness, tmp_path):
    go = lambda n=64, window=100, a=2, b=3, off=0: ask(harness, tmp_path, n, window, a, b, off, BLOCK)
    assert not isinstance(go(), tuple)
    for w in (-1, 65537):
        refused(go(window=w), "window %d outside [0, 65536]" % w)
    assert not isinstance(go(window=65536), tuple) and not isinstance(go(window=1), tuple)
    refused(go(a=-1), "a negative column count")
    refused(go(b=-1), "a negative column count")
    refused(go(a=33, b=32), "65 columns, at most 64")
    refused(go(a=2 ** 31 - 1, b=2 ** 31 - 1), "columns, at most 64")
    assert not isinstance(go(a=64, b=0), tuple) and not isinstance(go(a=0, b=64), tuple)
    refused(go(off=2 ** 32 - 63), "env_offset + N is beyond 2^32")
    assert not isinstance(go(off=2 ** 32 - 64), tuple)


def test_refusals_of_the_apply(harness, tmp_path):
    good = dict(reward=1, rs=1, done=1, ds=1, a=1, sa=2, b=1, sb=3)

    def go(window=100, ca=2, cb=3, **kw):
        v = dict(good, **kw)
        return ask(harness, tmp_path, 64, window, ca, cb, 0, BLOCK, v["reward"], v["rs"], v["done"], v["ds"], v["a"], v["sa"], v["b"], v["sb"])
    assert not isinstance(go(), tuple)
    refused(go(window=0), "no monitor is set")
    refused(go(reward=0), "reward is null")
    refused(go(done=0), "done is null")
    refused(go(rs=0), "reward_stride below 1")
    refused(go(ds=0), "done_stride below 1")
    refused(go(ds=-3), "done_stride below 1")
    refused(go(a=0), "cols_a is null and its width is 2")
    refused(go(b=0), "cols_b is null and its width is 3")
    refused(go(sa=1), "stride_a 1 below the width 2")
    refused(go(sb=2), "stride_b 2 below the width 3")
    assert not isinstance(go(sa=7, sb=9), tuple)
    assert not isinstance(go(ca=0, a=0, sa=0), tuple)            # (a block of width 0: neither pointer nor stride is looked at)
    assert not isinstance(go(cb=0, b=0, sb=-1), tuple)
