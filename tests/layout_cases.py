"""The state layouts of csrc/host_tables.cpp (reward history, motion clocks and held values, sensing counters and histories,
randomisation state) on the CPU: the cases the *_tables_host suites run through their harnesses' layout mode, the size every
allocation had before the layouts were functions - written out here, term by term, not taken from the code - and the runner.
The shapes are the smallest at which an offset term can be wrong: n = 1, an odd n (4-byte members behind one another: nothing may
assume 8), every count at 1 and at its limit, and the empty case."""
import os
import subprocess

NS = (1, 3)
J = 25                      # the T-rex's joints: 3J = 75 observation columns, action rows J or 2J wide


def run_layout(exe, tmp_path, *numbers):
    """-> {line name: [bytes, clashes, misaligned, unused]} of one `<harness> layout <numbers file>` run"""
    path = os.path.join(str(tmp_path), "layout.txt")
    with open(path, "w") as f:
        f.write(" ".join(repr(float(x)) for x in numbers))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "layout", path], env=env, capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return {line.split()[0]: [int(x) for x in line.split()[1:]] for line in r.stdout.splitlines()}


def sound(got, size):
    """the allocation is `size` bytes; no byte has two owners, no member is off its alignment, no byte has no owner"""
    assert got == [size, 0, 0, 0], (got, size)


# reward history (n, A, J, T): previous actions [n][A] | previous qd [n][J] | timers [n][T] | held [n][T] | valid [n]
REWARD = [(n, A, j, T) for n in NS for (A, j) in ((1, 1), (J, J), (2 * J, J)) for T in (1, 32)]


def reward_bytes(n, A, j, T):
    return n * (A + j + 2 * T + 1) * 4 if T else 0


# motion (n, T): clocks t0 [n] f32 | k [n] i32, and held values [n][T]
MOTION = [(n, T) for n in NS for T in (1, 8)]


# sensing (n, G, delayed, action delay on, action columns): counters ep | k | started [n] each | delay [n][G]; history
# [9][n][delayed]; the action delay's counters [n] x 4 and history [9][n][cols]
SENSING = [(n, G, delayed, on, cols) for n in NS for G in (1, 64) for delayed in (0, 3 * J, 512)
           for (on, cols) in ((0, J), (1, 1), (1, J), (1, 2 * J))]


def sensing_bytes(n, G, delayed, on, cols):
    return {"counters": n * (3 + G) * 4 if G else 0, "hist": 9 * n * delayed * 4, "act_counters": n * 4 * 4 if on else 0,
            "act_hist": 9 * n * cols * 4 if on else 0}


# randomisation state (n, T, P): ep | k | started | off [P] | push_left [P] | push_force [P][3] | push_base [P][6] | values [T][32]
RANDOM = [(n, T, P) for n in NS for (T, P) in ((1, 0), (1, 1), (16, 0), (16, 4))]


def random_bytes(n, T, P):
    return n * (3 + P + P + 3 * P + 6 * P + T * 32) * 4 if T else 0
