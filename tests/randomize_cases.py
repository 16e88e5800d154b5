"""The cases of the episode-randomisation tests and the comparison they share: term lists over three models, done patterns that end
episodes every 5 to 9 rows at different rows per env, one reset of a third of the envs in the middle of the run, and compare(),
which holds what a device run (tests/test_gpu_randomize.py) - or a deliberately mistaken reference
(tests/test_randomize_cases_host.py, which qualifies these cases) - must satisfy against the reference tests/randomize_ref.py.
numpy only: no torch, no device. A helper, not a conftest.

The comparison, per output:
    values, command          bitwise the reference's f32 run (products and sums of f32 numbers in the header's order: IEEE)
    push_left                equal
    push_force               exactly zero where the reference's is; elsewhere within 4 x the case's own bound: the largest deviation
                             of the reference's f32 run from its f64 run over the case, floored at 2 ulp (f32) of the largest `hi` of
                             the case's push terms (the device's sinf and cosf are not numpy's)
"""
import collections

import numpy as np

import randomize_ref as RR
from randomize_ref import COMMAND, FRICTION, KD, KP, MASS, MAX_FORCE, PUSH

Case = collections.namedtuple("Case", "name model nb nj n rows terms seed env_offset")


def bits(*elements):
    return sum(1 << i for i in elements)


def _small(nb, nj):
    """every kind once or twice on a small model: both push forms, both command forms, lo == hi, the three probabilities"""
    return [(MASS, 0, 0, 0, 0.8, 1.25, 0, 0, 0.0), (FRICTION, 0, 0, 0, 0.5, 1.25, 0, 0, 0.0), (KP, 0, 0, 0, 0.7, 1.3, 0, 0, 0.0),
            (KD, 0, 0, 1, 1.5, 1.5, 0, 0, 0.0), (MAX_FORCE, bits(nj - 1), 0, 0, 0.9, 1.1, 0, 0, 0.0),
            (PUSH, 0, 0, 0, 10.0, 50.0, 3, 2, 1.0), (PUSH, 0, nb - 1, 0, 0.0, 5.0, 1, 1, 0.5),
            (COMMAND, 0, 0, 0, -1.0, 1.0, 4, 0, 0.5), (COMMAND, 0, 1, 0, -0.3, 0.3, 0, 0, 0.0), (COMMAND, 0, 2, 0, -0.5, 0.5, 4, 0, 1.0)]


def _masks():
    """the T-rex: a shared and a per-body mass term with disjoint masks, gains on joints beyond the first Philox block"""
    return [(MASS, bits(0, 1, 2, 3), 0, 1, 0.9, 1.1, 0, 0, 0.0), (MASS, bits(5, 9, 17, 25), 0, 0, 0.5, 2.0, 0, 0, 0.0),
            (KP, bits(4, 7, 13, 24), 0, 0, 0.8, 1.2, 0, 0, 0.0), (KD, bits(6, 20, 21, 22, 23), 0, 1, 0.5, 1.5, 0, 0, 0.0),
            (PUSH, 0, 0, 0, 100.0, 300.0, 3, 2, 0.5), (PUSH, 0, 7, 0, 5.0, 5.0, 1, 1, 1.0), (PUSH, 0, 25, 0, 0.0, 20.0, 3, 2, 0.0),
            (COMMAND, 0, 0, 0, 0.0, 2.0, 4, 0, 0.0), (COMMAND, 0, 2, 0, -1.0, 1.0, 0, 0, 0.5)]


def _sixteen():
    """all 16 terms at once"""
    return [(MASS, bits(0), 0, 1, 0.9, 1.1, 0, 0, 0.0), (MASS, bits(*range(1, 26)), 0, 0, 0.8, 1.2, 0, 0, 0.0),
            (FRICTION, 0, 0, 0, 0.4, 1.0, 0, 0, 0.0),
            (KP, bits(*range(0, 12)), 0, 0, 0.8, 1.2, 0, 0, 0.0), (KP, bits(*range(12, 25)), 0, 1, 0.9, 1.1, 0, 0, 0.0),
            (KD, bits(*range(0, 25, 2)), 0, 0, 0.8, 1.2, 0, 0, 0.0), (KD, bits(*range(1, 25, 2)), 0, 0, 1.0, 1.0, 0, 0, 0.0),
            (MAX_FORCE, bits(3), 0, 0, 0.5, 1.0, 0, 0, 0.0), (MAX_FORCE, bits(*range(4, 25)), 0, 1, 0.9, 1.1, 0, 0, 0.0),
            (PUSH, 0, 0, 0, 50.0, 400.0, 3, 2, 1.0), (PUSH, 0, 1, 0, 1.0, 2.0, 1, 1, 0.5), (PUSH, 0, 12, 0, 0.0, 30.0, 3, 2, 0.5),
            (PUSH, 0, 25, 0, 10.0, 10.0, 1, 1, 1.0),
            (COMMAND, 0, 0, 0, -1.0, 1.5, 4, 0, 0.5), (COMMAND, 0, 1, 0, -0.3, 0.3, 0, 0, 0.0), (COMMAND, 0, 2, 0, -0.5, 0.5, 4, 0, 0.0)]


CASES = [
    Case("slab_n1", "slab", 2, 1, 1, 40, _small(2, 1), 21, 0),
    Case("chain_n2", "deep_chain", 7, 6, 2, 32, _small(7, 6), 22, 5),
    Case("chain_n7", "deep_chain", 7, 6, 7, 24, _small(7, 6), 2 ** 40 + 23, 1000),
    Case("trex_n65_masks", "trex", 26, 25, 65, 28, _masks(), 24, 0),
    Case("trex_n130_16_terms", "trex", 26, 25, 130, 24, _sixteen(), 25, 2 ** 32 - 130),
]
RESET_ROW = 11      # before this row's apply, the envs with e % 3 == 0 are marked by the reset call


def done_flags(case):
    """[rows, n] f32: episodes of 5 to 9 rows, drawn per env, so that they end at different rows"""
    rng = np.random.default_rng([case.seed % 2 ** 32, 77])
    done = np.zeros((case.rows, case.n), np.float32)
    for e in range(case.n):
        t = int(rng.integers(5, 10))
        while t < case.rows:
            done[t, e] = 1.0
            t += int(rng.integers(5, 10))
    return done


def reset_mask(case):
    return (np.arange(case.n) % 3 == 0).astype(np.uint8)


def reference(case, f32=False, mistake=None, env_offset=None, n=None, first_env=0):
    """-> [Row] over the case's rows; n, first_env: a shard of the case's envs (its done flags and reset mask cut accordingly)"""
    n = case.n if n is None else n
    sel = slice(first_env, first_env + n)
    r = RR.Randomizer(n, case.nb, case.nj, case.terms, case.seed, case.env_offset + first_env if env_offset is None else env_offset,
                      f32=f32, mistake=mistake)
    done, out = done_flags(case), []
    for t in range(case.rows):
        if t == RESET_ROW:
            r.reset(reset_mask(case)[sel])
        out.append(r.apply(done[t, sel]))
    return out


_REF = {}


def references(case):
    """(f32 run, f64 run) of the case, computed once and shared: leave them unchanged"""
    if case.name not in _REF:
        _REF[case.name] = (reference(case, f32=True), reference(case))
    return _REF[case.name]


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def force_bound(case):
    """4 x the largest |f32 run - f64 run| of the push forces over the case, floored at 2 ulp of the largest hi"""
    r32, r64 = references(case)
    dev = max(float(np.abs(a.push_force.astype(np.float64) - b.push_force).max(initial=0.0)) for a, b in zip(r32, r64))
    hi = max(t[5] for t in case.terms if t[0] == PUSH)
    return max(4.0 * dev, 2.0 * ulp32(hi))


def compare(case, got):
    """got: per row (values [n, T, 32] f32, push_force [n, P, 3] f32, push_left [n, P] int, command [n, 3] f32).
    -> dict(failures=[text], share=the largest push-force deviation / the bound)"""
    r32, r64 = references(case)
    bound, fails, share = force_bound(case), [], 0.0
    for t, (a, b, g) in enumerate(zip(r32, r64, got)):
        values, force, left, command = (np.asarray(x) for x in g)
        if values.astype(np.float32).tobytes() != a.values.astype(np.float32).tobytes():
            fails.append("row %d: values differ" % t)
        if not np.array_equal(left.astype(np.int64), a.push_left):
            fails.append("row %d: push_left differs" % t)
        if command.astype(np.float32).tobytes() != a.command.astype(np.float32).tobytes():
            fails.append("row %d: command differs" % t)
        zero = b.push_force == 0
        if (force[zero] != 0).any():
            fails.append("row %d: a force where none acts" % t)
        err = float(np.abs(force.astype(np.float64) - b.push_force).max(initial=0.0))
        share = max(share, err / bound)
        if err > bound:
            fails.append("row %d: push force off by %.3g, bound %.3g" % (t, err, bound))
    return dict(failures=fails, share=share)


def as_got(rows):
    """the rows of a reference run as a device run would deliver them"""
    return [(r.values.astype(np.float32), r.push_force.astype(np.float32), r.push_left.astype(np.int32), r.command.astype(np.float32))
            for r in rows]
