"""Qualifies the cases of tests/randomize_cases.py on the CPU, on the reference alone: every planted mistake of
tests/randomize_ref.py must change the output of at least one case beyond what compare() allows a device run, the correct reference
itself must pass, a shard must draw what the whole batch draws, and no case may pass vacuously - each run contains a push start,
a push cut short by a done and a command resampled inside an episode."""
import numpy as np
import pytest

import randomize_cases as RC
import randomize_ref as RR


@pytest.mark.parametrize("case", RC.CASES, ids=[c.name for c in RC.CASES])
def test_the_reference_passes_its_own_comparison(case):
    r32, r64 = RC.references(case)
    res = RC.compare(case, RC.as_got(r32))
    assert not res["failures"], res["failures"][:3]
    assert res["share"] <= 0.25 + 1e-12        # the f32 run lies within a quarter of the bound by construction
    assert RC.force_bound(case) < 1e-3 * max(t[5] for t in case.terms if t[0] == RR.PUSH)     # and the bound is a tight one


@pytest.mark.parametrize("case", RC.CASES, ids=[c.name for c in RC.CASES])
def test_no_case_passes_vacuously(case):
    rows = RC.references(case)[1]
    assert sum(r.starts for r in rows) > 0, "no push starts"
    assert sum(r.cuts for r in rows) > 0, "no push is cut by a done"
    assert sum(r.resamples for r in rows) > 0, "no command is resampled inside an episode"
    done = RC.done_flags(case)
    gaps = [np.diff(np.flatnonzero(done[:, e])) for e in range(case.n)]
    assert all(((g >= 5) & (g <= 9)).all() for g in gaps)
    assert 24 <= case.rows <= 40 and (case.n == 1 or len({tuple(np.flatnonzero(done[:, e])) for e in range(case.n)}) > 1)


@pytest.mark.parametrize("mistake", RR.MISTAKES)
def test_every_planted_mistake_is_caught_by_a_case(mistake):
    caught = [c.name for c in RC.CASES if RC.compare(c, RC.as_got(RC.reference(c, f32=True, mistake=mistake)))["failures"]]
    print(mistake, "caught by", caught)
    assert caught, "no case notices " + mistake


def test_a_shard_draws_what_the_whole_batch_draws():
    case = next(c for c in RC.CASES if c.name == "trex_n130_16_terms")
    whole = RC.references(case)[0]
    half = case.n // 2
    for first in (0, half):
        part = RC.reference(case, f32=True, n=half, first_env=first)
        for w, p in zip(whole, part):
            assert np.array_equal(w.values[first:first + half], p.values) and np.array_equal(w.push_left[first:first + half], p.push_left)
            assert np.array_equal(w.push_force[first:first + half], p.push_force) and np.array_equal(w.command[first:first + half], p.command)


def test_the_sizes_models_and_terms_the_cases_must_cover():
    assert sorted(c.n for c in RC.CASES) == [1, 2, 7, 65, 130]
    assert {(c.nb, c.nj) for c in RC.CASES} == {(2, 1), (7, 6), (26, 25)}
    assert any(len(c.terms) == RR.MAXTERMS for c in RC.CASES)
    terms = [RR.Term(*t) for c in RC.CASES for t in c.terms]
    assert {(t.interval, t.duration) for t in terms if t.kind == RR.PUSH} == {(3, 2), (1, 1)}
    assert {t.interval for t in terms if t.kind == RR.COMMAND} == {0, 4}
    assert {t.probability for t in terms if t.kind in (RR.PUSH, RR.COMMAND)} == {0.0, 0.5, 1.0}
    assert any(t.lo == t.hi for t in terms)
    for c in RC.CASES:
        mass = [RR.Term(*t) for t in c.terms if t[0] == RR.MASS]
        if len(mass) == 2:
            assert mass[0].shared != mass[1].shared and not (mass[0].mask & mass[1].mask)
            break
    else:
        raise AssertionError("no case has a shared and a per-body mass term")
