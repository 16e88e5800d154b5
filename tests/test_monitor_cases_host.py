"""Qualifies the cases of tests/monitor_cases.py on the CPU, on the reference alone (tests/monitor_ref.py): every planted mistake
must change the expected result of at least one case, the reference must repeat itself, and the cases must hold what they are there
for - the sizes, windows and column blocks, a call that finishes more episodes than the window holds, one that finishes exactly W,
two-bit reasons, a NaN reward, envs abandoned in the middle of an episode."""
import numpy as np
import pytest

import monitor_cases as MC
import monitor_ref as MR


@pytest.fixture(scope="module")
def expected():
    return {c.name: MC.run(c) for c in MC.CASES}


def differs(case, want, mistake):
    states, summary, _, _ = MC.run(case, mistake)
    if any(MC.same_state(a, b) for a, b in zip(want[0], states)):
        return True
    return MC.summary_failures(summary, want[1], want[2]) != []


def test_the_reference_repeats_itself(expected):
    for c in MC.CASES:
        states, summary, bounds, _ = MC.run(c)
        assert not any(MC.same_state(a, b) for a, b in zip(expected[c.name][0], states))
        assert not MC.summary_failures(summary, expected[c.name][1], bounds)


@pytest.mark.parametrize("mistake", MR.MISTAKES)
def test_every_planted_mistake_changes_a_case(mistake, expected):
    caught = [c.name for c in MC.CASES if differs(c, expected[c.name], mistake)]
    print(mistake, "caught by", caught)
    assert caught, "no case notices " + mistake


def test_the_sizes_windows_and_columns_the_cases_must_cover():
    assert {c.n for c in MC.CASES} == {1, 2, 65, 257, 600}
    assert {c.window for c in MC.CASES} == {1, 3, 100, 1000}
    assert {(c.cols_a, c.cols_b) for c in MC.CASES} == {(0, 0), (1, 0), (5, 3), (32, 32)}
    assert {c.pattern for c in MC.CASES} == {"none", "every", "bernoulli", "all_at", "exactly_w"}
    assert MC.T == 40
    assert any(c.pad[0] > 1 and c.pad[1] > 1 and c.pad[2] > 0 and c.pad[3] > 0 for c in MC.CASES)
    assert any(c.env_offset + c.n == 2 ** 32 for c in MC.CASES)


def test_no_case_is_there_for_nothing(expected):
    for c in MC.CASES:
        reward, done, reason, cols = MC.arrays(c)
        per_call = (done != 0).sum(axis=1)
        if c.pattern == "none":
            assert per_call.sum() == 0 and np.isnan(expected[c.name][1][MR.RET_MEAN]) and expected[c.name][1][MR.T] == MC.T
        if c.pattern == "every":
            assert (per_call == c.n).all()
        if c.pattern == "all_at":
            assert per_call[c.burst_call] == c.n > c.window
        if c.pattern == "exactly_w":
            assert per_call[c.burst_call] == c.window and expected[c.name][0][c.burst_call - 1]["total"] % c.window != 0
        if c.nan_at is not None:
            assert np.isnan(reward[c.nan_at]) and np.isnan(expected[c.name][0][-1]["ring_return"]).any()
        if c.reset_call is not None:
            before = expected[c.name][0][c.reset_call - 1]
            if c.pattern != "every" and c.n >= 65:
                assert (before["len"][MC.reset_mask(c)] > 0).any()          # episodes are under way when they are abandoned
    finished = np.concatenate([MC.arrays(c)[2][MC.arrays(c)[1] != 0] for c in MC.CASES])
    assert set(finished.tolist()) == set(range(8))                              # reasons 0 to 7, two- and three-bit ones included
    assert any(c.window > c.n and c.pattern == "every" for c in MC.CASES)       # N records in one call with W > N ...
    assert any(c.window < c.n and c.pattern in ("every", "all_at") for c in MC.CASES)   # ... and with W < N
