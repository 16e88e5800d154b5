"""Qualifies tests/sensing_cases.py - the cases and the comparison tests/test_gpu_sensing.py holds the device to - on the reference
tests/sensing_ref.py alone, without a GPU: the reference's Philox reproduces Random123's known answers; its streams have the
moments and the independence their sample counts allow; no two (env, column, step, episode) share a draw; a ramp shows the delay,
hold and restart rules; the reference's own f32 run passes the comparison; and each of six deliberate mistakes is caught by at least
one case."""
import numpy as np
import pytest

import sensing_cases as SC
import sensing_ref as SR

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = SR.philox4x32(counter, key)
    assert " ".join("%08x" % int(x) for x in got) == want


def test_philox_is_vectorised_as_it_is_scalar():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (4, 50), dtype=np.uint64)
    r = SR.philox4x32(tuple(c), (123, 456))
    for i in (0, 17, 49):
        one = SR.philox4x32(tuple(int(x) for x in c[:, i]), (123, 456))
        assert [int(x) for x in one] == [int(x[i]) for x in r]


def _stream(stream, n=64, blocks=16, steps=64):
    """the words of one stream over n envs x blocks x steps, as the reference numbers them: [steps, n, 4 * blocks]"""
    e, b = np.arange(n)[:, None], np.arange(blocks)[None, :]
    out = []
    for k in range(steps):
        r = SR.philox4x32((e, k, (stream << 16) | b, 1), SR.key_of(5))
        out.append(np.stack(r, -1).reshape(n, 4 * blocks))
    return np.stack(out)


def test_stream_moments_and_lag_one_correlation():
    """N = 64 x 64 x 64 = 262 144 samples per stream: a mean is within 5 sigma / sqrt(N), a variance within 5 sqrt(kurtosis - 1) sigma^2
    / sqrt(N) (kurtosis 3 for the normal, 1.8 for the uniform), a lag-one correlation - along the steps, and along the columns -
    within 5 / sqrt(N)"""
    w = _stream(SR.WHITE)
    N = w.size
    uni = 2.0 * SR.u_half_open(w) - 1.0
    r4 = [w[..., j::4] for j in range(4)]
    z = np.stack(SR.normals(r4), -1).reshape(w.shape)
    for x, var, kurt in ((uni, 1.0 / 3.0, 1.8), (z, 1.0, 3.0)):
        assert abs(x.mean()) < 5 * np.sqrt(var / N)
        assert abs(x.var() - var) < 5 * np.sqrt(kurt - 1.0) * var / np.sqrt(N)
        for a, b in ((x[1:], x[:-1]), (x[..., 1:], x[..., :-1]), (x[:, 1:], x[:, :-1])):
            assert abs(np.mean(a * b) / var) < 5 / np.sqrt(a.size)
    assert np.isfinite(z).all() and np.abs(z).max() < np.sqrt(-2 * np.log(2.0 ** -24)) + 1e-9     # u' > 0: no infinity
    f32 = np.stack(SR.normals(r4, f32=True), -1).reshape(w.shape)
    assert f32.dtype == np.float32 and np.abs(f32 - z).max() < 1e-5
    d = SR.draw_int(_stream(SR.DELAY)[..., 0], 2, 8)
    assert d.min() == 2 and d.max() == 8 and abs(d.mean() - 5.0) < 5 * 2.0 / np.sqrt(d.size)


def test_no_two_draws_share_a_counter():
    """(env, column, step, episode) -> (counter, output index) is one to one over the streams, and so - but for chance, which 2^-32
    x pairs makes negligible here - are the words"""
    seen, words = set(), []
    for stream in (SR.WHITE, SR.BIAS):
        for ep in (1, 2):
            for k in range(3 if stream == SR.WHITE else 1):
                for e in range(5):
                    for c in range(16):
                        key = (e, k, (stream << 16) | (c >> 2), ep, c & 3)
                        assert key not in seen
                        seen.add(key)
                        words.append(int(SR.philox4x32(key[:4], (9, 9))[c & 3]))
    assert len(set(words)) == len(words)


def test_a_ramp_shows_delay_hold_and_restart():
    """one env, three pure-delay groups of delays 0, 1 and 8 over a ramp row[c] = 100 t + c; a done row at t = 12"""
    groups = [(0, 1, 0, 0.0, 0.0, 0.0, 0, 0), (1, 1, 0, 0.0, 0.0, 0.0, 1, 1), (2, 1, 0, 0.0, 0.0, 0.0, 8, 8)]
    s = SR.Sensors(1, 3, 2, groups, seed=3)
    seen = []
    for t in range(24):
        row = np.array([[100 * t, 100 * t + 1, 100 * t + 2, 0.5, float(t == 12)]], np.float32)
        seen.append(s.apply(row).out[0])
    seen = np.array(seen)
    t = np.arange(24)
    start = np.where(t >= 12, 12, 0)
    assert (seen[:, 0] == 100 * t).all()
    assert (seen[:, 1] == 100 * np.maximum(t - 1, start) + 1).all()
    assert (seen[:, 2] == 100 * np.maximum(t - 8, start) + 2).all()        # holds its first reading, then runs 8 late
    assert (seen[:, 3] == 0.5).all() and (seen[:, 4] == (t == 12)).all()
    assert s.ep[0] == 2 and s.k[0] == 11
    s.reset(np.array([1]))
    assert s.apply(np.array([[7, 8, 9, 0, 0]], np.float32)).out[0, :3].tolist() == [7, 8, 9] and s.ep[0] == 3 and s.k[0] == 0


def test_bias_is_held_and_redrawn_per_episode():
    s = SR.Sensors(4, 8, 2, [(0, 8, 0, 0.0, 0.25, 0.0, 0, 0)], seed=1)
    zero = np.zeros((4, 10), np.float32)
    a, b = s.apply(zero).out[:, :8], s.apply(zero).out[:, :8]
    assert (a == b).all() and (np.abs(a) <= 0.25).all() and len(np.unique(a)) == 32
    done = zero.copy()
    done[2, 9] = 1.0
    c = s.apply(done).out[:, :8]
    assert (c[[0, 1, 3]] == a[[0, 1, 3]]).all() and (c[2] != a[2]).all()


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_the_f32_run_of_the_reference_passes(case):
    ref, _ = SC.reference(case)
    f32, _ = SC.reference(case, f32=True)
    r = SC.compare(case, ref, [a.out for a in f32], factor=1.0 + 1e-9)          # (its own deviation IS the bound)
    assert not r["failures"], r["failures"][:5]
    assert r["left_out"] <= 0.01 and r["ulps"] <= 2.0
    r64 = SC.compare(case, ref, [a.out.astype(np.float32) for a in ref])
    assert not r64["failures"], r64["failures"][:5]
    print("%s: bound %.3g, left out %.3f %%, %.2f ulp" % (case.name, SC.gaussian_bound(case), 100 * r["left_out"], r["ulps"]))


def test_the_derived_bound_is_of_the_order_of_f32_rounding():
    """the bound is the reference's own: between one f32 ulp of the largest value and what unit-sigma Box-Muller in f32 gives (1.6e-6
    measured over 4 M draws) scaled by the case's largest sigma, with room for the larger operands of these rows"""
    for case in SC.CASES:
        b = SC.gaussian_bound(case)
        assert 2.0 ** -24 < b < 2e-5, (case.name, b)


@pytest.mark.parametrize("mistake", SR.MISTAKES)
def test_each_mistake_is_caught(mistake):
    caught = []
    for case in SC.CASES:
        ref, _ = SC.reference(case)
        bad, _ = SC.reference(case, mistake=mistake)
        if SC.compare(case, ref, [a.out.astype(np.float32) for a in bad])["failures"]:
            caught.append(case.name)
    print(mistake, "caught by", caught)
    assert caught


def test_the_cases_cover_what_they_claim():
    assert sorted(c.n for c in SC.CASES) == [1, 63, 64, 65, 257] and sorted({c.D for c in SC.CASES}) == [3, 75, 93, 512]
    assert sorted({len(c.groups) for c in SC.CASES}) == [1, 6, 64]
    assert any(g[0] == 5 and g[1] == 7 for c in SC.CASES for g in c.groups)
    assert {0, 1, 8} <= {g[7] for c in SC.CASES for g in c.groups}
    assert {True, False} == {c.in_place for c in SC.CASES} and any(c.pad for c in SC.CASES)
    for c in SC.CASES:                            # every case meets done rows, and not only done rows
        flags = np.array([SC.rows_of(c, t)[:, c.D + 1] for t in range(SC.STEPS)])
        assert flags.any() and not flags.all()
