"""The cases of tests/trainer_cases.py on the CPU, by oracle/ppo_oracle.py alone: every learner case is well-conditioned (no sample
on the edge of a clip() or max() branch, module docstring there) and exercises both clips, the act cases clip an observation and
reach the tanh branches they are built for, and the parameter packing is the layout rule of include/trex_policy.h. This is what
lets tests/test_gpu_trainer_edges.py trust the arrays it feeds to the kernels."""
import math
import types

import numpy as np
import pytest

import trainer_cases as tc
from oracle import ppo_oracle as P

LEARN_NAMES = sorted(tc.learn_specs())


def test_case_tables_hold_what_the_kernels_tiling_needs():
    """the shapes at which the kernels take another path are in the tables (a table edited by mistake fails here)"""
    assert (96, 32) in tc.LEARN_DIMS and (1, 1) in tc.LEARN_DIMS and (126, 32, 97) in tc.ACT_CASES and (1, 1, 1) in tc.ACT_CASES
    tiles = sorted({-(-mb // 32) for mb, _ in tc.LEARN_MBS})
    assert tiles == [1, 2, 64, 65, 128]                    # the reduce kernel sums 64 tiles per trip
    assert {(4096, 75), (2049, 126), (1, 1)} <= {(n, D) for n, D, _ in tc.OBSERVE_CASES}
    assert max(-(-n // 64) for n, _, _ in tc.OBSERVE_CASES) == 64      # the merge takes 32 workgroups per trip
    assert all(D <= 96 for D, _ in tc.LEARN_DIMS) and all(D <= 126 and A <= 32 for D, A, _ in tc.ACT_CASES)
    assert tc.layout_rule(126, 32)[1] <= 32768             # adam_kernel's limit


@pytest.mark.parametrize("D,A", sorted(set(tc.LEARN_DIMS + tc.ADAM_DIMS + [(d, a) for d, a, _ in tc.ACT_CASES])))
def test_params_round_trip_through_the_layout_rule(D, A):
    lay, count = tc.layout_rule(D, A)
    offs = [lay[n][0] for n in tc.PARAM_NAMES]
    assert all(o % 4 == 0 for o in offs) and count % 4 == 0 and list(lay) == tc.PARAM_NAMES
    ends = [o + math.prod(lay[n][1]) for n, o in zip(tc.PARAM_NAMES, offs)]
    assert all(0 <= nxt - e < 4 for e, nxt in zip(ends, offs[1:] + [count]))       # blocks in order, only the pad between them
    kern = types.SimpleNamespace(layout=lay, param_count=count)
    params = tc.make_params(D, A, np.random.default_rng(D * 100 + A))
    theta = tc._params_to_theta(lay, count, params)
    assert theta.dtype == np.float32 and theta.shape == (count,)
    back = tc._theta_to_params(kern, theta)
    assert sorted(back) == sorted(params)
    for k in params:
        assert back[k].shape == params[k].shape and np.array_equal(back[k], params[k]), k
    # weights are stored [in][out]: element [k][j] of pi.W1 is the oracle's weight[j][k]
    assert theta[lay["pi.W1"][0] + (D - 1) * tc.HID + 5] == params["pi.0.weight"][5, D - 1]
    assert theta[lay["logstd"][0] + A - 1] == params["logstd"][A - 1]
    used = np.zeros(count, bool)
    for n in tc.PARAM_NAMES:
        used[lay[n][0]:lay[n][0] + math.prod(lay[n][1])] = True
    assert (theta[~used] == 0).all()
    # and the other way round: a flat vector survives, pads excepted
    flat = np.arange(1, count + 1, dtype=np.float32)
    again = tc._params_to_theta(lay, count, tc._theta_to_params(kern, flat))
    assert np.array_equal(again[used], flat[used])
    # gradients flatten the same way
    assert np.array_equal(tc._grads_to_flat(kern, params)[used], theta.astype(np.float64)[used])


@pytest.mark.parametrize("name", LEARN_NAMES)
def test_learner_case_is_well_conditioned_and_exercises_both_clips(name):
    case = tc.learn_case_by_name(name)
    mb = case["mb"]
    assert case["idx"].shape == (mb,) and len(set(case["idx"].tolist())) == mb and case["N"] == case["first"] + mb + 100
    for k in ("obs", "act", "logp_old", "value_old", "ret", "adv"):
        assert np.array_equal(case[k], tc.f32r(case[k])), k          # what the kernel reads is what the oracle read
    assert np.abs(case["obs"]).max() <= tc.CLIP_OBS
    q = tc.learn_quantities(case)                                    # recomputed here, from the oracle
    for rule, bad in tc.learn_violations(q).items():
        assert not bad.any(), (rule, int(bad.sum()))
    # the same, spelled out from the oracle's outputs
    c, m = tc.CLIPRANGE, tc.MARGIN
    ratio = q["out"]["ratio"]
    assert (np.abs(ratio - (1 - c)) >= m).all() and (np.abs(ratio - (1 + c)) >= m).all()
    dv = q["out"]["value"] - case["value_old"][case["idx"]]
    assert (np.abs(dv - c) >= m).all() and (np.abs(dv + c) >= m).all()
    assert np.isfinite(ratio).all() and ratio.max() < 50
    a = case["adv"][case["idx"]]
    assert abs(float(case["adv_stats"][0]) - a.mean()) <= 1e-7 * max(1.0, abs(a.mean()))
    if mb >= 64:
        assert 0.1 <= q["pg_clip"].mean() <= 0.9 and 0.1 <= q["vf_clip"].mean() <= 0.9
        # ... and inside the clipped samples both branches of each max() carry samples (a gradient and a zero)
        for on, first, second in ((q["pg_clip"], q["l1"], q["l2"]), (q["vf_clip"], q["e1"], q["e2"])):
            share = (first[on] >= second[on]).mean()
            assert 0.05 <= share <= 0.95
    assert case["nudged"] <= max(2, mb // 20)                         # the nudge is a correction of a few samples, not a redesign


@pytest.mark.parametrize("index", range(len(tc.ACT_CASES)))
def test_act_case_clips_an_observation(index):
    D, A, n = tc.ACT_CASES[index]
    case = tc.act_case(D, A, n, index)
    assert case["row_stride"] - D == tc.ACT_STRIDE_EXTRA[index % 3] and case["rows"].shape == (n, case["row_stride"])
    assert (np.abs(case["obs_n"]) == tc.CLIP_OBS).any() and np.isfinite(case["actions"]).all()
    if n * D > 1:
        assert (np.abs(case["obs_n"]) < tc.CLIP_OBS).any()
    # the expected outputs are the oracle's
    mean, logstd, value = P.policy_forward(case["params"], case["obs_n"])
    assert np.array_equal(case["actions"], P.sample_action(mean, logstd, case["noise"])) and np.array_equal(case["value"], value)


def test_act_tanh_cases_reach_their_branch():
    """series: every hidden pre-activation below 0.1 (tanh_fast's polynomial); saturated: most above 20, some beyond 44.4, where
    exp2(2 |x| log2 e) overflows f32 (2^128) - and some units left in the ordinary branch"""
    pre = tc.preactivations
    s = tc.act_case(75, 25, 33, 0, "series")
    assert max(np.abs(z).max() for z in pre(s["params"], s["obs_n"]).values()) < 0.1
    assert min(np.abs(z).max() for z in pre(s["params"], s["obs_n"]).values()) > 0.01       # not trivially zero
    t = tc.act_case(75, 25, 33, 1, "saturated")
    for z in pre(t["params"], t["obs_n"]).values():
        assert (np.abs(z) > 20).mean() > 0.5 and (np.abs(z) > 44.4).mean() > 0.2 and (np.abs(z) < 10).mean() > 0.05
    for c in (s, t):
        assert np.isfinite(c["actions"]).all() and np.isfinite(c["neglogp"]).all() and (np.abs(c["obs_n"]) == tc.CLIP_OBS).any()


def test_generated_sequences_are_deterministic_and_hold_their_patterns():
    a, b = tc.observe_sequence(65, 1, 6), tc.observe_sequence(65, 1, 6)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == 5
    dones = [r[:, 2] for r in a[1:]]
    assert dones[0].sum() == 0 and dones[1].all() and 0 < dones[2].sum() < 65 and dones[3].sum() == 1 and dones[3][-1] == 1
    for i, pat in enumerate(tc.GAE_DONE_PATTERNS):
        g = tc.gae_case(5, 1025, pat, i)
        rew = g["raw"] * g["scale"][:, None]
        assert (np.abs(rew) > 10).any() and (np.abs(rew) < 10).any()           # one rew_scale entry makes the rewards clip
        want = dict(zero=0, one=5 * 1025, first=1025, last=1025)[pat]
        assert g["done"].sum() == want
    assert tc.gae_case(5, 1025, "first", 2)["done"][0].all() and tc.gae_case(5, 1025, "last", 3)["done"][-1].all()
    c1, c2 = tc.learn_case(9, 17, 70, 7, 0.01, 102), tc.learn_case(9, 17, 70, 7, 0.01, 102)
    assert all(np.array_equal(c1[k], c2[k]) for k in ("obs", "act", "logp_old", "value_old", "ret", "adv", "perm"))
