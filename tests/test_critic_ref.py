"""tests/critic_ref.py - the f64 reference of the asymmetric actor-critic - against oracle/ppo_oracle.py, against finite
differences and against the layout rule of tests/trainer_cases.py; and the cases of tests/critic_cases.py qualified on the CPU.
Host-only."""
import numpy as np
import pytest

import critic_cases as cc
import critic_ref as CR
import trainer_cases as tc
from oracle import ppo_oracle as P


def _small(D, Dv, A, n, seed):
    rng = np.random.default_rng(seed)
    params = cc._mix(tc.make_params(D, A, rng), tc.make_params(Dv, A, rng))
    obs, obs_v = rng.standard_normal((n, D)), rng.standard_normal((n, Dv))
    mean, logstd, v = CR.forward(params, obs, obs_v)
    act = P.sample_action(mean, logstd, rng.standard_normal((n, A)))
    nlp_old = P.neglogp(mean, logstd, act) + 0.3 * rng.standard_normal(n)
    value_old = v + 0.3 * rng.standard_normal(n)
    ret = value_old + rng.standard_normal(n)
    adv = 2.0 * rng.standard_normal(n) + 0.5
    return params, obs, obs_v, act, nlp_old, value_old, adv, ret


def test_with_one_row_for_both_nets_it_is_the_oracle_exactly():
    params, obs, _, act, nlp_old, value_old, adv, ret = _small(7, 7, 3, 19, 1)
    want_out, want_g = P.ppo_loss_and_grads(params, obs, act, nlp_old, value_old, adv, ret, ent_coef=0.01)
    got_out, got_g = CR.loss_and_grads(params, obs, obs, act, nlp_old, value_old, adv, ret, ent_coef=0.01)
    assert set(got_g) == set(want_g) and set(got_out) == set(want_out)
    assert all(np.array_equal(got_g[k], want_g[k]) for k in want_g)
    assert all(np.array_equal(got_out[k], want_out[k]) for k in want_out)
    m, ls, v = CR.forward(params, obs, obs)
    m0, ls0, v0 = P.policy_forward(params, obs)
    assert np.array_equal(m, m0) and np.array_equal(v, v0) and ls is ls0


def test_every_gradient_block_against_central_differences():
    """D = 3, Dv = 5, A = 2, n = 7: d loss / d parameter by central differences, step 1e-6, for every element of every block. The
    samples are moved off the branch edges of max() and clip() first (a difference across an edge is no derivative)."""
    D, Dv, A, n = 3, 5, 2, 7
    for seed in range(2, 40):
        args = _small(D, Dv, A, n, seed)
        params, obs, obs_v, act, nlp_old, value_old, adv, ret = args
        out, _ = CR.loss_and_grads(*args, ent_coef=0.01)
        v = out["value"]
        vclip = value_old + np.clip(v - value_old, -0.2, 0.2)
        edges = np.concatenate([np.abs(out["ratio"] - 0.8), np.abs(out["ratio"] - 1.2), np.abs(np.abs(v - value_old) - 0.2),
                                np.abs((v - ret) ** 2 - (vclip - ret) ** 2)[np.abs(v - value_old) > 0.2]])
        if edges.min() > 1e-2:
            break
    else:
        raise AssertionError("no well-conditioned draw")
    _, grads = CR.loss_and_grads(*args, ent_coef=0.01)
    assert grads["vf.0.weight"].shape == (64, Dv) and grads["pi.0.weight"].shape == (64, D)
    h, worst = 1e-6, 0.0
    for key in cc.PI_KEYS + cc.VF_KEYS:
        flat = params[key].reshape(-1)          # a view: the elements are moved in place and put back
        num = np.empty_like(flat)
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + h
            up = CR.loss_and_grads(*args, ent_coef=0.01)[0]["loss"]
            flat[i] = keep - h
            dn = CR.loss_and_grads(*args, ent_coef=0.01)[0]["loss"]
            flat[i] = keep
            num[i] = (up - dn) / (2 * h)
        g = grads[key].reshape(-1)
        worst = max(worst, float(np.abs(num - g).max()))
        np.testing.assert_allclose(num, g, rtol=1e-5, atol=1e-8, err_msg=key)
    print("largest |finite difference - gradient| over all blocks: %.2e" % worst)


@pytest.mark.parametrize("D,A", [(1, 1), (75, 25), (93, 25), (126, 32)])
def test_layout_rule_with_a_critic_width(D, A):
    assert CR.layout_rule(D, A) == tc.layout_rule(D, A) == CR.layout_rule(D, A, D)
    for Dv in (1, 9, 96, 126):
        lay, count = CR.layout_rule(D, A, Dv)
        sym, _ = tc.layout_rule(D, A)
        assert list(lay) == tc.PARAM_NAMES and all(o % 4 == 0 for o, _ in lay.values()) and count % 4 == 0
        assert lay["vf.W1"] == (sym["vf.W1"][0], (Dv, 64))
        assert all(lay[k] == sym[k] for k in tc.PARAM_NAMES[:6])                           # the policy net does not move
        shift = lay["vf.b1"][0] - sym["vf.b1"][0]
        assert shift == ((Dv * 64 + 3) & ~3) - ((D * 64 + 3) & ~3)
        assert all(lay[k] == (sym[k][0] + shift, sym[k][1]) for k in tc.PARAM_NAMES[7:])   # what follows vf.W1 moves as one
        # the binding's own restatement (it rebuilds the layout from the 13 offsets the library reports)
        from trex_gym import critic_capi
        assert critic_capi.layout_with_critic({k: (o, tuple(s)) for k, (o, s) in sym.items()}, Dv) == (lay, count)


@pytest.mark.parametrize("index", range(len(cc.ACT_CASES)), ids=["D%d_Dv%d_A%d_n%d" % c for c in cc.ACT_CASES])
def test_act_cases_are_what_the_reference_computes(index):
    D, Dv, A, n = cc.ACT_CASES[index]
    c = cc.act_case(D, Dv, A, n, index)
    assert c["stride_v"] != c["row_stride"] and c["stride_v"] >= Dv and c["rows"].shape == (n, c["row_stride"])
    obs_n = CR.normalise(c["rows"][:, :D], c["stats"]["obs_mean"], c["stats"]["obs_var"])
    obs_v_n = CR.normalise(c["rows_v"][:, :Dv], c["stats_v"]["mean"], c["stats_v"]["var"])
    assert np.array_equal(obs_n, c["obs_n"]) and np.array_equal(obs_v_n, c["obs_v_n"])
    mean, logstd, value = CR.forward(c["params"], obs_n, obs_v_n)
    assert np.array_equal(P.sample_action(mean, logstd, c["noise"]), c["actions"]) and np.array_equal(value, c["value"])
    # the two halves differ: rows, moments, parameters
    k = min(D, Dv)
    assert n * k == 1 or not np.array_equal(c["rows"][:, :k], c["rows_v"][:, :k])     # (a single element: the generator's clipping value)
    assert not np.array_equal(c["stats"]["obs_mean"][:k], c["stats_v"]["mean"][:k])
    assert not np.array_equal(c["params"]["pi.2.weight"], c["params"]["vf.2.weight"])
    assert (np.abs(obs_n) == 10.0).any() and (np.abs(obs_v_n) == 10.0).any()


@pytest.mark.parametrize("index", range(len(cc.LEARN_CASES)), ids=["D%d_Dv%d_A%d_mb%d_first%d" % c for c in cc.LEARN_CASES])
def test_learn_cases_are_well_conditioned_and_made_of_their_halves(index):
    c = cc.learn_case_by_index(index)
    bad = tc.learn_violations(c["q"])
    assert not any(b.any() for b in bad.values()), {k: int(v.sum()) for k, v in bad.items()}
    g, gp, gv = c["q"]["grads"], c["pi"]["q"]["grads"], c["vf"]["q"]["grads"]
    for k in cc.PI_KEYS:
        assert np.array_equal(g[k], gp[k]), k                     # the same statements on the same numbers
    for k in cc.VF_KEYS:                                          # (the same samples in another order: the sums round differently)
        np.testing.assert_allclose(g[k], gv[k], rtol=1e-9, atol=1e-12 * np.abs(gv[k]).max(), err_msg=k)
    assert c["obs_v"].shape == (c["N"], c["Dv"]) and c["obs"].shape == (c["N"], c["D"])
    assert c["q"]["vf_clip"].any() and c["q"]["pg_clip"].any() or c["mb"] < 40
