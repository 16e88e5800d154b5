"""Qualifies the cases of tests/ik_cases.py on the f64 reference alone (tests/ik_ref.py), without a GPU: every reachable draw the
GPU tests use is solved by the reference to 1e-5 m / rad in 30 iterations at the defaults - so that the GPU's fixed bound of 1e-4
is ten times what the reference leaves - and the unreachable draws end at a stationary point with joints on their limits."""
import numpy as np
import pytest

import ik_cases as C
import ik_ref as IK

N = 67                      # the draws per form the GPU tests run
N_UNREACHABLE = 16
FORMS = ["pos4", "head_ori", "three_ori", "k1", "k8", "same_body", "one_leg", "one_leg_ori"]


def test_forms_cover_what_they_should(model):
    forms = {f.name: f for f in C.forms(model)}
    assert list(forms) == FORMS
    rows = {n: IK.task_rows(f.modes) for n, f in forms.items()}
    assert rows["head_ori"] == 15 and rows["three_ori"] == 21 and rows["k1"] == 3 and rows["k8"] == 24
    assert len(forms["k1"].links) == 1 and len(forms["k8"].links) == 8
    p = C.pick(model)
    lb, depth = np.asarray(model["link_body"], int), np.asarray(model["depth"], int)
    assert depth[lb[p["deepest"]]] == depth.max() and lb[p["head"]] == int(model["head_body"])
    # the two toes hang on different legs: their chains share no joint
    assert not set(C.chain_joints(model, p["toe_a"])) & set(C.chain_joints(model, p["toe_b"]))
    assert "toe" in model["link_names"][p["toe_a"]] and "toe" in model["link_names"][p["toe_b"]]
    sb = forms["same_body"]
    assert sb.links[0] == sb.links[1] and sb.points[0] != sb.points[1]
    leg = forms["one_leg"].joints
    assert leg == C.chain_joints(model, p["toe_a"]) and 0 < len(leg) < model["nb"] - 1
    # the rank-deficient task: two points of one body give a 6-row matrix of rank 5 at most (their distance cannot change), and
    # of no more than the number of joints that carry the body
    c = C.reachable(model, sb, 1)[0]
    pT, qT = IK.world_targets(model, c.state, c.targets["world"])
    _, A, _, _ = IK.error(model, c.state, sb.links, sb.points, sb.modes, pT, qT)
    sv = np.linalg.svd(A, compute_uv=False)
    assert int((sv > 1e-9 * sv[0]).sum()) == min(5, len(C.chain_joints(model, sb.links[0]))) and sv[5] < 1e-12 * sv[0]


@pytest.mark.parametrize("name", FORMS)
def test_reference_solves_every_reachable_draw(name, model):
    form = [f for f in C.forms(model) if f.name == name][0]
    lo, hi = IK.limits(model)
    worst = 0.0
    for i, c in enumerate(C.reachable(model, form, N)):
        assert (c.q_star >= lo).all() and (c.q_star <= hi).all() and np.abs(c.q_star - c.q_start).max() > 0.01
        r = C.reference(model, form, c, iterations=30)
        res = max(r["position_error"], r["orientation_error"])
        worst = max(worst, res)
        assert res <= 1e-5, (name, i, res)
        assert r["initial_error"] > 1e-3
    print("%s: largest reference residual after 30 iterations %.3g" % (name, worst))


def test_unreachable_draws_end_stationary_on_the_limits(model):
    form, cases = C.unreachable(model, N_UNREACHABLE)
    lo, hi = IK.limits(model)
    for i, c in enumerate(cases):
        r = C.reference(model, form, c, iterations=30)
        n = r["norms"]
        at_limit = int(((r["q"] <= lo) | (r["q"] >= hi)).sum())
        print("unreachable %d: |e| %.3f -> %.4f, change over the last 5 iterations %.2g, %d joints at a limit"
              % (i, n[0], n[-1], abs(n[-1] - n[-6]) / n[-1], at_limit))
        assert n[-1] > 0.3                                           # it IS out of reach
        assert n[-1] < n[0]                                          # the norm came down ...
        assert abs(n[-1] - n[-6]) <= 1e-3 * n[-1]                    # ... and is flat: a stationary point of the clamped iteration
        assert at_limit >= 2
        assert np.isfinite(r["q"]).all() and (r["q"] >= lo).all() and (r["q"] <= hi).all()
