"""tests/distill_ref.py qualified on the CPU, alone, before tests/test_gpu_distill.py measures the kernels with it.

Two independent witnesses:
  * the LOSSES against torch.distributions (kl_divergence of two Normals, f64) and a per-sample loop for the squared errors: this
    is what fixes the direction of the KL and the 1 / mb;
  * the analytic GRADIENTS against central differences of distill_ref.loss, per parameter block: on SAMPLE elements of every block
    (the largest in magnitude and a random draw), relative error |fd - g|_2 / |g|_2 over the sampled elements.

The allowed gradient error is measured from the step-size sweep of the reference itself (`PYTHONPATH=. python tests/test_distill_ref.py`
prints it): at h = 1e-3, 1e-4, 1e-5, 1e-6, 1e-7 the worst block of all cases and kinds below is off by 2.5e-6, 2.5e-8, 2.9e-8, 2.8e-7,
3.8e-6 - truncation (h^2) above h = 1e-4, rounding (a loss of about 30 known to 1e-16, over h, against gradient elements of 1e-2)
below 1e-5, a floor of 3e-8 between them. The test takes h = 1e-5 and allows FD_RTOL = 3e-7: ten times the floor measured there,
and more than four orders of magnitude below the effect of the smallest planted mistake (each moves its block by more than 1e-2).

The four planted mistakes (distill_ref.MISTAKES) are each rejected by one of the two witnesses: the KL taken the other way round and
a missing 1 / mb - wrong in the loss and its gradient alike, which central differences of the same wrong loss would pass - by the
loss witness; the teacher's variance dropped from the logstd gradient and vf_coef applied twice by the gradient witness."""
import numpy as np
import pytest

import distill_cases as dc
import distill_ref as DR

FD_H, FD_RTOL = 1e-5, 3e-7
HOST_SHAPES = ["dims_D1_A1", "dims_D33_A1", "dims_D75_A25", "mb31_first5"]
KEYS = [net + k for net in ("pi", "vf") for k in (".0.weight", ".0.bias", ".2.weight", ".2.bias", ".4.weight", ".4.bias")] + ["logstd"]


def _minibatch(name):
    c = dc.case_by_name(name)
    i = c["idx"]
    return c["params"], c["obs"][i], c["tmean"][i], c["tvalue"][i], c["tlogstd"]


def _sample(g, rng, k=12):
    """flat indices of a block: its k largest elements and k random ones"""
    flat = np.abs(g).reshape(-1)
    return np.unique(np.concatenate([np.argsort(flat)[-k:], rng.integers(0, flat.size, k)]))


def block_errors(name, kind, vf_coef, h, mistake=None):
    """{block: relative error of the analytic gradient against central differences of the (true) loss on its sampled elements}"""
    params, obs, tm, tv, tl = _minibatch(name)
    _, grads = DR.loss_and_grads(params, obs, tm, tv, tl, kind, vf_coef, mistake=mistake)
    rng = np.random.default_rng(7)
    out = {}
    for key in KEYS:
        g = np.asarray(grads[key], np.float64)
        idx = _sample(g, rng)
        fd = np.zeros(len(idx))
        for j, i in enumerate(idx):
            p = dict(params)
            for sign in (1.0, -1.0):
                w = params[key].copy()
                w.reshape(-1)[i] += sign * h
                p[key] = w
                fd[j] += sign * DR.loss(p, obs, tm, tv, tl, kind, vf_coef)[0]
        fd /= 2.0 * h
        ga = g.reshape(-1)[idx]
        denom = np.linalg.norm(ga)
        out[key] = np.linalg.norm(fd - ga) / denom if denom > 0 else np.linalg.norm(fd)
    return out


def witness_losses(name, kind, vf_coef):
    """(L_pi, L_vf) without distill_ref's formulas: torch.distributions for the KL, plain loops for the squared errors"""
    import torch
    params, obs, tm, tv, tl = _minibatch(name)
    mean, logstd, v = DR.forward(params, obs)
    n = len(v)
    if kind == DR.KL:
        N = torch.distributions.Normal
        t = N(torch.from_numpy(tm), torch.from_numpy(np.exp(tl)).expand(tm.shape))
        s = N(torch.from_numpy(mean), torch.from_numpy(np.exp(logstd)).expand(tm.shape))
        l_pi = float(torch.distributions.kl_divergence(t, s).sum(-1).mean())
    else:
        l_pi = sum(0.5 * float(np.dot(mean[i] - tm[i], mean[i] - tm[i])) for i in range(n)) / n
    l_vf = sum(0.5 * (v[i] - tv[i]) ** 2 for i in range(n)) / n
    return l_pi, l_vf


@pytest.mark.parametrize("kind", [k for _, k in dc.KINDS], ids=[n for n, _ in dc.KINDS])
@pytest.mark.parametrize("name", HOST_SHAPES)
def test_losses_agree_with_an_independent_witness(name, kind):
    params, obs, tm, tv, tl = _minibatch(name)
    for vf_coef in dc.VF_COEFS:
        out, _ = DR.loss_and_grads(params, obs, tm, tv, tl, kind, vf_coef)
        l, l_pi, l_vf = DR.loss(params, obs, tm, tv, tl, kind, vf_coef)
        w_pi, w_vf = witness_losses(name, kind, vf_coef)
        assert out["pi_loss"] > 0 and out["vf_loss"] > 0
        np.testing.assert_allclose([out["pi_loss"], out["vf_loss"], l_pi, l_vf], [w_pi, w_vf, w_pi, w_vf], rtol=1e-12)
        np.testing.assert_allclose([out["loss"], l], w_pi + vf_coef * w_vf, rtol=1e-12)


@pytest.mark.parametrize("kind", [k for _, k in dc.KINDS], ids=[n for n, _ in dc.KINDS])
@pytest.mark.parametrize("name", HOST_SHAPES)
def test_gradients_agree_with_central_differences(name, kind):
    err = block_errors(name, kind, 0.5, FD_H)
    print("%s kind %d: worst block %.2e" % (name, kind, max(err.values())))
    assert max(err.values()) <= FD_RTOL, err
    _, grads = DR.loss_and_grads(*_minibatch(name), kind, 0.5)
    assert all(np.abs(grads[k]).max() > 0 for k in KEYS if not (kind == DR.MSE and k == "logstd"))
    if kind == DR.MSE:
        assert not grads["logstd"].any()


def test_vf_coef_zero_and_an_absent_teacher_value():
    params, obs, tm, tv, tl = _minibatch("dims_D75_A25")
    a, ga = DR.loss_and_grads(params, obs, tm, tv, tl, DR.KL, 0.0)
    b, gb = DR.loss_and_grads(params, obs, tm, None, tl, DR.KL, 0.0)
    assert all(not ga[k].any() and not gb[k].any() for k in KEYS if k.startswith("vf."))
    assert all(np.array_equal(ga[k], gb[k]) for k in KEYS) and a["pi_loss"] == b["pi_loss"] and b["vf_loss"] == 0.0 < a["vf_loss"]


@pytest.mark.parametrize("mistake", DR.MISTAKES)
def test_planted_mistakes_are_rejected(mistake):
    name, vf_coef = "dims_D75_A25", 0.5
    params, obs, tm, tv, tl = _minibatch(name)
    out, _ = DR.loss_and_grads(params, obs, tm, tv, tl, DR.KL, vf_coef, mistake=mistake)
    w_pi, w_vf = witness_losses(name, DR.KL, vf_coef)
    loss_off = max(abs(out["pi_loss"] - w_pi) / w_pi, abs(out["vf_loss"] - w_vf) / w_vf)
    err = block_errors(name, DR.KL, vf_coef, FD_H, mistake=mistake)
    print("%s: losses off by %.2e; worst gradient block %.2e" % (mistake, loss_off, max(err.values())))
    caught_by_loss, caught_by_gradient = loss_off > 1e-12, max(err.values()) > FD_RTOL
    assert caught_by_loss == (mistake in ("kl_swapped", "no_inv_mb"))
    assert caught_by_gradient and max(err.values()) > 1e-2
    if mistake == "no_teacher_var":
        assert err["logstd"] > 1e-2 and max(v for k, v in err.items() if k != "logstd") <= FD_RTOL
    if mistake == "vf_coef_twice":
        assert min(v for k, v in err.items() if k.startswith("vf.")) > 1e-2 and max(v for k, v in err.items() if not k.startswith("vf.")) <= FD_RTOL


if __name__ == "__main__":
    for h in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
        worst = max(max(block_errors(n, k, 0.5, h).values()) for n in HOST_SHAPES for _, k in dc.KINDS)
        print("h %.0e: worst block, all cases and kinds: %.2e" % (h, worst))
