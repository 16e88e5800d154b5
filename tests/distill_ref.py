"""f64 restatement of policy distillation as include/trex_policy_distill.h defines it, written from the header: the forward pass is
oracle/ppo_oracle.py's (mlp_forward / mlp_backward imported, not copied, as tests/critic_ref.py does), the two losses and their
analytic gradients are stated here. tests/test_distill_ref.py qualifies this module alone - gradients against central differences
of `loss`, the losses against an independent witness - before tests/test_gpu_distill.py measures the kernels with it.
A helper, not a conftest."""
import numpy as np

from oracle.ppo_oracle import mlp_backward, mlp_forward

MSE, KL = 0, 1      # TREX_DISTILL_MSE, TREX_DISTILL_KL

# what tests/test_distill_ref.py plants to show that its checks can fail (never set by anything else)
MISTAKES = ("kl_swapped", "no_inv_mb", "no_teacher_var", "vf_coef_twice")


def forward(params, obs):
    """student: mean [n, A], logstd [A], value [n]"""
    mean, _ = mlp_forward(params, "pi", obs)
    value, _ = mlp_forward(params, "vf", obs)
    return mean, params["logstd"], value[:, 0]


def policy_terms(kind, mean, logstd, tmean, tlogstd):
    """per-sample policy loss [n]: half the squared error of the means, or KL(teacher || student) of the diagonal Gaussians"""
    d = mean - tmean
    if kind == MSE:
        return 0.5 * np.sum(d * d, -1)
    var_s, var_t = np.exp(2.0 * logstd), np.exp(2.0 * tlogstd)
    return np.sum(logstd - tlogstd + (var_t + d * d) / (2.0 * var_s) - 0.5, -1)


def loss(params, obs, tmean, tvalue, tlogstd, kind, vf_coef):
    """-> (L, L_pi, L_vf): means over the n samples; L = L_pi + vf_coef L_vf. tvalue None: L_vf = 0 (vf_coef must be 0)."""
    mean, logstd, v = forward(params, obs)
    l_pi = np.mean(policy_terms(kind, mean, logstd, tmean, tlogstd))
    l_vf = 0.0 if tvalue is None else 0.5 * np.mean((v - tvalue) ** 2)
    return l_pi + vf_coef * l_vf, l_pi, l_vf


def loss_and_grads(params, obs, tmean, tvalue, tlogstd, kind, vf_coef, mistake=None):
    """-> (dict(loss, pi_loss, vf_loss, mean, value), gradients in oracle naming: '<net>.<0|2|4>.<weight|bias>' [out, in], 'logstd').
    mistake: one of MISTAKES - a wrong statement on purpose, for the reference's own qualification."""
    assert mistake is None or mistake in MISTAKES
    n, A = tmean.shape
    mean, acts_pi = mlp_forward(params, "pi", obs)
    vout, acts_vf = mlp_forward(params, "vf", obs)
    v, logstd = vout[:, 0], params["logstd"]
    inv = 1.0 if mistake == "no_inv_mb" else 1.0 / n
    d = mean - tmean
    if kind == MSE:
        terms = 0.5 * np.sum(d * d, -1)
        dmean, dlogstd = d * inv, np.zeros(A)
    elif mistake == "kl_swapped":      # KL(student || teacher)
        var_s, var_t = np.exp(2.0 * logstd), np.exp(2.0 * tlogstd)
        terms = np.sum(tlogstd - logstd + (var_s + d * d) / (2.0 * var_t) - 0.5, -1)
        dmean, dlogstd = d / var_t * inv, np.sum(-1.0 + var_s / var_t + 0.0 * d, 0) * inv
    else:
        var_s, var_t = np.exp(2.0 * logstd), np.exp(2.0 * tlogstd)
        terms = np.sum(logstd - tlogstd + (var_t + d * d) / (2.0 * var_s) - 0.5, -1)
        dmean = d / var_s * inv
        dlogstd = np.sum(1.0 - ((0.0 if mistake == "no_teacher_var" else var_t) + d * d) / var_s, 0) * inv
    pi_loss = np.sum(terms) * inv
    grads = {}
    mlp_backward(params, "pi", acts_pi, dmean, grads)
    grads["logstd"] = dlogstd
    if tvalue is None:
        assert vf_coef == 0.0
        vf_loss, dv = 0.0, np.zeros(n)
    else:
        vf_loss = 0.5 * np.sum((v - tvalue) ** 2) * inv
        dv = vf_coef * (vf_coef if mistake == "vf_coef_twice" else 1.0) * (v - tvalue) * inv
    mlp_backward(params, "vf", acts_vf, dv[:, None], grads)
    return dict(loss=pi_loss + vf_coef * vf_loss, pi_loss=pi_loss, vf_loss=vf_loss, mean=mean, value=v), grads
