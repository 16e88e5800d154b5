"""ctypes binding of include/trex_policy_distill.h: policy distillation on a policy object (trex_policy_distill_minibatch_grad /
_distill_minibatch_step). A module of its own beside _capi.py, whose library handle, error check and argument checks it uses: the
signature table `_DISTILL_API` states the two C signatures once, and PolicyDistill(policy) holds the calls for one _capi.Policy -
the student. trex_gym.distill.Distill is the user of this module."""
import ctypes as C

from . import _capi
from ._capi import check, lib

MSE, KL = 0, 1                     # TREX_DISTILL_MSE, TREX_DISTILL_KL
KINDS = {"mse": MSE, "kl": KL}
LEARNER_MAX_OBS_DIM = 96           # the columns the learner stages per sample

_vp, _int, _f = C.c_void_p, C.c_int, C.c_float
_DISTILL_API = {
    "trex_policy_distill_minibatch_grad": (_int, [_vp] * 7 + [C.c_int64, _vp, _int, _int, _int, _f, _f, _vp, _vp]),
    "trex_policy_distill_minibatch_step": (_int, [_vp] * 9 + [C.c_int64, _vp, _int, _int, _int] + [_f] * 6 + [_vp, _vp]),
}
DISTILL_SYMBOLS = _capi._declare(_DISTILL_API)    # every symbol include/trex_policy_distill.h declares


def kind_of(loss):
    """"mse" / "kl" or the C constant -> the C constant (an unknown number passes: the C entry refuses it)"""
    if isinstance(loss, str):
        if loss not in KINDS:
            raise ValueError("distillation loss %r: expected one of %s" % (loss, sorted(KINDS)))
        return KINDS[loss]
    return int(loss)


class PolicyDistill:
    """The distillation calls of one _capi.Policy, the student. All tensors are torch tensors on the policy's device, owned by the
    caller: obs [N, D] the student's normalised observations, teacher_mean [N, A], teacher_value [N] (None with vf_coef 0),
    teacher_logstd [A] (None for "mse")."""

    def __init__(self, policy):
        self.policy = policy

    def _common(self, obs, teacher_mean, teacher_value, teacher_logstd, perm, first, mb):
        p = self.policy
        N = obs.numel() // p.D          # (the other buffers are checked against the student's observations)
        return N, (p._p(obs, N * p.D, "obs"), p._p(teacher_mean, N * p.A, "teacher_mean"), p._p(teacher_value, N, "teacher_value"),
                   p._p(teacher_logstd, p.A, "teacher_logstd"), N, p._p(perm, first + mb, "perm", "int64"), int(first), int(mb))

    def minibatch_grad(self, theta, grad, obs, teacher_mean, teacher_value, teacher_logstd, perm, first, mb, loss="kl", vf_coef=0.5,
                       grad_scale=1.0, loss_sums=None, stream=None):
        """The gradient of perm[first : first + mb] alone, times grad_scale (trex_policy_distill_minibatch_grad): two launches."""
        p = self.policy
        _, args = self._common(obs, teacher_mean, teacher_value, teacher_logstd, perm, first, mb)
        check(lib.trex_policy_distill_minibatch_grad(
            p.h, p._p(theta, p.param_count, "theta"), p._p(grad, p.param_count, "grad"), *args, kind_of(loss), float(vf_coef),
            float(grad_scale), p._p(loss_sums, 2, "loss_sums"), p._stream(stream)))

    def minibatch_step(self, theta, grad, m, v, obs, teacher_mean, teacher_value, teacher_logstd, perm, first, mb, loss="kl",
                       vf_coef=0.5, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, loss_sums=None, stream=None):
        """One distillation step on perm[first : first + mb] (trex_policy_distill_minibatch_step): three launches."""
        p = self.policy
        P = p.param_count
        _, args = self._common(obs, teacher_mean, teacher_value, teacher_logstd, perm, first, mb)
        check(lib.trex_policy_distill_minibatch_step(
            p.h, p._p(theta, P, "theta"), p._p(grad, P, "grad"), p._p(m, P, "m"), p._p(v, P, "v"), *args, kind_of(loss),
            float(vf_coef), float(lr), float(beta1), float(beta2), float(eps), float(max_grad_norm), p._p(loss_sums, 2, "loss_sums"),
            p._stream(stream)))
