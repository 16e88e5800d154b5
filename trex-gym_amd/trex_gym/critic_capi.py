"""ctypes binding of include/trex_policy_critic.h: the privileged critic of a policy object (trex_policy_set_critic /
_critic_observe / _critic_act / _critic_minibatch_grad / _critic_minibatch_step and the critic moments). A module of its own beside
_capi.py, whose library handle, error check and argument checks it uses: the signature table `_CRITIC_API` states the eight C
signatures once, and PolicyCritic(policy) holds the calls for one _capi.Policy. trex_gym.ppo.PPO(critic=True) is the user of this
module."""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import E_INVALID, TrexError, check, lib

MAX_CRITIC_DIM = 126          # trex_policy_set_critic
LEARNER_MAX_CRITIC_DIM = 96   # the trex_policy_critic_minibatch calls: the columns the learner stages per sample and net

_vp, _int, _f, _pd = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_double)
_CRITIC_API = {
    "trex_policy_set_critic": (_int, [_vp, _int, _vp]),
    "trex_policy_critic_dim": (_int, [_vp]),
    "trex_policy_critic_get_stats": (_int, [_vp, _pd, _vp]),
    "trex_policy_critic_set_stats": (_int, [_vp, _pd, _vp]),
    "trex_policy_critic_observe": (_int, [_vp, _vp, _int, _vp]),
    "trex_policy_critic_act": (_int, [_vp, _vp, _vp, _int, _vp, _int, _f] + [_vp] * 7 + [_int, _vp]),
    "trex_policy_critic_minibatch_grad": (_int, [_vp] * 10 + [C.c_int64, _vp, _int, _int, _vp] + [_f] * 4 + [_vp, _vp]),
    "trex_policy_critic_minibatch_step": (_int, [_vp] * 12 + [C.c_int64, _vp, _int, _int, _vp] + [_f] * 8 + [_vp, _vp]),
}
CRITIC_SYMBOLS = _capi._declare(_CRITIC_API)    # every symbol include/trex_policy_critic.h declares


def layout_with_critic(layout, dv):
    """a _capi.Policy layout {name: (offset, shape)} -> the layout with vf.W1 of dv rows: the same 13 blocks in the same order, each
    on a multiple of 4 floats -> (layout, count)"""
    out, o = {}, 0
    for name, (_, shape) in layout.items():
        shape = (int(dv), shape[1]) if name == "vf.W1" else tuple(shape)
        out[name] = (o, shape)
        o = (o + math.prod(shape) + 3) & ~3
    return out, o


class PolicyCritic:
    """The privileged critic of one _capi.Policy. All tensors are torch tensors on the policy's device, owned by the caller. While
    dim != 0 the policy's own act / minibatch_grad / minibatch_step refuse; `layout` and `param_count` are those in force (the
    policy object's own attributes keep describing the symmetric layout it was made with)."""

    def __init__(self, policy):
        self.policy = policy
        self.dim = 0
        self.layout, self.param_count = dict(policy.layout), policy.param_count

    def set(self, dim):
        """The critic width (trex_policy_set_critic): 1 .. 126, 0 clears. The critic moments start afresh; synchronises. -> dim"""
        p = self.policy
        check(lib.trex_policy_set_critic(p.h, int(dim), p._stream(None)))
        self.dim = int(dim)
        self.param_count = lib.trex_policy_param_count(p.h)
        off = (C.c_int * 13)()
        check(lib.trex_policy_param_offsets(p.h, off))
        self.layout = {n: (int(o), ((self.dim or p.D, p.H) if n == "vf.W1" else tuple(sh)))
                       for (n, (_, sh)), o in zip(p.layout.items(), off)}
        return self.dim

    def get_stats(self):
        """dict of the critic's running moments (host, f64): mean [Dv], var [Dv], count"""
        Dv = self.dim
        buf = (C.c_double * (2 * max(Dv, 1) + 1))()
        check(lib.trex_policy_critic_get_stats(self.policy.h, buf, self.policy._stream(None)))
        a = np.array(buf[:])
        return dict(mean=a[:Dv], var=a[Dv:2 * Dv], count=a[2 * Dv])

    def set_stats(self, st):
        Dv = self.dim
        a = np.concatenate([np.asarray(st["mean"], float).reshape(Dv), np.asarray(st["var"], float).reshape(Dv), [st["count"]]])
        check(lib.trex_policy_critic_set_stats(self.policy.h, (C.c_double * (2 * max(Dv, 1) + 1))(*a), self.policy._stream(None)))

    def _rows(self, rows_v, what="rows_v"):
        """a [n, stride] block or None -> (pointer, stride)"""
        p = self.policy
        if rows_v is None:
            return None, 0
        if not hasattr(rows_v, "dim") or rows_v.dim() != 2 or rows_v.shape[0] != p.n:
            raise TrexError(E_INVALID, "%s: expected a tensor of shape [%d, %d or more]" % (what, p.n, self.dim))
        stride = int(rows_v.shape[1])
        return p._p(rows_v, (p.n - 1) * stride + min(self.dim, stride), what), stride

    def observe(self, rows_v, stream=None):
        """Fold the columns [0, dim) of rows_v [n, stride] into the critic moments (trex_policy_critic_observe)."""
        ptr, stride = self._rows(rows_v)
        check(lib.trex_policy_critic_observe(self.policy.h, ptr, stride, self.policy._stream(stream)))

    def act(self, theta, rows, rows_v, noise, actions, obs_out=None, obs_v_out=None, act_out=None, logp_out=None, value_out=None,
            clip_obs=10.0, value_only=False, stream=None):
        """Policy.act with a critic row (trex_policy_critic_act). rows_v None: the policy alone (value_out and obs_v_out must be None);
        value_only: rows, noise and actions may be None."""
        p = self.policy
        n, D, A, Dv = p.n, p.D, p.A, self.dim
        rp = p._p(rows, (n - 1) * rows.shape[1] + min(D, rows.shape[1]), "rows") if rows is not None else None   # (a short stride: the C entry's refusal)
        vp, sv = self._rows(rows_v)
        check(lib.trex_policy_critic_act(
            p.h, p._p(theta, self.param_count, "theta"), rp, int(rows.shape[1]) if rows is not None else 0, vp, sv, float(clip_obs),
            p._p(noise, n * A, "noise"), p._p(actions, n * A, "actions"), p._p(obs_out, n * D, "obs_out"),
            p._p(obs_v_out, n * Dv, "obs_v_out"), p._p(act_out, n * A, "act_out"), p._p(logp_out, n, "logp_out"),
            p._p(value_out, n, "value_out"), int(bool(value_only)), p._stream(stream)))

    def adam(self, theta, grad, m, v, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, grad_norm_out=None, stream=None):
        """Policy.adam on vectors of the layout in force (trex_policy_adam: the C entry takes the count from the object, the
        policy's own binding checks lengths against the symmetric count it was made with)."""
        p, P = self.policy, self.param_count
        check(lib.trex_policy_adam(p.h, p._p(theta, P, "theta"), p._p(grad, P, "grad"), p._p(m, P, "m"), p._p(v, P, "v"), float(lr),
                                   float(beta1), float(beta2), float(eps), float(max_grad_norm),
                                   p._p(grad_norm_out, 1, "grad_norm_out"), p._stream(stream)))

    def minibatch_grad(self, theta, grad, obs, obs_v, act, logp, val, adv, ret, perm, first, mb, adv_stats, cliprange=0.2,
                       ent_coef=0.0, vf_coef=0.5, grad_scale=1.0, loss_sums=None, stream=None):
        """Policy.minibatch_grad with obs_v [N, dim] behind obs (trex_policy_critic_minibatch_grad)."""
        p = self.policy
        P, N, D, A = self.param_count, adv.numel(), p.D, p.A
        check(lib.trex_policy_critic_minibatch_grad(
            p.h, p._p(theta, P, "theta"), p._p(grad, P, "grad"), p._p(obs, N * D, "obs"), p._p(obs_v, N * self.dim, "obs_v"),
            p._p(act, N * A, "act"), p._p(logp, N, "logp"), p._p(val, N, "val"), p._p(adv, N, "adv"), p._p(ret, N, "ret"), N,
            p._p(perm, first + mb, "perm", "int64"), int(first), int(mb), p._p(adv_stats, 2, "adv_stats"), float(cliprange),
            float(ent_coef), float(vf_coef), float(grad_scale), p._p(loss_sums, 2, "loss_sums"), p._stream(stream)))

    def minibatch_step(self, theta, grad, m, v, obs, obs_v, act, logp, val, adv, ret, perm, first, mb, adv_stats, cliprange=0.2,
                       ent_coef=0.0, vf_coef=0.5, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, loss_sums=None,
                       stream=None):
        """Policy.minibatch_step with obs_v [N, dim] behind obs (trex_policy_critic_minibatch_step): three launches."""
        p = self.policy
        P, N, D, A = self.param_count, adv.numel(), p.D, p.A
        check(lib.trex_policy_critic_minibatch_step(
            p.h, p._p(theta, P, "theta"), p._p(grad, P, "grad"), p._p(m, P, "m"), p._p(v, P, "v"), p._p(obs, N * D, "obs"),
            p._p(obs_v, N * self.dim, "obs_v"), p._p(act, N * A, "act"), p._p(logp, N, "logp"), p._p(val, N, "val"),
            p._p(adv, N, "adv"), p._p(ret, N, "ret"), N, p._p(perm, first + mb, "perm", "int64"), int(first), int(mb),
            p._p(adv_stats, 2, "adv_stats"), float(cliprange), float(ent_coef), float(vf_coef), float(lr), float(beta1),
            float(beta2), float(eps), float(max_grad_norm), p._p(loss_sums, 2, "loss_sums"), p._stream(stream)))
