"""ctypes binding of include/trex_planner.h: the sampling-based planner on the device (MPPI / predictive sampling). A module of its
own beside _capi.py, whose library handle, error check and pointer checks it uses: the signature table `_PLANNER_API` states the C
signatures once, and PlannerHandle holds the calls of one TrexPlanner. The handle knows no batch: every buffer is a torch tensor on
the planner's device, owned by the caller. trex_gym.planner.Planner is the user of this module."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import check, lib

HOLD, LINEAR, CUBIC = 0, 1, 2              # TREX_PLAN_HOLD, _LINEAR, _CUBIC
KINDS = {"hold": HOLD, "linear": LINEAR, "cubic": CUBIC}
STREAM = 8                                 # TREX_PLAN_STREAM
MAX_SAMPLES, MAX_HORIZON, MAX_KNOTS, MAX_ACT = 4096, 256, 32, 64     # TREX_PLAN_MAXSAMPLES, _MAXHORIZON, _MAXKNOTS, _MAXACT

_vp, _int, _f, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
_PLANNER_API = {
    "trex_planner_create": (_int, [_int] * 7 + [C.POINTER(_vp)]),
    "trex_planner_destroy": (None, [_vp]),
    "trex_planner_info": (_int, [_vp] + [C.POINTER(_int)] * 6 + [C.POINTER(C.c_uint32), _vp]),
    "trex_planner_set_nominal": (_int, [_vp, _vp, _vp, _vp]),
    "trex_planner_get_nominal": (_int, [_vp, _vp, _vp]),
    "trex_planner_get_samples": (_int, [_vp, _vp, _vp]),
    "trex_planner_set_noise": (_int, [_vp] + [C.POINTER(_f)] * 3 + [C.c_uint64, C.c_uint32]),
    "trex_planner_sample": (_int, [_vp, _vp, _vp]),
    "trex_planner_update": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "trex_planner_shift": (_int, [_vp, _int, _vp]),
    "trex_planner_action": (_int, [_vp, _int, _vp, _vp]),
}
PLANNER_SYMBOLS = _capi._declare(_PLANNER_API)    # every symbol include/trex_planner.h declares


def kind_of(interpolation):
    """"hold" / "linear" / "cubic" or the C constant -> the C constant (an unknown number passes: the C entry refuses it)"""
    if isinstance(interpolation, str):
        if interpolation not in KINDS:
            raise ValueError("interpolation %r: expected one of %s" % (interpolation, sorted(KINDS)))
        return KINDS[interpolation]
    return int(interpolation)


class PlannerHandle:
    """One TrexPlanner: G groups of K samples, S steps, P knots, A action columns. N = G K; env e = g K + k."""

    def __init__(self, groups, samples, horizon, knots, act_dim, interpolation="cubic", device=0):
        self.h = None
        self.device = int(device)
        h = _vp()
        check(lib.trex_planner_create(int(groups), int(samples), int(horizon), int(knots), int(act_dim), kind_of(interpolation),
                                      self.device, C.byref(h)))
        self.h = h
        self.G, self.K, self.S, self.P, self.A = int(groups), int(samples), int(horizon), int(knots), int(act_dim)
        self.N = self.G * self.K
        self.kind = kind_of(interpolation)

    def close(self):
        if getattr(self, "h", None):
            lib.trex_planner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream(stream):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def _p(self, t, numel, what, dtype="float32"):
        return _capi._ptr(t, self.device, getattr(torch, dtype), numel, what)

    def info(self, stream=None):
        """dict(groups, samples, horizon, knots, act_dim, interpolation, it): `it` copied out - that synchronises the stream"""
        v = [_int() for _ in range(6)]
        it = C.c_uint32()
        check(lib.trex_planner_info(self.h, *[C.byref(x) for x in v], C.byref(it), self._stream(stream)))
        names = ("groups", "samples", "horizon", "knots", "act_dim", "interpolation")
        return dict(zip(names, (x.value for x in v)), it=it.value)

    def set_nominal(self, knots, mask=None, stream=None):
        """nominal[g] = knots[g] ([G, P, A]) for the groups with mask[g] != 0 (uint8 or bool [G]; None: all)"""
        check(lib.trex_planner_set_nominal(self.h, self._p(knots, self.G * self.P * self.A, "knots"),
                                           _capi._ptr(_capi._flags(mask, "mask"), self.device, None, self.G, "mask"), self._stream(stream)))

    def get_nominal(self, out=None, stream=None):
        out = torch.empty(self.G, self.P, self.A, device="cuda:%d" % self.device) if out is None else out
        check(lib.trex_planner_get_nominal(self.h, self._p(out, self.G * self.P * self.A, "knots"), self._stream(stream)))
        return out

    def get_samples(self, out=None, stream=None):
        out = torch.empty(self.N, self.P, self.A, device="cuda:%d" % self.device) if out is None else out
        check(lib.trex_planner_get_samples(self.h, self._p(out, self.N * self.P * self.A, "knots"), self._stream(stream)))
        return out

    def set_noise(self, sigma, lo, hi, seed=0, env_offset=0):
        """sigma, lo, hi: a scalar or A host values each. Synchronises the device; it = 0."""
        arrays = []
        for name, v in (("sigma", sigma), ("lo", lo), ("hi", hi)):
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (self.A,)) if np.ndim(v) == 0 else np.asarray(v, np.float32))
            if v.shape != (self.A,):
                raise ValueError("%s: expected a scalar or %d values, got shape %s" % (name, self.A, v.shape))
            arrays.append(v)
        ptr = [a.ctypes.data_as(C.POINTER(_f)) for a in arrays]
        check(lib.trex_planner_set_noise(self.h, ptr[0], ptr[1], ptr[2], int(seed) & (2 ** 64 - 1), int(env_offset)))

    def sample(self, actions, stream=None):
        """actions [S, N, A]: ONE launch - the samples' knots, the action block, it += 1"""
        check(lib.trex_planner_sample(self.h, self._p(actions, self.S * self.N * self.A, "actions"), self._stream(stream)))

    def update(self, reward, step_stride, env_stride, done=None, terminal=None, gamma=1.0, temperature=0.0, returns=None, weights=None,
               best=None, stats=None, stream=None):
        """reward, done: f32 tensors (or views into a row block) whose element (s, e) lies s step_stride + e env_stride floats
        behind their first: three launches. Outputs, each optional: returns [N], weights [N], best [G] int32, stats [G, 4]."""
        reach = (self.S - 1) * int(step_stride) + (self.N - 1) * int(env_stride) + 1
        check(lib.trex_planner_update(self.h, self._view(reward, reach, "reward"), int(step_stride), int(env_stride),
                                      self._view(done, reach, "done"), self._p(terminal, self.N, "terminal"), float(gamma), float(temperature),
                                      self._p(returns, self.N, "returns"), self._p(weights, self.N, "weights"),
                                      self._p(best, self.G, "best", "int32"), self._p(stats, 4 * self.G, "stats"), self._stream(stream)))

    def _view(self, t, reach, what):
        """void* of a strided f32 column: the tensor's first element, with `reach` floats of its storage behind it"""
        if t is None:
            return None
        if not t.is_cuda or t.device.index != self.device or t.dtype != torch.float32:
            raise _capi.TrexError(_capi.E_INVALID, "%s: expected an f32 tensor on cuda:%d, got %s on %s" % (what, self.device, t.dtype, t.device))
        left = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        if left < reach:
            raise _capi.TrexError(_capi.E_INVALID, "%s: expected at least %d elements behind the first, got %d" % (what, reach, left))
        return C.c_void_p(t.data_ptr())

    def shift(self, steps=1, stream=None):
        check(lib.trex_planner_shift(self.h, int(steps), self._stream(stream)))

    def action(self, actions, step=0, stream=None):
        """actions [G, A]: the nominal's clipped value at `step`"""
        check(lib.trex_planner_action(self.h, int(step), self._p(actions, self.G * self.A, "actions"), self._stream(stream)))
        return actions
