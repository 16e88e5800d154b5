"""ctypes binding of include/trex_joint_wrench.h: the joint force/torque sensor of a batch (trex_batch_joint_wrench) and the
generalised velocity with its backward difference (trex_batch_generalized_velocity). A module of its own beside _capi.py, whose
library handle, error check and argument checks it uses: the signature table `_JOINT_WRENCH_API` states the two C signatures once,
and BatchJointWrench(batch) holds the calls for one _capi.Batch. trex_gym.joint_sensor is the user of this module."""
import ctypes as C

import torch

from . import _capi
from ._capi import E_INVALID, TrexError, _shaped, check, lib

AXES_WORLD, AXES_LINK = 0, 1                       # TREX_AXES_WORLD, TREX_AXES_LINK (TREX_AXES_BASE is refused)
AXES = {"world": AXES_WORLD, "link": AXES_LINK}

_vp, _int, _f = C.c_void_p, C.c_int, C.c_float
_JOINT_WRENCH_API = {
    "trex_batch_joint_wrench": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp]),
    "trex_batch_generalized_velocity": (_int, [_vp, _vp, _vp, _f, _vp, _int, _vp, _vp]),
}
JOINT_WRENCH_SYMBOLS = _capi._declare(_JOINT_WRENCH_API)    # every symbol include/trex_joint_wrench.h declares


class BatchJointWrench:
    """The two calls for one _capi.Batch. All tensors are float32 torch tensors on the batch's device, owned by the caller."""

    def __init__(self, batch):
        self.batch = batch
        self.J, self.D, self.num_bodies = batch.J, 6 + batch.J, batch.model.num_bodies

    def _new(self, *shape):
        return torch.empty(self.batch.num_envs, *shape, dtype=torch.float32, device="cuda:%d" % self.batch.device)

    def joint_wrench(self, accel=None, wrench_a=None, wrench_b=None, axes=AXES_LINK, out=None, base_out=None, stream=None):
        """-> out [n, J, 6] (made here when None), one launch (trex_batch_joint_wrench): row k = the wrench the parent exerts on
        the child body of joint k (observation order) through the joint - force, then moment about the joint origin - at the
        current state, for the accelerations accel [n, D] (None: zeros) and the world's wrenches wrench_a + wrench_b, each
        [n, num_bodies, 6] or None (world axes, force at the COM, torque about it). axes: AXES_WORLD, AXES_LINK (the child body's
        frame) or their names. base_out [n, 6] or None: the same sums for the whole tree about the base origin, world axes."""
        b = self.batch
        n = b.num_envs
        if isinstance(axes, str):
            if axes not in AXES:
                raise TrexError(E_INVALID, "axes: expected 'world' or 'link', got %r" % (axes,))
            axes = AXES[axes]
        _shaped(accel, (n, self.D), "accel")
        _shaped(wrench_a, (n, self.num_bodies, 6), "wrench_a")
        _shaped(wrench_b, (n, self.num_bodies, 6), "wrench_b")
        _shaped(base_out, (n, 6), "base_out")
        out = self._new(self.J, 6) if out is None else _shaped(out, (n, self.J, 6), "out")
        nb6 = n * self.num_bodies * 6
        check(lib.trex_batch_joint_wrench(b.h, b._p(accel, "float32", n * self.D, "accel"), b._p(wrench_a, "float32", nb6, "wrench_a"),
                                          b._p(wrench_b, "float32", nb6, "wrench_b"), int(axes), b._p(out, "float32", n * self.J * 6, "out"),
                                          b._p(base_out, "float32", n * 6, "base_out"), b._stream(stream)))
        return out

    def generalized_velocity(self, vel=None, prev=None, inv_dt=0.0, done=None, done_column=0, accel=None, stream=None):
        """One launch (trex_batch_generalized_velocity): vel [n, D] or None receives the current generalised velocity - base
        linear, base angular, qd in observation order; with prev [n, D], accel [n, D] (required then) = (current - prev) * inv_dt
        in f32. vel may be prev itself: the latch. done: a float tensor [n], or a row block [n, stride] whose column done_column
        holds the flags; an env whose flag is non-zero gets a zero accel row. -> (vel, accel)."""
        b = self.batch
        n = b.num_envs
        _shaped(vel, (n, self.D), "vel")
        _shaped(prev, (n, self.D), "prev")
        _shaped(accel, (n, self.D), "accel")
        dp, ds = None, 0
        if done is not None:
            if not hasattr(done, "dim") or done.dim() not in (1, 2) or done.shape[0] != n:
                raise TrexError(E_INVALID, "done: expected a tensor of shape [%d] or [%d, columns]" % (n, n))
            ds = 1 if done.dim() == 1 else int(done.shape[1])
            if not 0 <= int(done_column) < ds:
                raise TrexError(E_INVALID, "done: column %d outside [0, %d)" % (done_column, ds))
            dp = C.c_void_p(b._p(done, "float32", n * ds, "done").value + 4 * int(done_column))
        check(lib.trex_batch_generalized_velocity(b.h, b._p(vel, "float32", n * self.D, "vel"), b._p(prev, "float32", n * self.D, "prev"),
                                                  float(inv_dt), dp, ds, b._p(accel, "float32", n * self.D, "accel"), b._stream(stream)))
        return vel, accel
