"""ctypes binding of include/trex_dynamics_derivatives.h: the derivatives of the inverse dynamics of a batch along the configuration
tangent and the generalised velocity (trex_batch_inverse_dynamics_derivatives). A module of its own beside _capi.py, whose library
handle, error check and argument checks it uses: the signature table `_DERIVATIVES_API` states the C signature once, and
BatchDerivatives(batch) holds the call for one _capi.Batch. trex_gym.derivatives is the user of this module."""
import ctypes as C

import torch

from . import _capi
from ._capi import E_INVALID, TrexError, _shaped, check, lib

BY_DIRECTION = 1                                   # TREX_DERIV_BY_DIRECTION

_vp, _int, _u32 = C.c_void_p, C.c_int, C.c_uint32
_DERIVATIVES_API = {
    "trex_batch_inverse_dynamics_derivatives": (_int, [_vp, _vp, _vp, _vp, _u32, _vp]),
}
DERIVATIVES_SYMBOLS = _capi._declare(_DERIVATIVES_API)      # every symbol include/trex_dynamics_derivatives.h declares


class BatchDerivatives:
    """The call for one _capi.Batch. All tensors are float32 torch tensors on the batch's device, owned by the caller."""

    def __init__(self, batch):
        self.batch = batch
        self.J, self.D = batch.J, 6 + batch.J

    def _new(self):
        return torch.empty(self.batch.num_envs, self.D, self.D, dtype=torch.float32, device="cuda:%d" % self.batch.device)

    def inverse_dynamics_derivatives(self, accel=None, dfdq=True, dfdv=True, flags=0, stream=None):
        """-> (dfdq, dfdv), one launch (trex_batch_inverse_dynamics_derivatives): the [n, D, D] derivatives of the generalised force
        M a + h at the current state and the accelerations accel [n, D] (None: zeros) along the configuration tangent and the
        generalised velocity. dfdq, dfdv: a tensor [n, D, D] to fill, True (made here) or None / False (not computed: no passes;
        returned as None). flags: 0 - out[n, i, j] = d f_i / d x_j - or BY_DIRECTION - out[n, j, i], the rhs layout of solve_mass."""
        b = self.batch
        n, D = b.num_envs, self.D
        _shaped(accel, (n, D), "accel")
        outs = []
        for name, o in (("dfdq", dfdq), ("dfdv", dfdv)):
            if o is None or o is False:
                outs.append(None)
            else:
                outs.append(self._new() if o is True else _shaped(o, (n, D, D), name))
        if outs[0] is None and outs[1] is None:
            raise TrexError(E_INVALID, "inverse_dynamics_derivatives: neither dfdq nor dfdv is asked for")
        check(lib.trex_batch_inverse_dynamics_derivatives(b.h, b._p(accel, "float32", n * D, "accel"), b._p(outs[0], "float32", n * D * D, "dfdq"),
                                                          b._p(outs[1], "float32", n * D * D, "dfdv"), int(flags), b._stream(stream)))
        return outs[0], outs[1]
