"""ctypes binding of include/trex_start_state.h: the start-state randomisation of a batch (trex_batch_set_start_state /
_apply_start_state / _start_state_reset / _start_state_info). A module of its own beside _capi.py, whose library handle, error check
and argument checks it uses: the signature table `_START_STATE_API` states the four C signatures once and is declared through
_capi's one declaration routine, and BatchStartState(batch) holds the calls for one _capi.Batch. trex_gym.start_state builds
specifications; a TrexVecEnv with start-state terms attached (trex_gym.start_state.attach) is the user of this module."""
import ctypes as C

from . import _capi
from ._capi import E_INVALID, TrexError, check, lib

(JOINT_POSITION, JOINT_VELOCITY, BASE_RPY, BASE_LINEAR_VELOCITY, BASE_ANGULAR_VELOCITY, BASE_POSITION,
 FLOOR_CLEARANCE) = range(7)                                    # TREX_START_*
KIND_NAMES = ("joint_position", "joint_velocity", "base_rpy", "base_linear_velocity", "base_angular_velocity", "base_position",
              "floor_clearance")
MAX_TERMS, ELEMENTS, STREAM = 16, 32, 7                         # TREX_START_MAXTERMS, the inner extent of values, TREX_START_STREAM


class TrexStartTerm(C.Structure):   # include/trex_start_state.h
    _fields_ = [("kind", C.c_int32), ("mask", C.c_uint32), ("index", C.c_int32), ("shared", C.c_int32), ("lo", C.c_float),
                ("hi", C.c_float)]


_vp, _int, _ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
_START_STATE_API = {
    "trex_batch_set_start_state": (_int, [_vp, C.POINTER(TrexStartTerm), _int, C.c_uint64, C.c_uint32]),
    "trex_batch_apply_start_state": (_int, [_vp, _vp, _int, _vp, _int, _vp]),
    "trex_batch_start_state_reset": (_int, [_vp, _vp, _vp]),
    "trex_batch_start_state_info": (_int, [_vp, _ip, _vp, _vp, _vp, _vp]),
}
START_STATE_SYMBOLS = _capi._declare(_START_STATE_API)    # every symbol include/trex_start_state.h declares


class BatchStartState:
    """The start-state randomisation of one _capi.Batch. All tensors are torch tensors on the batch's device, owned by the caller."""

    def __init__(self, batch):
        self.batch = batch
        self.num_terms = 0

    def set(self, terms=(), seed=0, env_offset=0):
        """The batch's terms (trex_batch_set_start_state): a sequence of (kind, mask, index, shared, lo, hi). seed: the Philox
        key; env_offset: the global index of the batch's env 0. Host values; an empty sequence clears. Every env starts afresh.
        -> the number of terms."""
        arr = (TrexStartTerm * max(len(terms), 1))()
        for o, (kind, mask, index, shared, lo, hi) in zip(arr, terms):
            o.kind, o.mask, o.index, o.shared, o.lo, o.hi = int(kind), int(mask), int(index), int(shared), float(lo), float(hi)
        check(lib.trex_batch_set_start_state(self.batch.h, arr, len(terms), int(seed) & (2 ** 64 - 1), int(env_offset)))
        self.num_terms = len(terms)
        return self.num_terms

    def apply(self, done, rows=None, column=0, stream=None):
        """ONE launch (trex_batch_apply_start_state): the envs whose done flag is set, that were marked by reset() or that see
        their first apply start an episode: their state is perturbed, and with rows [n, >= 3J + tail] their q, qd columns
        rewritten, the torque columns zeroed. done: f32, [n], or a row block [n, stride] whose column `column` holds the flags
        (the done column of the rows a step call wrote)."""
        b = self.batch
        n = b.num_envs
        if not hasattr(done, "dim") or done.dim() not in (1, 2) or done.shape[0] != n:
            raise TrexError(E_INVALID, "done: expected a tensor of shape [%d] or [%d, columns]" % (n, n))
        stride = 1 if done.dim() == 1 else int(done.shape[1])
        column = int(column)
        if not 0 <= column < stride:
            raise TrexError(E_INVALID, "done: column %d outside [0, %d)" % (column, stride))
        if rows is not None and (not hasattr(rows, "dim") or rows.dim() != 2 or rows.shape[0] != n):
            raise TrexError(E_INVALID, "rows: expected a tensor of shape [%d, columns]" % n)
        p = b._p(done, "float32", n * stride, "done")
        check(lib.trex_batch_apply_start_state(b.h, C.c_void_p(p.value + 4 * column), stride,
                                               None if rows is None else b._rows(rows, "rows"),
                                               0 if rows is None else int(rows.shape[1]), b._stream(stream)))

    def reset(self, mask=None, stream=None):
        """The envs with mask != 0 (uint8 or bool [n]; None: all) start an episode with their next apply
        (trex_batch_start_state_reset)."""
        check(lib.trex_batch_start_state_reset(self.batch.h, self.batch._mask(mask), self.batch._stream(stream)))

    def info(self, values=None, shift=None, lowest=None, stream=None):
        """-> the number of terms set (trex_batch_start_state_info); values [n, T, 32] f32, shift [n] f32 and lowest [n] int32
        (each optional) receive the draws of every env's current episode, the z shift of its floor placement and the collision
        point that decided it."""
        b = self.batch
        n, t = b.num_envs, C.c_int(0)
        check(lib.trex_batch_start_state_info(b.h, C.byref(t), b._p(values, "float32", n * max(self.num_terms, 1) * ELEMENTS, "values"),
                                              b._p(shift, "float32", n, "shift"), b._p(lowest, "int32", n, "lowest"),
                                              b._stream(stream)))
        return t.value
