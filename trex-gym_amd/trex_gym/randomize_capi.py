"""ctypes binding of include/trex_randomize.h: the episode randomisation of a batch (trex_batch_set_randomization /
_apply_randomization / _randomization_reset / _randomization_info). A module of its own beside _capi.py, whose library handle, error
check and argument checks it uses: the signature table `_RANDOMIZE_API` states the four C signatures once, and
BatchRandomization(batch) holds the calls for one _capi.Batch. trex_gym.randomize builds specifications; a TrexVecEnv with
randomisation attached (trex_gym.randomize.attach) is the user of this module."""
import ctypes as C

from . import _capi
from ._capi import E_INVALID, TrexError, check, lib

MASS, FRICTION, KP, KD, MAX_FORCE, PUSH, COMMAND = range(7)     # TREX_RAND_*
KIND_NAMES = ("mass", "friction", "kp", "kd", "max_force", "push", "command")
MAX_TERMS, MAX_PUSHES, ELEMENTS = 16, 4, 32                     # TREX_RAND_MAXTERMS, TREX_RAND_MAXPUSHES, the inner extent of values


class TrexRandomTerm(C.Structure):   # include/trex_randomize.h
    _fields_ = [("kind", C.c_int32), ("mask", C.c_uint32), ("index", C.c_int32), ("shared", C.c_int32), ("lo", C.c_float),
                ("hi", C.c_float), ("interval", C.c_int32), ("duration", C.c_int32), ("probability", C.c_float)]


_vp, _int, _ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
_RANDOMIZE_API = {
    "trex_batch_set_randomization": (_int, [_vp, C.POINTER(TrexRandomTerm), _int, C.c_uint64, C.c_uint32]),
    "trex_batch_apply_randomization": (_int, [_vp, _vp, _int, _vp, _vp]),
    "trex_batch_randomization_reset": (_int, [_vp, _vp, _vp]),
    "trex_batch_randomization_info": (_int, [_vp, _ip, _vp, _vp, _vp, _vp]),
}
RANDOMIZE_SYMBOLS = _capi._declare(_RANDOMIZE_API)    # every symbol include/trex_randomize.h declares


class BatchRandomization:
    """The episode randomisation of one _capi.Batch. All tensors are torch tensors on the batch's device, owned by the caller."""

    def __init__(self, batch):
        self.batch = batch
        self.num_terms = self.num_pushes = 0

    def set(self, terms=(), seed=0, env_offset=0):
        """The batch's terms (trex_batch_set_randomization): a sequence of (kind, mask, index, shared, lo, hi, interval,
        duration, probability). seed: the Philox key; env_offset: the global index of the batch's env 0. Host values; an empty
        sequence clears and puts gains, wrench, mass scale and friction back. Every env starts afresh. -> the number of terms."""
        arr = (TrexRandomTerm * max(len(terms), 1))()
        for o, (kind, mask, index, shared, lo, hi, interval, duration, probability) in zip(arr, terms):
            o.kind, o.mask, o.index, o.shared = int(kind), int(mask), int(index), int(shared)
            o.lo, o.hi, o.interval, o.duration, o.probability = float(lo), float(hi), int(interval), int(duration), float(probability)
        check(lib.trex_batch_set_randomization(self.batch.h, arr, len(terms), int(seed) & (2 ** 64 - 1), int(env_offset)))
        self.num_terms = len(terms)
        self.num_pushes = sum(1 for t in terms if int(t[0]) == PUSH)
        return self.num_terms

    def apply(self, done, commands=None, column=0, stream=None):
        """ONE launch (trex_batch_apply_randomization): the envs whose done flag is set, that were marked by reset() or that see
        their first apply start an episode and redraw; pushes and commands advance by one row. done: f32, [n], or a row block
        [n, stride] whose column `column` holds the flags (the done column of the rows a step call wrote). commands [n, 3] f32:
        needed with command terms."""
        b = self.batch
        if not hasattr(done, "dim") or done.dim() not in (1, 2) or done.shape[0] != b.num_envs:
            raise TrexError(E_INVALID, "done: expected a tensor of shape [%d] or [%d, columns]" % (b.num_envs, b.num_envs))
        stride = 1 if done.dim() == 1 else int(done.shape[1])
        column = int(column)
        if not 0 <= column < stride:
            raise TrexError(E_INVALID, "done: column %d outside [0, %d)" % (column, stride))
        p = b._p(done, "float32", b.num_envs * stride, "done")
        check(lib.trex_batch_apply_randomization(b.h, C.c_void_p(p.value + 4 * column), stride,
                                                 b._p(commands, "float32", 3 * b.num_envs, "commands"), b._stream(stream)))

    def reset(self, mask=None, stream=None):
        """The envs with mask != 0 (uint8 or bool [n]; None: all) start an episode with their next apply
        (trex_batch_randomization_reset)."""
        check(lib.trex_batch_randomization_reset(self.batch.h, self.batch._mask(mask), self.batch._stream(stream)))

    def info(self, values=None, push_force=None, push_left=None, stream=None):
        """-> the number of terms set (trex_batch_randomization_info); values [n, T, 32] f32, push_force [n, P, 3] f32 and
        push_left [n, P] int32 (each optional) receive the draws of every env's current episode and the state of its pushes."""
        b = self.batch
        n, t = b.num_envs, C.c_int(0)
        check(lib.trex_batch_randomization_info(b.h, C.byref(t), b._p(values, "float32", n * max(self.num_terms, 1) * ELEMENTS, "values"),
                                                b._p(push_force, "float32", n * max(self.num_pushes, 1) * 3, "push_force"),
                                                b._p(push_left, "int32", n * max(self.num_pushes, 1), "push_left"), b._stream(stream)))
        return t.value
