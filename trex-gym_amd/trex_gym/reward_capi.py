"""ctypes binding of include/trex_reward.h: the reward terms of a batch (trex_batch_set_reward / _reward_terms / _compose_reward /
_reward_reset). A module of its own beside _capi.py, whose library handle, error check and argument checks it uses: the signature
table `_REWARD_API` states the four C signatures once (tests/test_reward_capi_host.py compares it with the header), and
BatchRewards(batch) holds the calls for one _capi.Batch. trex_gym.rewards builds the specifications; TrexVecEnv(rewards=...) is
the user of this module."""
import ctypes as C

from . import _capi
from ._capi import E_INVALID, TrexError, check, lib


class TrexRewardTerm(C.Structure):   # include/trex_reward.h
    _fields_ = [("kind", C.c_int32), ("link", C.c_int32), ("mask", C.c_uint32), ("local_xyz", C.c_float * 3),
                ("weight", C.c_float), ("p0", C.c_float), ("p1", C.c_float)]


_vp, _int = C.c_void_p, C.c_int
_REWARD_API = {
    "trex_batch_set_reward": (_int, [_vp, C.POINTER(TrexRewardTerm), _int]),
    "trex_batch_reward_terms": (_int, [_vp]),
    "trex_batch_compose_reward": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp]),
    "trex_batch_reward_reset": (_int, [_vp, _vp, _vp]),
}
REWARD_SYMBOLS = _capi._declare(_REWARD_API)    # every symbol include/trex_reward.h declares


class BatchRewards:
    """The reward terms of one _capi.Batch. All tensors are torch tensors on the batch's device, owned by the caller."""

    def __init__(self, batch):
        self.batch = batch
        self.num_terms = 0

    def set_reward(self, terms=()):
        """The batch's reward terms (trex_batch_set_reward): a sequence of (kind, link, mask, local_xyz[3], weight, p0, p1) - kind
        a TREX_REW_* value, link a URDF link index. Host values, shared by all envs; an empty sequence clears. The terms' history
        starts afresh. -> T."""
        arr = (TrexRewardTerm * max(len(terms), 1))()
        for o, (kind, link, mask, xyz, weight, p0, p1) in zip(arr, terms):
            o.kind, o.link, o.mask = int(kind), int(link), int(mask)
            o.local_xyz[:] = [float(x) for x in xyz]
            o.weight, o.p0, o.p1 = float(weight), float(p0), float(p1)
        check(lib.trex_batch_set_reward(self.batch.h, arr, len(terms)))
        self.num_terms = len(terms)
        return self.num_terms

    def reward_terms(self):
        """T, the number of reward terms set (trex_batch_reward_terms)"""
        return check(lib.trex_batch_reward_terms(self.batch.h))

    def compose_reward(self, rows, actions=None, command=None, terms=None, stream=None):
        """Evaluate the reward terms (trex_batch_compose_reward) on rows [n, >= 3J + tail] - what step_rows just wrote -: column
        3J of every row becomes the weighted sum, terms [n, T] (optional) the weighted value of every term. actions [n, A]: the
        step's actions (needed by ACTION_RATE), command [n, 3]: vx, vy, yaw rate (needed by the tracking terms). One launch,
        stream-ordered; advances the terms' history - once per step."""
        b = self.batch
        n = b.num_envs
        if not hasattr(rows, "dim") or rows.dim() != 2 or rows.shape[0] != n:
            raise TrexError(E_INVALID, "rows: expected a tensor of shape [%d, columns]" % n)
        check(lib.trex_batch_compose_reward(b.h, b._rows(rows, "rows"), int(rows.shape[1]),
                                            b._p(actions, "float32", n * b.A, "actions"), b._p(command, "float32", n * 3, "command"),
                                            b._p(terms, "float32", n * self.num_terms, "terms"), b._stream(stream)))

    def reward_reset(self, mask=None, stream=None):
        """Invalidate the reward history of the envs with mask != 0 (uint8 or bool [n]; None: all) and zero their held values
        (trex_batch_reward_reset)."""
        check(lib.trex_batch_reward_reset(self.batch.h, self.batch._mask(mask), self.batch._stream(stream)))
