"""ctypes binding of include/trex_sensing.h: the sensor model of a batch (trex_batch_set_sensing / _apply_sensing / _sensing_reset
/ _set_action_delay / _delay_actions / _sensing_info). A module of its own beside _capi.py, whose library handle, error check and
argument checks it uses: the signature table `_SENSING_API` states the six C signatures once (tests/test_sensing_capi_host.py
compares it with the header), and BatchSensing(batch) holds the calls for one _capi.Batch. trex_gym.sensing builds specifications;
a TrexVecEnv with sensing attached (trex_gym.sensing.attach) is the user of this module."""
import ctypes as C

from . import _capi
from ._capi import E_INVALID, TrexError, check, lib

GAUSSIAN, UNIFORM = 0, 1          # TREX_SENSE_GAUSSIAN, TREX_SENSE_UNIFORM
MAX_DELAY, MAX_GROUPS = 8, 64     # TREX_SENSE_MAXDELAY, TREX_SENSE_MAXGROUPS


class TrexSenseGroup(C.Structure):   # include/trex_sensing.h
    _fields_ = [("col0", C.c_int32), ("width", C.c_int32), ("noise_kind", C.c_int32), ("noise", C.c_float), ("bias", C.c_float),
                ("quantum", C.c_float), ("delay_min", C.c_int32), ("delay_max", C.c_int32)]


_vp, _int, _ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
_SENSING_API = {
    "trex_batch_set_sensing": (_int, [_vp, C.POINTER(TrexSenseGroup), _int, C.c_uint64, C.c_uint32]),
    "trex_batch_apply_sensing": (_int, [_vp, _vp, _int, _vp, _int, _vp]),
    "trex_batch_sensing_reset": (_int, [_vp, _vp, _vp]),
    "trex_batch_set_action_delay": (_int, [_vp, _int, _int]),
    "trex_batch_delay_actions": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "trex_batch_sensing_info": (_int, [_vp, _ip, _ip, _ip, _ip, _vp, _vp, _vp]),
}
SENSING_SYMBOLS = _capi._declare(_SENSING_API)    # every symbol include/trex_sensing.h declares


class BatchSensing:
    """The sensor model of one _capi.Batch. All tensors are torch tensors on the batch's device, owned by the caller."""

    def __init__(self, batch):
        self.batch = batch
        self.num_groups = self.delayed_columns = 0
        self.action_delay = (0, 0)

    def set_sensing(self, groups=(), seed=0, env_offset=0):
        """The batch's groups (trex_batch_set_sensing): a sequence of (col0, width, noise_kind, noise, bias, quantum, delay_min,
        delay_max) over columns of the final row, 3J + E wide. seed: the Philox key; env_offset: the global index of the batch's
        env 0. Host values; an empty sequence clears. Every env starts afresh. -> the number of groups."""
        arr = (TrexSenseGroup * max(len(groups), 1))()
        for o, (col0, width, kind, noise, bias, quantum, dmin, dmax) in zip(arr, groups):
            o.col0, o.width, o.noise_kind = int(col0), int(width), int(kind)
            o.noise, o.bias, o.quantum = float(noise), float(bias), float(quantum)
            o.delay_min, o.delay_max = int(dmin), int(dmax)
        check(lib.trex_batch_set_sensing(self.batch.h, arr, len(groups), int(seed) & (2 ** 64 - 1), int(env_offset)))
        self._refresh()
        return self.num_groups

    def _refresh(self):
        i = self.info()
        self.num_groups, self.delayed_columns, self.action_delay = i["groups"], i["delayed_columns"], i["action_delay"]

    def _block(self, t, what):
        b = self.batch
        if not hasattr(t, "dim") or t.dim() != 2 or t.shape[0] != b.num_envs:
            raise TrexError(E_INVALID, "%s: expected a tensor of shape [%d, columns]" % (what, b.num_envs))
        width = b.observation_dim() + (5 if b.pen_in_rows else 2)
        return b._rows(t, what, width)

    def apply(self, rows, out=None, stream=None):
        """The sensors' view of rows [n, >= 3J + E + tail] into out (None: in place) - trex_batch_apply_sensing: the covered
        columns delayed, biased, noisy and quantised, everything else as found. One launch, stream-ordered; advances every env's
        row count - once per step and once per reset, behind the last compose of the row."""
        out = rows if out is None else out
        check(lib.trex_batch_apply_sensing(self.batch.h, self._block(rows, "rows"), int(rows.shape[1]), self._block(out, "out"),
                                           int(out.shape[1]), self.batch._stream(stream)))

    def reset(self, mask=None, stream=None):
        """The envs with mask != 0 (uint8 or bool [n]; None: all) start an episode with their next applied row and their next
        delayed action (trex_batch_sensing_reset)."""
        check(lib.trex_batch_sensing_reset(self.batch.h, self.batch._mask(mask), self.batch._stream(stream)))

    def set_action_delay(self, delay_min=0, delay_max=None):
        """The actuation latency in env-steps, drawn per env and episode in [delay_min, delay_max] (trex_batch_set_action_delay);
        0, 0 clears."""
        delay_max = delay_min if delay_max is None else delay_max
        check(lib.trex_batch_set_action_delay(self.batch.h, int(delay_min), int(delay_max)))
        self._refresh()

    def delay_actions(self, actions, out, done_prev=None, stream=None):
        """out [n, A] = the action rows the envs were given their delay ago (trex_batch_delay_actions); done_prev [n] uint8 or
        bool: the done flags of the previous step. One launch, stream-ordered."""
        b = self.batch
        n = b.num_envs * b.A
        check(lib.trex_batch_delay_actions(b.h, b._p(actions, "float32", n, "actions"), None if done_prev is None else b._mask(done_prev),
                                           b._p(out, "float32", n, "out"), b._stream(stream)))

    def info(self, delays=None, action_delays=None, stream=None):
        """dict(groups=G, delayed_columns=, action_delay=(min, max)) of what is set (trex_batch_sensing_info); delays [n, G] int32
        and action_delays [n] int32 (optional) receive what the envs drew for their current episode."""
        b = self.batch
        g, d, lo, hi = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib.trex_batch_sensing_info(b.h, C.byref(g), C.byref(d), C.byref(lo), C.byref(hi),
                                          b._p(delays, "int32", b.num_envs * max(self.num_groups, 1), "delays"),
                                          b._p(action_delays, "int32", b.num_envs, "action_delays"), b._stream(stream)))
        return dict(groups=g.value, delayed_columns=d.value, action_delay=(lo.value, hi.value))
