"""ctypes binding of include/trex_monitor.h: the episode monitor of a batch (trex_batch_set_monitor / _monitor_apply /
_monitor_reset / _monitor_summary / _monitor_info). A module of its own beside _capi.py, whose library handle, error check and
argument checks it uses: the signature table `_MONITOR_API` states the five C signatures once, and BatchMonitor(batch) holds the
calls for one _capi.Batch. A TrexVecEnv with a monitor attached (trex_gym.monitor.attach) is the user of this module."""
import ctypes as C

import torch

from . import _capi
from ._capi import E_INVALID, TrexError, check, lib

MAX_WINDOW, MAX_COLS = 65536, 64                               # TREX_MON_MAXWINDOW, TREX_MON_MAXCOLS
# the fields of the summary (TREX_MON_*), then the C column means
N, RET_MEAN, RET_MIN, RET_MAX, LEN_MEAN, LEN_MIN, LEN_MAX, WIN_REASON, TOTAL, BY_REASON, T, SUMMARY = 0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 16, 17
REASON_NAMES = ("limit", "head", "tilt", "clearance")          # the four buckets of by_reason
RING_FIELDS = (("ring_return", "float32"), ("ring_length", "int32"), ("ring_reason", "int32"), ("ring_env", "int32"),
               ("ring_t", "int32"), ("ring_cols", "float32"))
ENV_FIELDS = (("ret", "float64"), ("len", "int32"), ("episodes", "int32"), ("last_return", "float32"), ("last_length", "int32"),
              ("last_reason", "int32"), ("last_t", "int32"), ("last_cols", "float32"))

_vp, _int, _ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
_MONITOR_API = {
    "trex_batch_set_monitor": (_int, [_vp, _int, _int, _int, C.c_uint32]),
    "trex_batch_monitor_apply": (_int, [_vp, _vp, _int, _vp, _int, _vp, _vp, _int, _vp, _int, _vp]),
    "trex_batch_monitor_reset": (_int, [_vp, _vp, _vp]),
    "trex_batch_monitor_summary": (_int, [_vp, _vp, _vp]),
    "trex_batch_monitor_info": (_int, [_vp, _ip, _ip] + [_vp] * 15),
}
MONITOR_SYMBOLS = _capi._declare(_MONITOR_API)    # every symbol include/trex_monitor.h declares


def _column(t, n, column, what):
    """a [n] tensor, or column `column` of a [n, stride] block -> (the block, stride, column)"""
    if not hasattr(t, "dim") or t.dim() not in (1, 2) or t.shape[0] != n:
        raise TrexError(E_INVALID, "%s: expected a tensor of shape [%d] or [%d, columns]" % (what, n, n))
    stride = 1 if t.dim() == 1 else int(t.shape[1])
    column = int(column)
    if not 0 <= column < stride:
        raise TrexError(E_INVALID, "%s: column %d outside [0, %d)" % (what, column, stride))
    return t, stride, column


class BatchMonitor:
    """The episode monitor of one _capi.Batch. All tensors are torch tensors on the batch's device, owned by the caller; the
    unsigned 32-bit arrays of the header (env, t, episodes) are int32 tensors here - the same bits."""

    def __init__(self, batch):
        self.batch = batch
        self.window = self.cols_a = self.cols_b = self.cols = 0

    def set(self, window=100, cols_a=0, cols_b=0, env_offset=0):
        """The batch's monitor (trex_batch_set_monitor): a window of the last `window` finished episodes, two blocks of cols_a
        and cols_b columns summed per episode; env_offset: the global index of the batch's env 0. window 0 clears and frees.
        Every env starts afresh. -> the window."""
        check(lib.trex_batch_set_monitor(self.batch.h, int(window), int(cols_a), int(cols_b), int(env_offset)))
        self.window = int(window)
        self.cols_a, self.cols_b = (int(cols_a), int(cols_b)) if self.window else (0, 0)
        self.cols = self.cols_a + self.cols_b
        return self.window

    def _block(self, t, width, what):
        """a column block [n, stride >= width] or None -> (pointer, stride)"""
        b = self.batch
        if width == 0:
            return None, 0
        if t is None:
            raise TrexError(E_INVALID, "%s: missing, and its width is %d" % (what, width))
        if not hasattr(t, "dim") or t.dim() != 2 or t.shape[0] != b.num_envs or t.shape[1] < width:
            raise TrexError(E_INVALID, "%s: expected a tensor of shape [%d, %d or more]" % (what, b.num_envs, width))
        return b._p(t, "float32", b.num_envs * int(t.shape[1]), what), int(t.shape[1])

    def apply(self, reward, done, reason=None, cols_a=None, cols_b=None, reward_column=0, done_column=0, stream=None):
        """Once per step (trex_batch_monitor_apply, two launches): every env's return, length and column sums take the row in;
        the envs whose done flag is set finish an episode and enter the ring in ascending order. reward, done: f32, [n], or a row
        block [n, stride] whose column reward_column / done_column holds the values (the two tail columns of the rows a step
        call wrote). reason: int32 [n]; None is the batch's own reason buffer while termination is enabled, zeros otherwise.
        cols_a, cols_b: [n, width or more] f32, needed where the width set is not 0. Nothing of the caller's is written."""
        b = self.batch
        n = b.num_envs
        reward, rs, rc = _column(reward, n, reward_column, "reward")
        done, ds, dc = _column(done, n, done_column, "done")
        rp, dp = b._p(reward, "float32", n * rs, "reward"), b._p(done, "float32", n * ds, "done")
        ap, sa = self._block(cols_a, self.cols_a, "cols_a")
        bp, sb = self._block(cols_b, self.cols_b, "cols_b")
        check(lib.trex_batch_monitor_apply(b.h, C.c_void_p(rp.value + 4 * rc), rs, C.c_void_p(dp.value + 4 * dc), ds,
                                           b._p(reason, "int32", n, "reason"), ap, sa, bp, sb, b._stream(stream)))

    def reset(self, mask=None, stream=None):
        """The running episode of the envs with mask != 0 (uint8 or bool [n]; None: all) is abandoned and not recorded
        (trex_batch_monitor_reset)."""
        check(lib.trex_batch_monitor_reset(self.batch.h, self.batch._mask(mask), self.batch._stream(stream)))

    def summary(self, out=None, stream=None):
        """-> out, float64 [SUMMARY + cols] on the device (made here when None), filled by one launch
        (trex_batch_monitor_summary): the fields N .. T of this module, then the column means; stream-ordered, no host copy."""
        b = self.batch
        if out is None:
            out = torch.zeros(SUMMARY + self.cols, dtype=torch.float64, device="cuda:%d" % b.device)
        check(lib.trex_batch_monitor_summary(b.h, b._p(out, "float64", SUMMARY + self.cols, "out"), b._stream(stream)))
        return out

    def info(self, stream=None, **buffers):
        """-> (window, cols) (trex_batch_monitor_info); the keyword buffers, each optional, receive stream-ordered copies: the
        ring - ring_return [W] f32, ring_length, ring_reason, ring_env, ring_t [W] int32, ring_cols [W, C] f32 - and per env
        ret [n] f64, len, episodes [n] int32 and the last finished record: last_return [n] f32, last_length, last_reason, last_t
        [n] int32, last_cols [n, C] f32."""
        b = self.batch
        n, W, Cn = b.num_envs, max(self.window, 1), self.cols
        numel = dict(ring_cols=W * Cn, last_cols=n * Cn)
        unknown = set(buffers) - {k for k, _ in RING_FIELDS + ENV_FIELDS}
        if unknown:
            raise TypeError("info: unknown buffers %s" % sorted(unknown))
        ptrs = []
        for fields, count in ((RING_FIELDS, W), (ENV_FIELDS, n)):
            for name, dtype in fields:
                t = buffers.get(name)
                if t is not None and numel.get(name, count) == 0:
                    t = None                  # (no columns: nothing to copy)
                ptrs.append(b._p(t, dtype, numel.get(name, count), name))
        w, c = C.c_int(0), C.c_int(0)
        check(lib.trex_batch_monitor_info(b.h, C.byref(w), C.byref(c), *ptrs, b._stream(stream)))
        return w.value, c.value
