"""ctypes binding of include/trex_symmetry.h: the mirror maps of the device trainer. A module of its own beside _capi.py, whose
library handle, error check and pointer checks it uses: the signature table `_SYMMETRY_API` states the C signatures once, and
MirrorTable holds the calls of one TrexMirrorTable - a signed permutation of the columns of a row block. A table knows neither a
batch nor a policy: every buffer is a torch tensor on the table's device, owned by the caller."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import check, lib

MAX_WIDTH = 517                            # TREX_MIRROR_MAXWIDTH

_vp, _int, _i64 = C.c_void_p, C.c_int, C.c_int64
_pi32, _pi8 = C.POINTER(C.c_int32), C.POINTER(C.c_int8)
_SYMMETRY_API = {
    "trex_model_mirror_table": (_int, [_vp, _int, C.c_double, _pi32, _pi8, _pi32, C.POINTER(C.c_double), C.POINTER(_int)]),
    "trex_model_mirror_row_table": (_int, [_vp, _int, C.c_double, _vp, _int, _int, _int, _pi32, _pi8, _pi32, _pi8, C.POINTER(_int)]),
    "trex_mirror_action_table": (_int, [_pi32, _pi8, _int, _int, _pi32, _pi8]),
    "trex_mirror_command_table": (_int, [_int, _pi32, _pi8]),
    "trex_mirror_table_create": (_int, [_pi32, _pi8, _int, _int, C.POINTER(_vp)]),
    "trex_mirror_table_destroy": (None, [_vp]),
    "trex_mirror_table_info": (_int, [_vp, C.POINTER(_int), C.POINTER(_int)]),
    "trex_mirror_rows": (_int, [_vp, _vp, _int, _vp, _int, _int, _int, _vp]),
    "trex_mirror_augment": (_int, [_vp] * 10 + [_i64, _int, _int, _int, _vp]),
    "trex_policy_symmetrize_stats": (_int, [_vp, _vp, _vp, _vp]),
}
SYMMETRY_SYMBOLS = _capi._declare(_SYMMETRY_API)    # every symbol include/trex_symmetry.h declares


def _stream(stream):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)


RESIDUALS = ("mass_rel", "origin_m", "axis_rad", "com_m", "root_com_off_plane_m")     # residual_out [5], in order


def model_mirror_table(model, lateral=None, tol_pos=5e-3):
    """The mirror table of a compiled model (a _capi.Model): dict(lateral, pair [J] int32, sign [J] int8, body_pair [B] int32,
    residual: dict of RESIDUALS). lateral None searches for the axis. Host only. TrexError where the model has no such pairing."""
    J, B = model.num_joints, model.num_bodies
    pair, sign, body = np.zeros(J, np.int32), np.zeros(J, np.int8), np.zeros(B, np.int32)
    res, lat = (C.c_double * 5)(), _int()
    check(lib.trex_model_mirror_table(model.h, -1 if lateral is None else int(lateral), float(tol_pos), pair.ctypes.data_as(_pi32),
                                      sign.ctypes.data_as(_pi8), body.ctypes.data_as(_pi32), res, C.byref(lat)))
    return dict(lateral=lat.value, pair=pair, sign=sign, body_pair=body, residual=dict(zip(RESIDUALS, res[:])))


def row_table(model, channels, action_cols, tail=2, lateral=None, tol_pos=5e-3, extern_src=None, extern_sign=None):
    """(src, sign) of the composed row [q | qd | torque | channel columns | tail] of a compiled model under `channels`: a sequence
    of (kind, link, local_xyz[3], scale) as Batch.set_observation takes it. extern_src, extern_sign: the caller's table over the
    EXTERNAL columns, required where such a channel is set. Host only."""
    arr = (_capi.TrexObsChannel * max(len(channels), 1))()
    for o, (kind, link, xyz, scale) in zip(arr, channels):
        o.kind, o.link, o.scale = int(kind), int(link), float(scale)
        o.local_xyz[:] = [float(x) for x in xyz]
    src, sg, w = np.zeros(MAX_WIDTH, np.int32), np.zeros(MAX_WIDTH, np.int8), _int()
    es = None if extern_src is None else np.ascontiguousarray(extern_src, np.int32)
    eg = None if extern_sign is None else np.ascontiguousarray(extern_sign, np.int8)
    check(lib.trex_model_mirror_row_table(model.h, -1 if lateral is None else int(lateral), float(tol_pos), arr, len(channels),
                                          int(action_cols), int(tail), None if es is None else es.ctypes.data_as(_pi32),
                                          None if eg is None else eg.ctypes.data_as(_pi8), src.ctypes.data_as(_pi32),
                                          sg.ctypes.data_as(_pi8), C.byref(w)))
    return src[:w.value].copy(), sg[:w.value].copy()


def action_table(pair, sign, stiffness=False):
    """(src, sign) of an action block: the joint table, with stiffness actions a second block of the same permutation, sign +1"""
    pair, sign = np.ascontiguousarray(pair, np.int32), np.ascontiguousarray(sign, np.int8)
    A = pair.size * (2 if stiffness else 1)
    src, sg = np.zeros(A, np.int32), np.zeros(A, np.int8)
    check(lib.trex_mirror_action_table(pair.ctypes.data_as(_pi32), sign.ctypes.data_as(_pi8), int(pair.size), int(bool(stiffness)),
                                       src.ctypes.data_as(_pi32), sg.ctypes.data_as(_pi8)))
    return src, sg


def command_table(lateral):
    """(src, sign) of a velocity command (vx, vy, wz) in base axes"""
    src, sg = np.zeros(3, np.int32), np.zeros(3, np.int8)
    check(lib.trex_mirror_command_table(int(lateral), src.ctypes.data_as(_pi32), sg.ctypes.data_as(_pi8)))
    return src, sg


class MirrorTable:
    """One TrexMirrorTable of width W: the image of a row x is y[c] = sign[c] * x[src[c]], the sign applied as a sign-bit flip.
    src: a permutation of range(W); sign: +1 / -1 each. The host arrays stay readable as .src and .sign."""

    def __init__(self, src, sign, device=0):
        self.h = None
        self.device = int(device)
        self.src = np.ascontiguousarray(src, np.int32).reshape(-1)
        self.sign = np.ascontiguousarray(sign, np.int8).reshape(-1)
        if self.src.shape != self.sign.shape:
            raise ValueError("src has %d entries, sign %d" % (self.src.size, self.sign.size))
        self.width = int(self.src.size)
        h = _vp()
        check(lib.trex_mirror_table_create(self.src.ctypes.data_as(_pi32), self.sign.ctypes.data_as(_pi8),
                                           self.width, self.device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib.trex_mirror_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def involution(self):
        """applying the table twice reproduces a row bit for bit"""
        w, inv = _int(), _int()
        check(lib.trex_mirror_table_info(self.h, C.byref(w), C.byref(inv)))
        return bool(inv.value)

    def rows(self, x, out=None, n=None, in_stride=None, out_stride=None, stream=None):
        """out[e, c] = sign[c] * x[e, src[c]] for the first W columns of n rows; ONE launch. x, out: f32 [n, stride] tensors whose
        stride is their last dimension (or flat tensors with n and the strides given). out None: a new [n, W] tensor; out is x:
        in place. Columns of out beyond W are not written. -> out"""
        W = self.width
        if n is None:
            n = int(x.numel() // x.shape[-1]) if x.dim() > 1 else 1
        in_stride = int(x.shape[-1]) if in_stride is None else int(in_stride)
        if out is None:
            out = torch.empty(tuple(x.shape[:-1]) + (W,), dtype=torch.float32, device=x.device)
        out_stride = (int(out.shape[-1]) if out_stride is None else int(out_stride))
        check(lib.trex_mirror_rows(self.h, _capi._ptr(x, self.device, torch.float32, (n - 1) * in_stride + W, "in"), in_stride,
                                   _capi._ptr(out, self.device, torch.float32, (n - 1) * out_stride + W, "out"), out_stride,
                                   int(n), W, _stream(stream)))
        return out


def augment(obs_table, act_table, obs, act, logp, val, adv, ret, num_samples, critic_table=None, obs_v=None, stream=None):
    """ONE launch that fills the samples [num_samples, 2 num_samples) of every rollout buffer from the samples [0, num_samples): obs
    [2N, D], act [2N, A] (and obs_v [2N, Dv]) through their tables, logp, val, adv, ret [2N] copied. The mirrored samples keep the
    originals' log-probability, value, advantage and return: the rollout policy is treated as if it were symmetric."""
    N, dev = int(num_samples), obs_table.device
    D, A, Dv = obs_table.width, act_table.width, (critic_table.width if critic_table is not None else 0)
    p = lambda t, numel, what: _capi._ptr(t, dev, torch.float32, numel, what)
    check(lib.trex_mirror_augment(obs_table.h, act_table.h, critic_table.h if critic_table is not None else None,
                                  p(obs, 2 * N * D, "obs"), p(act, 2 * N * A, "act"), p(logp, 2 * N, "logp"), p(val, 2 * N, "val"),
                                  p(adv, 2 * N, "adv"), p(ret, 2 * N, "ret"), p(obs_v, 2 * N * Dv, "obs_v"), N, D, A, Dv,
                                  _stream(stream)))


def symmetrize_stats(policy, obs_table, critic_table=None, stream=None):
    """The running observation moments of `policy` (a _capi.Policy) become those of the stream in which every row is followed by its
    mirror image; the normalisation that `act` reads is refreshed. Idempotent. With critic_table the critic's moments alike."""
    check(lib.trex_policy_symmetrize_stats(policy.h, obs_table.h, critic_table.h if critic_table is not None else None, _stream(stream)))
