"""ctypes binding of include/trex_motion.h: the motion clip of a batch (trex_batch_set_motion / _motion_info / _motion_sample /
_set_motion_reward / _compose_motion_reward / _motion_reset). A module of its own beside _capi.py, whose library handle, error check
and argument checks it uses: the signature table `_MOTION_API` states the six C signatures once (tests/test_motion_capi_host.py
compares it with the header), and BatchMotion(batch) holds the calls for one _capi.Batch. trex_gym.motion builds clips and term
specifications; a TrexVecEnv with a clip attached (trex_gym.motion.attach) is the user of this module."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import E_INVALID, TrexError, check, lib


class TrexMotionTerm(C.Structure):   # include/trex_motion.h
    _fields_ = [("kind", C.c_int32), ("mask", C.c_uint32), ("weight", C.c_float), ("scale", C.c_float), ("aux", C.c_float)]


_vp, _int, _dp, _ip = C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)
_MOTION_API = {
    "trex_batch_set_motion": (_int, [_vp, _dp, _dp, _int, C.c_double, _int, _int]),
    "trex_batch_motion_info": (_int, [_vp, _ip, _dp, _ip, _ip]),
    "trex_batch_motion_sample": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "trex_batch_set_motion_reward": (_int, [_vp, C.POINTER(TrexMotionTerm), _int, C.c_float]),
    "trex_batch_compose_motion_reward": (_int, [_vp, _vp, _int, _vp, _vp]),
    "trex_batch_motion_reset": (_int, [_vp, _vp, _vp, _vp, _int, _vp]),
}
MOTION_SYMBOLS = _capi._declare(_MOTION_API)    # every symbol include/trex_motion.h declares


class BatchMotion:
    """The motion clip of one _capi.Batch. All tensors are torch tensors on the batch's device, owned by the caller."""

    def __init__(self, batch):
        self.batch = batch
        self.num_frames = self.num_terms = self.num_probes = 0

    def _f64(self, a, width, what):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        if a.ndim != 2 or a.shape[1] != width:
            raise TrexError(E_INVALID, "%s: expected an array of shape [frames, %d], got %s" % (what, width, a.shape))
        return a

    def set_motion(self, frames=None, frame_dt=1.0, loop=False, velocities=None, probe_set=-1):
        """The batch's clip (trex_batch_set_motion): frames [F, 7 + J] = base position, base quaternion xyzw, q in observation
        order; velocities [F, 6 + J] = base linear and angular world velocity, qd, or None: derived by central differences.
        probe_set: the set of set_link_probes whose points are the end effectors, -1 = none. Host values, shared by all envs;
        frames None (or empty) clears. The clocks start at zero and the motion terms are cleared. -> F."""
        J = self.batch.J
        if frames is None or len(frames) == 0:
            check(lib.trex_batch_set_motion(self.batch.h, None, None, 0, float(frame_dt), 0, -1))
        else:
            fr = self._f64(frames, 7 + J, "frames")
            ve = None
            if velocities is not None:
                ve = self._f64(velocities, 6 + J, "velocities")
                if ve.shape[0] != fr.shape[0]:
                    raise TrexError(E_INVALID, "velocities: %d frames, the clip has %d" % (ve.shape[0], fr.shape[0]))
            check(lib.trex_batch_set_motion(self.batch.h, fr.ctypes.data_as(_dp), None if ve is None else ve.ctypes.data_as(_dp),
                                            int(fr.shape[0]), float(frame_dt), 1 if loop else 0, int(probe_set)))
        info = self.info()
        self.num_frames, self.num_terms, self.num_probes = info["frames"], info["terms"], info["probes"]
        return self.num_frames

    def info(self):
        """dict(frames=F, duration=T seconds, terms=number of motion terms, probes=K) of what is set (trex_batch_motion_info)"""
        f, t, k, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        check(lib.trex_batch_motion_info(self.batch.h, C.byref(f), C.byref(d), C.byref(t), C.byref(k)))
        return dict(frames=f.value, duration=d.value, terms=t.value, probes=k.value)

    def sample(self, time=None, state=None, points=None, phase=None, stream=None):
        """The reference at time [n] (None: each env's own clock) into state [n, 13 + 2J] (the layout of get_state), points
        [n, K, 3] (the end effectors' world positions at the reference pose) and phase [n], each optional but not all three
        (trex_batch_motion_sample). One launch, stream-ordered; no clock moves."""
        b = self.batch
        n = b.num_envs
        check(lib.trex_batch_motion_sample(b.h, b._p(time, "float32", n, "time"), b._p(state, "float32", n * b.state_width, "state"),
                                           b._p(points, "float32", n * self.num_probes * 3, "points"),
                                           b._p(phase, "float32", n, "phase"), b._stream(stream)))

    def set_reward(self, terms=(), step_weight=1.0):
        """The batch's motion terms (trex_batch_set_motion_reward): a sequence of (kind, mask, weight, scale, aux) - kind a
        TREX_MOT_* value, mask the joints' bits (0 = all). step_weight: what the column found keeps. An empty sequence clears.
        The held values start at zero. -> T."""
        arr = (TrexMotionTerm * max(len(terms), 1))()
        for o, (kind, mask, weight, scale, aux) in zip(arr, terms):
            o.kind, o.mask, o.weight, o.scale, o.aux = int(kind), int(mask), float(weight), float(scale), float(aux)
        check(lib.trex_batch_set_motion_reward(self.batch.h, arr, len(terms), float(step_weight)))
        self.num_terms = len(terms)
        return self.num_terms

    def compose_reward(self, rows, terms=None, stream=None):
        """Evaluate the motion terms (trex_batch_compose_motion_reward) on rows [n, >= 3J + tail] - what step_rows just wrote,
        after reward_capi's compose if there is one -: column 3J of every row becomes step_weight * itself + the weighted sum,
        terms [n, T] (optional) the weighted value of every term. One launch, stream-ordered; advances the clocks - once per
        step."""
        b = self.batch
        n = b.num_envs
        if not hasattr(rows, "dim") or rows.dim() != 2 or rows.shape[0] != n:
            raise TrexError(E_INVALID, "rows: expected a tensor of shape [%d, columns]" % n)
        check(lib.trex_batch_compose_motion_reward(b.h, b._rows(rows, "rows"), int(rows.shape[1]),
                                                   b._p(terms, "float32", n * self.num_terms, "terms"), b._stream(stream)))

    def reset(self, mask=None, time=None, rows=None, stream=None):
        """Reference state initialisation (trex_batch_motion_reset): the envs with mask != 0 (uint8 or bool [n]; None: all) take
        the clip's state at time [n] (None: 0), motors on, clock at that time, held values zero; rows [n, >= 3J + tail]
        (optional): their q, qd columns rewritten, the torque columns zeroed."""
        b = self.batch
        n = b.num_envs
        if rows is not None and (not hasattr(rows, "dim") or rows.dim() != 2 or rows.shape[0] != n):
            raise TrexError(E_INVALID, "rows: expected a tensor of shape [%d, columns]" % n)
        check(lib.trex_batch_motion_reset(b.h, b._mask(mask), b._p(time, "float32", n, "time"),
                                          None if rows is None else b._rows(rows, "rows"), 0 if rows is None else int(rows.shape[1]),
                                          b._stream(stream)))
