"""ctypes binding of libtrex_hip.so (C-ABI in include/trex_batch.h).

There is NO CPU fallback: if the HIP library is missing, importing this module raises; if no GPU
is present, creating a batch raises TrexError (model loading is host-only and still works).

Every function's signature stands once, in the tables _BATCH_API / _POLICY_API below. A function the loaded library does
not export is left out when they are applied: a TREX_LIB built from an older tree (scripts/actuator_bench.py's A/B run)
still imports, and USING a function it lacks raises AttributeError - for every function now, where the ones older than the
actuator model used to fail the import. That the product library exports them all is tests/test_capi_host.py's check.
"""
import ctypes as C
import os

import numpy as np
import torch  # FIRST: torch brings its own HIP runtime; loading libtrex_hip.so before it would bind the system
#               runtime and leave the process with two of them

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TREX_LIB") or os.path.join(_HERE, "libtrex_hip.so")  # TREX_LIB: diagnostic builds

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "trex_gym: %s not found - build it with `python __graft_entry__.py` or "
        "`make -C trex-gym_amd/csrc` (hipcc --offload-arch=gfx950). The physics step has no CPU fallback."
        % LIB_PATH)

lib = C.CDLL(LIB_PATH)

PARAM_NAMES = ["dt", "substeps", "iterations", "gravity", "motor_kp", "motor_kd", "motor_max_force",
               "floor_z", "friction", "erp", "contact_erp", "contact_margin", "link_damping",
               "max_coordinate_velocity", "max_contacts"]


class TrexCamera(C.Structure):     # include/trex_batch.h
    _fields_ = [("distance", C.c_float), ("yaw_deg", C.c_float), ("pitch_deg", C.c_float), ("fov_deg", C.c_float),
                ("near_z", C.c_float), ("far_z", C.c_float), ("follow_base", C.c_int), ("target", C.c_float * 3)]


class TrexIkParams(C.Structure):   # include/trex_batch.h; the defaults are TREX_IK_DEFAULTS
    _fields_ = [("iterations", C.c_int32), ("damping", C.c_float), ("gain", C.c_float), ("max_step", C.c_float),
                ("tol_pos", C.c_float), ("tol_ori", C.c_float)]


class TrexObsChannel(C.Structure):   # include/trex_batch.h
    _fields_ = [("kind", C.c_int32), ("link", C.c_int32), ("local_xyz", C.c_float * 3), ("scale", C.c_float)]


# The signature tables: name -> (restype, argtypes), one per header, in the order SYMBOLS / POLICY_SYMBOLS list the names.
# tests/test_capi_host.py parses the headers and compares every entry - count, kind of each parameter, return kind.
# _vp: a handle, a device pointer or a stream; host arrays and out-parameters are typed pointers.
_vp, _int, _f, _d, _str = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_char_p
_pint, _pi32, _pf, _pd, _pstr = C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_char_p)

_BATCH_API = {
    "trex_last_error": (_str, []),
    "trex_model_load": (_int, [_str, _str, C.POINTER(_vp)]),
    "trex_model_destroy": (None, [_vp]),
    "trex_model_num_bodies": (_int, [_vp]),
    "trex_model_num_joints": (_int, [_vp]),
    "trex_model_num_urdf_joints": (_int, [_vp]),
    "trex_model_num_hull_vertices": (_int, [_vp]),
    "trex_model_total_mass": (_d, [_vp, _int]),
    "trex_model_joint_info": (_int, [_vp, _int, _pstr, _pint, _pd, _pd]),
    "trex_model_set_start_angle": (_int, [_vp, _str, _d]),
    "trex_model_set_start_pose": (_int, [_vp, _pd, _pd]),
    "trex_model_set_param": (_int, [_vp, _str, _d]),
    "trex_model_get_param": (_int, [_vp, _str, _pd]),
    "trex_model_get_array": (_int, [_vp, _str, _pd, _int]),
    "trex_batch_create": (_int, [_vp, _int, _int, C.POINTER(_vp)]),
    "trex_batch_destroy": (None, [_vp]),
    "trex_batch_num_envs": (_int, [_vp]),
    "trex_batch_set_reward_weights": (_int, [_vp, _f, _f, _f]),
    "trex_batch_reset": (_int, [_vp, _vp, _vp, _vp]),
    "trex_batch_step": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "trex_batch_get_state": (_int, [_vp, _vp, _vp]),
    "trex_batch_set_state": (_int, [_vp, _vp, _vp]),
    "trex_batch_set_motors_enabled": (_int, [_vp, _int, _vp]),
    "trex_batch_head_position": (_int, [_vp, _vp, _vp]),
    "trex_batch_set_domain": (_int, [_vp, _vp, _vp, _vp]),
    "trex_batch_contact_stats": (_int, [_vp, _vp, _vp, _vp]),
    "trex_batch_debug_step": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "trex_batch_launch_info": (_int, [_vp, _pint, _pint, _pint, _pint]),
    "trex_batch_time_steps": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp, _pf]),
    "trex_model_num_links": (_int, [_vp]),
    "trex_model_link_info": (_int, [_vp, _int, _pstr, _pint]),
    "trex_batch_link_transforms": (_int, [_vp, _vp, _vp]),
    "trex_model_use_primitive_collision": (_int, [_vp, _d, _int, _int]),
    "trex_model_fit_hull_primitives": (_int, [_vp, _int, _d, _int, _int, _pd, _int]),
    "trex_build_id": (_str, []),
    "trex_batch_step_rows": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _vp]),
    "trex_batch_reset_rows": (_int, [_vp, _vp, _vp, _int, _vp]),
    "trex_batch_set_episode_limit": (_int, [_vp, _int, _vp, _vp]),
    "trex_batch_get_episode_steps": (_int, [_vp, _vp, _vp]),
    "trex_batch_set_wave_balance": (_int, [_vp, _int]),
    "trex_batch_forget_buffers": (_int, [_vp]),
    "trex_batch_set_penalties_in_rows": (_int, [_vp, _int]),
    "trex_model_num_visuals": (_int, [_vp]),
    "trex_model_visual_info": (_int, [_vp, _int, _pstr, _pint, _pd, _pd]),
    "trex_batch_visual_transforms": (_int, [_vp, _vp, _vp]),
    "trex_batch_step_many": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "trex_batch_render": (_int, [_vp, C.POINTER(TrexCamera), _int, _int, _pi32, _int, _vp, _vp, _vp, _vp]),
    "trex_batch_set_external_wrench": (_int, [_vp, _vp, _vp]),
    "trex_batch_set_contact_sensor": (_int, [_vp, _int]),
    "trex_batch_contact_wrench": (_int, [_vp, _vp, _vp]),
    "trex_batch_set_control_mode": (_int, [_vp, _pi32]),
    "trex_batch_set_motor_gains": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "trex_batch_set_stiffness_actions": (_int, [_vp, _int, _f]),
    "trex_batch_inverse_dynamics": (_int, [_vp, _vp, _vp, _vp]),
    "trex_batch_mass_matrix": (_int, [_vp, _vp, _vp]),
    "trex_batch_jacobian": (_int, [_vp, _int, _pd, _vp, _vp]),
    "trex_batch_centroidal": (_int, [_vp, _vp, _vp]),
    "trex_batch_forward_dynamics": (_int, [_vp, _vp, _vp, _vp]),
    "trex_batch_solve_mass": (_int, [_vp, _vp, _int, _vp, _vp]),
    "trex_batch_ray_test": (_int, [_vp, _vp, _int, _int, _int, C.c_uint32, _int, _vp, _vp, _vp, _vp, _vp]),
    "trex_batch_set_link_probes": (_int, [_vp, _int, _pi32, _pd, _int]),
    "trex_batch_link_state": (_int, [_vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "trex_batch_set_proximity_shapes": (_int, [_vp, _pi32, _pd, _int, _pi32, _int]),
    "trex_batch_proximity": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "trex_batch_body_clearance": (_int, [_vp, _vp, _vp, _vp]),
    "trex_batch_set_termination": (_int, [_vp, _f, _f, _pf, _f]),
    "trex_batch_termination_info": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "trex_batch_inverse_kinematics": (_int, [_vp, _int, _pi32, _int, _vp, _vp, C.c_uint32, C.POINTER(TrexIkParams), _vp, _vp, _vp]),
    "trex_batch_set_observation": (_int, [_vp, C.POINTER(TrexObsChannel), _int, _pint]),
    "trex_batch_observation_dim": (_int, [_vp]),
    "trex_batch_compose_rows": (_int, [_vp, _vp, _int, _vp, _vp, _int, _vp, _int, _vp]),
}

_POLICY_API = {   # the trainer-side kernels, SURVEY 8f-1
    "trex_policy_create": (_int, [_int, _int, _int, _int, _int, C.POINTER(_vp)]),
    "trex_policy_destroy": (None, [_vp]),
    "trex_policy_param_count": (_int, [_vp]),
    "trex_policy_param_offsets": (_int, [_vp, _pint]),
    "trex_policy_get_stats": (_int, [_vp, _pd, _vp]),
    "trex_policy_set_stats": (_int, [_vp, _pd, _vp]),
    "trex_policy_get_returns": (_int, [_vp, _vp, _vp]),
    "trex_policy_observe": (_int, [_vp, _vp, _int, _int, _f, _vp, _vp, _vp, _vp]),
    "trex_policy_act": (_int, [_vp, _vp, _vp, _int, _f, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "trex_policy_gae": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _f, _f, _f, _vp]),
    "trex_policy_adam": (_int, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _vp, _vp]),
    "trex_policy_adam_reset": (_int, [_vp, _vp]),
    "trex_policy_minibatch_stats": (_int, [_vp, _vp, C.c_int64, _vp, _int, _int, _vp, _vp]),
    "trex_policy_minibatch_step": (_int, [_vp] * 11 + [C.c_int64, _vp, _int, _int, _vp] + [_f] * 8 + [_vp, _vp]),
    "trex_policy_minibatch_grad": (_int, [_vp] * 9 + [C.c_int64, _vp, _int, _int, _vp] + [_f] * 4 + [_vp, _vp]),
}


def _declare(table):
    """Give every function of `table` that the loaded library exports its restype and argtypes; -> the table's names."""
    for name, (restype, argtypes) in table.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return list(table)


SYMBOLS = _declare(_BATCH_API)            # every symbol include/trex_batch.h declares
POLICY_SYMBOLS = _declare(_POLICY_API)    # every symbol include/trex_policy.h declares


class TrexError(RuntimeError):
    """Raised where the reference would see pybullet.error / KeyError from the engine boundary."""

    def __init__(self, code, message):
        super().__init__("%s (code %d)" % (message, code))
        self.code = code


def check(code):
    if code < 0:
        raise TrexError(code, lib.trex_last_error().decode())
    return code


E_INVALID = -1   # TREX_E_INVALID


def build_id():
    return lib.trex_build_id().decode()


def _ptr(t, device=None, dtype=None, numel=None, what="tensor"):
    """torch tensor / None -> void* (device pointer). A host tensor, a tensor on another GPU, of another
    dtype or too short would be misread or fault the GPU, so it is refused here (TREX_E_INVALID); the
    C-ABI checks the raw pointer again (capi.cpp check_device_buffer)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise TrexError(E_INVALID, "%s: expected a tensor in device memory, got one on %s" % (what, t.device))
    if not t.is_contiguous():
        raise TrexError(E_INVALID, "%s: expected a contiguous tensor" % what)
    if device is not None and t.device.index != device:
        raise TrexError(E_INVALID, "%s: tensor on cuda:%s, batch on cuda:%d" % (what, t.device.index, device))
    if dtype is not None and t.dtype != dtype:
        raise TrexError(E_INVALID, "%s: expected dtype %s, got %s" % (what, dtype, t.dtype))
    if numel is not None and t.numel() < numel:
        raise TrexError(E_INVALID, "%s: expected at least %d elements, got %d" % (what, numel, t.numel()))
    return C.c_void_p(t.data_ptr())


def _shaped(t, shape, what):
    """t - a tensor, an array or None - as it is, where its shape is exactly the tuple `shape`; else TREX_E_INVALID."""
    if t is not None and tuple(t.shape) != shape:
        raise TrexError(E_INVALID, "%s: expected shape %s, got %s" % (what, shape, tuple(t.shape)))
    return t


def _flags(t, what):
    """t - a tensor of flags or None - as it is, where it is uint8 or bool (the same byte layout: the step hands `done` out as
    bool); else TREX_E_INVALID."""
    if t is not None and t.dtype not in (torch.uint8, torch.bool):
        raise TrexError(E_INVALID, "%s: expected dtype uint8 or bool, got %s" % (what, t.dtype))
    return t


def default_urdf_path():
    return os.path.join(_HERE, "..", "assets", "trex_collide.urdf")


class Model:
    """Compiled model (host side). Replaces loadURDF + joint/dynamics introspection."""

    def __init__(self, urdf_path=None, collisions_dir=None):
        self.urdf_path = os.path.abspath(urdf_path or default_urdf_path())
        h = _vp()
        check(lib.trex_model_load(self.urdf_path.encode(),
                                  collisions_dir.encode() if collisions_dir else None, C.byref(h)))
        self.h = h
        self.num_bodies = lib.trex_model_num_bodies(h)
        self.num_joints = lib.trex_model_num_joints(h)
        self.num_urdf_joints = lib.trex_model_num_urdf_joints(h)
        self.joint_names, self.urdf_joint_indices, lo, hi = [], [], [], []
        for k in range(self.num_joints):
            name, idx, l, u = C.c_char_p(), C.c_int(), C.c_double(), C.c_double()
            check(lib.trex_model_joint_info(h, k, C.byref(name), C.byref(idx), C.byref(l), C.byref(u)))
            self.joint_names.append(name.value.decode())
            self.urdf_joint_indices.append(idx.value)
            lo.append(l.value)
            hi.append(u.value)
        self.lower = np.array(lo)
        self.upper = np.array(hi)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib.trex_model_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def links(self):
        """[(name, body index)] of every URDF link, document order."""
        out = []
        for k in range(lib.trex_model_num_links(self.h)):
            name, body = C.c_char_p(), C.c_int()
            check(lib.trex_model_link_info(self.h, k, C.byref(name), C.byref(body)))
            out.append((name.value.decode(), body.value))
        return out

    def visuals(self):
        """[(mesh file, link index, xyz[3], quat_xyzw[4])] of every <visual> mesh, document order
        (tools/urdf_parsing.py:93-120: UrdfLink.visual_shapes)."""
        out = []
        for k in range(lib.trex_model_num_visuals(self.h)):
            name, link = C.c_char_p(), C.c_int()
            xyz, quat = (C.c_double * 3)(), (C.c_double * 4)()
            check(lib.trex_model_visual_info(self.h, k, C.byref(name), C.byref(link), xyz, quat))
            out.append((name.value.decode(), link.value, np.array(xyz[:]), np.array(quat[:])))
        return out

    def use_primitive_collision(self, max_radius=0.2, max_divisions=3, min_points=4):
        """Replace the convex hulls by fitted capsules / spheres (tools/mesh_primitives.py:323-402)."""
        check(lib.trex_model_use_primitive_collision(self.h, float(max_radius), int(max_divisions), int(min_points)))

    def fit_hull_primitives(self, group, max_radius=0.2, max_divisions=3, min_points=4):
        """[(p0, p1, radius)] fitted to convex hull `group` (body frame); p0 == p1 for a sphere."""
        n = check(lib.trex_model_fit_hull_primitives(self.h, group, max_radius, max_divisions, min_points, None, 0))
        out = np.zeros((n, 7))
        check(lib.trex_model_fit_hull_primitives(self.h, group, max_radius, max_divisions, min_points,
                                                 out.ctypes.data_as(C.POINTER(C.c_double)), n))
        return [(o[0:3].copy(), o[3:6].copy(), float(o[6])) for o in out]

    def total_mass(self, include_base_link=False):
        return lib.trex_model_total_mass(self.h, int(include_base_link))

    def set_start_angle(self, joint_name, angle):
        check(lib.trex_model_set_start_angle(self.h, joint_name.encode(), float(angle)))

    def set_start_pose(self, xyz, rpy):
        a = (C.c_double * 3)(*xyz)
        b = (C.c_double * 3)(*rpy)
        check(lib.trex_model_set_start_pose(self.h, a, b))

    def set_param(self, name, value):
        check(lib.trex_model_set_param(self.h, name.encode(), float(value)))

    def get_param(self, name):
        v = C.c_double()
        check(lib.trex_model_get_param(self.h, name.encode(), C.byref(v)))
        return v.value

    def array(self, name):
        n = check(lib.trex_model_get_array(self.h, name.encode(), None, 0))
        out = np.zeros(n)
        check(lib.trex_model_get_array(self.h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), n))
        return out


class Batch:
    """N env copies on one GPU; all tensors are torch CUDA(HIP) tensors owned by the caller."""

    def __init__(self, model, num_envs, device=0):
        self.model = model
        self.num_envs = int(num_envs)
        self.device = int(device)
        h = _vp()
        check(lib.trex_batch_create(model.h, self.num_envs, self.device, C.byref(h)))
        self.h = h
        self.J = model.num_joints
        self.A = self.J                 # columns of an action row: J, or 2J with stiffness actions
        self.state_width = 13 + 2 * self.J

    def close(self):
        if getattr(self, "h", None):
            lib.trex_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream(stream):
        if stream is None:
                return C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return C.c_void_p(stream)

    def set_reward_weights(self, distance, energy, drift):
        check(lib.trex_batch_set_reward_weights(self.h, distance, energy, drift))

    def _p(self, t, dtype, numel, what):
        return _ptr(t, self.device, getattr(torch, dtype), numel, what)

    def _mask(self, mask):
        """reset mask [n]: uint8 or bool"""
        return _ptr(_flags(mask, "mask"), self.device, None, self.num_envs, "mask")

    def _rows(self, rows, what, width=None, steps=None):
        """void* of the row block rows [n, stride] (with steps=S: [S, n, stride]), long enough for `width` columns in its last
        row: 3J + tail where None, 3J + E + tail for the composed block; the tail is reward | done, and the three penalties
        with penalties in the rows."""
        if width is None:
            width = 3 * self.J + (5 if self.pen_in_rows else 2)
        count, stride = (self.num_envs, rows.shape[1]) if steps is None else (steps * self.num_envs, rows.shape[2])
        return self._p(rows, "float32", (count - 1) * stride + width, what)

    def set_wave_balance(self, mode):
        """-1 auto (on from 2048 envs), 0 off (workgroup k runs env k), 1 on: include/trex_batch.h."""
        check(lib.trex_batch_set_wave_balance(self.h, int(mode)))

    def forget_buffers(self):
        check(lib.trex_batch_forget_buffers(self.h))

    pen_in_rows = False

    def set_penalties_in_rows(self, enabled):
        """Row-block calls write the three penalties to columns 3J+2 .. 3J+4 (row_stride >= 3J + 5): include/trex_batch.h."""
        self.pen_in_rows = bool(enabled)
        check(lib.trex_batch_set_penalties_in_rows(self.h, 1 if enabled else 0))

    def reset(self, obs_out=None, mask=None, stream=None):
        n, J = self.num_envs, self.J
        check(lib.trex_batch_reset(self.h, self._mask(mask), self._p(obs_out, "float32", n * 3 * J, "obs_out"),
                                   self._stream(stream)))

    def step(self, actions, obs, reward, done, penalties=None, stream=None):
        n, J = self.num_envs, self.J
        check(lib.trex_batch_step(self.h, self._p(actions, "float32", n * self.A, "actions"), self._p(obs, "float32", n * 3 * J, "obs"),
                                  self._p(reward, "float32", n, "reward"), self._p(done, "uint8", n, "done"),
                                  self._p(penalties, "float32", 3 * n, "penalties"), self._stream(stream)))

    def step_rows(self, actions, rows, penalties=None, stream=None, done=None):
        """One step writing the [n, stride] row block obs | reward | done (stride = rows.shape[1] >= 3J + 2);
        done [n] uint8 or bool, optional: the flags once more as bytes."""
        n = self.num_envs
        _flags(done, "done")
        check(lib.trex_batch_step_rows(self.h, self._p(actions, "float32", n * self.A, "actions"),
                                       self._rows(rows, "rows"), int(rows.shape[1]), self._p(penalties, "float32", 3 * n, "penalties"),
                                       _ptr(done, self.device, None, n, "done"), self._stream(stream)))

    def step_many(self, actions, rows, penalties=None, done=None, stream=None):
        """S env-steps in one launch: actions [S, n, J], rows [S, n, stride] (obs | reward | done per row)."""
        n, J, S = self.num_envs, self.J, int(actions.shape[0])
        _flags(done, "done")
        if rows.dim() != 3 or int(rows.shape[0]) != S or int(rows.shape[1]) != n:
            raise TrexError(E_INVALID, "rows: expected shape [%d, %d, >= %d], got %s" % (S, n, 3 * J + 2, tuple(rows.shape)))
        check(lib.trex_batch_step_many(self.h, self._p(actions, "float32", S * n * self.A, "actions"),
                                       self._rows(rows, "rows", steps=S), int(rows.shape[2]), S,
                                       self._p(penalties, "float32", 3 * S * n, "penalties"), _ptr(done, self.device, None, S * n, "done"),
                                       self._stream(stream)))

    def reset_rows(self, rows, mask=None, stream=None):
        check(lib.trex_batch_reset_rows(self.h, self._mask(mask), self._rows(rows, "rows"), int(rows.shape[1]), self._stream(stream)))

    def set_episode_limit(self, max_episode_steps, episode_steps=None, stream=None):
        """Episode limit inside the step launch (0 = off); episode_steps [n] int32 sets the per-env counts."""
        check(lib.trex_batch_set_episode_limit(self.h, int(max_episode_steps), self._p(episode_steps, "int32", self.num_envs, "episode_steps"),
                                               self._stream(stream)))

    def get_episode_steps(self, out, stream=None):
        check(lib.trex_batch_get_episode_steps(self.h, self._p(out, "int32", self.num_envs, "episode_steps"), self._stream(stream)))

    def debug_step(self, actions, obs, debug, stream=None):
        n, J = self.num_envs, self.J
        check(lib.trex_batch_debug_step(self.h, self._p(actions, "float32", n * self.A, "actions"),
                                        self._p(obs, "float32", n * 3 * J, "obs"), self._p(debug, "float32", 4096, "debug"),
                                        self._stream(stream)))

    def get_state(self, out, stream=None):
        check(lib.trex_batch_get_state(self.h, self._p(out, "float32", self.num_envs * self.state_width, "state"),
                                       self._stream(stream)))

    def set_state(self, state, stream=None):
        check(lib.trex_batch_set_state(self.h, self._p(state, "float32", self.num_envs * self.state_width, "state"),
                                       self._stream(stream)))

    def set_motors_enabled(self, enabled, stream=None):
        check(lib.trex_batch_set_motors_enabled(self.h, int(enabled), self._stream(stream)))

    def head_position(self, out, stream=None):
        check(lib.trex_batch_head_position(self.h, self._p(out, "float32", 3 * self.num_envs, "out"), self._stream(stream)))

    def link_transforms(self, out, stream=None):
        check(lib.trex_batch_link_transforms(self.h, self._p(out, "float32", None, "out"), self._stream(stream)))

    def visual_transforms(self, out, stream=None):
        check(lib.trex_batch_visual_transforms(self.h, self._p(out, "float32", None, "out"), self._stream(stream)))

    def set_domain(self, mass_scale=None, friction=None, stream=None):
        n = self.num_envs
        check(lib.trex_batch_set_domain(self.h, self._p(mass_scale, "float32", n * self.model.num_bodies, "mass_scale"),
                                        self._p(friction, "float32", n, "friction"), self._stream(stream)))

    def set_external_wrench(self, wrench=None, stream=None):
        """External wrench [n, num_bodies, 6] f32 on the batch's device: fx fy fz at each moving body's COM, tx ty tz about
        it, world axes (include/trex_batch.h). Copied; held for every substep of every later env-step until replaced.
        None clears it (the default kernels again)."""
        _shaped(wrench, (self.num_envs, self.model.num_bodies, 6), "wrench")
        check(lib.trex_batch_set_external_wrench(self.h, self._p(wrench, "float32", self.num_envs * self.model.num_bodies * 6,
                                                                 "wrench"), self._stream(stream)))

    from .actuators import CONTROL_MODES     # TREX_CTRL_*

    def set_control_mode(self, modes=None):
        """Per-joint control modes, shared by all envs: a sequence of J ints (0 position, 1 velocity, 2 torque) or mode names
        in observation order, or None = all position (include/trex_batch.h)."""
        if modes is None:
            check(lib.trex_batch_set_control_mode(self.h, None))
            return
        modes = list(modes)
        if len(modes) != self.J:
            raise TrexError(E_INVALID, "modes: expected %d entries, got %d" % (self.J, len(modes)))
        vals = []
        for m in modes:
            if isinstance(m, str):
                if m not in self.CONTROL_MODES:
                    raise TrexError(E_INVALID, "modes: unknown control mode %r (position, velocity, torque)" % (m,))
                m = self.CONTROL_MODES[m]
            vals.append(int(m))
        check(lib.trex_batch_set_control_mode(self.h, (C.c_int32 * self.J)(*vals)))

    def set_motor_gains(self, kp=None, kd=None, max_force=None, stream=None):
        """Per-env, per-joint motor gains, each [n, J] f32 on the batch's device in observation order, or None = the model
        parameter; all three None clears (include/trex_batch.h). Copied."""
        shape = (self.num_envs, self.J)
        for name, t in (("kp", kp), ("kd", kd), ("max_force", max_force)):
            _shaped(t, shape, name)
        nJ = self.num_envs * self.J
        check(lib.trex_batch_set_motor_gains(self.h, self._p(kp, "float32", nJ, "kp"), self._p(kd, "float32", nJ, "kd"),
                                             self._p(max_force, "float32", nJ, "max_force"), self._stream(stream)))

    def set_stiffness_actions(self, enabled=True, kp_max=1.0):
        """On: every action row is [2J] - J targets, then J stiffnesses kp clipped to [0, kp_max], kd = sqrt(2 kp) - in step,
        step_rows, step_many and time_steps (include/trex_batch.h); off: [J] again."""
        check(lib.trex_batch_set_stiffness_actions(self.h, 1 if enabled else 0, float(kp_max)))
        self.A = 2 * self.J if enabled else self.J

    def set_contact_sensor(self, enabled=True):
        """On: the step and reset launches record each env's floor-contact wrench per body (include/trex_batch.h);
        off: they stop (the default kernels again)."""
        check(lib.trex_batch_set_contact_sensor(self.h, 1 if enabled else 0))

    def contact_wrench(self, out=None, stream=None):
        """The contact sensor's values into out [n, num_bodies, 6] f32 on the batch's device (made when None) and returned:
        force at each body's COM and torque about it, world axes, the mean over the solves since the env's last
        observation."""
        if out is None:
            out = torch.empty(self.num_envs, self.model.num_bodies, 6, dtype=torch.float32, device=self.device)
        check(lib.trex_batch_contact_wrench(self.h, self._p(out, "float32", self.num_envs * self.model.num_bodies * 6, "out"),
                                            self._stream(stream)))
        return out

    # ---- dynamics queries (include/trex_batch.h): read the state, write `out` (made when None) and return it
    def _out(self, out, *shape):
        if out is None:
            return torch.empty(self.num_envs, *shape, dtype=torch.float32, device=self.device)
        return _shaped(out, (self.num_envs,) + shape, "out")

    def inverse_dynamics(self, accel=None, out=None, stream=None):
        """[n, D] generalised force M a + h of accel [n, D] (None = zeros) at the current state, D = 6 + J: base force, base
        torque about the base origin, joint torques in observation order. Rigid-body terms only."""
        D = 6 + self.J
        _shaped(accel, (self.num_envs, D), "accel")
        out = self._out(out, D)
        check(lib.trex_batch_inverse_dynamics(self.h, self._p(accel, "float32", self.num_envs * D, "accel"),
                                              self._p(out, "float32", self.num_envs * D, "out"), self._stream(stream)))
        return out

    def mass_matrix(self, out=None, stream=None):
        """[n, D, D] joint-space inertia matrix, both triangles."""
        D = 6 + self.J
        out = self._out(out, D, D)
        check(lib.trex_batch_mass_matrix(self.h, self._p(out, "float32", self.num_envs * D * D, "out"), self._stream(stream)))
        return out

    def jacobian(self, link, position=None, out=None, stream=None):
        """[n, 6, D] Jacobian of the point `position` (link frame, None = the link origin) of URDF link index `link`: rows 0..2
        its world linear velocity, rows 3..5 the link's world angular velocity, per unit generalised velocity."""
        D = 6 + self.J
        out = self._out(out, 6, D)
        xyz = (C.c_double * 3)(*([0.0, 0.0, 0.0] if position is None else [float(x) for x in position]))
        check(lib.trex_batch_jacobian(self.h, int(link), xyz, self._p(out, "float32", self.num_envs * 6 * D, "out"),
                                      self._stream(stream)))
        return out

    def set_link_probes(self, set, links, positions=None):
        """Probe set `set` (0..7) <- the points `positions` [K, 3] (link frames; None = the link origins) of the URDF link
        indices `links` [K] (trex_batch_set_link_probes); an empty `links` frees the set. Host values, shared by all envs."""
        links = np.ascontiguousarray(np.asarray(links, dtype=np.int64).reshape(-1))
        K = int(links.size)
        if K and (links.min() < np.iinfo(np.int32).min or links.max() > np.iinfo(np.int32).max):
            raise TrexError(E_INVALID, "links: expected link indices")
        links = links.astype(np.int32)
        pos = np.zeros((K, 3)) if positions is None else np.ascontiguousarray(np.asarray(positions, dtype=np.float64))
        _shaped(pos, (K, 3), "positions")
        check(lib.trex_batch_set_link_probes(self.h, int(set), links.ctypes.data_as(C.POINTER(C.c_int32)),
                                             pos.ctypes.data_as(C.POINTER(C.c_double)), K))

    def link_state(self, set, axes=0, proper=False, accel=None, pose=None, velocity=None, acceleration=None, stream=None, probes=None):
        """Kinematics of the probes of set `set` at the current state (trex_batch_link_state): pose [n, K, 7], velocity and
        acceleration [n, K, 6] f32 device tensors, each optional, written in place; accel [n, D] or None = zeros. axes: 0 world,
        1 link, 2 base; proper: + g z on the linear acceleration. probes: K, where the caller knows it - the sizes the buffers
        are checked against before the call (the library checks them against the set's size either way)."""
        n, D = self.num_envs, 6 + self.J
        _shaped(accel, (n, D), "accel")
        K = None if probes is None else int(probes)
        def ptr(t, width, what):
            if K is not None:
                _shaped(t, (n, K, width), what)
            return self._p(t, "float32", 0 if t is None or K is None else n * K * width, what)
        check(lib.trex_batch_link_state(self.h, int(set), int(axes), 1 if proper else 0, self._p(accel, "float32", n * D, "accel"),
                                        ptr(pose, 7, "pose"), ptr(velocity, 6, "velocity"), ptr(acceleration, 6, "acceleration"),
                                        self._stream(stream)))

    def inverse_kinematics(self, set, modes, target, q_out, frame=0, q_init=None, joint_mask=None, info=None, iterations=20,
                           damping=0.01, gain=0.1, max_step=0.2, tol_pos=0.0, tol_ori=0.0, stream=None):
        """Joint angles that bring the K probes of set `set` to the targets target [n, K, 7] (xyz + quaternion xyzw), by damped
        least squares in one launch (trex_batch_inverse_kinematics). modes [K] host: 1 position, 2 orientation, 3 both; frame:
        0 world, 2 base; q_init [n, J] or None = the current joint angles; joint_mask: bit k = joint k (observation order) may
        move, None = all; q_out [n, J] (may be q_init) and info [n, 4] (optional) are written in place."""
        n, J = self.num_envs, self.J
        modes = np.ascontiguousarray(np.asarray(modes, dtype=np.int64).reshape(-1))
        K = int(modes.size)
        if K and (modes.min() < 0 or modes.max() > 255):
            raise TrexError(E_INVALID, "modes: expected values 1..3")
        modes = modes.astype(np.int32)
        _shaped(target, (n, K, 7), "target")
        _shaped(q_init, (n, J), "q_init")
        _shaped(q_out, (n, J), "q_out")
        mask = (1 << J) - 1 if joint_mask is None else int(joint_mask)
        if not 0 <= mask < 1 << 32:
            raise TrexError(E_INVALID, "joint_mask: expected a 32-bit mask")
        prm = TrexIkParams(int(iterations), float(damping), float(gain), float(max_step), float(tol_pos), float(tol_ori))
        check(lib.trex_batch_inverse_kinematics(self.h, int(set), modes.ctypes.data_as(C.POINTER(C.c_int32)), int(frame),
                                                self._p(target, "float32", n * K * 7, "target"),
                                                self._p(q_init, "float32", n * J, "q_init"), mask, C.byref(prm),
                                                self._p(q_out, "float32", n * J, "q_out"), self._p(info, "float32", n * 4, "info"),
                                                self._stream(stream)))

    def set_proximity_shapes(self, bodies, capsules=None, pairs=None):
        """The batch's proximity table (trex_batch_set_proximity_shapes): bodies [C] the body of each capsule, capsules [C, 7] =
        p0 xyz, p1 xyz, radius in the body frame, pairs [P, 2] the bodies (A, B) of each pair to report. Host values, shared by all
        envs; an empty `bodies` frees the table."""
        bodies = np.ascontiguousarray(np.asarray(bodies, dtype=np.int64).reshape(-1))
        Cn = int(bodies.size)
        caps = np.zeros((Cn, 7)) if capsules is None else np.ascontiguousarray(np.asarray(capsules, dtype=np.float64))
        _shaped(caps, (Cn, 7), "capsules")
        pr = np.zeros((0, 2), np.int64) if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int64))
        if pr.size == 0:
            pr = pr.reshape(0, 2)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise TrexError(E_INVALID, "pairs: expected shape (P, 2), got %s" % (pr.shape,))
        for name, x in (("bodies", bodies), ("pairs", pr)):
            if x.size and (x.min() < np.iinfo(np.int32).min or x.max() > np.iinfo(np.int32).max):
                raise TrexError(E_INVALID, "%s: expected body indices" % name)
        bodies, pr = bodies.astype(np.int32), np.ascontiguousarray(pr.astype(np.int32))
        check(lib.trex_batch_set_proximity_shapes(self.h, bodies.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  caps.ctypes.data_as(C.POINTER(C.c_double)), Cn,
                                                  pr.ctypes.data_as(C.POINTER(C.c_int32)), int(pr.shape[0])))

    def proximity(self, distance, point_a=None, point_b=None, normal=None, capsule=None, stream=None, pairs=None):
        """Closest points of every pair of the proximity table at the current state (trex_batch_proximity): distance [n, P],
        point_a, point_b and normal [n, P, 3] f32, capsule [n, P, 2] int32 device tensors, all but distance optional, written in
        place. pairs: P, where the caller knows it - the sizes the buffers are checked against before the call (the library
        checks them against the table's size either way)."""
        n = self.num_envs
        P = None if pairs is None else int(pairs)
        def ptr(t, width, what, dtype="float32"):
            if P is not None:
                _shaped(t, (n, P) if width == 1 else (n, P, width), what)
            return self._p(t, dtype, 0 if t is None or P is None else n * P * width, what)
        check(lib.trex_batch_proximity(self.h, ptr(distance, 1, "distance"), ptr(point_a, 3, "point_a"), ptr(point_b, 3, "point_b"),
                                       ptr(normal, 3, "normal"), ptr(capsule, 2, "capsule", "int32"), self._stream(stream)))

    def body_clearance(self, clearance=None, lowest=None, stream=None):
        """Height of the lowest collision point of every body above the floor at the current state (trex_batch_body_clearance):
        clearance [n, num_bodies] f32 on the batch's device (made when None, and returned; +inf for a body without points),
        lowest [n, num_bodies, 3] optional: that point's world position."""
        nb = self.model.num_bodies
        clearance = self._out(clearance, nb)
        _shaped(lowest, (self.num_envs, nb, 3), "lowest")
        check(lib.trex_batch_body_clearance(self.h, self._p(clearance, "float32", self.num_envs * nb, "clearance"),
                                            self._p(lowest, "float32", self.num_envs * nb * 3, "lowest"), self._stream(stream)))
        return clearance

    def set_termination(self, head_height=None, max_tilt=None, clear_min=None, penalty=0.0):
        """Fall termination inside the step calls (trex_batch_set_termination): head_height - the head point's least height above
        the floor, max_tilt - the base's largest tilt from its start orientation, rad in (0, pi], clear_min - [num_bodies] host
        values, the clearance each body has to keep (NaN: not watched); None switches a criterion off, all three None the
        feature. penalty: taken from the reward of the terminating step."""
        nan = float("nan")
        cm = None
        if clear_min is not None:
            a = np.ascontiguousarray(np.asarray(clear_min, dtype=np.float32).reshape(-1))
            if a.size != self.model.num_bodies:
                raise TrexError(E_INVALID, "clear_min: expected %d entries, got %d" % (self.model.num_bodies, a.size))
            cm = a.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.trex_batch_set_termination(self.h, nan if head_height is None else float(head_height),
                                             nan if max_tilt is None else float(max_tilt), cm, float(penalty)))

    def termination_info(self, reason=None, values=None, terminal_obs=None, stream=None):
        """What the last step call's predicate left (trex_batch_termination_info), copied into the tensors given: reason [n]
        int32 (bits 1 head, 2 tilt, 4 clearance), values [n, 3] f32 (head height, cos tilt, least clearance margin),
        terminal_obs [n, 3J] f32."""
        n = self.num_envs
        check(lib.trex_batch_termination_info(self.h, self._p(reason, "int32", n, "reason"), self._p(values, "float32", 3 * n, "values"),
                                              self._p(terminal_obs, "float32", n * 3 * self.J, "terminal_obs"), self._stream(stream)))

    def set_observation(self, channels=()):
        """The batch's observation channels (trex_batch_set_observation): a sequence of (kind, link, local_xyz[3], scale) - kind a
        TREX_OBS_* value, link a URDF link index (EXTERNAL: its column count). Host values, shared by all envs; an empty sequence
        clears. -> E, the columns the channels add to a composed row."""
        arr = (TrexObsChannel * max(len(channels), 1))()
        for o, (kind, link, xyz, scale) in zip(arr, channels):
            o.kind, o.link, o.scale = int(kind), int(link), float(scale)
            o.local_xyz[:] = [float(x) for x in xyz]
        extra = C.c_int()
        check(lib.trex_batch_set_observation(self.h, arr, len(channels), C.byref(extra)))
        self.obs_extra = extra.value
        return extra.value

    obs_extra = 0

    def observation_dim(self):
        """3J + E (trex_batch_observation_dim)"""
        return check(lib.trex_batch_observation_dim(self.h))

    def compose_rows(self, rows, out, actions=None, extern=None, stream=None):
        """The extended rows obs | channels | tail (trex_batch_compose_rows) into out [n, >= 3J + E + tail] from rows [n, >= 3J +
        tail] - what step_rows / reset_rows wrote -, actions [n, A] or None (PREV_ACTION reads zeros) and extern [n, X] or None:
        the columns the EXTERNAL channels copy. One launch, stream-ordered; the state is only read."""
        n, J = self.num_envs, self.J
        tail = 5 if self.pen_in_rows else 2
        for t, what in ((rows, "rows"), (out, "out"), (extern, "extern")):
            if t is not None and (not hasattr(t, "dim") or t.dim() != 2 or t.shape[0] != n):
                raise TrexError(E_INVALID, "%s: expected a tensor of shape [%d, columns]" % (what, n))
        check(lib.trex_batch_compose_rows(self.h, self._rows(rows, "rows"), int(rows.shape[1]),
                                          self._p(actions, "float32", n * self.A, "actions"),
                                          self._p(extern, "float32", None, "extern"), 0 if extern is None else int(extern.shape[1]),
                                          self._rows(out, "out", 3 * J + self.obs_extra + tail), int(out.shape[1]), self._stream(stream)))

    def centroidal(self, out=None, stream=None):
        """[n, 16]: COM position, COM velocity, linear momentum, angular momentum about the COM, kinetic energy, potential
        energy, total mass, 0."""
        out = self._out(out, 16)
        check(lib.trex_batch_centroidal(self.h, self._p(out, "float32", self.num_envs * 16, "out"), self._stream(stream)))
        return out

    def forward_dynamics(self, force=None, out=None, stream=None):
        """[n, D] accelerations M^-1 (force - h) for the generalised force `force` [n, D] (None = zeros) at the current state:
        the inverse of inverse_dynamics. `out` may be `force` itself."""
        D = 6 + self.J
        _shaped(force, (self.num_envs, D), "force")
        out = self._out(out, D)
        check(lib.trex_batch_forward_dynamics(self.h, self._p(force, "float32", self.num_envs * D, "force"),
                                              self._p(out, "float32", self.num_envs * D, "out"), self._stream(stream)))
        return out

    def solve_mass(self, rhs=None, out=None, stream=None):
        """[n, K, D] = M^-1 applied to the K rows rhs[e, k, :] of every env (None = the identity, K = D: M^-1 itself). A
        [n, D] rhs counts as K = 1 and returns [n, D]. `out` may be `rhs` itself."""
        D = 6 + self.J
        if rhs is None:
            shape = (D, D)
        elif rhs.dim() in (2, 3) and rhs.shape[0] == self.num_envs and rhs.shape[-1] == D:
            shape = tuple(rhs.shape[1:])
        else:
            raise TrexError(E_INVALID, "rhs: expected shape (%d, K, %d) or (%d, %d), got %s"
                            % (self.num_envs, D, self.num_envs, D, tuple(rhs.shape)))
        K = shape[0] if len(shape) == 2 else 1
        out = self._out(out, *shape)
        numel = self.num_envs * K * D
        check(lib.trex_batch_solve_mass(self.h, self._p(rhs, "float32", numel, "rhs"), K,
                                        self._p(out, "float32", numel, "out"), self._stream(stream)))
        return out

    def contact_stats(self, count=None, normal_impulse=None, stream=None):
        n = self.num_envs
        check(lib.trex_batch_contact_stats(self.h, self._p(count, "int32", n, "count"),
                                           self._p(normal_impulse, "float32", n, "normal_impulse"), self._stream(stream)))

    def render(self, camera, width, height, env_ids=None, rgb=None, depth=None, seg=None, stream=None):
        """Ray-cast views of the envs (trex_batch_render): camera = trex_gym.render.Camera (or anything with its fields),
        env_ids = host sequence of env indices (None = all n in order); rgb [V, H, W, 3] uint8, depth [V, H, W] float32,
        seg [V, H, W] int32 device tensors, any of them None."""
        cam = TrexCamera(float(camera.distance), float(camera.yaw), float(camera.pitch), float(camera.fov), float(camera.near),
                         float(camera.far), 1 if camera.target is None else 0,
                         (C.c_float * 3)(*([0.0] * 3 if camera.target is None else [float(x) for x in camera.target])))
        if env_ids is None:
            ids, V = None, self.num_envs
        else:
            arr = np.ascontiguousarray(np.asarray(env_ids, dtype=np.int64).reshape(-1))
            if arr.size == 0 or np.any(arr < np.iinfo(np.int32).min) or np.any(arr > np.iinfo(np.int32).max):
                raise TrexError(E_INVALID, "env_ids: expected a non-empty list of env indices")
            arr = arr.astype(np.int32)
            ids, V = arr.ctypes.data_as(C.POINTER(C.c_int32)), int(arr.size)
        px = V * max(int(width), 0) * max(int(height), 0)
        check(lib.trex_batch_render(self.h, C.byref(cam), int(width), int(height), ids, V if env_ids is not None else 0,
                                    self._p(rgb, "uint8", 3 * px, "rgb"), self._p(depth, "float32", px, "depth"),
                                    self._p(seg, "int32", px, "seg"), self._stream(stream)))

    def ray_test(self, rays, link=-1, shared=None, body_mask=0xFFFFFFFF, hit_floor=True, fraction=None, body=None, position=None,
                 normal=None, stream=None):
        """Ray casts against the geometry render() draws (trex_batch_ray_test): rays [n, R, 6] f32 on the batch's device, or
        [R, 6] for one pattern shared by every env (shared defaults from the rank) - from xyz, to xyz in the frame of URDF link
        index `link` (-1: world). body_mask: bit b = body b may be hit; hit_floor: the floor may be. Outputs, device tensors:
        fraction [n, R] f32 (made when None, and returned), body [n, R] int32, position and normal [n, R, 3] f32, each optional."""
        if not hasattr(rays, "dim") or rays.dim() not in (2, 3) or rays.shape[-1] != 6:
            raise TrexError(E_INVALID, "rays: expected a tensor of shape [n, R, 6] or [R, 6]")
        if shared is None:
            shared = rays.dim() == 2
        n, R = self.num_envs, int(rays.shape[-2])
        _shaped(rays, (R, 6) if shared else (n, R, 6), "rays")
        mask = int(body_mask)
        if not 0 <= mask <= 0xFFFFFFFF:
            raise TrexError(E_INVALID, "body_mask: expected a 32-bit mask, got %r" % (body_mask,))
        if fraction is None and rays.is_cuda:
            fraction = torch.empty(n, R, dtype=torch.float32, device=rays.device)
        for name, t, shape in (("fraction", fraction, (n, R)), ("body", body, (n, R)), ("position", position, (n, R, 3)),
                               ("normal", normal, (n, R, 3))):
            _shaped(t, shape, name)
        check(lib.trex_batch_ray_test(self.h, self._p(rays, "float32", (1 if shared else n) * R * 6, "rays"), R, 1 if shared else 0,
                                      int(link), mask, 1 if hit_floor else 0, self._p(fraction, "float32", n * R, "fraction"),
                                      self._p(body, "int32", n * R, "body"), self._p(position, "float32", n * R * 3, "position"),
                                      self._p(normal, "float32", n * R * 3, "normal"), self._stream(stream)))
        return fraction

    def launch_info(self):
        g, b, l, a = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib.trex_batch_launch_info(self.h, C.byref(g), C.byref(b), C.byref(l), C.byref(a)))
        return dict(grid=g.value, block=b.value, lds_bytes=l.value, alg_bytes_per_env_step=a.value)

    def time_steps(self, actions, obs, reward, done, steps, stream=None):
        ms = C.c_float()
        n, J = self.num_envs, self.J
        check(lib.trex_batch_time_steps(self.h, self._p(actions, "float32", n * self.A, "actions"), self._p(obs, "float32", n * 3 * J, "obs"),
                                        self._p(reward, "float32", n, "reward"), self._p(done, "uint8", n, "done"), int(steps),
                                        self._stream(stream), C.byref(ms)))
        return ms.value


class Policy:
    """Trainer-side kernels of include/trex_policy.h for N envs on one GPU: VecNormalize state + MlpPolicy.step +
    GAE + Adam. All tensors are torch HIP tensors owned by the caller; the parameter vector is ONE flat f32 tensor."""

    PARAM_NAMES = ["pi.W1", "pi.b1", "pi.W2", "pi.b2", "pi.W3", "pi.b3", "vf.W1", "vf.b1", "vf.W2", "vf.b2", "vf.W3", "vf.b3",
                   "logstd"]

    def __init__(self, num_envs, obs_dim, act_dim, hidden=64, device=0):
        self.n, self.D, self.A, self.H, self.device = int(num_envs), int(obs_dim), int(act_dim), int(hidden), int(device)
        h = _vp()
        check(lib.trex_policy_create(self.n, self.D, self.A, self.H, self.device, C.byref(h)))
        self.h = h
        self.param_count = lib.trex_policy_param_count(h)
        off = (C.c_int * 13)()
        check(lib.trex_policy_param_offsets(h, off))
        D, A, H = self.D, self.A, self.H
        shapes = [(D, H), (H,), (H, H), (H,), (H, A), (A,), (D, H), (H,), (H, H), (H,), (H, 1), (1,), (A,)]
        self.layout = {n: (int(o), sh) for n, o, sh in zip(self.PARAM_NAMES, off, shapes)}

    def close(self):
        if getattr(self, "h", None):
            lib.trex_policy_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _p(self, t, numel, what, dtype="float32"):
        return _ptr(t, self.device, getattr(torch, dtype), numel, what)

    _stream = staticmethod(Batch._stream)

    def get_stats(self):
        """dict of VecNormalize's running statistics (host, f64)."""
        D = self.D
        buf = (C.c_double * (2 * D + 5))()
        check(lib.trex_policy_get_stats(self.h, buf, self._stream(None)))
        a = np.array(buf[:])
        return dict(obs_mean=a[:D], obs_var=a[D:2 * D], obs_count=a[2 * D], ret_mean=a[2 * D + 1], ret_var=a[2 * D + 2],
                    ret_count=a[2 * D + 3], raw_reward_sum=a[2 * D + 4])

    def set_stats(self, st):
        D = self.D
        a = np.concatenate([np.asarray(st["obs_mean"], float).reshape(D), np.asarray(st["obs_var"], float).reshape(D),
                            [st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"], st.get("raw_reward_sum", 0.0)]])
        check(lib.trex_policy_set_stats(self.h, (C.c_double * (2 * D + 5))(*a), self._stream(None)))

    def get_returns(self, out):
        check(lib.trex_policy_get_returns(self.h, self._p(out, self.n, "ret"), self._stream(None)))

    def observe(self, rows, with_reward=True, gamma=0.99, raw_rew_out=None, done_out=None, rew_scale_out=None, stream=None):
        n = self.n
        check(lib.trex_policy_observe(self.h, self._p(rows, (n - 1) * rows.shape[1] + self.D + (2 if with_reward else 0), "rows"),
                                      int(rows.shape[1]), int(bool(with_reward)), float(gamma), self._p(raw_rew_out, n, "raw_rew_out"),
                                      self._p(done_out, n, "done_out"), self._p(rew_scale_out, 1, "rew_scale_out"),
                                      self._stream(stream)))

    def act(self, theta, rows, noise, actions, obs_out=None, act_out=None, logp_out=None, value_out=None, clip_obs=10.0,
            value_only=False, stream=None):
        n, D, A = self.n, self.D, self.A
        check(lib.trex_policy_act(self.h, self._p(theta, self.param_count, "theta"), self._p(rows, (n - 1) * rows.shape[1] + D, "rows"),
                                  int(rows.shape[1]), float(clip_obs), self._p(noise, n * A, "noise"), self._p(actions, n * A, "actions"),
                                  self._p(obs_out, n * D, "obs_out"), self._p(act_out, n * A, "act_out"),
                                  self._p(logp_out, n, "logp_out"), self._p(value_out, n, "value_out"), int(bool(value_only)),
                                  self._stream(stream)))

    def gae(self, raw_rew, rew_scale, done, values, adv, ret, gamma=0.99, lam=0.95, clip_rew=10.0, stream=None):
        T, n = int(raw_rew.shape[0]), self.n
        check(lib.trex_policy_gae(self.h, self._p(raw_rew, T * n, "raw_rew"), self._p(rew_scale, T, "rew_scale"),
                                  self._p(done, T * n, "done"), self._p(values, (T + 1) * n, "values"), self._p(adv, T * n, "adv"),
                                  self._p(ret, T * n, "ret"), T, float(gamma), float(lam), float(clip_rew), self._stream(stream)))

    def adam(self, theta, grad, m, v, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, grad_norm_out=None, stream=None):
        P = self.param_count
        check(lib.trex_policy_adam(self.h, self._p(theta, P, "theta"), self._p(grad, P, "grad"), self._p(m, P, "m"), self._p(v, P, "v"),
                                   float(lr), float(beta1), float(beta2), float(eps), float(max_grad_norm),
                                   self._p(grad_norm_out, 1, "grad_norm_out"), self._stream(stream)))

    def adam_reset(self, stream=None):
        check(lib.trex_policy_adam_reset(self.h, self._stream(stream)))

    def minibatch_stats(self, adv, perm, num_minibatches, mb, out, stream=None):
        N = adv.numel()
        check(lib.trex_policy_minibatch_stats(self.h, self._p(adv, N, "adv"), N, self._p(perm, num_minibatches * mb, "perm", "int64"),
                                              int(num_minibatches), int(mb), self._p(out, 2 * num_minibatches, "stats_out"),
                                              self._stream(stream)))

    def minibatch_grad(self, theta, grad, obs, act, logp, val, adv, ret, perm, first, mb, adv_stats, cliprange=0.2, ent_coef=0.0,
                       vf_coef=0.5, grad_scale=1.0, loss_sums=None, stream=None):
        """The gradient of perm[first : first + mb] alone, times grad_scale (no clip, no Adam): the data-parallel trainer's
        half of a minibatch step (include/trex_policy.h)."""
        P, N, D, A = self.param_count, adv.numel(), self.D, self.A
        check(lib.trex_policy_minibatch_grad(
            self.h, self._p(theta, P, "theta"), self._p(grad, P, "grad"), self._p(obs, N * D, "obs"), self._p(act, N * A, "act"),
            self._p(logp, N, "logp"), self._p(val, N, "val"), self._p(adv, N, "adv"), self._p(ret, N, "ret"), N,
            self._p(perm, first + mb, "perm", "int64"), int(first), int(mb), self._p(adv_stats, 2, "adv_stats"), float(cliprange),
            float(ent_coef), float(vf_coef), float(grad_scale), self._p(loss_sums, 2, "loss_sums"), self._stream(stream)))

    def minibatch_step(self, theta, grad, m, v, obs, act, logp, val, adv, ret, perm, first, mb, adv_stats, cliprange=0.2,
                       ent_coef=0.0, vf_coef=0.5, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, loss_sums=None,
                       stream=None):
        """One PPO2 minibatch step on perm[first : first + mb] (include/trex_policy.h): three launches."""
        P, N, D, A = self.param_count, adv.numel(), self.D, self.A
        check(lib.trex_policy_minibatch_step(
            self.h, self._p(theta, P, "theta"), self._p(grad, P, "grad"), self._p(m, P, "m"), self._p(v, P, "v"),
            self._p(obs, N * D, "obs"), self._p(act, N * A, "act"), self._p(logp, N, "logp"), self._p(val, N, "val"),
            self._p(adv, N, "adv"), self._p(ret, N, "ret"), N, self._p(perm, first + mb, "perm", "int64"), int(first), int(mb),
            self._p(adv_stats, 2, "adv_stats"), float(cliprange), float(ent_coef), float(vf_coef), float(lr), float(beta1),
            float(beta2), float(eps), float(max_grad_norm), self._p(loss_sums, 2, "loss_sums"), self._stream(stream)))
