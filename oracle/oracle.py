"""ORACLE (test infrastructure): ctypes binding of oracle/trex_oracle.c.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import trex_model

_HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_ORDER = ["dt", "substeps", "iterations", "gravity", "motor_kp", "motor_kd", "motor_max_force",
               "floor_z", "friction", "erp", "contact_erp", "contact_margin", "link_damping",
               "max_coordinate_velocity", "max_contacts"]
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def build(force=False):
    out = os.path.join(_HERE, "_build")
    libs = [os.path.join(out, "liboracle_f64.so"), os.path.join(out, "liboracle_f32.so")]
    src = os.path.join(_HERE, "trex_oracle.c")
    stale = force or any(not os.path.exists(l) or os.path.getmtime(l) < os.path.getmtime(src)
                         for l in libs)
    if stale:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
    return libs


def _d(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(_dp)


def _i(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(_ip)


class Oracle:
    """One model + any number of env states. precision: 'f64' (oracle of record) or 'f32'."""

    def __init__(self, model, params=None, precision="f64"):
        libs = build()
        self.lib = lib = C.CDLL(libs[0] if precision == "f64" else libs[1])
        self.model = model
        self.params = dict(trex_model.default_params())
        if params:
            self.params.update(params)
        assert lib.oracle_param_count() == len(PARAM_ORDER)
        lib.oracle_model_create.restype = C.c_void_p
        lib.oracle_state_create.restype = C.c_void_p
        lib.oracle_state_create.argtypes = [C.c_void_p]
        lib.oracle_reward.restype = C.c_double
        m = model
        keep = []
        def d(x):
            a, p = _d(x); keep.append(a); return p
        def i(x):
            a, p = _i(x); keep.append(a); return p
        prm = np.array([self.params[k] for k in PARAM_ORDER], np.float64)
        self.h = lib.oracle_model_create(
            C.c_int(m["nb"]), i(m["parent"]), d(m["joint_axis"]), d(m["joint_pos"]), d(m["joint_rot"]),
            d(m["q_lower"]), d(m["q_upper"]), d(m["joint_damping"]), d(m["mass"]), d(m["com"]),
            d(m["inertia"]), i(m["obs_order"]), C.c_int(m["head_body"]), d(m["head_point"]),
            C.c_int(len(m["hull_xyz"])), d(m["hull_xyz"]), d(m.get("hull_radius", np.zeros(len(m["hull_xyz"])))),
            i(m["hull_start"]), d(m["sphere_center"]),
            d(m["sphere_radius"]), d(m["q_start"]), d(m["base_start_pos"]), d(m["base_start_quat"]),
            d(prm))
        assert self.h
        self.h = C.c_void_p(self.h)
        self.nb = m["nb"]
        self.nj = self.nb - 1
        self.nd = 6 + self.nj

    def set_param(self, name, value):
        self.params[name] = value
        self.lib.oracle_model_set_param(self.h, C.c_int(PARAM_ORDER.index(name)), C.c_double(value))

    # ---- states
    def new_state(self):
        return C.c_void_p(self.lib.oracle_state_create(self.h))

    def copy_state(self, s):
        t = self.new_state()
        self.lib.oracle_state_copy(t, s)
        return t

    def set_domain(self, s, mass_scale=None, friction=None):
        ms = None
        if mass_scale is not None:
            a, ms = _d(mass_scale)
        self.lib.oracle_set_domain(self.h, s, ms, C.c_double(self.params["friction"] if friction is None else friction))

    def get_state(self, s):
        out = np.zeros(13 + 2 * self.nj)
        self.lib.oracle_get_state(self.h, s, out.ctypes.data_as(_dp))
        return out

    def set_state(self, s, vec):
        a, p = _d(vec)
        assert a.size == 13 + 2 * self.nj
        self.lib.oracle_set_state(self.h, s, p)

    def set_warmstart(self, s, factor):
        """PGS warm start of this state's solves (include/trex_batch.h, "warmstart"); 0 = cold, the default"""
        self.lib.oracle_set_warmstart(s, C.c_double(factor))

    def set_external_wrench(self, s, w):
        """w [nb, 6] = fx fy fz at the COM, tx ty tz about it, world axes (the C-ABI's layout), held until replaced; None clears it"""
        if w is None:
            self.lib.oracle_set_external_wrench(s, None)
        else:
            a, p = _d(w)
            assert a.shape == (self.nb, 6)
            self.lib.oracle_set_external_wrench(s, p)

    def warm_record(self, s):
        """the record of the state's last solve: hull vertices [k] and (normal, friction x, friction y) impulses [k, 3], k <= 13"""
        vert, lam = np.zeros(13, np.int32), np.zeros((13, 3))
        k = self.lib.oracle_warm_record(s, vert.ctypes.data_as(_ip), lam.ctypes.data_as(_dp))
        return vert[:k].copy(), lam[:k].copy()

    def set_motors_on(self, s, on):
        self.lib.oracle_set_motors_on(s, C.c_int(int(on)))

    # ---- env semantics
    def reset(self, s):
        self.lib.oracle_reset(self.h, s)
        return self.observe(s)

    def observe(self, s):
        obs = np.zeros(3 * self.nj)
        self.lib.oracle_observe(self.h, s, obs.ctypes.data_as(_dp))
        return obs

    def step(self, s, action, weights=(1.0, 0.005, 0.002)):
        a, ap = _d(action)
        w, wp = _d(weights)
        obs = np.zeros(3 * self.nj)
        rew = C.c_double()
        pen = np.zeros(3)
        self.lib.oracle_step(self.h, s, ap, wp, obs.ctypes.data_as(_dp), C.byref(rew), pen.ctypes.data_as(_dp))
        return obs, rew.value, pen

    def substep(self, s, target=None):
        if target is None:
            self.lib.oracle_substep(self.h, s, None)
        else:
            a, p = _d(target)
            self.lib.oracle_substep(self.h, s, p)

    def reward(self, s, weights=(1.0, 0.005, 0.002)):
        w, wp = _d(weights)
        pen = np.zeros(3)
        r = self.lib.oracle_reward(self.h, s, wp, pen.ctypes.data_as(_dp))
        return r, pen

    def head_position(self, s):
        out = np.zeros(3)
        self.lib.oracle_head_position(self.h, s, out.ctypes.data_as(_dp))
        return out

    # ---- diagnostics
    def forward_dynamics(self, s, tau=None, with_damping=False):
        qdd = np.zeros(self.nj)
        ba = np.zeros(6)
        tp = None
        if tau is not None:
            t, tp = _d(tau)
        self.lib.oracle_forward_dynamics(self.h, s, tp, C.c_int(int(with_damping)),
                                         qdd.ctypes.data_as(_dp), ba.ctypes.data_as(_dp))
        return qdd, ba

    def minv(self, s):
        out = np.zeros((self.nd, self.nd))
        self.lib.oracle_minv(self.h, s, out.ctypes.data_as(_dp))
        return out

    def body_poses(self, s):
        pos = np.zeros((self.nb, 3))
        rot = np.zeros((self.nb, 9))
        self.lib.oracle_body_poses(self.h, s, pos.ctypes.data_as(_dp), rot.ctypes.data_as(_dp))
        return pos, rot.reshape(self.nb, 3, 3)

    def contacts(self, s):
        n = 64
        body, lam, pos, dist = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        k = self.lib.oracle_contacts(s, body.ctypes.data_as(_dp), lam.ctypes.data_as(_dp),
                                     pos.ctypes.data_as(_dp), dist.ctypes.data_as(_dp))
        return body[:k].astype(int), lam[:k], pos[:k], dist[:k]

    def limit_rows(self, s):
        return self.lib.oracle_limit_rows(s)

    def energy(self, s):
        out = np.zeros(8)
        self.lib.oracle_energy(self.h, s, out.ctypes.data_as(_dp))
        return dict(ke=out[0], pe=out[1], momentum=out[2:8])


def default_asset_urdf():
    return os.path.join(_HERE, "..", "trex-gym_amd", "assets", "trex_collide.urdf")
