"""numpy restatement of the start-state randomisation (include/trex_start_state.h), written from the header's definition and not
from the kernel: the stream and counters over the Philox4x32-10 of tests/sensing_ref.py, the episode counts, the draws of an
episode, the six operations in their fixed order and the floor placement over the forward kinematics of tests/dynamics_ref.py. The
arithmetic runs in f64 - the reference proper - or, with f32=True, with every product and sum rounded to f32 as the header orders
them: that run is what the device must give bitwise wherever no sinf, cosf or forward kinematics is involved (the draws, q, qd, the
offsets on a state that is not rotated, the episode counts), and its deviation from the f64 run is what tests/start_state_cases.py
derives the bounds of the quaternion, the rotated velocities and the placement from.

A state is a row of trex_batch_get_state: pos 3 | quat xyzw 4 | v 3 | w 3 | q J | qd J, joints in observation order. `model` is the
compiled model of oracle/trex_model.py. numpy only: no torch, no device. A helper, not a conftest."""
import collections

import numpy as np

import dynamics_ref as DR
from sensing_ref import key_of, philox4x32, u_half_open

(JOINT_POSITION, JOINT_VELOCITY, BASE_RPY, BASE_LINEAR_VELOCITY, BASE_ANGULAR_VELOCITY, BASE_POSITION, FLOOR_CLEARANCE) = range(7)
KINDS, MAXTERMS, TL, STREAM = 7, 16, 32, 7
Term = collections.namedtuple("Term", "kind mask index shared lo hi")
# one apply: the states after it [n, 13 + 2J], first [n] bool (the envs that started), values [n, T, 32], ep [n], shift [n],
# lowest [n] (-1: none), gap [n]: the height by which the second lowest collision point lies above the lowest (inf: no placement)
Applied = collections.namedtuple("Applied", "state first values ep shift lowest gap")


def elements(term, nj):
    """the elements a term covers, ascending: joints in observation order for the joint kinds, [0] otherwise"""
    if term.kind in (JOINT_POSITION, JOINT_VELOCITY):
        return [i for i in range(nj) if term.mask == 0 or (term.mask >> i) & 1]
    return [0]


def rpy_quat(rpy, dt):
    """the quaternion xyzw of R = Rz(yaw) Ry(pitch) Rx(roll), from the cosines and sines of the half angles"""
    h = np.asarray(rpy, dt) * dt(0.5)
    (cr, cp, cy), (sr, sp, sy) = np.cos(h), np.sin(h)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], dt)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def point_heights(model, state, dt):
    """the height of every collision point less its radius, relative to the base origin: [nv]"""
    rel = np.array(state, dt)
    rel[0:3] = 0
    k = DR.Kin(model, rel, dtype=dt)
    hs = np.asarray(model["hull_start"]).astype(int)
    xyz, rad = np.asarray(model["hull_xyz"], dt), np.asarray(model["hull_radius"], dt)
    out = np.zeros(hs[model["nb"]], dt)
    for b in range(model["nb"]):
        out[hs[b]:hs[b + 1]] = (xyz[hs[b]:hs[b + 1]] @ k.R[b][2] + k.p[b][2]) - rad[hs[b]:hs[b + 1]]
    return out


class StartState:
    """The start-state terms of a batch of n envs and what trex_batch_apply_start_state does to the states it finds."""

    def __init__(self, model, n, terms, seed=0, env_offset=0, floor_z=0.0, f32=False):
        self.model, self.n, self.nj = model, n, model["nb"] - 1
        self.terms = [Term(*t) for t in terms]
        self.key, self.env_offset, self.f32 = key_of(seed), int(env_offset), f32
        self.dt = np.float32 if f32 else np.float64
        self.floor_z = self.dt(np.float32(floor_z))
        oo = np.asarray(model["obs_order"])
        self.lower = np.asarray(model["q_lower"], np.float32)[oo].astype(self.dt)
        self.upper = np.asarray(model["q_upper"], np.float32)[oo].astype(self.dt)
        self.ep = np.zeros(n, np.int64)
        self.started = np.zeros(n, bool)
        self.values = np.zeros((n, len(self.terms), TL), self.dt)
        self.shift = np.zeros(n, self.dt)
        self.lowest = np.full(n, -1, np.int64)

    def reset(self, mask=None):
        self.started[np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0] = False

    def _value(self, t, src):
        """[n]: the uniform value of term t from the word of element src"""
        term, dt = self.terms[t], self.dt
        e = self.env_offset + np.arange(self.n)
        r = philox4x32((e, np.zeros(self.n, np.int64), (STREAM << 16) | (8 * t + (src >> 2)), self.ep), self.key)
        lo, hi, u = dt(np.float32(term.lo)), dt(np.float32(term.hi)), u_half_open(r[src & 3]).astype(dt)
        v = lo + (hi - lo) * u
        assert v.dtype == dt
        return v

    def apply(self, done, state):
        """state [n, 13 + 2J] as found (f32-exact numbers) -> Applied; the envs that are not starting keep their rows"""
        n, J, dt = self.n, self.nj, self.dt
        first = (np.asarray(done) != 0) | ~self.started
        self.ep += first
        self.started[:] = True
        s = np.array(state, dt)
        assert s.shape == (n, 13 + 2 * J)
        rpy, rotate = np.zeros((n, 3), dt), False
        offsets, clearance = [], None
        for t, term in enumerate(self.terms):
            for i in elements(term, J):
                v = self._value(t, 0 if term.shared else i)
                self.values[:, t, i] = np.where(first, v, self.values[:, t, i])
                if term.kind == JOINT_POSITION:
                    s[:, 13 + i] = np.minimum(np.maximum(s[:, 13 + i] + v, self.lower[i]), self.upper[i])
                elif term.kind == JOINT_VELOCITY:
                    s[:, 13 + J + i] = s[:, 13 + J + i] + v
                elif term.kind == BASE_RPY:
                    rpy[:, term.index], rotate = v, True
                elif term.kind == FLOOR_CLEARANCE:
                    clearance = v
                else:
                    col = {BASE_LINEAR_VELOCITY: 7, BASE_ANGULAR_VELOCITY: 10, BASE_POSITION: 0}[term.kind] + term.index
                    offsets.append((col, v))
        gap = np.full(n, np.inf)
        for e in np.flatnonzero(first):
            if rotate:
                r = rpy_quat(rpy[e], dt)
                quat = quat_mul(r, s[e, 3:7])
                s[e, 3:7] = quat / np.sqrt((quat * quat).sum())
                R = DR.quat_to_mat(r, dt)
                s[e, 7:10], s[e, 10:13] = R @ s[e, 7:10], R @ s[e, 10:13]
            for col, v in offsets:
                s[e, col] = s[e, col] + v[e]
            if clearance is not None:
                h = point_heights(self.model, s[e], dt)
                self.shift[e], self.lowest[e] = 0, -1
                if len(h):
                    k = int(np.argmin(h))      # (the first of equal heights)
                    z = (self.floor_z + clearance[e]) - h[k]
                    self.shift[e], self.lowest[e] = z - s[e, 2], k
                    s[e, 2] = z
                    if len(h) > 1:
                        gap[e] = float(np.delete(h, k).min() - h[k])
        assert s.dtype == dt
        s = np.where(first[:, None], s, np.array(state, dt))
        return Applied(s, first.copy(), self.values.copy(), self.ep.copy(), self.shift.copy(), self.lowest.copy(), gap)
