"""Motion clips for a TrexVecEnv, attached by attach(env, clip, ...) (include/trex_motion.h): a reference motion kept on the device,
tracking terms against it composed into the reward column, a phase observation, and reference state initialisation (RSI) - the
three parts of the DeepMimic recipe, each one launch.

A Clip is F frames [pos 3 | quat xyzw 4 | q J] at a fixed frame interval, with optional per-frame velocities [v 3 | w 3 | qd J]
(world axes; derived by central differences when absent). loop=True makes time wrap modulo T = (F - 1) frame_dt; the base x and
y advance by pos[F-1] - pos[0] per cycle, z and the orientation do not accumulate. loop=False holds the last frame past the end.

A specification of tracking terms is a list of Term(kind, mask, weight, scale, aux); every constructor below returns such a list,
so they add up. Hats mark the reference at the env's clock:

    pose(w, scale, joints)           exp(-scale * sum (q_j - q^_j)^2)       hinge angles, not DeepMimic's quaternion differences
    velocity(w, scale, joints)       exp(-scale * sum (qd_j - qd^_j)^2)
    end_effector(w, scale)           exp(-scale * sum_k |r_k - r^_k|^2), the end effectors relative to the base link, in its axes
    root_pose(w, scale, angle)       exp(-scale * (|p - p^|^2 + angle * theta^2)), theta the angle between base and reference
    root_velocity(w, scale, angular) exp(-scale * (|v - v^|^2 + angular * |w - w^|^2))

    imitation(model)                 the preset: DeepMimic's weights 0.65 / 0.1 / 0.15 / 0.1 on pose / velocity / end effector /
                                     root pose and its scales 2 / 0.1 / 40 / 10, CARRIED OVER UNCHANGED AND NOT TUNED for this model

`joints` are joint names or indices in observation order (None = all joints). as_tuples() / from_tuples() turn a specification
into plain data and back - what a checkpoint stores."""
import collections
import math

import numpy as np

KINDS = {"pose": 0, "velocity": 1, "end_effector": 2, "root_pose": 3, "root_velocity": 4}     # TREX_MOT_*
MAX_TERMS, MAX_FRAMES, MAX_END_EFFECTORS = 8, 4096, 8      # csrc/motion_limits.h
NLERP_DOT = 0.9995                                         # above it the slerp is a normalised lerp
Term = collections.namedtuple("Term", "kind mask weight scale aux")


def _term(kind, weight, scale, aux=0.0, mask=None):
    vals = (float(weight), float(scale), float(aux))
    if not all(math.isfinite(x) for x in vals):
        raise ValueError("%s: weight and parameters must be finite" % kind)
    if not vals[1] > 0.0 or vals[2] < 0.0:
        raise ValueError("%s: scale must be positive and the second parameter not negative" % kind)
    if mask is not None:
        mask = tuple(m if isinstance(m, str) else int(m) for m in mask)
    return [Term(kind, mask, *vals)]


def pose(weight=1.0, scale=2.0, joints=None):
    return _term("pose", weight, scale, mask=joints)


def velocity(weight=1.0, scale=0.1, joints=None):
    return _term("velocity", weight, scale, mask=joints)


def end_effector(weight=1.0, scale=40.0):
    return _term("end_effector", weight, scale)


def root_pose(weight=1.0, scale=10.0, angle=1.0):
    return _term("root_pose", weight, scale, angle)


def root_velocity(weight=1.0, scale=1.0, angular=1.0):
    return _term("root_velocity", weight, scale, angular)


def imitation(model=None, end_effectors=True):
    """DeepMimic's tracking reward: 0.65 pose + 0.1 velocity + 0.15 end effector + 0.1 root pose (its centre-of-mass term, taken
    at the base) with its scales 2 / 0.1 / 40 / 10. The numbers are the paper's, for a humanoid of 34 degrees of freedom with
    quaternion pose differences; here the pose term sums hinge angles. They are NOT tuned for `model` (which is not read).
    end_effectors=False leaves that term out, for a clip without end effectors."""
    spec = pose(0.65, 2.0) + velocity(0.1, 0.1)
    if end_effectors:
        spec += end_effector(0.15, 40.0)
    return spec + root_pose(0.1, 10.0, 1.0)


PRESETS = {"imitation": imitation}


def flatten(spec):
    """a specification given as terms, lists of terms or a mix -> [Term]"""
    out = []
    for c in spec:
        if isinstance(c, Term):
            out.append(c)
        else:
            out += flatten(c)
    return out


def _kind(c):
    if isinstance(c.kind, str):
        if c.kind not in KINDS:
            raise ValueError("unknown motion term kind %r (%s)" % (c.kind, ", ".join(KINDS)))
        return KINDS[c.kind]
    if not 0 <= int(c.kind) < len(KINDS):
        raise ValueError("unknown motion term kind %r (0 .. %d)" % (c.kind, len(KINDS) - 1))
    return int(c.kind)


def names(spec):
    """One name per term, for logs: "motion/" + the kind; a repeated name gets #2, #3, ..."""
    by_value = {v: k for k, v in KINDS.items()}
    out, seen = [], {}
    for c in flatten(spec):
        name = "motion/" + by_value[_kind(c)]
        seen[name] = seen.get(name, 0) + 1
        out.append(name if seen[name] == 1 else "%s#%d" % (name, seen[name]))
    return out


def resolve(spec, joint_index):
    """[Term] -> ([(kind value, mask bits, weight, scale, aux)] for BatchMotion.set_reward, needs end effectors?). joint_index:
    name or index -> joint index in observation order."""
    out, effectors = [], False
    for c in flatten(spec):
        k = _kind(c)
        bits = 0
        for j in c.mask or ():
            bits |= 1 << joint_index(j)
        out.append((k, bits, float(c.weight), float(c.scale), float(c.aux)))
        effectors |= k == 2
    if len(out) > MAX_TERMS:
        raise ValueError("motion: %d terms, at most %d" % (len(out), MAX_TERMS))
    return out, effectors


def as_tuples(spec):
    """plain lists / strings / numbers: what torch.save(..., weights_only) round-trips"""
    return [[c.kind, None if c.mask is None else list(c.mask), float(c.weight), float(c.scale), float(c.aux)] for c in flatten(spec)]


def from_tuples(data):
    return [Term(k, None if m is None else tuple(m), float(w), float(s), float(a)) for k, m, w, s, a in data]


def _slerp(a, b, u):
    """shortest-arc slerp of two unit quaternions, normalised lerp where their dot product exceeds NLERP_DOT"""
    d = float(np.dot(a, b))
    if d < 0.0:
        b, d = -b, -d
    if d > NLERP_DOT:
        q = (1.0 - u) * a + u * b
        return q / np.linalg.norm(q)
    th = math.acos(d)
    return (math.sin((1.0 - u) * th) * a + math.sin(u * th) * b) / math.sin(th)


class Clip:
    """frames [F, 7 + J] f64 (base position, base quaternion xyzw, q in observation order), frame_dt seconds between frames,
    velocities [F, 6 + J] or None (derived on the way to the device)."""

    def __init__(self, frames, frame_dt, loop=False, velocities=None):
        self.frames = np.array(frames, dtype=np.float64)
        if self.frames.ndim != 2 or self.frames.shape[1] < 8 or not 2 <= self.frames.shape[0] <= MAX_FRAMES:
            raise ValueError("Clip: frames must be [F, 7 + J] with 2 <= F <= %d, got %s" % (MAX_FRAMES, self.frames.shape))
        self.frame_dt, self.loop = float(frame_dt), bool(loop)
        if not self.frame_dt > 0.0 or not math.isfinite(self.frame_dt):
            raise ValueError("Clip: frame_dt must be positive, got %r" % (frame_dt,))
        self.velocities = None if velocities is None else np.array(velocities, dtype=np.float64)
        if self.velocities is not None and self.velocities.shape != (self.frames.shape[0], self.frames.shape[1] - 1):
            raise ValueError("Clip: velocities must be [F, 6 + J] = %s, got %s"
                             % ((self.frames.shape[0], self.frames.shape[1] - 1), self.velocities.shape))

    @property
    def num_frames(self):
        return self.frames.shape[0]

    @property
    def num_joints(self):
        return self.frames.shape[1] - 7

    @property
    def duration(self):
        return (self.num_frames - 1) * self.frame_dt

    def save(self, path):
        """an .npz of plain arrays (no pickle)"""
        vel = np.zeros((0, 0)) if self.velocities is None else self.velocities
        with open(path, "wb") as f:      # (np.savez would append ".npz" to a path without it)
            np.savez(f, frames=self.frames, frame_dt=np.float64(self.frame_dt), loop=np.int64(self.loop), velocities=vel)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            vel = z["velocities"]
            return cls(z["frames"], float(z["frame_dt"]), bool(int(z["loop"])), vel if vel.size else None)

    @classmethod
    def from_states(cls, states, frame_dt, loop=False, limits=None):
        """a sequence of get_state() rows [F, 13 + 2J] (one env's, a recorded rollout) as a clip, velocities included.
        limits: (lower [J], upper [J]) in observation order - the angles are clamped into them: a simulated joint can stand a
        little beyond its stop, and a clip beyond a limit by more than 1e-6 is refused."""
        s = np.asarray(states.detach().cpu().numpy() if hasattr(states, "detach") else states, dtype=np.float64)
        if s.ndim != 2 or (s.shape[1] - 13) % 2 or s.shape[1] < 15:
            raise ValueError("from_states: expected [F, 13 + 2J] state rows, got %s" % (s.shape,))
        J = (s.shape[1] - 13) // 2
        q = s[:, 13:13 + J] if limits is None else np.clip(s[:, 13:13 + J], limits[0], limits[1])
        return cls(np.concatenate([s[:, :7], q], 1), frame_dt, loop, np.concatenate([s[:, 7:13], s[:, 13 + J:]], 1))

    @classmethod
    def from_keyframes(cls, times, poses, frame_dt, loop=False):
        """keyframes poses [M, 7 + J] at increasing `times` [M] (seconds, the first is the clip's time 0), resampled every
        frame_dt with the interpolation of the device: linear in position and q, slerp (nlerp for close ends) in the
        quaternion. The last frame is the last multiple of frame_dt not beyond the last keyframe."""
        times, poses = np.asarray(times, np.float64).reshape(-1), np.asarray(poses, np.float64)
        if poses.ndim != 2 or len(times) != len(poses) or len(times) < 2 or not (np.diff(times) > 0).all():
            raise ValueError("from_keyframes: times [M] increasing and poses [M, 7 + J], M >= 2")
        quat = poses[:, 3:7] / np.linalg.norm(poses[:, 3:7], axis=1, keepdims=True)
        F = int(math.floor((times[-1] - times[0]) / frame_dt + 1e-9)) + 1      # (a span that is a whole number of frames but for rounding)
        out = np.zeros((F, poses.shape[1]))
        for f in range(F):
            t = min(times[0] + f * frame_dt, times[-1])
            k = min(int(np.searchsorted(times, t, side="right")) - 1, len(times) - 2)
            u = (t - times[k]) / (times[k + 1] - times[k])
            out[f] = (1.0 - u) * poses[k] + u * poses[k + 1]
            out[f, 3:7] = _slerp(quat[k], quat[k + 1], u)
        return cls(out, frame_dt, loop)


def attach(env, clip, terms=None, end_effectors=(), rsi=False, step_weight=1.0, probe_set=7, seed=0):
    """Give the TrexVecEnv `env` the clip and its tracking terms (the arguments: TrexVecEnv._set_motion). The env's constructor
    takes no `motion` keyword - its signature is a recorded one -, so this function is the way in; it is called once, before the
    first step. -> env."""
    env._set_motion(clip, terms=terms, end_effectors=end_effectors, rsi=rsi, step_weight=step_weight, probe_set=probe_set, seed=seed)
    return env


def phase_columns(env):
    """[n, 2] = sin, cos of 2 pi phase of every env's clock: what observations.external(2) takes through
    external=motion.phase_columns. One sample launch and three small torch ops."""
    import torch
    ph = getattr(env, "_motion_phase", None)
    if ph is None:
        ph = env._motion_phase = torch.zeros(env.num_envs, device=env.device)
    env.motion_api.sample(phase=ph)
    a = ph * (2.0 * math.pi)
    return torch.stack([torch.sin(a), torch.cos(a)], 1)
