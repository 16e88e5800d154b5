"""The start-state randomisation of a TrexVecEnv, attached by attach(env, spec, seed) (include/trex_start_state.h): the state an
episode starts IN - joint angles, joint velocities, base attitude, base velocity, base position - perturbed on the device by one
launch per step and reset, for the envs whose episode has just started, and the robot then placed on the floor. The counterpart of
trex_gym.randomize, which redraws everything but the state. The launch perturbs the state it finds: the model's start pose behind
a plain reset, the instant of the clip behind RSI (trex_gym.motion), so that noise on an RSI state stays a perturbation of it.

A specification is a list of Term(kind, mask, index, shared, lo, hi); every constructor below returns such a list, so they add up:

    joint_position(lo, hi, joints=None, shared=False)    added to the joint angles (None: all), clamped to the joint limits
    joint_velocity(lo, hi, joints=None, shared=False)    added to the joint velocities
    base_rpy(axis, lo, hi)                               axis 0 roll, 1 pitch, 2 yaw (rad): a rotation of the whole found state
    base_linear_velocity(axis, lo, hi)                   world axes, added after the rotation
    base_angular_velocity(axis, lo, hi)
    base_position(axis, lo, hi)
    floor_clearance(lo, hi)                              last of all: the lowest collision point at lo..hi above the floor

    typical(env)                                         untuned magnitudes of the kind locomotion trainers start episodes with

Deviations, stated once: no settle substep runs behind the perturbation; joint angles are clamped to the limits, not redrawn; the
rotation is about the base inertial origin; without a floor_clearance term, penetration of the floor is the caller's to avoid.
as_tuples() / from_tuples() turn a specification into plain data and back - what a checkpoint stores."""
import collections
import math

from .start_state_capi import (BASE_ANGULAR_VELOCITY, BASE_LINEAR_VELOCITY, BASE_POSITION, BASE_RPY, FLOOR_CLEARANCE, JOINT_POSITION,
                               JOINT_VELOCITY, KIND_NAMES, MAX_TERMS)

Term = collections.namedtuple("Term", "kind mask index shared lo hi")


def _bounds(lo, hi, what):
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("%s: lo and hi must be finite with lo <= hi, got (%r, %r)" % (what, lo, hi))
    return lo, hi


def _mask(elements, what):
    """None (all) or indices in [0, 32) -> the bit mask (0: all)"""
    if elements is None:
        return 0
    bits = 0
    for i in elements:
        if not 0 <= int(i) < 32:
            raise ValueError("%s: element %r outside [0, 32)" % (what, i))
        bits |= 1 << int(i)
    if bits == 0:
        raise ValueError("%s: an empty selection (None selects all)" % what)
    return bits


def _joints(kind, lo, hi, joints, shared):
    """joints: None, or indices in observation order / joint names (resolved when the spec is attached)"""
    lo, hi = _bounds(lo, hi, KIND_NAMES[kind])
    if joints is not None and any(isinstance(j, str) for j in joints):
        return [Term(kind, tuple(joints), 0, int(bool(shared)), lo, hi)]
    return [Term(kind, _mask(joints, KIND_NAMES[kind]), 0, int(bool(shared)), lo, hi)]


def joint_position(lo, hi, joints=None, shared=False):
    return _joints(JOINT_POSITION, lo, hi, joints, shared)


def joint_velocity(lo, hi, joints=None, shared=False):
    return _joints(JOINT_VELOCITY, lo, hi, joints, shared)


def _axis(kind, axis, lo, hi):
    lo, hi = _bounds(lo, hi, KIND_NAMES[kind])
    if not 0 <= int(axis) <= 2:
        raise ValueError("%s: axis 0, 1 or 2, got %r" % (KIND_NAMES[kind], axis))
    return [Term(kind, 0, int(axis), 0, lo, hi)]


def base_rpy(axis, lo, hi):
    return _axis(BASE_RPY, axis, lo, hi)


def base_linear_velocity(axis, lo, hi):
    return _axis(BASE_LINEAR_VELOCITY, axis, lo, hi)


def base_angular_velocity(axis, lo, hi):
    return _axis(BASE_ANGULAR_VELOCITY, axis, lo, hi)


def base_position(axis, lo, hi):
    return _axis(BASE_POSITION, axis, lo, hi)


def floor_clearance(lo, hi):
    lo, hi = _bounds(lo, hi, "floor_clearance")
    return [Term(FLOOR_CLEARANCE, 0, 0, 0, lo, hi)]


def flatten(spec):
    """a specification given as terms, lists of terms or a mix -> [Term]"""
    out = []
    for t in spec:
        if isinstance(t, Term):
            out.append(t)
        else:
            out += flatten(t)
    return out


def merge(*specs):
    """The terms of the specifications as one list, in the order given - the order the batch numbers them in, which the random
    numbers of a term depend on. ValueError: more than 16 terms or two floor_clearance terms. (Overlaps are the batch's to refuse:
    a mask of 0 covers what only the model knows.)"""
    terms = flatten(specs)
    if len(terms) > MAX_TERMS:
        raise ValueError("merge: %d terms, at most %d" % (len(terms), MAX_TERMS))
    if sum(1 for t in terms if t.kind == FLOOR_CLEARANCE) > 1:
        raise ValueError("merge: at most one floor_clearance term")
    return terms


def scaled(spec, factor):
    """every range of the specification `factor` times as wide about its centre; a floor_clearance term as it is"""
    f, out = float(factor), []
    if f == 1.0:
        return flatten(spec)
    for t in flatten(spec):
        if t.kind == FLOOR_CLEARANCE:
            out.append(t)
        else:
            mid, half = 0.5 * (t.lo + t.hi), 0.5 * (t.hi - t.lo) * f
            out.append(t._replace(lo=mid - half, hi=mid + half))
    return out


def typical(env=None, scale=1.0, clearance=None):
    """Untuned magnitudes of the kind locomotion trainers start episodes with (legged_gym: joint angles scaled 0.5..1.5 about the
    default, base velocities +-0.5 m/s; Isaac Lab: +-0.1 rad, yaw anywhere), not fitted to this robot and not shown to help:
        joint angles           +-0.1 rad, one draw per joint, clamped to the limits
        joint velocities       +-0.5 rad/s
        roll, pitch            +-0.05 rad
        yaw                    +-pi
        base linear velocity   +-0.3 m/s in x and y, +-0.1 m/s in z
        base angular velocity  +-0.3 rad/s about every axis
        floor clearance        clearance = (lo, hi) metres (None: no placement - the perturbed pose may touch or leave the floor)
    scale widens or narrows every range about its centre. env is not looked at: the terms cover all joints of any model."""
    spec = [joint_position(-0.1, 0.1), joint_velocity(-0.5, 0.5), base_rpy(0, -0.05, 0.05), base_rpy(1, -0.05, 0.05),
            base_rpy(2, -math.pi, math.pi), base_linear_velocity(0, -0.3, 0.3), base_linear_velocity(1, -0.3, 0.3),
            base_linear_velocity(2, -0.1, 0.1), base_angular_velocity(0, -0.3, 0.3), base_angular_velocity(1, -0.3, 0.3),
            base_angular_velocity(2, -0.3, 0.3)]
    spec = scaled(spec, scale)
    if clearance is not None:
        spec += floor_clearance(*clearance)
    return merge(spec)


PRESETS = {"typical": typical}


def resolve(spec, joint_index):
    """the merged terms with joint names turned into mask bits: joint_index(name) -> the joint's place in observation order"""
    out = []
    for t in merge(spec):
        if isinstance(t.mask, tuple):
            t = t._replace(mask=_mask([joint_index(j) if isinstance(j, str) else int(j) for j in t.mask], KIND_NAMES[t.kind]))
        out.append(t)
    return out


def as_tuples(spec):
    """plain lists of numbers: what torch.save(..., weights_only) round-trips (joint names resolved: after attach)"""
    return [[int(t.kind), int(t.mask), int(t.index), int(t.shared), float(t.lo), float(t.hi)] for t in flatten(spec)]


def from_tuples(data):
    return [Term(int(a), int(b), int(c), int(d), float(e), float(f)) for a, b, c, d, e, f in data]


def attach(env, spec, seed=0):
    """Give the env start-state randomisation (TrexVecEnv._set_start_state): `spec` - terms, constructors' lists or a mix - is
    applied by one launch per step and reset behind the step call, to the envs whose episode just started - at the episode limit,
    by a fall or by reset_tensor alike -, behind RSI and before the randomisation, the channels and the sensor model, which all see
    the final state. The env then has `start_api` (start_state_capi.BatchStartState), `start_values` [n, T, 32], a tensor that
    start_api.info(values=env.start_values) fills, and `start_state`, the recorded specification. The Philox key is `seed`, the env
    offset the env's first global env index, so that a sharded run draws what the whole run draws. spec None takes it all off
    again."""
    env._set_start_state(spec, seed=seed)
    return env
