"""The episode randomisation of a TrexVecEnv, attached by attach(env, spec, seed) (include/trex_randomize.h): what a locomotion
training loop redraws when an episode starts - mass scale, friction, motor gains - or at an interval inside it - pushes, the
velocity command -, drawn on the device by one launch per step, so that a captured rollout replays.

A specification is a list of Term(kind, mask, index, shared, lo, hi, interval, duration, probability); every constructor below
returns such a list, so they add up:

    mass(lo, hi, bodies=None, shared=False)      the mass scale of the bodies (None: all): one draw each, or one for all
    friction(lo, hi)                             the friction coefficient itself
    kp / kd / max_force(lo, hi, joints=None, shared=False)   a factor on the gains the batch had when the spec was attached
    push(body_or_link, lo, hi, interval, duration, probability)   a horizontal force of lo..hi newtons at the body's COM
    command(component, lo, hi, interval=0, zero_probability=0)    component 0..2 (vx, vy, yaw rate) of env.commands

    typical(env)                                 untuned magnitudes of the kind locomotion trainers randomise with

Deviations, stated once: the settle substep of a reset inside the step launch still runs with the ending episode's mass and
friction; a push is held per env-step, not per substep; pushes are horizontal and act at the COM; each command component is drawn
independently. as_tuples() / from_tuples() turn a specification into plain data and back - what a checkpoint stores."""
import collections
import math

from .randomize_capi import COMMAND, FRICTION, KD, KIND_NAMES, KP, MASS, MAX_FORCE, MAX_PUSHES, MAX_TERMS, PUSH

Term = collections.namedtuple("Term", "kind mask index shared lo hi interval duration probability")


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


def _scaled(kind, lo, hi, elements, shared):
    lo, hi = _bounds(lo, hi, KIND_NAMES[kind])
    return [Term(kind, _mask(elements, KIND_NAMES[kind]), 0, int(bool(shared)), lo, hi, 0, 0, 0.0)]


def mass(lo, hi, bodies=None, shared=False):
    return _scaled(MASS, lo, hi, bodies, shared)


def friction(lo, hi):
    lo, hi = _bounds(lo, hi, "friction")
    return [Term(FRICTION, 0, 0, 1, lo, hi, 0, 0, 0.0)]


def kp(lo, hi, joints=None, shared=False):
    return _scaled(KP, lo, hi, joints, shared)


def kd(lo, hi, joints=None, shared=False):
    return _scaled(KD, lo, hi, joints, shared)


def max_force(lo, hi, joints=None, shared=False):
    return _scaled(MAX_FORCE, lo, hi, joints, shared)


def _probability(p, what):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("%s: a probability lies in [0, 1], got %r" % (what, p))
    return p


def push(body_or_link, lo, hi, interval, duration, probability=1.0):
    """a body index, or the name of a URDF link (resolved to its body when the spec is attached)"""
    lo, hi = _bounds(lo, hi, "push")
    if int(interval) < 1 or int(duration) < 1:
        raise ValueError("push: interval and duration are at least 1 env-step")
    index = body_or_link if isinstance(body_or_link, str) else int(body_or_link)
    return [Term(PUSH, 0, index, 0, lo, hi, int(interval), int(duration), _probability(probability, "push"))]


def command(component, lo, hi, interval=0, zero_probability=0.0):
    lo, hi = _bounds(lo, hi, "command")
    if not 0 <= int(component) <= 2:
        raise ValueError("command: component 0 (vx), 1 (vy) or 2 (yaw rate), got %r" % (component,))
    if int(interval) < 0:
        raise ValueError("command: interval 0 (per episode only) or a number of env-steps")
    return [Term(COMMAND, 0, int(component), 0, lo, hi, int(interval), 0, _probability(zero_probability, "command"))]


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
    numbers of a term depend on. ValueError: more than 16 terms or more than 4 pushes. (Overlaps are the batch's to refuse: a mask
    of 0 covers what only the model knows.)"""
    terms = flatten(specs)
    if len(terms) > MAX_TERMS:
        raise ValueError("merge: %d terms, at most %d" % (len(terms), MAX_TERMS))
    if sum(1 for t in terms if t.kind == PUSH) > MAX_PUSHES:
        raise ValueError("merge: at most %d push terms" % MAX_PUSHES)
    return terms


def scaled(spec, factor):
    """every range of the specification `factor` times as wide about its centre (pushes: hi times factor); intervals, durations
    and probabilities as they are"""
    f, out = float(factor), []
    if f == 1.0:
        return flatten(spec)
    for t in flatten(spec):
        if t.kind == PUSH:
            out.append(t._replace(lo=t.lo * f, hi=t.hi * f))
        else:
            mid, half = 0.5 * (t.lo + t.hi), 0.5 * (t.hi - t.lo) * f
            out.append(t._replace(lo=mid - half, hi=mid + half))
    return out


def typical(env, scale=1.0, push_force=300.0, command_range=(1.0, 0.3, 0.5), command_interval=250):
    """Untuned magnitudes of the kind locomotion trainers randomise with (legged_gym: friction 0.5..1.25, added base mass, a push
    every 15 s, commands resampled every 10 s), not fitted to this robot:
        mass scale             0.9..1.1 per body
        friction               0.5..1.25
        kp, kd                 0.8..1.2 of the nominal, per joint
        max_force              0.9..1.1 of the nominal, one draw for all joints
        push                   0..push_force newtons on body 0 every 200 env-steps for 5 (push_force 0: no push term)
        command                vx, vy, yaw rate uniform in +-command_range, an exact 0 one time in ten, resampled every
                               command_interval env-steps (only where the env has reward terms, which are what tracks a command)
    scale widens or narrows every range about its centre."""
    spec = [mass(0.9, 1.1), friction(0.5, 1.25), kp(0.8, 1.2), kd(0.8, 1.2), max_force(0.9, 1.1, shared=True)]
    if push_force > 0:
        spec.append(push(0, 0.0, float(push_force), 200, 5, 1.0))
    if getattr(env, "rewards", None) is not None and command_range is not None:
        for c, half in enumerate(command_range):
            if half > 0:
                spec.append(command(c, -float(half), float(half), int(command_interval), 0.1))
    return merge(scaled(spec, scale))


PRESETS = {"typical": typical}


def as_tuples(spec):
    """plain lists of numbers: what torch.save(..., weights_only) round-trips (link names resolved: after attach)"""
    return [[int(t.kind), int(t.mask), int(t.index), int(t.shared), float(t.lo), float(t.hi), int(t.interval), int(t.duration),
             float(t.probability)] for t in flatten(spec)]


def from_tuples(data):
    return [Term(int(a), int(b), int(c), int(d), float(e), float(f), int(g), int(h), float(i)) for a, b, c, d, e, f, g, h, i in data]


def attach(env, spec, seed=0):
    """Give the env episode randomisation (TrexVecEnv._set_randomization): `spec` - terms, constructors' lists or a mix - is
    redrawn by one launch per step and reset behind the step call, for the envs whose episode just ended - at the episode limit,
    by a fall or by reset_tensor alike. The env then has `random_api` (randomize_capi.BatchRandomization), `random_values`
    [n, T, 32], a tensor that random_api.info(values=env.random_values) fills, and `randomization`, the recorded specification. Command terms
    write env.commands. The Philox key is `seed`, the env offset the env's first global env index, so that a sharded run draws what
    the whole run draws. The env must own neither `pushes` nor `gains` (trex_gym.perturb): one owner per buffer. spec None takes
    it all off again and puts gains, wrench, mass scale and friction back."""
    env._set_randomization(spec, seed=seed)
    return env
