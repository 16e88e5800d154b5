"""The sensor model of a TrexVecEnv, attached by attach(env, spec, ...) (include/trex_sensing.h): what the policy reads is the row
the env composed, seen through sensors - on the device, one launch per step -, and what the motors get is the policy's action some
env-steps late.

A specification is a list of Group(col0, width, noise_kind, noise, bias, quantum, delay_min, delay_max) over observation columns;
every constructor below returns such a list, so they add up, and merge() folds those over the same columns into one group:

    columns(env, what)              [(col0, width)]: "q", "qd", "torque", or a channel of the env's observations by index or kind
    noise(cols, std= | uniform=)    white noise per step: Gaussian of that standard deviation, or uniform of that half-width
    bias(cols, half_width)          an offset per env and column, uniform in [-half_width, half_width], held through an episode
    quantize(cols, quantum)         the resolution: values rounded to a multiple of quantum
    latency(cols, steps | (lo, hi)) whole env-steps, drawn per env and episode; a sensor holds its first reading until then

    typical(env)                    untuned magnitudes for q, qd and the channels of observations.locomotion

Deviations from a real sensor, stated once: delays are whole env-steps, a bias is uniform and constant within an episode, a delayed
action holds the episode's first action. as_tuples() / from_tuples() turn a specification into plain data and back - what a
checkpoint stores."""
import collections
import math

from .sensing_capi import GAUSSIAN, MAX_DELAY, MAX_GROUPS, UNIFORM

Group = collections.namedtuple("Group", "col0 width noise_kind noise bias quantum delay_min delay_max")


def columns(env, what):
    """[(col0, width)] of the env's final row: "q", "qd", "torque" (J columns each); an int: the env's observation channel of that
    index; any other string: every channel of that kind (observations.KINDS), one range each."""
    J = env.J
    fixed = {"q": (0, J), "qd": (J, J), "torque": (2 * J, J)}
    if isinstance(what, str) and what in fixed:
        return [fixed[what]]
    from . import observations as O
    chans = O.from_tuples(env.observations or [])
    out, col = [], 3 * J
    for k, c in enumerate(chans):
        w = O.width(c, env.A)
        if (isinstance(what, str) and c.kind == what) or (not isinstance(what, str) and k == int(what)):
            out.append((col, w))
        col += w
    if not out:
        raise ValueError("columns: the env has no observation channel %r" % (what,))
    return out


def _ranges(cols):
    """(col0, width), a range, or a list of either -> [(col0, width)]"""
    if isinstance(cols, range):
        if cols.step != 1 or len(cols) < 1:
            raise ValueError("a range of columns must be contiguous and not empty")
        return [(cols.start, len(cols))]
    if isinstance(cols, tuple) and len(cols) == 2 and all(isinstance(x, int) for x in cols):
        return [cols]
    out = []
    for c in cols:
        out += _ranges(c)
    return out


def _groups(cols, **kw):
    base = dict(noise_kind=GAUSSIAN, noise=0.0, bias=0.0, quantum=0.0, delay_min=0, delay_max=0)
    base.update(kw)
    return [Group(int(c), int(w), **base) for c, w in _ranges(cols)]


def _magnitude(x, what):
    x = float(x)
    if not (x >= 0.0 and math.isfinite(x)):
        raise ValueError("%s must be finite and not negative" % what)
    return x


def noise(columns, std=None, uniform=None):
    if (std is None) == (uniform is None):
        raise ValueError("noise: one of std= (Gaussian) and uniform= (half-width)")
    if std is not None:
        return _groups(columns, noise_kind=GAUSSIAN, noise=_magnitude(std, "std"))
    return _groups(columns, noise_kind=UNIFORM, noise=_magnitude(uniform, "uniform"))


def bias(columns, half_width):
    return _groups(columns, bias=_magnitude(half_width, "half_width"))


def quantize(columns, quantum):
    return _groups(columns, quantum=_magnitude(quantum, "quantum"))


def delay_range(steps):
    """steps or (min, max) -> (min, max), checked"""
    lo, hi = (steps, steps) if isinstance(steps, int) else steps
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= MAX_DELAY:
        raise ValueError("a delay must lie in 0 <= min <= max <= %d env-steps, got (%d, %d)" % (MAX_DELAY, lo, hi))
    return lo, hi


def latency(columns, steps):
    lo, hi = delay_range(steps)
    return _groups(columns, delay_min=lo, delay_max=hi)


def flatten(spec):
    """a specification given as groups, lists of groups or a mix -> [Group]"""
    out = []
    for g in spec:
        if isinstance(g, Group):
            out.append(g)
        else:
            out += flatten(g)
    return out


def merge(*specs):
    """Fold the groups of the specifications that cover the same columns into one group each - noise(c, ...) + bias(c, ...) +
    latency(c, ...) is one sensor -, sorted by column. ValueError: two of them set the same property of a range, or two ranges
    overlap without being equal."""
    out = {}
    for g in flatten(specs):
        key = (g.col0, g.width)
        if key not in out:
            out[key] = g
            continue
        h = out[key]
        for name, on in (("noise", g.noise > 0), ("bias", g.bias > 0), ("quantum", g.quantum > 0), ("delay", g.delay_max > 0)):
            if on and ((getattr(h, name) > 0) if name != "delay" else h.delay_max > 0):
                raise ValueError("merge: columns [%d, %d) get their %s twice" % (g.col0, g.col0 + g.width, name))
        out[key] = Group(g.col0, g.width, g.noise_kind if g.noise > 0 else h.noise_kind, max(g.noise, h.noise), max(g.bias, h.bias),
                         max(g.quantum, h.quantum), max(g.delay_min, h.delay_min), max(g.delay_max, h.delay_max))
    groups = [out[k] for k in sorted(out)]
    for a, b in zip(groups, groups[1:]):
        if a.col0 + a.width > b.col0:
            raise ValueError("merge: columns [%d, %d) and [%d, %d) overlap" % (a.col0, a.col0 + a.width, b.col0, b.col0 + b.width))
    if len(groups) > MAX_GROUPS:
        raise ValueError("merge: %d groups, at most %d" % (len(groups), MAX_GROUPS))
    return groups


def scaled(spec, factor):
    """every magnitude - noise, bias - of the specification times `factor`; resolutions and delays as they are"""
    return [g._replace(noise=g.noise * float(factor), bias=g.bias * float(factor)) for g in flatten(spec)]


def typical(env, scale=1.0, delay=0):
    """Untuned magnitudes of the kind locomotion trainers randomise their observations with (legged_gym's noise scales are of this
    order: joint angle 0.01 rad, joint velocity 1.5 rad/s, linear velocity 0.1 m/s, angular velocity 0.2 rad/s, gravity 0.05,
    height 0.1 m), over q, qd and those channels of observations.locomotion the env has:
        q                      Gaussian 0.005 rad, bias 0.01 rad, a 12-bit encoder: 2 pi / 4096
        qd                     Gaussian 0.3 rad/s (a differentiated encoder)
        projected gravity      Gaussian 0.02, bias 0.02 (the attitude estimate drifts)
        base linear velocity   Gaussian 0.1 m/s (a state estimator's output)
        base angular velocity  Gaussian 0.05 rad/s, bias 0.02 rad/s (a gyro)
        base and point height  Gaussian 0.02 m
    scale multiplies noise and bias; delay - steps or (min, max) - is the latency of all of these columns. The torque columns,
    contact forces, point positions and external columns stay clean."""
    q, qd = columns(env, "q"), columns(env, "qd")
    spec = [noise(q, std=0.005), bias(q, 0.01), quantize(q, 2.0 * math.pi / 4096.0), noise(qd, std=0.3)]
    per_kind = (("projected_gravity", 0.02, 0.02), ("base_linear_velocity", 0.1, 0.0), ("base_angular_velocity", 0.05, 0.02),
                ("base_height", 0.02, 0.0), ("point_height", 0.02, 0.0))
    have = {c[0] for c in (env.observations or [])}
    for kind, std, off in per_kind:
        if kind in have:
            c = columns(env, kind)
            spec += [noise(c, std=std)] + ([bias(c, off)] if off else [])
    spec = scaled(spec, scale)
    if delay_range(delay)[1] > 0:
        spec += latency(sorted({(g.col0, g.width) for g in spec}), delay)
    return merge(spec)


PRESETS = {"typical": typical}


def as_tuples(spec):
    """plain lists of numbers: what torch.save(..., weights_only) round-trips"""
    return [[int(g.col0), int(g.width), int(g.noise_kind), float(g.noise), float(g.bias), float(g.quantum), int(g.delay_min),
             int(g.delay_max)] for g in flatten(spec)]


def from_tuples(data):
    return [Group(int(a), int(b), int(c), float(d), float(e), float(f), int(g), int(h)) for a, b, c, d, e, f, g, h in data]


def attach(env, spec, action_delay=0, seed=0):
    """Give the env a sensor model (TrexVecEnv._set_sensing): `spec` - groups, constructors' lists or a mix; merged - is applied
    to every row the env composes, by one launch per step and reset behind the last compose; action_delay - steps or (min, max) -
    delays the actions before the step call, by one more launch. The env then has `sense_api` (sensing_capi.BatchSensing),
    `clean_rows` and `clean_obs`, the block before the launch, while `rows` and `obs` hold what the policy reads, and `sensing`,
    the recorded specification. The Philox key is `seed`, the env offset the env's first global env index, so that a sharded run
    draws what the whole run draws. An empty spec sets only the action delay; spec None takes it all off again."""
    env._set_sensing(spec, action_delay=action_delay, seed=seed)
    return env
