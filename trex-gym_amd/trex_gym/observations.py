"""Observation channels for TrexVecEnv(observations=[...]) (trex_batch_set_observation / trex_batch_compose_rows,
include/trex_batch.h): extra columns behind the reference's [q | qd | torque], computed on the device from the state the 3J
columns were taken at, in the one launch that writes the row the trainer reads.

A specification is a list of Channel(kind, link, xyz, scale); every constructor below returns such a list, so they add up:

    gravity()          3  world (0, 0, -1) in the base link's axes: the tilt
    base_velocity()    6  linear (of the base link's origin) and angular velocity, base axes
    base_height()      1  base link's origin above the floor
    point(link, xyz)   3 / 3 / 1 per part asked for: position relative to the base link (base axes), velocity (base axes), height
    contact_force(l)   1  vertical floor-contact force on the body of link l (the env switches the contact sensor on)
    prev_action()      A  the action of the step that produced the row; zeros at the start of an episode
    external(k)        k  columns the caller supplies (TrexVecEnv(external=...)): ray distances, proximity, commands

    locomotion(model)  18 = gravity + base velocity + height + contact force and position of the two feet: D' = 93

`link` is a URDF link name or index; `scale` multiplies every value of the channel. as_tuples() / from_tuples() turn a
specification into plain data and back - what a checkpoint stores.
"""
import collections

KINDS = {"projected_gravity": 0, "base_linear_velocity": 1, "base_angular_velocity": 2, "base_height": 3, "point_position": 4,
         "point_velocity": 5, "point_height": 6, "contact_force": 7, "prev_action": 8, "external": 9}     # TREX_OBS_*
MAX_CHANNELS, MAX_DIM = 64, 512            # csrc/observation_limits.h
Channel = collections.namedtuple("Channel", "kind link xyz scale")
_ZERO = (0.0, 0.0, 0.0)


def gravity(scale=1.0):
    return [Channel("projected_gravity", 0, _ZERO, float(scale))]


def base_velocity(linear=True, angular=True, scale=1.0):
    return ([Channel("base_linear_velocity", 0, _ZERO, float(scale))] if linear else []) + \
           ([Channel("base_angular_velocity", 0, _ZERO, float(scale))] if angular else [])


def base_height(scale=1.0):
    return [Channel("base_height", 0, _ZERO, float(scale))]


def point(link, xyz=_ZERO, position=True, velocity=False, height=False, scale=1.0):
    xyz = tuple(float(x) for x in xyz)
    if len(xyz) != 3:
        raise ValueError("point: xyz must have 3 entries")
    parts = (("point_position", position), ("point_velocity", velocity), ("point_height", height))
    return [Channel(kind, link, xyz, float(scale)) for kind, on in parts if on]


def contact_force(link, scale=1.0):
    return [Channel("contact_force", link, _ZERO, float(scale))]


def prev_action(scale=1.0):
    return [Channel("prev_action", 0, _ZERO, float(scale))]


def external(k, scale=1.0):
    if int(k) < 1:
        raise ValueError("external: k must be at least 1")
    return [Channel("external", int(k), _ZERO, float(scale))]


def locomotion(model, device=None):
    """What a walking policy needs of the base and the feet, 18 columns. The feet are those of trex_gym.termination.foot_links:
    found with one clearance query on a reset batch of one env of `model` on `device` (None: the current HIP device)."""
    import types

    import torch

    from .termination import foot_links
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    feet = foot_links(types.SimpleNamespace(model=model, device=dev))
    if len(feet) != 2:
        raise ValueError("locomotion: the model stands on %d feet, the preset is written for 2" % len(feet))
    spec = gravity() + base_velocity() + base_height()
    for l in feet:
        spec += contact_force(l) + point(l)
    return spec


PRESETS = {"locomotion": locomotion}


def flatten(spec):
    """a specification given as channels, lists of channels or a mix -> [Channel]"""
    out = []
    for c in spec:
        if isinstance(c, Channel):
            out.append(c)
        else:
            out += flatten(c)
    return out


def width(channel, action_cols):
    k = KINDS[channel.kind] if isinstance(channel.kind, str) else int(channel.kind)
    return 1 if k in (3, 6, 7) else action_cols if k == 8 else int(channel.link) if k == 9 else 3


def resolve(spec, link_index, action_cols):
    """[Channel] -> ([(kind value, link index or k, xyz, scale)] for Batch.set_observation, E, needs the contact sensor?, columns of
    the EXTERNAL channels). link_index: name or index -> URDF link index."""
    out, extra, contact, ext = [], 0, False, 0
    for c in flatten(spec):
        if isinstance(c.kind, str) and c.kind not in KINDS:
            raise ValueError("unknown observation channel kind %r (%s)" % (c.kind, ", ".join(KINDS)))
        k = KINDS[c.kind] if isinstance(c.kind, str) else int(c.kind)
        link = link_index(c.link) if k in (4, 5, 6, 7) else int(c.link)
        out.append((k, link, tuple(float(x) for x in c.xyz), float(c.scale)))
        extra += width(c, action_cols)
        contact |= k == 7
        ext += int(c.link) if k == 9 else 0
    return out, extra, contact, ext


def as_tuples(spec):
    """plain lists / strings / numbers: what torch.save(..., weights_only) round-trips"""
    return [[c.kind, c.link if isinstance(c.link, str) else int(c.link), [float(x) for x in c.xyz], float(c.scale)] for c in flatten(spec)]


def from_tuples(data):
    return [Channel(k, l, tuple(x), float(s)) for k, l, x, s in data]
