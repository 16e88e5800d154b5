"""Reward terms for TrexVecEnv(rewards=[...]) (trex_batch_set_reward / trex_batch_compose_reward, include/trex_reward.h): the
reward column of the row the trainer reads, composed on the device from terms evaluated at the row's own instant, in one more
launch per step. The reference's reward is one of the terms (`step`), so a specification can keep it, weigh it or drop it.

A specification is a list of Term(kind, link, mask, xyz, weight, p0, p1); every constructor below returns such a list, so they add
up. reward = sum of weight * value; a penalty is a negative weight. Ts = dt * substeps, c = env.commands (vx, vy, yaw rate).

    step(w)                          the step's own reward: the reference's three terms, less any fall penalty
    alive(w)                         1
    track_lin_vel(w, sigma)          exp(-|v_xy - c_xy|^2 / sigma), base axes
    track_ang_vel(w, sigma)          exp(-(w_z - c_2)^2 / sigma)
    lin_vel_z(w)  ang_vel_xy(w)      v_z^2;  w_x^2 + w_y^2
    orientation(w)                   g_x^2 + g_y^2 of the projected gravity: 0 upright, 1 on its side
    base_height(w, target)           (height of the base link's origin - target)^2
    point_height(w, link, target, xyz)
    torque(w, joints)  joint_vel(w, joints)  joint_acc(w, joints)  power(w, joints)  joint_pose(w, joints)
    joint_limit(w, soft, joints)     how far past the inner `soft` fraction of its range a joint stands
    action_rate(w)                   |a - a_prev|^2 over the action row, as passed
    contact_count(w, links, threshold)     how many of the links' bodies press on the floor with more than `threshold` N
    foot_air_time(w, link, threshold, offset)   on touchdown, the time the foot was in the air - offset
    foot_slip(w, link, threshold, xyz)     the point's horizontal speed^2 while the foot's body is in contact

    locomotion(model)                the preset: velocity tracking, a quiet upright base, small torques and smooth actions, feet
                                     that swing without sliding, nothing but the feet on the floor

`link` / `links` are URDF link names or indices, `joints` joint names or indices in observation order (None = all joints).
as_tuples() / from_tuples() turn a specification into plain data and back - what a checkpoint stores.
"""
import collections
import math

KINDS = {"step": 0, "alive": 1, "track_lin_vel": 2, "track_ang_vel": 3, "lin_vel_z": 4, "ang_vel_xy": 5, "orientation": 6,
         "base_height": 7, "point_height": 8, "torque": 9, "joint_vel": 10, "joint_acc": 11, "action_rate": 12, "joint_limit": 13,
         "power": 14, "joint_pose": 15, "contact_count": 16, "foot_air_time": 17, "foot_slip": 18}     # TREX_REW_*
MAX_TERMS = 32                             # csrc/reward_limits.h
TRACKING, JOINT_SUMS, LINKED, CONTACT = (2, 3), (9, 10, 11, 13, 14, 15), (8, 17, 18), (16, 17, 18)
# mask: the joints of a joint sum / the links of contact_count, as a tuple of names or indices; None = all joints
Term = collections.namedtuple("Term", "kind link mask xyz weight p0 p1")
_ZERO = (0.0, 0.0, 0.0)


def _term(kind, weight, link=0, mask=None, xyz=_ZERO, p0=0.0, p1=0.0):
    xyz = tuple(float(x) for x in xyz)
    if len(xyz) != 3:
        raise ValueError("%s: xyz must have 3 entries" % kind)
    vals = xyz + (float(weight), float(p0), float(p1))
    if not all(math.isfinite(x) for x in vals):
        raise ValueError("%s: weight, parameters and xyz must be finite" % kind)
    if mask is not None:
        mask = tuple(m if isinstance(m, str) else int(m) for m in mask)
    return [Term(kind, link if isinstance(link, str) else int(link), mask, xyz, float(weight), float(p0), float(p1))]


def step(weight=1.0):
    return _term("step", weight)


def alive(weight=1.0):
    return _term("alive", weight)


def _sigma(kind, sigma):
    if not float(sigma) > 0.0:
        raise ValueError("%s: sigma must be positive, got %r" % (kind, sigma))
    return float(sigma)


def track_lin_vel(weight=1.0, sigma=0.25):
    return _term("track_lin_vel", weight, p0=_sigma("track_lin_vel", sigma))


def track_ang_vel(weight=1.0, sigma=0.25):
    return _term("track_ang_vel", weight, p0=_sigma("track_ang_vel", sigma))


def lin_vel_z(weight=-1.0):
    return _term("lin_vel_z", weight)


def ang_vel_xy(weight=-1.0):
    return _term("ang_vel_xy", weight)


def orientation(weight=-1.0):
    return _term("orientation", weight)


def base_height(weight=-1.0, target=0.0):
    return _term("base_height", weight, p0=target)


def point_height(weight, link, target=0.0, xyz=_ZERO):
    return _term("point_height", weight, link=link, xyz=xyz, p0=target)


def torque(weight=-1.0, joints=None):
    return _term("torque", weight, mask=joints)


def joint_vel(weight=-1.0, joints=None):
    return _term("joint_vel", weight, mask=joints)


def joint_acc(weight=-1.0, joints=None):
    return _term("joint_acc", weight, mask=joints)


def action_rate(weight=-1.0):
    return _term("action_rate", weight)


def joint_limit(weight=-1.0, soft=0.9, joints=None):
    if not 0.0 < float(soft) <= 1.0:
        raise ValueError("joint_limit: soft must lie in (0, 1], got %r" % (soft,))
    return _term("joint_limit", weight, mask=joints, p0=soft)


def power(weight=-1.0, joints=None):
    return _term("power", weight, mask=joints)


def joint_pose(weight=-1.0, joints=None):
    return _term("joint_pose", weight, mask=joints)


def contact_count(weight, links, threshold=1.0):
    return _term("contact_count", weight, mask=tuple(links), p0=threshold)


def foot_air_time(weight, link, threshold=1.0, offset=0.0):
    return _term("foot_air_time", weight, link=link, p0=threshold, p1=offset)


def foot_slip(weight, link, threshold=1.0, xyz=_ZERO):
    return _term("foot_slip", weight, link=link, xyz=xyz, p0=threshold)


def locomotion(model, device=None):
    """A walking task on the commands (vx, vy, yaw rate): the step's own reward kept in the breakdown at weight 0, velocity
    tracking, penalties on what the base should not do, on torques, joint accelerations and action changes, air time and slip per
    foot, and a penalty for every body that is no foot and presses on the floor (the tail among them). The torque weight is
    sized for this robot - 4.8 t, joint torques of 1e5 N m: a sum of squares of 1e11 under random actions. The feet are those of
    trex_gym.termination.foot_links / foot_bodies, found on a reset batch of one env of `model` on `device` (None: the current
    HIP device)."""
    import types

    import torch

    from .termination import foot_bodies, foot_links
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    env = types.SimpleNamespace(model=model, device=dev)
    feet, limbs = foot_links(env), set(foot_bodies(env))
    first_link = {}
    for l, b in enumerate(model.array("link_body").astype(int)):
        first_link.setdefault(int(b), l)
    others = [first_link[b] for b in range(model.num_bodies) if b not in limbs and b in first_link]     # (the base body included)
    spec = step(0.0) + track_lin_vel(1.0, 0.25) + track_ang_vel(0.5, 0.25)
    spec += lin_vel_z(-2.0) + ang_vel_xy(-0.05) + orientation(-1.0) + torque(-2e-12) + joint_acc(-2.5e-7) + action_rate(-0.01)
    for l in feet:
        spec += foot_air_time(1.0, l, threshold=1.0, offset=0.3) + foot_slip(-0.1, l, threshold=1.0)
    return spec + contact_count(-1.0, others, threshold=1.0)


PRESETS = {"locomotion": locomotion}


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
            raise ValueError("unknown reward term kind %r (%s)" % (c.kind, ", ".join(KINDS)))
        return KINDS[c.kind]
    if not 0 <= int(c.kind) < len(KINDS):
        raise ValueError("unknown reward term kind %r (0 .. %d)" % (c.kind, len(KINDS) - 1))
    return int(c.kind)


def names(spec):
    """One name per term, for logs: the kind, with the link where the term names one; a repeated name gets #2, #3, ..."""
    by_value = {v: k for k, v in KINDS.items()}
    out, seen = [], {}
    for c in flatten(spec):
        k = _kind(c)
        name = by_value[k] + ("[%s]" % (c.link,) if k in LINKED else "")
        seen[name] = seen.get(name, 0) + 1
        out.append(name if seen[name] == 1 else "%s#%d" % (name, seen[name]))
    return out


def resolve(spec, link_index, joint_index, link_body):
    """[Term] -> ([(kind value, link index, mask bits, xyz, weight, p0, p1)] for BatchRewards.set_reward, needs the contact sensor?, needs
    the commands?, needs the actions?). link_index / joint_index: name or index -> URDF link index / joint index in observation
    order; link_body: URDF link index -> body."""
    out, contact, command, actions = [], False, False, False
    for c in flatten(spec):
        k = _kind(c)
        vals = tuple(float(x) for x in c.xyz) + (float(c.weight), float(c.p0), float(c.p1))
        if len(vals) != 6 or not all(math.isfinite(x) for x in vals):
            raise ValueError("reward term %r: weight, parameters and xyz must be finite" % (c.kind,))
        if k in TRACKING and not c.p0 > 0.0:
            raise ValueError("reward term %r: sigma must be positive" % (c.kind,))
        if k == 13 and not 0.0 < c.p0 <= 1.0:
            raise ValueError("reward term %r: soft must lie in (0, 1]" % (c.kind,))
        link = link_index(c.link) if k in LINKED else 0
        bits = 0
        if k in JOINT_SUMS:
            for j in c.mask or ():
                bits |= 1 << joint_index(j)
        elif k == 16:
            for l in c.mask or ():
                bits |= 1 << link_body(link_index(l))
        out.append((k, link, bits, vals[:3]) + vals[3:])
        contact |= k in CONTACT
        command |= k in TRACKING
        actions |= k == 12
    if len(out) > MAX_TERMS:
        raise ValueError("rewards: %d terms, at most %d" % (len(out), MAX_TERMS))
    return out, contact, command, actions


def as_tuples(spec):
    """plain lists / strings / numbers: what torch.save(..., weights_only) round-trips"""
    return [[c.kind, c.link, None if c.mask is None else list(c.mask), [float(x) for x in c.xyz], float(c.weight), float(c.p0), float(c.p1)]
            for c in flatten(spec)]


def from_tuples(data):
    return [Term(k, l, None if m is None else tuple(m), tuple(x), float(w), float(p0), float(p1)) for k, l, m, x, w, p0, p1 in data]
