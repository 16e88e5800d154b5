"""Helpers for fall termination (TrexVecEnv.set_termination; include/trex_batch.h trex_batch_set_termination): which bodies the
robot stands on - the feet - and which therefore should stay clear of the floor: the sensible `keep_clear`."""
import numpy as np
import torch

from . import _capi

REASONS = {1: "head", 2: "tilt", 4: "clearance"}     # TREX_TERM_HEAD / _TILT / _CLEARANCE


def reason_names(reason):
    """the criteria behind a termination reason, e.g. 5 -> ['head', 'clearance']"""
    return [name for bit, name in REASONS.items() if int(reason) & bit]


def reset_clearance(env):
    """[num_bodies] numpy: the floor clearance of every body in the reset state of `env` (a TrexVecEnv) - one query on a reset
    batch of one env of the same model; `env` itself is not touched."""
    m = env.model
    probe = _capi.Batch(m, 1, env.device.index)
    try:
        probe.reset()
        c = torch.empty(1, m.num_bodies, device=env.device)
        probe.body_clearance(c)
        return c[0].cpu().numpy()
    finally:
        probe.forget_buffers()
        probe.close()


def support_bodies(env):
    """Body indices the robot stands on in its reset pose: those whose lowest point is within the model's contact_margin of
    the lowest point of the whole robot. (Not "below contact_margin above the floor": the reference's start pose hangs the T-rex
    0.39 m over the floor and lets it drop, so in the reset state nothing touches yet. For a model that starts on the floor the
    two readings agree.)"""
    c = reset_clearance(env)
    return [int(b) for b in np.flatnonzero(c < c[np.isfinite(c)].min() + env.model.get_param("contact_margin"))]


def foot_bodies(env):
    """The feet as whole limbs: for every support body, the subtree under its nearest ancestor that branches (the T-rex: the
    tarsometatarsus with its toes)."""
    parent = env.model.array("parent").astype(int)
    nb = len(parent)
    kids = [[c for c in range(nb) if parent[c] == b] for b in range(nb)]
    feet = set()
    for b in support_bodies(env):
        top = b
        while parent[top] > 0 and len(kids[top]) < 2:
            top = parent[top]
        stack = [top]
        while stack:
            x = stack.pop()
            feet.add(int(x))
            stack += kids[x]
    return sorted(feet)


def foot_links(env):
    """One URDF link index per foot, in body order: of every limb of foot_bodies(), the first link of its first support body (the
    T-rex: the end of the middle toe of either leg, which carries the standing robot). A foot has several bodies on the floor;
    this names one of them - a point to follow and a body whose contact force tells a stance from a swing."""
    parent = env.model.array("parent").astype(int)
    nb = len(parent)
    kids = [[k for k in range(nb) if parent[k] == b] for b in range(nb)]
    link_body = env.model.array("link_body").astype(int)
    first = {}                                    # top body of the limb -> its first support body
    for b in support_bodies(env):
        top = b
        while parent[top] > 0 and len(kids[top]) < 2:
            top = parent[top]
        first.setdefault(top, b)
    return [int(np.flatnonzero(link_body == first[top])[0]) for top in sorted(first)]


def fall_bodies(env):
    """The bodies with collision geometry that are no part of a foot, as URDF link indices (one per body):
    keep_clear=fall_bodies(env) ends an episode when anything but a foot touches the floor."""
    m = env.model
    feet = set(foot_bodies(env))
    hs = m.array("hull_start").astype(int)
    first_link = {}
    for l, b in enumerate(m.array("link_body").astype(int)):
        first_link.setdefault(int(b), l)
    return [first_link[b] for b in range(m.num_bodies) if b not in feet and hs[b + 1] > hs[b] and b in first_link]
