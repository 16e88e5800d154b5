"""External forces on the batched env (trex_batch_set_external_wrench): pybullet's applyExternalForce /
applyExternalTorque and random pushes, built with torch only (they run on CPU tensors too).

The batch takes one wrench per env and moving body, [n, num_bodies, 6] = force (N) at the body's centre of mass and
torque (N m) about it, world axes, held for every substep of the env-steps that follow (include/trex_batch.h).

    link_wrench     forces on URDF LINKS (index or name; WORLD_FRAME or LINK_FRAME; any point) -> that body wrench
    RandomPushes    horizontal pushes on one body, drawn on the device without a host sync (push recovery, training noise)

and, the other way round, what the contact sensor (trex_batch_contact_wrench) reports in the same [n, num_bodies, 6] layout:

    link_contact_forces    the floor-contact force on the bodies of URDF links (the feet), summed per entry
    contact_flags          which bodies carry floor load
"""
import math

import numpy as np
import torch

WORLD_FRAME, LINK_FRAME = "world", "link"     # pybullet's p.WORLD_FRAME / p.LINK_FRAME


class LinkTable:
    """What link_wrench needs of a model: link -> body map, the body <- link transforms ("link_tf": link = body o tf) and the
    body COMs in body frames ("com"). from_model(model) reads them from a trex_gym._capi.Model."""

    def __init__(self, link_names, link_body, link_tf, com):
        self.link_names = list(link_names)
        self.link_body = np.asarray(link_body).astype(np.int64)
        self.link_tf = np.asarray(link_tf, np.float64).reshape(-1, 12)
        self.com = np.asarray(com, np.float64).reshape(-1, 3)
        self.num_bodies = len(self.com)

    @classmethod
    def from_model(cls, model):
        return cls([name for name, _ in model.links()], model.array("link_body"), model.array("link_tf"), model.array("com"))

    def index(self, link):
        if isinstance(link, str):
            if link not in self.link_names:
                raise KeyError("unknown link '%s'" % link)
            return self.link_names.index(link)
        link = int(link)
        if not 0 <= link < len(self.link_names):
            raise IndexError("link index %d out of range [0, %d)" % (link, len(self.link_names)))
        return link


def quat_to_matrix(q):
    """[..., 4] xyzw -> [..., 3, 3]"""
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def link_wrench(table, link_poses, link, force, point=None, frame=WORLD_FRAME, wrench=None):
    """Force `force` on link `link` (index or name) at `point` -> the wrench on the link's body, added into `wrench`
    ([n, num_bodies, 6], made of zeros when None) and returned.

    link_poses: [n, L, 7] world poses of the links (TrexVecEnv.link_transforms(): xyz + quaternion xyzw).
    force, point: [3] or [n, 3]. frame=WORLD_FRAME: both in world coordinates; LINK_FRAME: both in the link's frame
    (rotated and placed with the link's pose). point=None: at the body's COM (a pure force, no moment).
    The body receives F (world) at its COM and the torque (p - c) x F, c its COM. The moment arm is taken at the poses
    given - the state of the call - and is NOT re-evaluated per substep, nor is a LINK_FRAME force turned with the link
    during the step (the batch holds the wrench constant over the env-step)."""
    if frame not in (WORLD_FRAME, LINK_FRAME):
        raise ValueError("frame must be '%s' or '%s'" % (WORLD_FRAME, LINK_FRAME))
    k = table.index(link)
    n = link_poses.shape[0]
    dev, dt = link_poses.device, link_poses.dtype
    b = int(table.link_body[k])
    pl = link_poses[:, k, :3]
    Rl = quat_to_matrix(link_poses[:, k, 3:7])
    tf = torch.as_tensor(table.link_tf[k], dtype=dt, device=dev)
    Rt, tt = tf[:9].reshape(3, 3), tf[9:]
    Rb = Rl @ Rt.T                                         # link = body o tf  ->  body = link o tf^-1
    pb = pl - Rb @ tt
    c = pb + Rb @ torch.as_tensor(table.com[b], dtype=dt, device=dev)     # the body's COM, world
    F = torch.as_tensor(force, dtype=dt, device=dev).expand(n, 3)
    if frame == LINK_FRAME:
        F = (Rl @ F.unsqueeze(-1)).squeeze(-1)
    if wrench is None:
        wrench = torch.zeros(n, table.num_bodies, 6, dtype=dt, device=dev)
    wrench[:, b, :3] += F
    if point is not None:
        p = torch.as_tensor(point, dtype=dt, device=dev).expand(n, 3)
        if frame == LINK_FRAME:
            p = pl + (Rl @ p.unsqueeze(-1)).squeeze(-1)
        wrench[:, b, 3:] += torch.linalg.cross(p - c, F, dim=-1)
    return wrench


def link_contact_forces(table, wrench, links):
    """Floor-contact forces [n, K, 3] of K entries from a sensor wrench [n, num_bodies, 6]. links: a sequence of K entries,
    each a link (index or name) or a sequence of links; an entry sums the force part over the DISTINCT bodies of its links
    (links joined by fixed joints share a body, which counts once)."""
    cols = []
    for entry in links:
        group = [entry] if isinstance(entry, (str, int, np.integer)) else list(entry)
        bodies = sorted({int(table.link_body[table.index(l)]) for l in group})
        cols.append(wrench[:, bodies, :3].sum(1))
    return torch.stack(cols, 1)


def contact_flags(wrench, threshold=0.0):
    """[n, num_bodies] bool from a sensor wrench [n, num_bodies, 6]: the body's normal (z) contact force exceeds
    `threshold` N. Bodies off the floor report exact zeros, so threshold 0 flags every body the floor pushes."""
    return wrench[..., 2] > threshold


class RandomPushes:
    """Horizontal pushes on body `body` of every env, drawn on the tensors' device with no host sync.

    Every `interval` env-steps each env that is not being pushed starts a push with probability `probability`: a force
    of uniform direction in the horizontal plane and uniform magnitude in [0, max_force] N, held for `duration` env-steps
    (at the body's COM: no moment). A push ends early when its env ends its episode (done). Call step(done) once per
    env-step, BEFORE the step launch, with the done flags of the previous step: it returns the forces [n, 3] of this
    step; wrench(num_bodies, done) the same as a [n, num_bodies, 6] wrench."""

    def __init__(self, num_envs, body=0, interval=100, probability=0.5, max_force=1000.0, duration=5, generator=None,
                 device=None):
        if interval < 1 or duration < 1:
            raise ValueError("interval and duration must be >= 1 env-step")
        if not 0.0 <= probability <= 1.0:
            raise ValueError("probability must lie in [0, 1]")
        self.num_envs, self.body = int(num_envs), int(body)
        self.interval, self.probability, self.max_force, self.duration = int(interval), float(probability), float(max_force), int(duration)
        if device is None:
            device = generator.device if generator is not None else torch.device("cpu")
        self.device = torch.device(device)
        self.generator = generator
        self.force = torch.zeros(self.num_envs, 3, device=self.device)
        self.left = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)    # env-steps left of the push
        self.t = 0                                                                         # env-steps seen (host counter)

    def _rand(self, *shape):
        return torch.rand(*shape, generator=self.generator, device=self.device)

    def step(self, done=None):
        if done is not None:
            self.left.masked_fill_(done.to(self.device).bool(), 0)     # the episode ended: its push with it
        if self.t % self.interval == 0:
            start = (self.left == 0) & (self._rand(self.num_envs) < self.probability)
            ang = self._rand(self.num_envs) * (2.0 * math.pi)
            mag = self._rand(self.num_envs) * self.max_force
            f = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang), torch.zeros_like(mag)], -1)
            self.force = torch.where(start.unsqueeze(-1), f, self.force)
            self.left = torch.where(start, torch.full_like(self.left, self.duration), self.left)
        self.t += 1
        active = self.left > 0
        out = torch.where(active.unsqueeze(-1), self.force, torch.zeros_like(self.force))
        self.left = torch.clamp(self.left - 1, min=0)
        return out

    def wrench(self, num_bodies, done=None):
        w = torch.zeros(self.num_envs, num_bodies, 6, device=self.device)
        w[:, self.body, :3] = self.step(done)
        return w


class RandomGains:
    """Per-env motor strength and gain randomisation, beside RandomPushes: every env that is reset draws one scale for kp, one
    for kd and one for max_force, uniform in the given (low, high) ranges, applied to the nominal values of all its joints
    (domain randomisation of the actuators; sim-to-real work randomises these first). draw(mask) returns the [n, J] tensors
    for TrexVecEnv.set_motor_gains(**...): envs with mask == 0 keep their last draw. TrexVecEnv(...).gains = RandomGains(...)
    makes reset_tensor() draw and apply them."""

    def __init__(self, num_envs, num_joints, kp=5e-3, kd=0.1, max_force=3e5, kp_scale=(0.8, 1.2), kd_scale=(0.8, 1.2),
                 max_force_scale=(0.8, 1.2), generator=None, device=None):
        for name, (lo, hi) in (("kp_scale", kp_scale), ("kd_scale", kd_scale), ("max_force_scale", max_force_scale)):
            if not 0.0 <= lo <= hi:
                raise ValueError("%s: expected 0 <= low <= high, got (%g, %g)" % (name, lo, hi))
        self.num_envs, self.num_joints = int(num_envs), int(num_joints)
        if device is None:
            device = generator.device if generator is not None else torch.device("cpu")
        self.device = torch.device(device)
        self.generator = generator
        self.nominal = (float(kp), float(kd), float(max_force))
        self.ranges = (tuple(kp_scale), tuple(kd_scale), tuple(max_force_scale))
        self.scale = torch.ones(3, self.num_envs, device=self.device)        # kp, kd, max_force scale of every env

    def draw(self, mask=None):
        u = torch.rand(3, self.num_envs, generator=self.generator, device=self.device)
        lo = torch.tensor([r[0] for r in self.ranges], device=self.device).unsqueeze(1)
        hi = torch.tensor([r[1] for r in self.ranges], device=self.device).unsqueeze(1)
        new = lo + (hi - lo) * u
        self.scale = new if mask is None else torch.where(mask.to(self.device).bool().unsqueeze(0), new, self.scale)
        out = [(v * self.scale[k]).unsqueeze(1).expand(self.num_envs, self.num_joints).contiguous()
               for k, v in enumerate(self.nominal)]
        return dict(kp=out[0], kd=out[1], max_force=out[2])
