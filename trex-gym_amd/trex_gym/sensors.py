"""Range sensors on the batched env: ray patterns for TrexVecEnv.ray_test (trex_batch_ray_test) and a sensor that reads metres.

A pattern is a [R, 6] float32 tensor - from xyz, to xyz per ray - in the frame of the link the sensor is mounted on (or the
world's), shared by every env: the batch evaluates the frame at each env's current state.

    fan         a lidar fan: n_yaw x n_pitch rays of one length from one origin
    grid_down   a height scanner: nx x ny vertical rays
    RaySensor   a pattern on a link of an env; read() -> distances [n, R] in metres

An inertial sensor on the same env (TrexVecEnv.link_state / trex_batch_link_state):

    Imu         accelerometer + gyro at a point of a link; read() -> (specific force, angular velocity) in the link's axes
"""
import math

import torch


def fan(origin=(0.0, 0.0, 0.0), yaw_range=(-math.pi / 2, math.pi / 2), pitch_range=(0.0, 0.0), n_yaw=16, n_pitch=1, length=10.0):
    """[n_yaw * n_pitch, 6]: rays of `length` metres from `origin`, yaw (about +z, from +x towards +y) and pitch (up from the
    xy plane) in radians, each range covered end to end (one value: the range's middle). Pitch-major order: ray p * n_yaw + y."""
    def span(r, n):
        lo, hi = float(r[0]), float(r[1])
        return torch.tensor([0.5 * (lo + hi)], dtype=torch.float64) if n == 1 else torch.linspace(lo, hi, n, dtype=torch.float64)
    if n_yaw < 1 or n_pitch < 1:
        raise ValueError("fan: n_yaw and n_pitch must be >= 1")
    yaw, pitch = span(yaw_range, int(n_yaw)), span(pitch_range, int(n_pitch))
    P, Y = torch.meshgrid(pitch, yaw, indexing="ij")
    d = torch.stack([torch.cos(P) * torch.cos(Y), torch.cos(P) * torch.sin(Y), torch.sin(P)], -1).reshape(-1, 3)
    o = torch.tensor([float(x) for x in origin], dtype=torch.float64).expand_as(d)
    return torch.cat([o, o + float(length) * d], 1).to(torch.float32)


def grid_down(x_range=(-0.5, 0.5), y_range=(-0.5, 0.5), nx=4, ny=4, top=0.0, length=5.0):
    """[nx * ny, 6]: rays from (x, y, top) straight down the frame's -z to (x, y, top - length), x-major order: ray i * ny + j."""
    def span(r, n):
        lo, hi = float(r[0]), float(r[1])
        return torch.tensor([0.5 * (lo + hi)], dtype=torch.float64) if n == 1 else torch.linspace(lo, hi, n, dtype=torch.float64)
    if nx < 1 or ny < 1:
        raise ValueError("grid_down: nx and ny must be >= 1")
    X, Y = torch.meshgrid(span(x_range, int(nx)), span(y_range, int(ny)), indexing="ij")
    x, y = X.reshape(-1), Y.reshape(-1)
    z = torch.full_like(x, float(top))
    return torch.stack([x, y, z, x, y, z - float(length)], 1).to(torch.float32)


class RaySensor:
    """A ray pattern mounted on a link of a TrexVecEnv. link: name or index (None: the world frame); pattern: [R, 6];
    bodies: the body indices the rays may hit (None: all - a sensor inside a hull looks out of it either way); floor: whether
    they may hit the floor. The pattern is moved to the env's device once."""

    def __init__(self, env, link, pattern, bodies=None, floor=True):
        pattern = torch.as_tensor(pattern)
        if pattern.dim() != 2 or pattern.shape[1] != 6:
            raise ValueError("pattern must have shape (R, 6), got %s" % (tuple(pattern.shape),))
        self.env, self.link = env, link
        self.pattern = pattern.to(device=env.device, dtype=torch.float32).contiguous()
        self.bodies = None if bodies is None else list(bodies)
        self.floor = bool(floor)
        self.length = (self.pattern[:, 3:] - self.pattern[:, :3]).norm(dim=1)   # [R] metres
        self.num_rays = int(self.pattern.shape[0])

    def cast(self, positions=False, normals=False):
        """The raw result of TrexVecEnv.ray_test for the pattern: (fraction, body[, position][, normal])."""
        return self.env.ray_test(self.pattern, self.link, positions, normals, self.bodies, self.floor)

    def read(self):
        """[n, R] distances in metres along each ray to what it hits; the ray's full length where it hits nothing."""
        return self.cast()[0] * self.length


class Imu:
    """An accelerometer and a gyro at `position` (link frame) of link `link` (name or index) of a TrexVecEnv. It holds one of
    the env's probe sets until close()."""

    def __init__(self, env, link, position=(0.0, 0.0, 0.0)):
        self.env = env
        self.probes = env.link_probes(link, [float(x) for x in position])
        self.gravity = float(env.model.get_param("gravity"))
        self.interval = float(env.model.get_param("substeps")) * float(env.model.get_param("dt"))   # seconds per env-step
        self._last_v = None   # [n, 3] world velocity of the point at the previous read()

    def close(self):
        self.probes.close()

    def static(self):
        """(specific_force [n, 3], angular_velocity [n, 3]) in link axes at the current state with the joint and base
        accelerations taken as zero: gravity, centripetal and Coriolis terms only. At rest: the link's view of (0, 0, g)."""
        s = self.env.link_state(self.probes, accel=None, axes="link", proper=True, velocity=True, acceleration=True)
        return s.linear_acceleration[:, 0], s.angular_velocity[:, 0]

    def read(self, done=None):
        """(specific_force [n, 3], angular_velocity [n, 3]) in link axes. The specific force is the change of the point's world
        velocity since the previous read(), over one env-step (substeps x dt), plus g z, in the link's current axes: what an
        accelerometer integrates over the env-step, contact impulses included. On the first call, and for the envs whose `done`
        ([n], bool or uint8: their episode has just been restarted) is set, static()'s values: no difference is taken across
        an episode boundary. Call it once after every step."""
        f0, gyro = self.static()
        w = self.env.link_state(self.probes, axes="world", velocity=True)
        v = w.linear_velocity[:, 0]
        if self._last_v is None:
            force = f0
        else:
            a = (v - self._last_v) / self.interval
            a[:, 2] += self.gravity
            force = (quat_rotate_inverse(w.orientation[:, 0], a))
            if done is not None:
                force = torch.where(torch.as_tensor(done, device=force.device).bool().view(-1, 1), f0, force)
        self._last_v = v.clone()
        return force, gyro


def quat_rotate_inverse(q, v):
    """R(q)^T v for unit quaternions q [..., 4] xyzw: a world vector in the axes of the frame q orients."""
    u, w = -q[..., :3], q[..., 3:]
    t = 2.0 * torch.cross(u, v, dim=-1)
    return v + w * t + torch.cross(u, t, dim=-1)
