"""Camera of the batched renderer (trex_batch_render, include/trex_batch.h) and pybullet's matrix conventions.

The renderer ray-casts the collision hulls the physics holds (not the visual meshes, which are not shipped), so its
pictures are not pybullet's pixels; the camera is pybullet's: computeViewMatrixFromYawPitchRoll with upAxisIndex=2 and
computeProjectionMatrixFOV, with the reference's defaults (trex_env.py:156-181). The matrices below are the 16-float
column-major lists pybullet returns, for code ported from the reference that feeds them elsewhere.
"""
import math

import numpy as np

RENDER_HEIGHT = 720   # trex_env.py:22-23
RENDER_WIDTH = 960


class Camera:
    """distance, yaw / pitch in degrees, vertical fov in degrees, near / far planes; target None = follow each env's base
    position (trex_env.py:157), else a fixed world point (x, y, z)."""

    def __init__(self, distance=10.0, yaw=90.0, pitch=-30.0, fov=60.0, near=0.1, far=100.0, target=None):
        self.distance, self.yaw, self.pitch, self.fov, self.near, self.far = (float(distance), float(yaw), float(pitch),
                                                                            float(fov), float(near), float(far))
        self.target = None if target is None else tuple(float(x) for x in target)

    def __repr__(self):
        return ("Camera(distance=%g, yaw=%g, pitch=%g, fov=%g, near=%g, far=%g, target=%r)"
                % (self.distance, self.yaw, self.pitch, self.fov, self.near, self.far, self.target))

    def eye_up(self, target=None):
        """(eye, up) in world coordinates: eye = target + Rz(yaw) Rx(pitch) (0, -distance, 0), up = Rz(yaw) Rx(pitch) z."""
        t = np.zeros(3) if target is None else np.asarray(target, np.float64)
        y, p = math.radians(self.yaw), math.radians(self.pitch)
        off = self.distance * np.array([math.cos(p) * math.sin(y), -math.cos(p) * math.cos(y), -math.sin(p)])
        up = np.array([math.sin(p) * math.sin(y), -math.sin(p) * math.cos(y), math.cos(p)])
        return t + off, up

    def view_matrix(self, target=None):
        """pybullet's computeViewMatrixFromYawPitchRoll(target, distance, yaw, pitch, roll=0, upAxisIndex=2): 16 floats,
        column-major. target defaults to the fixed target (or the origin for a follow-base camera)."""
        if target is None:
            target = self.target if self.target is not None else (0.0, 0.0, 0.0)
        t = np.asarray(target, np.float64)
        eye, up = self.eye_up(t)
        f = t - eye
        f /= np.linalg.norm(f)
        s = np.cross(f, up)
        s /= np.linalg.norm(s)
        u = np.cross(s, f)
        m = np.eye(4)
        m[0, :3], m[1, :3], m[2, :3] = s, u, -f
        m[0, 3], m[1, 3], m[2, 3] = -s @ eye, -u @ eye, f @ eye
        return [float(x) for x in m.T.reshape(-1)]

    def projection_matrix(self, aspect=RENDER_WIDTH / RENDER_HEIGHT):
        """pybullet's computeProjectionMatrixFOV(fov, aspect, near, far): OpenGL perspective, 16 floats, column-major."""
        ys = 1.0 / math.tan(math.radians(self.fov) / 2)
        n, f = self.near, self.far
        m = np.zeros((4, 4))
        m[0, 0], m[1, 1] = ys / aspect, ys
        m[2, 2], m[2, 3], m[3, 2] = (f + n) / (n - f), 2 * f * n / (n - f), -1.0
        return [float(x) for x in m.T.reshape(-1)]


def depth_to_zbuffer(depth, near=0.1, far=100.0):
    """Linear eye-space depth (what trex_batch_render writes) -> pybullet's non-linear depth buffer in [0, 1]
    (getCameraImage's depthImg; its inverse is far * near / (far - (far - near) * zbuffer)). Works on numpy arrays and
    torch tensors."""
    return far * (depth - near) / ((far - near) * depth)


def tile_images(images):
    """[V, H, W, C] -> one near-square grid image (baselines' tile_images): ceil(sqrt(V)) columns, black padding."""
    images = np.asarray(images)
    V, H, W, Cc = images.shape
    cols = int(math.ceil(math.sqrt(V)))
    rows = int(math.ceil(V / cols))
    out = np.zeros((rows * H, cols * W, Cc), images.dtype)
    for k in range(V):
        r, c = divmod(k, cols)
        out[r * H:(r + 1) * H, c * W:(c + 1) * W] = images[k]
    return out
