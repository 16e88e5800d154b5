"""Host side of the renderer (no GPU): the hull planes the library computes ("hull_plane" / "hull_plane_start",
include/trex_batch.h), the camera conventions of trex_gym.render, and the numpy reference ray caster (tests/render_ref.py)
on scenes with a known answer."""
import glob
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as rr  # noqa: E402

from trex_gym import _capi  # noqa: E402
from trex_gym.render import Camera, depth_to_zbuffer, tile_images  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OBJ_DIR = os.path.join(ROOT, "trex-gym_amd", "assets", "collisions")


def _signature(points):   # rigid-motion invariant: sorted distances to the centroid
    return np.sort(np.linalg.norm(points - points.mean(0), axis=1))


def _objs():
    out = []
    for f in sorted(glob.glob(os.path.join(OBJ_DIR, "COL_*.obj"))):
        v, t = rr.obj_mesh(f)
        out.append((f, v, t, _signature(v)))
    return out


def _check_planes(model):
    from scipy.spatial import ConvexHull
    pl = model.array("hull_plane").reshape(-1, 4)
    st = model.array("hull_plane_start").astype(int)
    xyz = model.array("hull_xyz").reshape(-1, 3)
    gs = model.array("hull_group_start").astype(int)
    assert len(st) == len(gs) and st[0] == 0 and st[-1] == len(pl)
    objs = _objs()
    for g in range(len(gs) - 1):
        pts = xyz[gs[g]:gs[g + 1]]
        P = pl[st[g]:st[g + 1]]
        assert len(P) >= 4, g
        scale = np.ptp(pts, axis=0).max()
        n, d = P[:, :3], P[:, 3]
        np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
        s = pts @ n.T - d                                       # [V, K]
        assert s.max() <= 1e-9 * scale, (g, s.max())            # every vertex inside every plane
        assert (s >= -1e-9 * scale).sum(axis=0).min() >= 3, g   # every plane touches >= 3 vertices
        vol = rr.plane_polytope_volume(n, d)
        # the polytope the planes bound IS the convex hull of the points (qhull, independent of the library)
        assert abs(vol / ConvexHull(pts).volume - 1) < 1e-9, g
        # ... and the OBJ of the same hull: its triangulation folds a few edges inward (its volume lies 2e-5 .. 1.4e-3
        # below that of the convex hull of its own vertices), so it bounds the volume from below
        sig = _signature(pts)
        match = [(v, t) for f, v, t, sg in objs if len(sg) == len(sig) and np.abs(sg - sig).max() < 1e-5 * scale]
        assert len(match) == 1, g
        v, t = match[0]
        obj_vol = rr.mesh_volume(v, t)
        assert abs(ConvexHull(v).volume / vol - 1) < 1e-6, g   # (OBJ vertices are written to 7 digits)
        assert 0 <= vol / obj_vol - 1 < 2e-3, (g, vol / obj_vol - 1)


def test_hull_planes_obj_model():
    _check_planes(_capi.Model())


def test_hull_planes_dae_model(reference_assets):
    _check_planes(_capi.Model(os.path.join(reference_assets, "trex.urdf"), os.path.join(reference_assets, "collisions")))


def test_hull_planes_primitive_model_has_none():
    m = _capi.Model()
    m.use_primitive_collision(0.2)
    assert m.array("hull_plane").size == 0
    assert (m.array("hull_plane_start") == 0).all()


def test_camera_view_matrix():
    V = np.array(Camera().view_matrix((0, 0, 0))).reshape(4, 4).T     # column-major -> matrix
    R, t = V[:3, :3], V[:3, 3]
    eye = -R.T @ t
    np.testing.assert_allclose(eye, [10 * math.cos(math.radians(30)), 0, 5.0], atol=1e-12)
    np.testing.assert_allclose(eye, [8.660254, 0, 5.0], atol=1e-6)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    assert R[2] @ np.array([-1.0, 0, 0]) < 0      # looking along -x (the camera looks down -z_cam)
    assert R[1, 2] > 0                            # world z is up on the screen
    # a fixed target moves the eye with it
    V2 = np.array(Camera(target=(1, 2, 3)).view_matrix()).reshape(4, 4).T
    np.testing.assert_allclose(-V2[:3, :3].T @ V2[:3, 3], eye + [1, 2, 3], atol=1e-12)


def test_camera_projection_matrix():
    P = np.array(Camera().projection_matrix(4 / 3)).reshape(4, 4).T
    f = 1 / math.tan(math.radians(30))
    want = np.array([[f * 3 / 4, 0, 0, 0], [0, f, 0, 0], [0, 0, -100.1 / 99.9, -20.0 / 99.9], [0, 0, -1, 0]])
    np.testing.assert_allclose(P, want, atol=1e-12)


def test_depth_to_zbuffer_inverts_pybullet_formula():
    z = np.array([0.1, 1.0, 10.0, 100.0])
    zb = depth_to_zbuffer(z, 0.1, 100.0)
    np.testing.assert_allclose(zb[[0, -1]], [0.0, 1.0], atol=1e-12)
    np.testing.assert_allclose(100.0 * 0.1 / (100.0 - 99.9 * zb), z, rtol=1e-12)


def test_tile_images_near_square():
    imgs = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    t = tile_images(imgs)
    assert t.shape == (4, 9, 3)
    np.testing.assert_array_equal(t[2:4, 3:6], imgs[4])
    assert (t[2:4, 6:9] == 0).all()


def _scene_render(scene, W=200, H=150, fov=40.0, dist=6.0):
    eye, dirs, _ = rr.camera_rays(dist, 90.0, -30.0, fov, W, H, (0, 0, 1.0))
    return rr.render(scene, np.eye(3)[None], np.zeros((1, 3)), eye, dirs, 0.1, 100.0), eye, dirs


def _projected_edge_count(mask):
    return int((mask[1:] != mask[:-1]).sum() + (mask[:, 1:] != mask[:, :-1]).sum())


def test_reference_caster_sphere_area():
    r = 0.5
    scene = rr.Scene(np.array([[0, 0, 1.0]]), np.array([r]), [0, 1], [0, 1], floor_z=-100.0)
    (seg, depth, rgb, sm, _), eye, dirs = _scene_render(scene)
    mask = seg == 0
    W, H = 200, 150
    # analytic: the sphere's silhouette is an ellipse in the image; at the image centre it is a circle of angular radius
    # asin(r / D), i.e. a disc of radius tan(asin(r / D)) in tangent units -> pixels: / (tan(fov/2) / (H/2))
    D = 6.0
    rad_px = math.tan(math.asin(r / D)) / (math.tan(math.radians(20)) / (H / 2))
    area = math.pi * rad_px ** 2
    assert abs(mask.sum() - area) <= _projected_edge_count(mask), (mask.sum(), area)
    # depth at the centre pixels = D - r
    assert abs(depth[mask].min() - (D - r)) < 2e-3
    assert (seg[~mask] == -2).all()
    # the margin is small exactly along the silhouette
    edge = np.zeros_like(mask)
    edge[1:] |= mask[1:] != mask[:-1]
    edge[:-1] |= mask[1:] != mask[:-1]
    assert sm[~edge].min() > 0


def test_reference_caster_cube_area():
    h = 0.5
    cube = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (1 - h, 1 + h)])
    scene = rr.Scene(cube, np.zeros(8), [0, 8], [0, 8], floor_z=-100.0)
    (seg, depth, rgb, sm, rm), eye, dirs = _scene_render(scene)
    mask = seg == 0
    # analytic: project the 8 corners with the same camera, the silhouette is their convex hull in the image plane
    from scipy.spatial import ConvexHull
    _, _, f = rr.camera_rays(6.0, 90.0, -30.0, 40.0, 200, 150, (0, 0, 1.0))
    y, p = math.radians(90.0), math.radians(-30.0)
    up0 = np.array([math.sin(p) * math.sin(y), -math.sin(p) * math.cos(y), math.cos(p)])
    rgt = np.cross(f, up0); rgt /= np.linalg.norm(rgt)
    u = np.cross(rgt, f)
    ty = math.tan(math.radians(20)); tx = ty * 200 / 150
    pts = []
    for c in cube:
        v = c - eye
        z = v @ f
        pts.append([(v @ rgt / z / tx + 1) * 100, (1 - v @ u / z / ty) * 75])
    area = ConvexHull(np.array(pts)).volume
    assert abs(mask.sum() - area) <= _projected_edge_count(mask), (mask.sum(), area)
    assert (rgb[mask] != rgb[~mask][0]).any(axis=-1).all()   # the cube is shaded, not sky-coloured
