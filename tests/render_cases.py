"""Case tables for the renderer (trex_batch_render, csrc/render.hip) at the edges of its tiling, culling and clipping: ragged and
tiny frames, the near plane through the hulls, an eye inside a hull or below the floor, a far plane that crops, extreme fields of
view and aspect ratios; and the generated models (tests/synthetic_models.py) with bent joints, for the pose pass of the ray kernels
(csrc/render_pose.h). numpy only: tests/test_render_cases_host.py qualifies every case on the f64 reference caster
(tests/render_ref.py) alone, before a GPU sees it; tests/test_gpu_render_edges.py renders the same cases. A helper, not a conftest.

A case is (camera, frame, state). It only counts if the reference is DECIDED on it - tests/gpu_render_support.py::render_compare leaves out
the pixels whose reference margin is below 1e-4 m and allows 0.5 % of label disagreements among them, so a case made mostly of
such pixels would pass whatever the kernel does - and if it REACHES the path it is named for. qualify() and paths_reached() state
both conditions; a case that fails them is repaired by moving its camera, never by loosening them.
"""
import os

import numpy as np

import render_ref as rr

MARGIN = 1e-4              # m: the threshold of tests/gpu_render_support.py::render_compare
SEG_SHARE_CAP = 0.0025     # share of pixels with seg_margin < MARGIN: half of what render_compare tolerates as disagreement
TINY_PIXELS, TINY_MARGIN = 400, 1e-3     # frames under 400 pixels: no pixel at all near a decision (0.5 % of them is < 2 pixels)
RGB_PIXELS, RGB_SHARE_CAP = 1000, 0.05   # frames of 1000 pixels or more: share with rgb_margin < MARGIN
RGB_USED_MIN = 0.93        # GPU side: share of pixels the rgb comparison uses = 1 - 5 % - 0.5 % - a little for f32 poses
SKY_RGB = (153, 191, 235)  # render_ref.SKY through floor(255 c + 0.5)

# ---------------------------------------------------------------- cameras
# name -> (distance, yaw, pitch, fov, near, far, target); target None = follow the env's base. Yaws stay off multiples of 90: at
# yaw 90 the image rows run along the floor's checker lines, and a tenth of a small frame's floor pixels lie within 1e-4 of one.
CAMERAS = {
    "far_view":    (6.0, 30.0, -20.0, 50.0, 0.1, 100.0, None),      # the baseline: CAMERAS[1] of test_gpu_render.py, following the base
    "near_cuts":   (1.2, 60.0, -15.0, 75.0, 0.8, 50.0, None),       # the near plane through the hulls: pl < 0, shaded from inside
    "inside":      (0.3, 90.0, -10.0, 90.0, 0.05, 50.0, None),      # the eye inside the pelvis hull: every pixel that body at depth = near
    "below_floor": (6.0, 30.0, 20.0, 60.0, 0.1, 100.0, (0.0, 0.0, 0.5)),   # eye z = 0.5 - 6 sin 20 = -1.55: the floor at near, everywhere
    "far_crops":   (6.0, 30.0, -20.0, 50.0, 0.1, 6.0, None),        # the far plane through the animal and the floor
    "all_sky":     (6.0, 30.0, -20.0, 50.0, 0.1, 4.0, None),        # nothing within far
    "wide":        (3.0, 120.0, -35.0, 150.0, 0.1, 100.0, None),    # cull tangents of 3.7 and more
    "narrow":      (30.0, 75.0, -10.0, 5.0, 0.1, 100.0, None),      # cull tangents of 0.04, depth about 30
    "down":        (8.0, 45.0, -90.0, 60.0, 0.1, 100.0, None),      # straight down: forward = -z, up from the yaw alone
    "low":         (4.0, 250.0, -2.0, 100.0, 0.1, 100.0, None),     # grazing floor rays, the horizon in the frame
}
FIELDS = ("distance", "yaw", "pitch", "fov", "near", "far", "target")

# frames (width, height); the tile is 16 x 16
FULL_FRAMES = [(100, 75), (33, 41), (17, 15), (16, 16), (17, 16), (16, 17), (1, 1), (15, 1), (1, 40), (1, 4096), (4096, 1)]
SHORT_FRAMES = [(100, 75), (33, 41)]
FULL_CAMERAS = ("far_view", "near_cuts")
PRIMITIVE_CAMERAS = ("far_view", "near_cuts", "inside", "far_crops")      # also rendered with primitive (sphere) collision
MAIN_FRAME = (100, 75)
EXACT_FRAMES = [(33, 41), (100, 75)]

STATE_NAMES = ("reset", "crouch33", "crouch60", "random20", "crouch33_far")
STANDING = (1, 2, 4)       # indices of the states that stand on the floor
BASE_SHIFT = (50.0, -40.0, 0.0)


# Primitive (sphere) collision: the fitted spheres lie INSIDE the hulls and none is thicker than 0.4 m, so three of the four
# cameras do not reach their path on them from where they stand for the hulls (measured on the reference: 370 near-cut pixels,
# no sphere around the eye, 86 body pixels within far). They are moved, the conditions stay. A target ("eye" | "target", body,
# point) anchors the eye or the target at a point of a body, for every state: the centre of one of the body's larger spheres.
# near_cuts becomes a close-up (0.6 m, the near plane 5 cm in front of the sphere's centre); a close-up of spheres puts a
# silhouette within 1e-3 m of some pixel of every tiny frame, so the frames under 400 pixels - of which no count is asked - keep
# the tabled camera, whose near plane cuts 1 to 7 of their pixels.
PRIMITIVE_CAMERAS_MOVED = {
    "near_cuts": (0.6, 150.0, -15.0, 75.0, 0.55, 50.0, ("target", 13, (-0.3833, 0.1320, 0.1961))),
    "inside":    (0.3, 90.0, -10.0, 90.0, 0.05, 50.0, ("eye", 2, (0.0295, 0.2539, -0.0275))),
    "far_crops": (6.0, 30.0, -20.0, 50.0, 0.1, 7.0, None),
}

# (collision, camera, frame) -> (yaw, pitch) added, degrees. Frames under 400 pixels must not hold ONE pixel within 1e-3 m of a
# decision (qualify()); where the camera as tabled leaves one on some state, it is turned by the smallest step (|yaw| + |pitch|)
# of a 0.5 degree grid that leaves none on any state.
NUDGE = {
    ("hulls", "far_view", (17, 15)): (-0.5, 0.0), ("hulls", "far_view", (17, 16)): (-0.5, 0.0),
    ("hulls", "near_cuts", (16, 16)): (-0.5, 0.0),
    ("primitives", "far_view", (17, 15)): (0.5, 0.0), ("primitives", "far_view", (17, 16)): (0.0, -1.0),
    ("primitives", "near_cuts", (17, 15)): (0.5, 2.0), ("primitives", "near_cuts", (16, 16)): (-1.5, -2.5),
    ("primitives", "near_cuts", (17, 16)): (-6.0, 2.0), ("primitives", "near_cuts", (16, 17)): (1.0, -3.0),
}


# A 4096 x 1 frame at the tabled fields of view (50, 75 degrees) is one row of 4096 rays fanned over +-89.97 degrees: all of it
# floor, at ONE depth, out to 28 km on either side. Which checker square a point 28 km away lies in is no question f32 can answer
# (one ulp there is 2 mm; the margin of the comparison is 0.1 mm), so the row is rendered at a vertical field of view of 1 degree:
# tan_x is still 4096 tan_y, the floor it sweeps ends 500 m out, and the animal is some tens of pixels of it.
FRAME_FOV = {(4096, 1): 1.0}
HP_ULPS = 4.0              # f32 ulps allowed to the kernel's hit point eye + t dir on the floor (condition())


def case_camera(name, collision="hulls", frame=None):
    """the CAMERAS-style tuple a case (camera name, collision, frame (W, H)) is rendered with"""
    frame = None if frame is None else tuple(frame)
    c = CAMERAS[name]
    tiny = frame is not None and frame[0] * frame[1] < TINY_PIXELS
    if collision == "primitives" and name in PRIMITIVE_CAMERAS_MOVED and not (name == "near_cuts" and tiny):
        c = PRIMITIVE_CAMERAS_MOVED[name]
    dy, dp = NUDGE.get((collision, name, frame), (0.0, 0.0))
    return (c[0], c[1] + dy, c[2] + dp, FRAME_FOV.get(frame, c[3])) + c[4:]


def eye_offset(distance, yaw, pitch):
    """eye - target: Rz(yaw) Rx(pitch) (0, -distance, 0) (include/trex_batch.h)"""
    y, p = np.radians(yaw), np.radians(pitch)
    return distance * np.array([np.cos(p) * np.sin(y), -np.cos(p) * np.cos(y), -np.sin(p)])


def resolve(cam, R=None, p=None):
    """-> trex_gym.render.Camera of a CAMERAS-style tuple; an anchored target is resolved on the body poses (R, p) to a fixed
    world point, rounded to f32 as the C-ABI takes it (so the reference and the kernel see the same eye)."""
    from trex_gym.render import Camera
    c = dict(zip(FIELDS, cam))
    t = c["target"]
    if t is not None and isinstance(t[0], str):
        kind, b, pt = t
        w = np.asarray(p[b], np.float64) + np.asarray(R[b], np.float64) @ np.asarray(pt, np.float64)
        if kind == "eye":
            w = w - eye_offset(c["distance"], c["yaw"], c["pitch"])
        c["target"] = tuple(float(x) for x in w.astype(np.float32))
    return Camera(**c)


def anchored(cam):
    """True if the camera's target depends on the state (one render call per state)"""
    return cam[6] is not None and isinstance(cam[6][0], str)


def frames(name):
    return FULL_FRAMES if name in FULL_CAMERAS else SHORT_FRAMES


def trex_states(oracle64):
    """[5, 63] f32, STATE_NAMES: the oracle's reset state (the base hangs at z = 3), two states of the committed crouch rollout
    standing on the floor, one of the random rollout in the air, and the first standing one moved by BASE_SHIFT."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_rollout.npz"))
    s = oracle64.new_state()
    oracle64.reset(s)
    far = gold["crouch_state"][33].copy()
    far[:3] += BASE_SHIFT
    return np.stack([oracle64.get_state(s), gold["crouch_state"][33], gold["crouch_state"][60], gold["random_state"][20],
                     far]).astype(np.float32)


def oracle_poses(orc, state):
    """(R [nb, 3, 3], p [nb, 3], base [3]) of the bodies by the f64 oracle at an (f32-valued) state"""
    s = orc.new_state()
    orc.set_state(s, np.asarray(state, np.float64))
    pos, rot = orc.body_poses(s)
    return rot, pos, np.asarray(state, np.float64)[:3].copy()


def oracle_scene(om, floor_z):
    """render_ref.Scene from the oracle model's hull arrays (the library's arrays are the same: tests/test_model_oracle.py)"""
    xyz = np.asarray(om["hull_xyz"], np.float64).reshape(-1, 3)
    return rr.Scene(xyz, om.get("hull_radius", np.zeros(len(xyz))), om["hull_group_start"], om["hull_start"], floor_z)


def condition(ref, eye, dirs):
    """The reference's rgb margin of a floor pixel is the distance of its hit point from the nearest checker line - in exact
    arithmetic. The kernel's hit point eye + t dir is f32: HP_ULPS ulps of its larger coordinate are taken off that distance,
    so that a pixel counts as decided only if f32 can decide it (2.4e-6 m at 5 m, 3e-5 m at 64 m, 1.9e-4 m at 400 m).
    -> the reference tuple with that rgb margin."""
    seg, dep, rgb, smg, rmg = ref
    hp = np.asarray(eye)[None, None, :2] + dep[..., None] * dirs[..., :2]
    res = HP_ULPS * 2.0 ** -23 * np.abs(hp).max(axis=-1)
    return seg, dep, rgb, smg, np.where(seg == -1, rmg - res, rmg)


def view_rays(c, W, H, base):
    """(eye, dirs) of a resolved Camera for an env whose base is at `base`"""
    eye, dirs, _ = rr.camera_rays(c.distance, c.yaw, c.pitch, c.fov, W, H, base if c.target is None else c.target)
    return eye, dirs


def reference(scene, R, p, base, cam, W, H):
    """render_ref.render of one view, conditioned: cam a CAMERAS-style tuple, base the env's base position (a follow-base
    camera's target)"""
    c = resolve(cam, R, p)
    eye, dirs = view_rays(c, W, H, base)
    return condition(rr.render(scene, R, p, eye, dirs, c.near, c.far), eye, dirs)


# ---------------------------------------------------------------- the conditions
def margin_shares(ref):
    """(share of pixels with seg_margin < MARGIN, smallest seg_margin, share with rgb_margin < MARGIN)"""
    sm, rm = ref[3], ref[4]
    return float((sm < MARGIN).mean()), float(sm.min()), float((rm < MARGIN).mean())


def qualify(ref, what, rgb_share=True):
    """The reference is decided on this view (module docstring). rgb_share False: the generated models, whose jittered plates
    are many nearly coplanar facets (the rgb comparison leaves those pixels out; seg and depth stay fully checked)."""
    H, W = ref[0].shape
    seg_share, seg_min, rgb_sh = margin_shares(ref)
    assert seg_share <= SEG_SHARE_CAP, (what, seg_share)
    if W * H < TINY_PIXELS:
        assert seg_min >= TINY_MARGIN, (what, seg_min)
    if rgb_share and W * H >= RGB_PIXELS:
        assert rgb_sh <= RGB_SHARE_CAP, (what, rgb_sh)
    assert (ref[4] >= MARGIN).any(), what          # (a 1 x 1 frame too leaves the colour comparison something to compare)


def paths_reached(name, cam, W, H, seg, depth, state=None):
    """What a picture of case `name` (camera tuple `cam`) must show for the case to reach its path; asserted on the reference (host test) and again
    on the GPU's own seg / depth. state: index into STATE_NAMES, None for a generated model.
    The counts of near_cuts, far_crops and the (1, 4096) strip are geometry of an animal STANDING on the floor under a camera
    that follows its base; the hanging reset state and the airborne random one are rendered and compared all the same, but
    their floor lies beyond far_crops' far plane and their legs hang elsewhere, so the counts are asked of STANDING only."""
    near, far = np.float32(cam[4]), np.float32(cam[5])
    seg, depth = np.asarray(seg), np.asarray(depth)
    body = seg >= 0
    at_near = depth.astype(np.float32) == near
    what = (name, W, H, state)
    if name == "inside":
        assert body.all() and at_near.all() and len(np.unique(seg)) == 1, what
    elif name == "below_floor":
        assert (seg == -1).all() and at_near.all(), what
    elif name == "all_sky":
        assert (seg == -2).all() and (depth.astype(np.float32) == far).all(), what
    standing = state in STANDING
    if name == "near_cuts" and (W, H) == MAIN_FRAME and standing:
        assert (body & at_near).sum() >= 600 and len(np.unique(seg[body])) >= 8, (what, (body & at_near).sum(), np.unique(seg[body]))
    if name == "far_crops" and (W, H) == MAIN_FRAME and standing:
        counts = [int(body.sum()), int((seg == -1).sum()), int((seg == -2).sum())]
        assert min(counts) >= 100 and depth.astype(np.float32).max() == far, (what, counts)
    if (W, H) == (1, 4096) and standing:
        assert body.sum() >= 500, (what, body.sum())


# ---------------------------------------------------------------- generated models with bent joints
SYNTH_MODELS = ("deep_chain", "bushy", "big_body", "full_masks")
SYNTH_FRAME = (49, 35)
SYNTH_LABELS = dict(deep_chain=6, bushy=12)      # bodies with a hull seen by the outside camera of the bent state, at least
SYNTH_TILT = (0.17, -0.11, 0.08)                 # rotation vector of the bent state's base, rad


def synth_extent(om):
    """largest distance of a hull vertex from the base origin at q = 0, by the oracle's own forward kinematics"""
    from oracle import oracle as O
    import synthetic_models as sm
    orc = O.Oracle(om)
    R, p, _ = oracle_poses(orc, sm.flat_state(om, 0.0))
    hs = np.asarray(om["hull_start"]).astype(int)
    xyz = np.asarray(om["hull_xyz"], np.float64).reshape(-1, 3)
    return max(float(np.linalg.norm(xyz[hs[b]:hs[b + 1]] @ R[b].T + p[b], axis=1).max()) for b in range(om["nb"]) if hs[b + 1] > hs[b])


# model -> (yaw of the outside camera, yaw of the close one): the first of a 20 degree grid at which the reference is decided on
# both states (seg share <= 0.0006) and, close, the near plane cuts at least 20 body pixels
SYNTH_YAW = dict(deep_chain=(40.0, 200.0), bushy=(300.0, 40.0), big_body=(40.0, 40.0), full_masks=(40.0, 40.0))


def synth_cameras(name, om):
    """{'outside', 'close'} CAMERAS-style tuples scaled to the model: outside at 2.5 x the extent, pitch -35, fov 55; close at
    0.6 x the extent, fov 90, with the near plane (0.25 m) through the bodies. deep_chain is 1.4 m long and 5 cm thick: 0.6 x
    its extent from the base the near plane meets nothing, so its close camera stands 0.3 m from the hull of its second link."""
    ext = synth_extent(om)
    yo, yc = SYNTH_YAW[name]
    close = (0.6 * ext, yc, -35.0, 90.0, 0.25, 50.0, None)
    if name == "deep_chain":
        close = (0.3, yc, -35.0, 90.0, 0.25, 50.0, ("target", 2, (0.11, 0.0, 0.0)))
    return {"outside": (2.5 * ext, yo, -35.0, 55.0, 0.1, 50.0, None), "close": close}


def synth_states(name, om, sampled):
    """[2, 13 + 2J] f32: the FIRST of the model's sampled states (tests/synthetic_models.py::state_set), and a bent one: base
    at z = 1 with a tilted quaternion, every joint at a random point of 10 .. 90 % of its range."""
    import synthetic_models as sm
    rng = np.random.default_rng(909 + len(name))
    lo, hi = np.asarray(om["q_lower"], np.float64), np.asarray(om["q_upper"], np.float64)
    q = lo + (hi - lo) * rng.uniform(0.1, 0.9, om["nb"])
    v = np.asarray(SYNTH_TILT)
    ang = np.linalg.norm(v)
    quat = tuple(np.sin(ang / 2) * v / ang) + (np.cos(ang / 2),)
    return np.stack([np.asarray(sampled[0], np.float64), sm.flat_state(om, 1.0, q, quat=quat)]).astype(np.float32)


SYNTH_RAY_HITS = 10        # of the 200 segments around the bent state, at least this many end on a body


def synth_segments(base, extent, count=200, seed=11):
    """[n, count, 6] f32 world segments, both ends within +-0.5 x the model's extent of each env's base [n, 3]"""
    rng = np.random.default_rng(seed)
    base = np.asarray(base, np.float64).reshape(-1, 1, 1, 3)
    ends = base + 0.5 * extent * rng.uniform(-1.0, 1.0, (base.shape[0], count, 2, 3))
    return ends.reshape(base.shape[0], count, 6).astype(np.float32)
