"""A generated, EXACTLY mirror-symmetric biped for the tests of the mirror maps (include/trex_symmetry.h): the T-rex asset is only
approximately symmetric, so exactness is tested here. Built with synthetic_models.Builder; a helper, not a conftest.

biped(directory, lateral): lateral 0 or 1 is the axis of URDF link 0's frame normal to the sagittal plane. Every right-hand number
is the left-hand one with the lateral component negated in the SAME decimal text, so the two sides agree to the last bit:
  * a trunk whose inertial frame is turned about the lateral axis (link 0's frame and body 0's differ by a rotation and an offset);
  * two legs of three hinges: hip about the lateral axis (sign +1), knee about an OBLIQUE axis behind a joint frame turned about
    the lateral axis (sign +1), ankle about the lateral axis with the right axis written negated (sign -1, limits mirrored);
  * a neck whose axis lies in the sagittal plane (self-paired, sign -1), a tail yaw about the vertical (self-paired, sign -1) and a
    tail pitch about the lateral axis behind it (self-paired, sign +1);
  * hulls whose vertices are mirrored exactly.
PLANTED lists the four mistakes of tests/symmetry_ref.py as keyword arguments for its builders."""
import numpy as np

from synthetic_models import SMALL_PARAMS, Builder

JOINTS = ["ankle_left", "ankle_right", "hip_left", "hip_right", "knee_left", "knee_right", "neck", "tail_pitch", "tail_yaw"]   # sorted
PAIR = [1, 0, 3, 2, 5, 4, 6, 7, 8]
SIGN = [-1, -1, 1, 1, 1, 1, -1, 1, -1]
NB, NJ = 10, 9
FOOT_POINT = (0.03, 0.05, -0.02)      # (lateral, forward, up) of the LEFT probe in its shank's frame

# the planted mistakes: (name, keyword arguments of symmetry_ref.model_table, of symmetry_ref.row_table)
PLANTED = [("wrong_sign", dict(wrong_sign=4), {}), ("swapped_pair", dict(swapped_pair=2), {}),
           ("unmirrored_probe", {}, dict(unmirrored_probe=True)), ("axial_as_polar", {}, dict(axial_as_polar=True))]


def _frame(lateral):
    """(lateral, forward, up) -> xyz of link 0's frame"""
    return (lambda l, f, u: (l, f, u)) if lateral == 0 else (lambda l, f, u: (f, l, u))


def biped(directory, lateral=0):
    assert lateral in (0, 1)
    P = _frame(lateral)
    rng = np.random.default_rng(220 + lateral)
    b = Builder(directory, "biped_lat%d" % lateral)
    about_lateral = lambda angle: P(angle, 0.0, 0.0)      # rpy of a turn about the lateral axis (roll for x, pitch for y)

    def half_box(half, centre):
        """box corners, jittered, the lateral-negative half the exact image of the positive half: (left set, right set) for a
        paired link take [pos | neg] and its image; a self-paired link takes it as it is"""
        hl, hf, hu = half
        pos = np.array([[hl, f * hf, u * hu] for f in (-1, 1) for u in (-1, 1)], float) + rng.uniform(-2e-4, 2e-4, (4, 3))
        inner = np.array([[-hl, f * hf, u * hu] for f in (-1, 1) for u in (-1, 1)], float) + rng.uniform(-2e-4, 2e-4, (4, 3))
        return pos + np.asarray(centre), inner + np.asarray(centre)

    def xyz(v, side=1.0):
        """rows (lateral, forward, up), the lateral component times side -> xyz"""
        v = np.atleast_2d(np.asarray(v, float)) * np.array([side, 1.0, 1.0])
        return np.stack(P(v[:, 0], v[:, 1], v[:, 2]), 1)

    def self_paired(name, mass, half, com_fu, centre_fu):
        pos, _ = half_box(half, (0.0,) + tuple(centre_fu))
        pos[:, 0] = np.abs(pos[:, 0])
        verts = np.concatenate([xyz(pos), xyz(pos, -1.0)])
        b.link(name, mass, P(*half), com=P(0.0, *com_fu), com_rpy=about_lateral(0.1 if name == "trunk" else 0.0),
               hulls=[(verts, (0, 0, 0), (0, 0, 0))])

    self_paired("trunk", 6.0, (0.10, 0.20, 0.08), (0.012, -0.015), (0.0, 0.0))
    parts = dict(thigh=(1.6, (0.03, 0.04, 0.12), (0.008, 0.004, -0.12)), shank=(1.1, (0.025, 0.03, 0.12), (-0.004, 0.006, -0.11)),
                 foot=(0.7, (0.04, 0.10, 0.02), (0.006, 0.03, -0.02)))
    hulls = {n: half_box(h, (0.0, c[1], c[2])) for n, (_, h, c) in parts.items()}
    for side, tag in ((1.0, "left"), (-1.0, "right")):
        for n, (mass, half, com) in parts.items():
            verts = np.concatenate(hulls[n])
            b.link("%s_%s" % (n, tag), mass, P(*half), com=tuple(xyz(com, side)[0]), hulls=[(xyz(verts, side), (0, 0, 0), (0, 0, 0))])
        ax = lambda v: tuple(xyz(v)[0])
        oblique = np.array([0.9, 0.3, 0.2])
        b.joint("hip_" + tag, "trunk", "thigh_" + tag, xyz=tuple(xyz((0.13, 0.02, -0.07), side)[0]), axis=ax((1.0, 0.0, 0.0)),
                lower=-0.9, upper=0.7, damping=0.01)
        # the image of an axial vector a is -S a: the lateral component stays, the other two change sign
        b.joint("knee_" + tag, "thigh_" + tag, "shank_" + tag, xyz=tuple(xyz((0.01, 0.015, -0.25), side)[0]), rpy=about_lateral(0.2),
                axis=ax(oblique * (1.0 if side > 0 else np.array([1.0, -1.0, -1.0]))), lower=-0.2, upper=1.3, damping=0.02)
        lim = (-0.5, 0.8) if side > 0 else (-0.8, 0.5)
        b.joint("ankle_" + tag, "shank_" + tag, "foot_" + tag, xyz=tuple(xyz((0.0, -0.01, -0.24), side)[0]), axis=ax((side, 0.0, 0.0)),
                lower=lim[0], upper=lim[1], damping=0.01)
    self_paired("head", 0.9, (0.05, 0.07, 0.05), (0.05, 0.03), (0.05, 0.03))
    self_paired("tail_a", 0.8, (0.04, 0.10, 0.03), (-0.10, 0.0), (-0.10, 0.0))
    self_paired("tail_b", 0.5, (0.03, 0.10, 0.02), (-0.10, 0.005), (-0.10, 0.0))
    b.joint("neck", "trunk", "head", xyz=P(0.0, 0.21, 0.09), axis=P(0.0, 0.6, 0.8), lower=-0.6, upper=0.6, damping=0.01)
    b.joint("tail_yaw", "trunk", "tail_a", xyz=P(0.0, -0.21, 0.02), axis=P(0.0, 0.0, 1.0), lower=-0.7, upper=0.7, damping=0.01)
    b.joint("tail_pitch", "tail_a", "tail_b", xyz=P(0.0, -0.2, 0.0), rpy=about_lateral(-0.15), axis=P(1.0, 0.0, 0.0), lower=-0.4, upper=0.9,
            damping=0.01)
    return b.write(), dict(nb=NB, lateral=lateral, pair=PAIR, sign=SIGN, joints=JOINTS, params=SMALL_PARAMS)


def compile_biped(directory, lateral=0):
    """-> (urdf path, props, oracle model dict)"""
    from oracle import trex_model as tm
    path, props = biped(directory, lateral)
    return path, props, tm.compile_model(path)


def locomotion_channels(model, lateral, probe=FOOT_POINT):
    """a `locomotion`-style specification on the biped - gravity, base velocities, base height, and per foot a contact force and a
    probe with position, velocity and height - as (kind, link, local_xyz, scale) tuples; the right probe is the left one's image"""
    import symmetry_ref as R
    P = _frame(lateral)
    chans = [(R.PROJECTED_GRAVITY, 0, (0, 0, 0), 1.0), (R.BASE_LINEAR_VELOCITY, 0, (0, 0, 0), 1.0), (R.BASE_ANGULAR_VELOCITY, 0, (0, 0, 0), 0.5),
             (R.BASE_HEIGHT, 0, (0, 0, 0), 1.0)]
    for side, tag in ((1.0, "left"), (-1.0, "right")):
        link = model["link_names"].index("shank_" + tag)
        xyz = tuple(float(v) for v in P(side * probe[0], probe[1], probe[2]))
        chans += [(R.CONTACT_FORCE, model["link_names"].index("foot_" + tag), (0, 0, 0), 1.0), (R.POINT_POSITION, link, xyz, 1.0),
                  (R.POINT_VELOCITY, link, xyz, 0.25), (R.POINT_HEIGHT, link, xyz, 1.0)]
    return chans


def random_states(model, count, seed=0, lateral=0):
    """[count, 13 + 2 J] states: a base pose with a tilt, velocities, joint angles within the limits (observation order)"""
    rng = np.random.default_rng(seed)
    nj, oo = model["nb"] - 1, model["obs_order"]
    out = np.zeros((count, 13 + 2 * nj))
    for s in out:
        s[0:3] = rng.uniform(-0.5, 0.5, 3) + (0, 0, 1.0)
        q = rng.normal(size=4) * (0.25, 0.25, 0.25, 1.0)
        s[3:7] = q / np.linalg.norm(q)
        s[7:13] = rng.uniform(-1.0, 1.0, 6)
        s[13:13 + nj] = rng.uniform(model["q_lower"][oo], model["q_upper"][oo])
        s[13 + nj:] = rng.uniform(-2.0, 2.0, nj)
    return out


def lowest_vertex(model, state):
    """world z of the lowest hull vertex in `state`"""
    import dynamics_ref as D
    k = D.Kin(model, state)
    hs = model["hull_start"]
    return min((k.p[b] + model["hull_xyz"][hs[b]:hs[b + 1]] @ k.R[b].T)[:, 2].min() for b in range(model["nb"]) if hs[b + 1] > hs[b])


def step_states(model, lateral=0, seed=21):
    """16 states for the oracle-step test with their kind: 6 airborne (tilted, moving), 5 standing on both feet, 5 with one foot down
    (the other leg drawn up at hip and knee). A state on the floor is placed with its lowest hull vertex a few millimetres above
    the floor, inside the contact margin. -> [(kind, state)]"""
    rng = np.random.default_rng(seed)
    nj, oo = model["nb"] - 1, model["obs_order"]
    names = model["obs_joint_names"]
    out = []
    for k in range(16):
        kind = "airborne" if k < 6 else "standing" if k < 11 else "one_foot"
        s = np.zeros(13 + 2 * nj)
        q = rng.uniform(-0.08, 0.08, nj)
        if kind == "airborne":
            s[0:3] = rng.uniform(-0.3, 0.3, 3) + (0, 0, 1.5)
            quat = rng.normal(size=4) * (0.2, 0.2, 0.2, 1.0)
            s[7:13] = rng.uniform(-0.8, 0.8, 6)
            q = rng.uniform(model["q_lower"][oo], model["q_upper"][oo]) * 0.7
        else:
            s[0:3] = (rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 0.645 + rng.uniform(0.0, 0.008))
            quat = np.concatenate([rng.normal(size=3) * 0.01, [1.0]])
            s[7:13] = rng.uniform(-0.05, 0.05, 6)
            if kind == "one_foot":
                side = "left" if k % 2 else "right"
                q[names.index("hip_" + side)] = -0.6
                q[names.index("knee_" + side)] = 1.0
        s[3:7] = quat / np.linalg.norm(quat)
        s[13:13 + nj] = q
        s[13 + nj:] = rng.uniform(-0.3, 0.3, nj)
        if kind != "airborne":      # the lowest hull vertex a few millimetres above the floor: inside the contact margin
            s[2] += 0.0005 + rng.uniform(0.001, 0.006) - lowest_vertex(model, s)
        out.append((kind, s))
    return out
