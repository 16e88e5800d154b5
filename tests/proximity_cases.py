"""Synthetic geometry cases of the proximity query (include/trex_batch.h, "proximity between bodies"): two world capsules per
case, designed in the world around a centre close to the base origin of the test state, then carried into the frames of two
bodies with the reference's f64 inverse pose at that state and rounded to f32 - what the batch's table holds. At the test state
the batch therefore sees the designed geometry up to that rounding (1e-8 m); at any other state it sees the two capsules in
general position, and is compared with the reference all the same.

Each case names the region of the (s, t) square its closest points lie in - "point" (a sphere), "end", "interior", or "any" where
the closest points are not unique (parallel axes that overlap lengthwise) - and tests/test_proximity_cases_host.py holds the
reference to it. The two `fallback` cases have axis distance 0: the normal is (0, 0, 1) by convention."""
import numpy as np

import dynamics_ref as R
import proximity_ref as PR

BODY_A, BODY_B = 0, 1        # the base and its first child: the shortest chains, so that the GPU's f32 poses keep the two
#                              fallback cases' axis distance (0 by design) below the 1e-6 m of the convention
ANGLES = [sg * a for a in (1e-2, 1e-3, 1e-4, 1e-5) for sg in (1, -1)]


def _cap(p0, p1, r):
    return (np.array(p0, np.float64), np.array(p1, np.float64), float(r))


def cases():
    """[dict(name, a, b: (p0, p1, radius) relative to the centre, region: (of s, of t), fallback)]"""
    out = []

    def add(name, a, b, region, fallback=False):
        out.append(dict(name=name, a=_cap(*a), b=_cap(*b), region=region, fallback=fallback))

    X0, X1 = (-0.3, 0, 0), (0.3, 0, 0)
    add("sphere_sphere", ((0, 0, 0), (0, 0, 0), 0.1), ((0.5, 0.2, 0.1), (0.5, 0.2, 0.1), 0.15), ("point", "point"))
    add("sphere_capsule_interior", ((0.05, 0.4, 0.1), (0.05, 0.4, 0.1), 0.1), (X0, X1, 0.05), ("point", "interior"))
    add("sphere_capsule_end", ((0.6, 0.3, 0), (0.6, 0.3, 0), 0.1), (X0, X1, 0.05), ("point", "end"))
    add("end_to_end", ((-0.5, 0, 0), (-0.1, 0, 0), 0.04), ((0.2, 0.1, 0), (0.6, 0.3, 0.1), 0.06), ("end", "end"))
    add("t_end_to_interior", ((0.02, 0.2, 0), (0.02, 0.6, 0.1), 0.05), (X0, X1, 0.07), ("end", "interior"))
    add("skew_interior_interior", (X0, X1, 0.05), ((0.05, -0.25, 0.3), (-0.02, 0.3, 0.28), 0.08), ("interior", "interior"))
    add("collinear", ((-0.5, 0, 0), (-0.1, 0, 0), 0.03), ((0.2, 0, 0), (0.6, 0, 0), 0.05), ("end", "end"))
    add("parallel_overlapping", (X0, X1, 0.05), ((-0.1, 0.25, 0), (0.5, 0.25, 0), 0.06), ("any", "any"))
    add("parallel_disjoint", (X0, X1, 0.05), ((0.5, 0.25, 0), (0.9, 0.25, 0), 0.06), ("end", "end"))
    mid = np.array([0.05, 0.2, 0.0])
    for th in ANGLES:
        c, s = np.cos(th), np.sin(th)
        # coplanar: B turned about z in the plane of A - the lines meet far away, the closest points are at an end of B
        u = 0.2 * np.array([c, s, 0.0])
        add("near_parallel_coplanar_%+.0e" % th, (X0, X1, 0.05), (mid - u, mid + u, 0.06), ("interior", "end"))
        # offset: B turned about the common perpendicular y - skew lines that pass each other at B's middle
        u = 0.2 * np.array([c, 0.0, s])
        add("near_parallel_offset_%+.0e" % th, (X0, X1, 0.05), (mid - u, mid + u, 0.06), ("interior", "interior"))
    add("crossing_axes", (X0, X1, 0.05), ((0, -0.3, 0), (0, 0.3, 0), 0.07), ("interior", "interior"), fallback=True)
    add("concentric_spheres", ((0, 0, 0), (0, 0, 0), 0.1), ((0, 0, 0), (0, 0, 0), 0.15), ("point", "point"), fallback=True)
    add("capsule_inside_capsule", (X0, X1, 0.3), ((-0.1, 0.05, 0.02), (0.1, 0.06, 0.03), 0.05), ("interior", "any"))
    add("radius_zero", (X0, X1, 0.0), ((0.05, -0.25, 0.3), (-0.02, 0.3, 0.28), 0.0), ("interior", "interior"))
    return out


def centre(state):
    """where the cases are built: a point 0.1 m from the base origin of the test state"""
    return np.asarray(state, np.float64)[0:3] + np.array([0.06, -0.05, 0.06])


def table(model, state, case):
    """(bodies [2], capsules [2, 7] f32-exact, pairs [(A, B)]) that put the case's two capsules where it designs them at `state`"""
    k = R.Kin(model, state)
    c = centre(state)
    rows = []
    for body, (p0, p1, r) in ((BODY_A, case["a"]), (BODY_B, case["b"])):
        inv = lambda x: k.R[body].T @ (c + x - k.p[body])
        rows.append(np.concatenate([inv(p0), inv(p1), [r]]))
    return np.array([BODY_A, BODY_B], np.int32), PR.round_table(rows), [(BODY_A, BODY_B)]


def region_of(u, sphere):
    if sphere:
        return "point"
    return "end" if u in (0.0, 1.0) else "interior"
