"""The renderer's edge cases (tests/render_cases.py) on the f64 reference caster alone, before a GPU sees them (no GPU here): every
(camera, frame, state) is DECIDED - few pixels near a change of label or colour, none at all in a tiny frame - and REACHES the path
it is named for. Poses by the f64 oracle, the scene by qhull on the oracle model's hull arrays (tests/render_ref.py).

What tests/test_gpu_render_edges.py compares on the GPU is only as good as these cases: render_compare leaves out the pixels whose
reference margin is below 1e-4 m, so a case is fair only if that leaves nearly all of them in."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cases as rc  # noqa: E402
import synthetic_models as sm  # noqa: E402


@pytest.fixture(scope="module")
def trex(model, oracle64):
    """states, their f64 poses, and the scene per collision kind: computed once, shared, never changed"""
    from oracle import trex_model as tm
    states = rc.trex_states(oracle64)
    fz = oracle64.params["floor_z"]
    return dict(states=states, poses=[rc.oracle_poses(oracle64, s) for s in states],
                scenes=dict(hulls=rc.oracle_scene(model, fz), primitives=rc.oracle_scene(tm.use_primitive_collision(model, 0.2), fz)))


def test_states_are_what_the_table_says(trex, oracle64):
    st = trex["states"]
    assert st.shape == (5, 63) and st.dtype == np.float32
    assert abs(st[0, 2] - 3.0) < 1e-3                                    # reset: the base hangs at z = 3
    np.testing.assert_allclose(st[4, :3] - st[1, :3], rc.BASE_SHIFT, atol=1e-5)
    assert (st[4, 3:] == st[1, 3:]).all()
    fz = oracle64.params["floor_z"]
    for k, (R, p, _) in enumerate(trex["poses"]):
        hs = oracle64.model["hull_start"]
        low = min((oracle64.model["hull_xyz"][hs[b]:hs[b + 1]] @ R[b].T + p[b])[:, 2].min() for b in range(oracle64.nb) if hs[b + 1] > hs[b])
        assert (low - fz < 0.05) == (k in rc.STANDING), (k, low)         # standing: a hull vertex within 5 cm of the floor


CASES = [("hulls", n) for n in rc.CAMERAS] + [("primitives", n) for n in rc.PRIMITIVE_CAMERAS]


@pytest.mark.parametrize("collision,name", CASES)
def test_trex_cases_qualify_on_the_reference(collision, name, trex):
    scene = trex["scenes"][collision]
    for (W, H) in rc.frames(name):
        cam = rc.case_camera(name, collision, (W, H))
        for k, (R, p, base) in enumerate(trex["poses"]):
            ref = rc.reference(scene, R, p, base, cam, W, H)
            what = (collision, name, W, H, rc.STATE_NAMES[k])
            seg_share, seg_min, rgb_share = rc.margin_shares(ref)
            print("%s: seg share %.4f min margin %.1e rgb share %.4f; body %d floor %d sky %d"
                  % (what, seg_share, seg_min, rgb_share, (ref[0] >= 0).sum(), (ref[0] == -1).sum(), (ref[0] == -2).sum()))
            rc.qualify(ref, what)
            rc.paths_reached(name, cam, W, H, ref[0], ref[1], k)


def test_exact_cases_have_exact_colours(trex):
    """all_sky on the reference is the sky colour everywhere (what the GPU test asserts bytewise)"""
    R, p, base = trex["poses"][1]
    ref = rc.reference(trex["scenes"]["hulls"], R, p, base, rc.case_camera("all_sky"), 33, 41)
    assert (ref[2] == np.array(rc.SKY_RGB, np.uint8)).all()


def test_moved_cameras_and_nudges_are_needed():
    """the table moves a camera only where it says it must: every nudge is of a frame under 400 pixels, by at most 6 degrees"""
    for (collision, name, frame), (dy, dp) in rc.NUDGE.items():
        assert frame in rc.frames(name) and frame[0] * frame[1] < rc.TINY_PIXELS and max(abs(dy), abs(dp)) <= 6.0
        assert collision == "hulls" or name in rc.PRIMITIVE_CAMERAS
    for name in rc.CAMERAS:
        yaw = rc.CAMERAS[name][1]
        assert name == "inside" or min(yaw % 90.0, 90.0 - yaw % 90.0) >= 10.0, name     # (inside sees no floor)


# ---------------------------------------------------------------- the generated models with bent joints
@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    from oracle import oracle as O
    out = {}
    for n in rc.SYNTH_MODELS:
        path, props, om = sm.compile_both(n, tmp_path_factory.mktemp(n))
        orc = O.Oracle(om, params=props["params"])
        states = rc.synth_states(n, om, sm.state_set(n, om, props["params"])["states"])
        out[n] = dict(om=om, orc=orc, states=states, scene=rc.oracle_scene(om, orc.params["floor_z"]), cams=rc.synth_cameras(n, om))
    return out


@pytest.mark.parametrize("name", rc.SYNTH_MODELS)
def test_generated_models_qualify_on_the_reference(name, synth):
    """seg / depth conditions as for the T-rex. The rgb share is not asked: big_body's jittered underside is many nearly coplanar
    facets, and a third of its pixels lie within 1e-4 m of the edge between two of them."""
    m = synth[name]
    om = m["om"]
    W, H = rc.SYNTH_FRAME
    hulled = [b for b in range(om["nb"]) if om["hull_start"][b + 1] > om["hull_start"][b]]
    # the bent state is bent: every joint 10 .. 90 % of its range, the base tilted and clear of the floor
    J = om["nb"] - 1
    q = m["states"][1][13:13 + J].astype(np.float64)
    lo, hi = om["q_lower"][om["obs_order"]], om["q_upper"][om["obs_order"]]
    frac = (q - lo) / (hi - lo)
    assert frac.min() >= 0.1 - 1e-6 and frac.max() <= 0.9 + 1e-6 and abs(m["states"][1][6]) < 0.999
    for e, st in enumerate(m["states"]):
        R, p, base = rc.oracle_poses(m["orc"], st)
        for cname, cam in m["cams"].items():
            ref = rc.reference(m["scene"], R, p, base, cam, W, H)
            what = (name, cname, ("sampled", "bent")[e])
            seg_share, seg_min, rgb_share = rc.margin_shares(ref)
            labels = set(ref[0][ref[0] >= 0])
            print("%s: seg share %.4f min margin %.1e rgb share %.4f; labels %d of %d; at near %d"
                  % (what, seg_share, seg_min, rgb_share, len(labels), len(hulled), (ref[1] == cam[4]).sum()))
            rc.qualify(ref, what, rgb_share=False)
            if cname == "close":
                assert ((ref[0] >= 0) & (ref[1] == cam[4])).sum() >= 20, what        # the near plane cuts a body
            if cname == "outside" and e == 1:
                assert labels <= set(hulled)
                assert len(labels) >= rc.SYNTH_LABELS.get(name, 2), (what, sorted(labels))
                if name == "deep_chain":
                    assert labels == set(hulled), (what, sorted(labels))                 # every hull-bearing body: all 6


@pytest.mark.parametrize("name", ["deep_chain", "bushy"])
def test_ray_segments_of_the_bent_models_qualify(name, synth):
    """the segments tests/test_gpu_render_edges.py casts at these models: at most 2 % marginal (the cap of tests/ray_ref.py), and
    enough of them end on a body of the bent state"""
    import ray_ref as ry
    m = synth[name]
    rays = rc.synth_segments(m["states"][:, :3], rc.synth_extent(m["om"])).astype(np.float64)
    for e, st in enumerate(m["states"]):
        R, p, _ = rc.oracle_poses(m["orc"], st)
        _, lab, _, _, mg, _ = ry.cast(m["scene"], R, p, rays[e, :, :3], rays[e, :, 3:])
        print("%s %s: body hits %d floor %d marginal %.4f" % (name, ("sampled", "bent")[e], (lab >= 0).sum(), (lab == -1).sum(), (mg < ry.MARGIN).mean()))
        assert (mg < ry.MARGIN).mean() <= ry.MARGINAL_CAP, (name, e)
        if e == 1:
            assert (lab >= 0).sum() >= rc.SYNTH_RAY_HITS, (name, (lab >= 0).sum())
