"""CPU checks of the generated models (tests/synthetic_models.py): the C++ loader and the oracle's model compiler agree on every
one of them; each model has, by the compiled arrays and the documented rules of device_model.h restated in synthetic_models.py,
the property it was built for; the loader refuses what lies one step outside the limits; and the state sets the GPU tests step
from contain - by Oracle.contacts alone - the contact situations they are meant to.

A one-link URDF (no joints) LOADS: one body, zero joints, empty joint list (asserted below)."""
import numpy as np
import pytest

import synthetic_models as sm

ARRAYS = ["parent", "depth", "joint_axis", "joint_pos", "joint_rot", "q_lower", "q_upper", "joint_damping", "mass", "com",
          "inertia", "obs_order", "head_point", "hull_xyz", "hull_start", "hull_group_start", "sphere_center", "sphere_radius",
          "q_start", "base_start_pos", "base_start_quat", "revolute_joint_indices", "link_body", "link_tf"]


@pytest.fixture(scope="module")
def capi():
    from trex_gym import _capi
    return _capi


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (urdf path, props, oracle model)"""
    return {n: sm.compile_both(n, tmp_path_factory.mktemp(n)) for n in list(sm.MODELS) + list(sm.KINEMATIC_MODELS)}


@pytest.fixture(scope="module")
def sets(built):
    return {n: sm.state_set(n, om, props["params"]) for n, (_, props, om) in built.items()}


@pytest.fixture(scope="module")
def contacts(built, sets):
    """name -> per state, the (body, lambda, position, distance) arrays of Oracle.contacts after one env-step"""
    from oracle import oracle as O
    out = {}
    for n, (_, props, om) in built.items():
        orc = O.Oracle(om, params=props["params"])
        out[n] = [sm.oracle_step_contacts(orc, s, a)[2] for s, a in zip(sets[n]["states"], sets[n]["actions"])]
    return out


@pytest.mark.parametrize("name", list(sm.MODELS) + list(sm.KINEMATIC_MODELS))
def test_loader_matches_the_oracle_compiler(name, capi, built):
    path, props, om = built[name]
    m = capi.Model(path)
    assert m.num_bodies == om["nb"] == props["nb"] and m.num_joints == om["nb"] - 1
    assert m.joint_names == om["obs_joint_names"]
    assert m.urdf_joint_indices == list(om["revolute_joint_indices"])
    assert abs(m.total_mass(True) - om["total_mass"]) < 1e-9
    for k in ARRAYS:
        got, want = m.array(k), np.asarray(om[k], float).reshape(-1)
        assert got.shape == want.shape, k
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg=k)
    assert int(m.array("head_body")[0]) == om["head_body"] == 0        # no head link: the reward point is the base COM
    np.testing.assert_allclose(om["head_point"], om["com"][0])
    assert [n for n, _ in m.links()] == om["link_names"]
    for k, v in props["params"].items():
        m.set_param(k, v)
        assert m.get_param(k) == v
    # unit axes out of non-unit <axis> elements
    np.testing.assert_allclose(np.linalg.norm(om["joint_axis"][1:], axis=1), 1.0, atol=1e-12)


def test_properties_from_the_compiled_arrays(built):
    verts = {n: list(np.diff(om["hull_start"])) for n, (_, _, om) in built.items()}
    groups = {n: int((np.diff(om["hull_group_start"]) > 0).sum()) for n, (_, _, om) in built.items()}
    for n, (_, props, om) in built.items():
        par, depth = om["parent"], om["depth"]
        assert om["nb"] <= sm.MAX_BODIES and depth.max() == props["depth"] <= sm.MAX_DEPTH, n
        assert np.bincount(par[1:], minlength=om["nb"]).max() <= sm.MAX_CHILDREN, n
        assert np.all(par[1:] < np.arange(1, om["nb"])) and np.all(depth[1:] == depth[par[1:]] + 1), n
        assert groups[n] <= 512, n                                         # drawable primitives of the renderer
    # deep_chain: the sixth level, a hull-less body inside the chain, oblique axes, rotated joint frames
    om = built["deep_chain"][2]
    assert list(om["depth"]) == [0, 1, 2, 3, 4, 5, 6] and sm.MAX_DEPTH == 6
    assert verts["deep_chain"][3] == 0 and all(v > 0 for i, v in enumerate(verts["deep_chain"]) if i != 3)
    assert np.all(np.sort(np.abs(om["joint_axis"][1:]), axis=1)[:, 1] > 0.02)        # at least two components: no axis is +-x, y, z
    assert all(np.abs(om["joint_rot"][i].reshape(3, 3) - np.eye(3)).max() > 0.04 for i in range(1, 7))
    assert list(om["obs_order"]) != sorted(om["obs_order"])
    # big_body: one body over 1024 vertices -> swept by size although every mask word is free
    v = verts["big_body"]
    assert v[0] == built["big_body"][1]["big_vertices"] > 1024 and max(v[1:]) <= 256
    assert sm.swept_bodies(v) == built["big_body"][1]["swept"] == [0]
    assert sum(w for w, _ in sm.mask_plan(v)) == 8 * 5 <= sm.CM_WORDS
    assert 2 <= len(v) - 1 <= 6
    # full_masks: ten 32-word bodies take all 320 words; the eleventh and the small twelfth find no room
    v = verts["full_masks"]
    plan = sm.mask_plan(v)
    assert all(256 < x <= 1024 for x in v[:11]) and 0 < v[11] <= 256
    assert [w for w, _ in plan] == [32] * 10 + [0, 0] and plan[9][1] + 32 == sm.CM_WORDS
    assert np.cumsum([w for w, _ in plan])[-1] == sm.CM_WORDS
    assert sm.swept_bodies(v) == built["full_masks"][1]["swept"] == [10, 11]
    # the T-rex rule for comparison: one 32-word and 23 8-word bodies = 216 words
    assert sum(w for w, _ in sm.mask_plan([840] + [200] * 23 + [0, 0])) == 216
    # many_hulls: more hull groups than scan-unit lanes, several per body -> one unit per body
    v = verts["many_hulls"]
    assert groups["many_hulls"] == built["many_hulls"][1]["hull_groups"] > sm.MAX_UNITS
    assert sm.scan_units(v, groups["many_hulls"]) == (6, True)
    gs, hs = built["many_hulls"][2]["hull_group_start"], built["many_hulls"][2]["hull_start"]
    assert all(((gs[:-1] >= hs[b]) & (gs[:-1] < hs[b + 1])).sum() == 6 for b in range(6))
    for n in ("deep_chain", "big_body", "full_masks", "bushy", "slab"):
        assert not sm.scan_units(verts[n], groups[n])[1], n
    # bushy: 26 bodies, 4 moving children on the base and on a body at depth 2, depth 6, merged links, hull-less leaves
    _, props, om = built["bushy"]
    nchild = np.bincount(om["parent"][1:], minlength=26)
    four = np.flatnonzero(nchild == 4)
    assert om["nb"] == 26 and sorted(om["depth"][four]) == props["four_children_depths"] == [0, 2]
    assert [om["body_names"][b] for b in four] == props["four_children"]
    assert om["n_merged"].sum() - 26 == props["merged_links"] == 6 and len(om["link_names"]) == 32
    leaves = [b for b in range(26) if nchild[b] == 0]
    bare = [b for b in range(26) if verts["bushy"][b] == 0]
    assert sorted(om["body_names"][b] for b in bare) == props["hull_less"] and set(bare) < set(leaves) and len(bare) < len(leaves)
    assert om["depth"].max() == 6
    # slab
    assert built["slab"][2]["nb"] == 2 and abs(built["slab"][2]["mass"].sum() - built["slab"][1]["total_mass"]) < 1e-12


@pytest.mark.parametrize("kind,word", [("depth7", "deeper than 6"), ("children5", "more than 4 moving children"),
                                       ("bodies27", "26")])
def test_models_outside_the_limits_are_refused(kind, word, capi, tmp_path):
    with pytest.raises(capi.TrexError) as e:
        capi.Model(sm.refused(tmp_path, kind))
    assert e.value.code == -4 and word in str(e.value)                     # TREX_E_UNSUPPORTED


def test_one_link_urdf_loads(capi, tmp_path):
    m = capi.Model(sm.refused(tmp_path, "one_link"))
    assert m.num_bodies == 1 and m.num_joints == 0 and m.joint_names == []
    assert len(m.array("hull_xyz")) == 24 and list(m.array("hull_start")) == [0, 8]


@pytest.mark.parametrize("name", list(sm.MODELS))
def test_state_sets_are_deterministic_and_mostly_kept(name, built, sets):
    _, props, om = built[name]
    ss = sets[name]
    assert 10 <= ss["total"] <= 41 and ss["dropped"] <= 0.1 * ss["total"], (ss["dropped"], ss["total"])
    again = sm.state_set(name, om, props["params"])
    assert again["states"].tobytes() == ss["states"].tobytes() and again["actions"].tobytes() == ss["actions"].tobytes()
    floor = 0.0005
    assert ss["states"][:, 2].min() > floor                                 # the base frame never starts below the floor


def test_state_sets_hold_the_contact_situations(built, sets, contacts):
    def per_state(name):
        return [dict(zip(*np.unique(c[0], return_counts=True))) for c in contacts[name]]
    # every model: airborne, landing and resting states
    for n in sm.MODELS:
        counts = [len(c[0]) for c in contacts[n]]
        assert min(counts) == 0 and max(counts) >= 4, n
        assert counts[-1] > 0, n
    # big_body: the swept plate keeps 2, 3 and 4 points, alone and with 1, 2 - 3 and 4 - 5 other bodies - and these are the RESTING
    # combinations: the last state of the scenario with flaps `down` level has exactly the plate and those flaps touching
    from oracle import oracle as O
    _, props, om = built["big_body"]
    big = [d for d in per_state("big_body") if 0 in d]
    assert {d[0] for d in big} >= {2, 3, 4}
    orc = O.Oracle(om, params=props["params"])
    scen = sets["big_body"]["scenario"]
    at_rest = {}
    for i, down in enumerate(sm.BIG_DOWN):
        k = np.flatnonzero(scen == i)[-1]
        assert set(per_state("big_body")[k]) == {0} | {f + 1 for f in down}, (i, per_state("big_body")[k])
        at_rest[len(down)] = (per_state("big_body")[k][0], sm.lane_loads(orc, om, sets["big_body"]["states"][k]))
    assert {n: v[0] for n, v in at_rest.items()} == {0: 4, 1: 4, 2: 4, 3: 3, 4: 2, 5: 2}
    assert [at_rest[n][1]["GS"] for n in range(6)] == [64, 32, 16, 16, 8, 8]
    for n, (_, ll) in at_rest.items():
        # swept, and the dense underside inside the margin: more than 4 vertices for every lane of any group - the non-cached passes
        assert ll["form"] == "swept" and ll["in_margin"][0] > 1000 > 4 * 64 and 0 not in ll["per_lane"], n
    # full_masks: (a) masked 32-word bodies touching ALONE - no swept body in contact, so the masks are read - in every lane-group
    # size, in the cached form (every lane owns at most 4 in-margin vertices) and in the re-reading form, at K = 2, 3 and 4
    _, props, om = built["full_masks"]
    orc = O.Oracle(om, params=props["params"])
    fm = per_state("full_masks")
    loads = [sm.lane_loads(orc, om, s) for s in sets["full_masks"]["states"]]
    seen = set()
    for d, ll in zip(fm, loads):
        if ll["form"] in ("cached", "reread") and set(d) == set(ll["active"]) and all(d[b] == ll["K"] for b in d):
            assert max(ll["active"]) <= 9 and min(ll["per_lane"].values()) >= 1
            assert (max(ll["per_lane"].values()) <= 4) == (ll["form"] == "cached")
            seen.add((ll["GS"], ll["form"], ll["K"]))
    assert {(g, f) for g, f, _ in seen} == {(g, f) for g in (64, 32, 16, 8) for f in ("cached", "reread")}, seen
    for form in ("cached", "reread"):
        assert {k for _, f, k in seen if f == form} == {2, 3, 4}, seen
    assert any(1 <= b <= 9 for d, ll in zip(fm, loads) if ll["form"] != "one" for b in ll["active"])     # mask offsets beyond word 32
    assert {tuple(ll["active"]) for ll in loads if ll["form"] == "reread"} >= {tuple(t) for t in sm.FULL_FLAT}
    assert {tuple(ll["active"]) for ll in loads if ll["form"] == "cached"} >= {tuple(t) for t in sm.FULL_LEGS}
    # (b) both bodies swept for lack of room hold contacts: one point each among all 12, four each next to the masked hub
    assert {d[10] for d in fm if 10 in d} >= {1, 4} and {d[11] for d in fm if 11 in d} >= {1, 4}
    assert any(ll["form"] == "swept" and 0 in ll["active"] and 10 in ll["active"] for ll in loads)
    assert any(len(d) == 12 for d in fm)
    # deep_chain: the body at depth 6 and the bodies on both sides of the hull-less one touch; the hull-less one never does
    dc = per_state("deep_chain")
    assert any(6 in d for d in dc)
    assert any(2 in d and 4 in d for d in dc) and not any(3 in d for d in dc)
    # many_hulls: every body touches in some state
    assert set().union(*[set(d) for d in per_state("many_hulls")]) == set(range(6))
    # bushy: more touching bodies than max_contacts - an oracle with twice the budget lists more than 13 bodies where
    # the model's own lists exactly 13, one point each
    _, props, om = built["bushy"]
    wide = O.Oracle(om, params=dict(props["params"], max_contacts=26))
    over = 0
    for s, a, c in zip(sets["bushy"]["states"], sets["bushy"]["actions"], contacts["bushy"]):
        nwide = len(set(sm.oracle_step_contacts(wide, s, a)[2][0]))
        if nwide > 13:
            assert len(c[0]) == 13 == len(set(c[0]))
            over += 1
    assert over >= 3
    # slab: box and flap both flat on the floor
    assert per_state("slab")[-1] == {0: 4, 1: 4}
