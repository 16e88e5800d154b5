"""CPU checks that keep tests/test_gpu_dynamics_models.py from being vacuous. The bounds of tests/dynamics_model_cases.py come
from the reference's f32 run alone and lie under the caps; they TELL: each of four deliberate model mistakes - a leaf's mass dropped,
link_tf ignored, one joint-origin rotation ignored, two observation slots swapped - moves the f64 reference by at least 100 x the
bound on every model and metric it applies to, and the table of where each applies is asserted, so that a mistake which silently
stops applying fails here; the reference obeys, exactly, the structure the GPU test demands of the device outputs; the reference
agrees with each model's own oracle; and the models are what they were chosen for."""
import numpy as np
import pytest

import dynamics_model_cases as DC
import dynamics_ref as R
from state_sets import built_models, oracle_state
from tolerances import DYNAMICS_CAPS as CAPS, DYNAMICS_TOL as TOL

SEPARATION = 100.0
ALL, NO_JAC = DC.METRICS, tuple(k for k in DC.METRICS if k != "jac")
TREES = ("deep_chain", "bushy", "mount_first")
# (mistake, model) -> the metrics it moves. The mass of a body is not in a Jacobian; link_tf is in nothing else; on slab the one
# joint's origin is not turned, every link frame is its body's, and one joint has no other order
APPLIES = {("leaf_mass", m): NO_JAC for m in DC.MODELS}
APPLIES.update({("link_tf", m): ("jac",) for m in TREES})
APPLIES.update({("joint_rot", m): ALL for m in TREES})
APPLIES.update({("obs_slots", m): ALL for m in TREES})


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return built_models(DC.MODELS, tmp_path_factory)


@pytest.mark.parametrize("name", DC.MODELS)
def test_bounds_come_from_the_f32_run_and_lie_under_the_caps(name, built):
    c = DC.case(name, built[name])
    assert all(v.dtype == np.float32 for v in c["ref32"].values()) and all(v.dtype == np.float64 for v in c["ref"].values())
    print("%s d32:   %s" % (name, {k: "%.3g" % c["d32"][k] for k in DC.METRICS}))
    print("%s bound: %s" % (name, {k: "%.3g" % c["bound"][k] for k in DC.METRICS}))
    print("%s identities of the f32 run: %s, bounds %s" % (name, {k: "%.3g" % v for k, v in c["res32"].items()},
                                                           {k: "%.3g" % v for k, v in c["id_bound"].items()}))
    for k in DC.METRICS:
        assert 0 < c["d32"][k] < CAPS[k], (name, k, c["d32"][k])
        assert c["bound"][k] == min(CAPS[k], max(TOL[k], 4 * c["d32"][k])) and TOL[k] <= c["bound"][k] <= CAPS[k]
    for k in DC.IDENTITIES:
        assert 0 < c["res32"][k] and c["id_bound"][k] <= 1e-4, (name, k)


def test_the_bounds_tell(built):
    applies, reached = {}, {k: set() for k in DC.METRICS}
    for name in DC.MODELS:
        c = DC.case(name, built[name])
        for mk in DC.MISTAKES:
            d = DC.mistake_devs(c, mk)
            print("%-11s %-9s %s" % (name, mk, {k: "%.3g = %.0f x bound" % (v, v / c["bound"][k]) for k, v in d.items() if v}))
            moved = tuple(k for k in DC.METRICS if d[k] != 0.0)
            if moved:
                applies[(mk, name)] = moved
            for k in moved:
                assert d[k] >= SEPARATION * c["bound"][k], (name, mk, k, d[k], c["bound"][k])
                reached[k].add(mk)
    assert applies == APPLIES
    assert all(len(v) >= 2 for v in reached.values()), reached


@pytest.mark.parametrize("name", DC.MODELS)
def test_reference_obeys_the_structure_exactly(name, built):
    c = DC.case(name, built[name])
    om = c["om"]
    assert DC.structure_faults(om, c["ref"]) == [] and DC.structure_faults(om, c["ref32"]) == []
    # the structure is not empty: on every model with a branch some entries are demanded to be 0, and the check sees one that is not
    D = 6 + om["nb"] - 1
    rel, chains = DC.related_columns(om), DC.chain_columns(om)
    assert rel.shape == (D, D) and (rel == rel.T).all() and rel.diagonal().all()
    assert (name in ("deep_chain", "slab")) == bool(rel.all())
    assert all(len(ch) == int(om["depth"][om["link_body"][l]]) for l, ch in enumerate(chains))
    for key in ("jac", "mass"):
        out = {k: v.copy() for k, v in c["ref"].items()}
        if key == "jac":
            l = int(np.argmax([len(ch) for ch in chains]))
            off = [col for col in range(6, D) if col not in chains[l]]
            if not off:
                out["jac"][0, l, 1, 4, 1] = 1e-30          # the base block instead
            else:
                out["jac"][0, l, 1, 2, off[0]] = 1e-30
        else:
            i, j = np.argwhere(~rel)[0] if not rel.all() else (0, 1)
            out["mass"][-1, i, j] = 1e-30
        assert len(DC.structure_faults(om, out)) == 1, (name, key)
    # the identities hold in f64 to rounding, and the reference's Jacobian rows give the velocity of its own recursion
    res = DC.identity_devs(om, c["cases"], c["acc"], c["ref"])
    assert max(res.values()) < 1e-12, res


@pytest.mark.parametrize("name", DC.MODELS)
def test_reference_agrees_with_the_models_own_oracle(name, built):
    """tests/test_dynamics_ref.py ties the reference to the oracle on the T-rex; here on each tree: the oracle's forward dynamics
    returns the accelerations the torques were drawn from, inverse dynamics undoes it, M inverts the oracle's M^-1, and energy
    and momentum are the oracle's"""
    c = DC.case(name, built[name])
    om, orc = c["om"], DC.oracle_of(built[name])
    inv = np.argsort(R.perm_to_oracle(om))
    D = 6 + om["nb"] - 1
    assert np.abs(c["acc64"] - c["drawn"]).max() < 1e-7 * np.abs(c["drawn"]).max()
    for e, (s, ms) in enumerate(c["cases"]):
        h = c["ref"]["id_zero"][e]
        f = R.inverse_dynamics(om, s, c["acc64"][e], ms, DC.G)
        assert R.block_dev(f, np.concatenate([np.zeros(6), c["taus"][e]]), np.abs(h[:6]).max(), np.abs(c["taus"][e]).max()) < 1e-8
        os_ = oracle_state(orc, s, ms)
        assert np.abs(c["ref"]["mass"][e] @ orc.minv(os_)[np.ix_(inv, inv)] - np.eye(D)).max() < 1e-8
        en, cr = orc.energy(os_), c["ref"]["cent"][e]
        co = cr.copy()
        co[6:9], co[12], co[13] = en["momentum"][3:6], en["ke"], en["pe"]
        co[3:6] = co[6:9] / cr[14]
        co[9:12] = en["momentum"][0:3] - np.cross(cr[0:3] - s[0:3], co[6:9])
        assert DC.cent_dev(cr, co) < 1e-8
    assert sum(ms is not None for _, ms in c["cases"]) == 2 and c["cases"][-1][1] is not None and c["cases"][-2][1] is not None
    assert len(c["cases"]) == DC.N == 12


@pytest.mark.parametrize("name", DC.MODELS)
def test_mass_scales_move_the_reference(name, built):
    """what tests/test_gpu_dynamics_models.py::test_mass_scale asks of the device: without their per-body mass scales the last two
    states lie more than 100 x the bound away in id_zero, mass and cent, and not at all in the Jacobian"""
    c = DC.case(name, built[name])
    plain = DC.reference_outputs(c["om"], [(s, None) for s, _ in c["cases"][-2:]], c["acc"][-2:])
    moved = DC.metric_devs(c["taus"][-2:], plain, {k: x[-2:] for k, x in c["ref"].items()}, round_trip_of_ref=True)
    assert moved["jac"] == 0.0 and all(moved[k] > SEPARATION * c["bound"][k] for k in ("id_zero", "id_roundtrip", "mass", "cent")), moved


def test_models_are_what_they_are_chosen_for(built):
    tf_of = lambda om: np.asarray(om["link_tf"], np.float64).reshape(-1, 12)
    eye = np.eye(3).reshape(-1)
    # bushy: two bodies at different depths with four moving children each; every welded link behind a moved and turned frame
    om = built["bushy"]["om"]
    par, depth = np.asarray(om["parent"], int), np.asarray(om["depth"], int)
    four = [b for b in range(om["nb"]) if (par[1:] == b).sum() == 4]
    assert om["nb"] == 26 and len(four) >= 2 and len(set(depth[four])) >= 2 and 0 in depth[four] and 2 in depth[four]
    names, bodies, lb, tf = list(om["link_names"]), list(om["body_names"]), np.asarray(om["link_body"], int), tf_of(om)
    welded = [l for l in range(len(names)) if names[l] != bodies[lb[l]]]
    assert len(welded) == 6
    for l in welded:
        assert np.abs(tf[l][:9] - eye).max() > 1e-2 and np.abs(tf[l][9:]).max() > 1e-2, names[l]
    oo = list(om["obs_order"])
    assert oo != sorted(oo) and oo != sorted(oo, reverse=True) and 6 + om["nb"] - 1 == 31
    # mount_first: URDF link 0 in a moving body at depth 2, behind a turned frame; a side branch
    om = built["mount_first"]["om"]
    assert om["link_body"][0] != 0 and om["depth"][om["link_body"][0]] == 2 and np.abs(tf_of(om)[0][:9] - eye).max() > 1e-2
    assert (np.asarray(om["parent"], int)[1:] == 0).sum() == 2 and 6 + om["nb"] - 1 == 10
    # slab: D = 7; deep_chain: depth 6, oblique axes that are no unit vectors, D = 12
    assert 6 + built["slab"]["om"]["nb"] - 1 == 7
    om = built["deep_chain"]["om"]
    assert max(om["depth"]) == 6 and 6 + om["nb"] - 1 == 12
    ax = np.asarray(om["joint_axis"], np.float64)[1:]
    assert np.all(np.sort(np.abs(ax), axis=1)[:, 1] > 0.02)
