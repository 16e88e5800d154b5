"""Qualifies tests/symmetry_ref.py alone, on the CPU, on the generated exactly symmetric bipeds (tests/symmetry_models.py): every map
is an involution; the mass matrix and the bias forces of tests/dynamics_ref.py and every kinematic channel of
tests/observation_ref.py are equivariant under the reference's tables; each of the four planted mistakes breaks one of these.

BOUNDS, from f64 rounding. An entry of M (or of h) is a sum over the 10 bodies of products of a few dozen factors of magnitude at
most `scale` = max |M| (max |h|); each side of a comparison carries at most about 10 bodies x 100 operations x 2^-53 = 1.1e-13 of
it in relative error, and the two sides differ in operation order throughout. The bound is 1e-12 x scale: 4.5 times the sum of both
sides' worst cases. A channel value is a chain of at most 6 frames, a few hundred operations on magnitudes up to 4 (metres, m/s
scaled): the same 1e-12 x max(1, |value|). A planted mistake must exceed its bound by more than 1e6."""
import numpy as np
import pytest

import dynamics_ref as D
import observation_ref as OBS
import symmetry_models as SM
import symmetry_ref as R

REL = 1e-12
SEPARATION = 1e6


@pytest.fixture(scope="module", params=[0, 1])
def biped(request, tmp_path_factory):
    lateral = request.param
    path, props, model = SM.compile_biped(tmp_path_factory.mktemp("biped%d" % lateral), lateral)
    states = SM.random_states(model, 6, seed=3 + lateral)
    return dict(lateral=lateral, model=model, props=props, states=states, mm=R.model_table(model))


def test_the_model_table_is_the_generated_one(biped):
    mm, model = biped["mm"], biped["model"]
    assert mm["lateral"] == biped["lateral"] == R.model_table(model, biped["lateral"])["lateral"]
    assert model["obs_joint_names"] == SM.JOINTS and model["nb"] == SM.NB
    assert mm["pair"].tolist() == SM.PAIR and mm["sign"].tolist() == SM.SIGN
    assert all(v == 0.0 for v in mm["residual"].values()), mm["residual"]      # exactly symmetric: the same decimal text on both sides
    for other in {0, 1, 2} - {biped["lateral"]}:
        with pytest.raises(R.Refused):
            R.model_table(model, other)


def test_every_map_is_an_involution(biped):
    model, mm = biped["model"], biped["mm"]
    chans = SM.locomotion_channels(model, biped["lateral"]) + [(R.PREV_ACTION, 0, (0, 0, 0), 1.0), (R.EXTERNAL, 3, (0, 0, 0), 1.0)]
    for stiff in (False, True):
        A = SM.NJ * (2 if stiff else 1)
        assert R.check_table(*R.action_table(mm["pair"], mm["sign"], stiff))
        for tail in (2, 5):
            src, sign = R.row_table(model, mm, chans, A, tail, extern_src=[1, 0, 2], extern_sign=[1, 1, -1])
            assert len(src) == 3 * SM.NJ + OBS.extra_dim(chans, A) + tail and R.check_table(src, sign)
    assert R.check_table(*R.command_table(biped["lateral"]))
    rng = np.random.default_rng(0)
    x = rng.normal(size=(5, len(src))).astype(np.float32)
    x[0, :4] = [np.nan, np.inf, -0.0, 0.0]
    twice = R.mirror_rows(src, sign, R.mirror_rows(src, sign, x))
    assert twice.tobytes() == x.tobytes()
    mean, var = rng.normal(size=len(src)), rng.uniform(0.5, 2.0, len(src))
    once = R.symmetrize_stats(src, sign, mean, var)
    again = R.symmetrize_stats(src, sign, *once)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(once, again))
    # the moments of the stream that holds every row and its image: checked on a sample, in f64
    rows = rng.normal(size=(64, len(src)))
    both = np.concatenate([rows, R.mirror_rows_f64(src, sign, rows)])
    m, v = R.symmetrize_stats(src, sign, rows.mean(0), rows.var(0))
    assert np.abs(m - both.mean(0)).max() < 1e-14 and np.abs(v - both.var(0)).max() < 1e-13
    for s in biped["states"]:
        back = R.mirror_state(model, mm, R.mirror_state(model, mm, s))
        back[3:7] *= np.sign(back[3:7] @ s[3:7])
        assert np.abs(back - s).max() < 1e-14 * 4


def _velocity_map(mm):
    """the signed permutation of a generalised velocity [v 3 | w 3 | qd J] for a reflection of world x: (P, sign)"""
    nj = len(mm["pair"])
    src = np.concatenate([np.arange(6), 6 + mm["pair"]])
    sign = np.concatenate([[-1, 1, 1], [1, -1, -1], mm["sign"]]).astype(float)
    P = np.zeros((6 + nj, 6 + nj))
    P[np.arange(6 + nj), src] = sign
    return P


def _dynamics_defect(model, mm, tables, states):
    """the largest equivariance defect of M and of h under `tables`, each relative to its bound"""
    worst = 0.0
    P = _velocity_map(tables)
    for s in states:
        s2 = R.mirror_state(model, tables, s)
        M, M2 = D.mass_matrix(model, s), D.mass_matrix(model, s2)
        h, h2 = D.inverse_dynamics(model, s), D.inverse_dynamics(model, s2)
        worst = max(worst, np.abs(M2 - P @ M @ P.T).max() / (REL * np.abs(M).max()), np.abs(h2 - P @ h).max() / (REL * np.abs(h).max()))
    return worst


def _channel_defect(model, mm, lateral, states, table_kw=None, model_kw=None):
    """rows(mirror s) against mirror(rows(s)) on the locomotion-style channels, PREV_ACTION and EXTERNAL, relative to the bound"""
    tables = R.model_table(model, **(model_kw or {}))
    chans = SM.locomotion_channels(model, lateral) + [(R.PREV_ACTION, 0, (0, 0, 0), 1.0), (R.EXTERNAL, 3, (0, 0, 0), 1.0)]
    es, eg = [1, 0, 2], [1, 1, -1]
    src, sign = R.row_table(model, tables, chans, SM.NJ, 2, extern_src=es, extern_sign=eg, **(table_kw or {}))
    a_t = R.action_table(tables["pair"], tables["sign"])
    rng = np.random.default_rng(5)
    worst = 0.0
    for s in states:
        act, ext, fz = rng.normal(size=SM.NJ), rng.normal(size=3), rng.uniform(0, 5, model["nb"])
        row = np.concatenate([s[13:13 + SM.NJ], s[13 + SM.NJ:], rng.normal(size=SM.NJ), [0.3, 0.0]])     # q | qd | torque | reward, done
        full = OBS.compose(model, s, chans, row, 2, action=act, extern=ext, contact_fz=fz)
        # the mirrored scene: the true mirror state (never a planted one), its row, action, externals and contact forces
        s2 = R.mirror_state(model, mm, s)
        row2 = np.concatenate([R.mirror_rows_f64(np.concatenate([mm["pair"] + b * SM.NJ for b in range(3)]), np.tile(mm["sign"], 3), row[:3 * SM.NJ]), row[3 * SM.NJ:]])
        full2 = OBS.compose(model, s2, chans, row2, 2, action=R.mirror_rows_f64(*R.action_table(mm["pair"], mm["sign"]), act),
                            extern=R.mirror_rows_f64(es, eg, ext), contact_fz=fz[mm["body_pair"]])
        want = R.mirror_rows_f64(src, sign, full)
        worst = max(worst, (np.abs(full2 - want) / (REL * np.maximum(1.0, np.abs(full2)))).max())
    del a_t
    return worst


def test_dynamics_and_channels_are_equivariant_and_every_planted_mistake_is_seen(biped, record_property):
    model, mm, states = biped["model"], biped["mm"], biped["states"]
    dyn = _dynamics_defect(model, mm, mm, states)
    chan = _channel_defect(model, mm, biped["lateral"], states)
    record_property("defect_over_bound", dict(dynamics=dyn, channels=chan))
    print("lateral %d: dynamics defect %.3g, channel defect %.3g of the bound" % (biped["lateral"], dyn, chan))
    assert dyn <= 1.0 and chan <= 1.0
    for name, model_kw, table_kw in SM.PLANTED:
        bad = R.model_table(model, **model_kw)
        seen = max(_dynamics_defect(model, mm, bad, states) if model_kw else 0.0,
                   _channel_defect(model, mm, biped["lateral"], states, table_kw, model_kw))
        print("  planted %-18s %.3g of the bound" % (name, seen))
        assert seen > SEPARATION, name


def test_the_trex_is_paired_and_its_asymmetry_reported():
    """the asset is only approximately symmetric: the table exists; its residuals are printed (scripts/symmetry_bench.py records
    them in the profile), not asserted"""
    from oracle import oracle as O, trex_model as tm
    model = tm.compile_model(O.default_asset_urdf())
    mm = R.model_table(model)
    names = model["obs_joint_names"]
    spine = sorted(names[k] for k in range(25) if mm["pair"][k] == k)
    assert spine == sorted("joint_" + n for n in ("atlas_axis", "cranium", "vertebra_cervical_03", "vertebra_cervical_09", "vertebra_caudal_02",
                                                  "vertebra_caudal_10", "vertebra_caudal_24"))
    assert sorted(names[k] for k in range(25) if mm["sign"][k] < 0) == ["joint_cranium", "joint_vertebra_caudal_10"]
    for k in range(25):
        if mm["pair"][k] != k:
            assert names[k].replace("_left", "_right") == names[mm["pair"][k]] or names[k].replace("_right", "_left") == names[mm["pair"][k]]
    r = mm["residual"]
    print("T-rex residuals:", r)
    assert all(np.isfinite(v) and v >= 0 for v in r.values())


def _step_rows(orc, model, chans, state, action):
    """one full oracle step (f64) from `state` under `action`: (next state, its composed row [q | qd | torque 0 | channels | 0 0], the
    number of contacts of the last substep)"""
    import synthetic_models as SYN
    _, _, contacts = SYN.oracle_step_contacts(orc, state, action)
    s = orc.new_state()
    orc.set_state(s, np.asarray(state, np.float64))
    orc.set_motors_on(s, 1)
    orc.step(s, np.asarray(action, np.float64))
    x = orc.get_state(s)
    row = np.concatenate([x[13:], np.zeros(SM.NJ), [0.0, 0.0]])
    return x, OBS.compose(model, x, chans, row, 2), len(contacts[0])


def test_one_oracle_step_sees_every_planted_mistake(biped, record_property):
    """One full oracle step, f64, on 16 states of the symmetric biped - 6 airborne, 5 standing, 5 with one foot down -: the step from
    the mirrored state under the mirrored action against the mirror image of the step. The defect of the CORRECT tables is measured
    and recorded, not bounded: it is not zero where there are contacts, because the PGS sweep visits its rows in an order that is not
    mirrored. Asserted: each planted mistake's defect exceeds the correct tables' by 10 x, on all but at most 4 of the 16 states.
    The defect is the largest |difference| over the composed row of the next state (q, qd and every kinematic channel), each column
    over max(1, |value|)."""
    from oracle import oracle as O
    model, mm, lateral = biped["model"], biped["mm"], biped["lateral"]
    orc = O.Oracle(model, params=biped["props"]["params"])
    chans = [c for c in SM.locomotion_channels(model, lateral) if c[0] != R.CONTACT_FORCE]
    oo = model["obs_order"]
    rng = np.random.default_rng(9)

    def defect(tables, table_kw, state, action, first):
        src, sign = R.row_table(model, tables, chans, SM.NJ, 2, **table_kw)
        a_src, a_sign = R.action_table(tables["pair"], tables["sign"])
        _, row2, _ = _step_rows(orc, model, chans, R.mirror_state(model, tables, state), R.mirror_rows_f64(a_src, a_sign, action))
        want = R.mirror_rows_f64(src, sign, first)
        return (np.abs(row2 - want) / np.maximum(1.0, np.abs(want))).max()

    kinds, base, dropped = [], [], {name: 0 for name, _, _ in SM.PLANTED}
    for kind, state in SM.step_states(model, lateral):
        action = rng.uniform(model["q_lower"][oo], model["q_upper"][oo]) * 0.5
        _, first, ncontacts = _step_rows(orc, model, chans, state, action)
        d0 = defect(mm, {}, state, action, first)
        kinds.append((kind, ncontacts))
        base.append(d0)
        for name, model_kw, table_kw in SM.PLANTED:
            d = defect(R.model_table(model, **model_kw), table_kw, state, action, first)
            dropped[name] += not d > 10 * max(d0, 1e-13)
    by_kind = {k: max(d for (kk, _), d in zip(kinds, base) if kk == k) for k in ("airborne", "standing", "one_foot")}
    record_property("oracle_step_defect", by_kind)
    print("lateral %d: one oracle step, the correct tables' equivariance defect by kind %s; contacts %s; states dropped per planted mistake %s"
          % (lateral, {k: "%.3g" % v for k, v in by_kind.items()}, [n for _, n in kinds], dropped))
    assert sum(n > 0 for (k, n) in kinds if k != "airborne") >= 8 and all(n == 0 for (k, n) in kinds if k == "airborne")
    assert all(n <= 4 for n in dropped.values()), dropped
