"""Kernel K8 on the GPU (include/trex_batch.h: trex_batch_body_clearance, trex_batch_set_termination, trex_batch_termination_info)
against the f64 restatement tests/termination_ref.py, on the states and thresholds of tests/termination_cases.py - qualified on the
CPU by tests/test_termination_cases_host.py - and, for the three-launch step sequence, bitwise against a batch with termination
off that is reset from outside.

Tolerances (TOL): 4 x the largest deviation measured on these very states on an MI355X (profiles/r19_termination.txt), never above
the caps: 1e-5 x max(1 m, the env's largest |position| entry) for heights (clearance, lowest point, head height, clearance margin),
1e-5 for cos tilt. Heights are compared per env over that scale.

What the predicate judges is the state AFTER the step launch, which no reference knows beforehand: the tests take it from a twin
batch with termination off - the step launch is the same launch, so its state is bitwise the judged one - and evaluate the
reference there. A judged state within the tolerance of a threshold could be decided either way; the tests assert that there is
none instead of leaving one out. On the qualified states themselves the decision is checked through the query: the kernel's
clearances, the head position and the tilt put every one of them on the reference's side of every threshold."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import gpu_support
import termination_cases as TC
import termination_ref as TR
from conftest import ASSET_URDF
from gpu_support import DEV, guarded, guards_intact
from state_sets import built_models

pytestmark = pytest.mark.gpu
NB, J = 26, 25

# Largest deviations measured on an MI355X (profiles/r19_termination.txt), over the N = 67 samples of both collision models, the
# judged states of the decision tests and the generated models. Tolerance = 4 x measured, never above the cap; no cap binds.
MEASURED = dict(clearance=2.63e-7, lowest=3.13e-7, head=1.19e-7, cos_tilt=9.93e-8, margin=1.67e-7)
CAPS = dict(clearance=1e-5, lowest=1e-5, head=1e-5, cos_tilt=1e-5, margin=1e-5)
TOL = {k: min(4 * v, CAPS[k]) for k, v in MEASURED.items()}
NEVER = dict(head_height=-1.0e3, max_tilt=float(np.pi))     # thresholds in force that no state reaches


def make_vec(n, collision="hulls", urdf=ASSET_URDF, **kw):
    return gpu_support.make_vec(n, urdf, collision=collision, **kw)


def load(v, cases, idx=None):
    """cases[idx[e]] (all, in order, when idx is None) into the envs of v: state and - where a case has one - mass scales"""
    idx = np.arange(len(cases)) if idx is None else np.asarray(idx)
    assert len(idx) == v.num_envs
    v.reset()
    if any(cases[k]["mass_scale"] is not None for k in idx):
        ms = np.array([np.ones(v.model.num_bodies, np.float32) if cases[k]["mass_scale"] is None else cases[k]["mass_scale"] for k in idx])
        v.set_domain(torch.tensor(ms))
    v.set_state(torch.tensor(np.array([cases[k]["state"] for k in idx], np.float32)))


def scale_of(state):
    return max(1.0, float(np.abs(np.asarray(state)[:3]).max()))


def query(v, lowest=True):
    """body_clearance through the raw binding into guarded buffers -> (clearance [n, nb], lowest [n, nb, 3] or None) as f64"""
    n, nb = v.num_envs, v.model.num_bodies
    wc, c = guarded((n, nb))
    wl, low = guarded((n, nb, 3)) if lowest else (None, None)
    v.batch.body_clearance(c, low)
    torch.cuda.synchronize()
    assert guards_intact(wc, (n, nb)) and (not lowest or guards_intact(wl, (n, nb, 3)))
    return c.cpu().numpy().astype(np.float64), None if low is None else low.cpu().numpy().astype(np.float64)


def clearance_dev(got_c, got_low, refs, states):
    """largest deviations of a query from the reference, per env over its scale: dict(clearance, lowest)"""
    w = dict(clearance=0.0, lowest=0.0)
    for e, (r, s) in enumerate(zip(refs, states)):
        sc = scale_of(s)
        fin = np.isfinite(r["clearance"])
        assert np.array_equal(np.isinf(got_c[e]), ~fin) and (got_c[e][~fin] > 0).all()
        if fin.any():
            w["clearance"] = max(w["clearance"], np.abs(got_c[e][fin] - r["clearance"][fin]).max() / sc)
        if got_low is not None:
            assert np.isnan(got_low[e][~fin]).all()
            if fin.any():
                # the point itself may be another vertex of (nearly) the same height: its height is what is compared, and the
                # point has to be one of the body's within the tolerance
                w["lowest"] = max(w["lowest"], np.abs(got_low[e][fin, 2] - r["lowest"][fin, 2]).max() / sc)
    return w


def judged(cases, idx, collision, actions, thr_kw, **kw):
    """one step of the envs holding cases[idx] with termination on (thr_kw) and of their twin with it off ->
    dict(reason, values, tobs, rows_on, rows_off, state_off = the judged states, done_on)"""
    out = {}
    for on in (False, True):
        v = make_vec(len(idx), collision, **kw)
        load(v, cases, idx)
        if on:
            v.set_termination(**thr_kw)
        v.step_tensor(actions)
        torch.cuda.synchronize()
        tag = "on" if on else "off"
        out["rows_" + tag], out["done_" + tag] = v.rows.clone(), v.done.clone()
        out["state_" + tag] = v.get_state().clone()
        if on:
            out["reason"] = v.termination_reason.cpu().numpy().copy()
            out["values"] = v.termination_values.cpu().numpy().astype(np.float64)
            out["tobs"] = v.terminal_obs.clone()
        v.close()
    return out


def reference_at(built, states, mass_scales=None):
    return [TR.evaluate(built.o64, built.om, np.asarray(s, np.float64), None if mass_scales is None else mass_scales[e])
            for e, s in enumerate(states)]


def actions_for(n, seed, model):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    lo = torch.tensor(model.lower, dtype=torch.float32, device=DEV)
    hi = torch.tensor(model.upper, dtype=torch.float32, device=DEV)
    return lo + (hi - lo) * torch.rand(n, len(model.lower), generator=gen, device=DEV)


def thr_kwargs(thr, penalty=0.0):
    return dict(head_height=thr["head_height"], max_tilt=thr["max_tilt"], keep_clear={thr["link"]: thr["clear"]}, penalty=penalty)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collision", ("hulls", "primitives"))
def test_values_n67(collision):
    """clearance and lowest point at N = 67 on the qualified states against the reference; termination_values on the judged
    states of one step; every qualified state of the sample on the reference's side of every threshold"""
    built, cases = TC.states(collision)
    thr = TC.search(collision)
    idx = TC.sample(collision)
    ref = [TC.reference(collision)[k] for k in idx]
    v = make_vec(len(idx), collision)
    load(v, cases, idx)
    c, low = query(v)
    c2, _ = query(v, lowest=False)
    assert c.tobytes() == c2.tobytes()                               # lowest NULL: the same clearances
    head = v.head_position().cpu().numpy().astype(np.float64)[:, 2] - float(built.o64.params["floor_z"])
    w = clearance_dev(c, low, ref, [cases[k]["state"] for k in idx])
    w["head"] = max(abs(head[e] - r["head"]) / scale_of(cases[k]["state"]) for e, (k, r) in enumerate(zip(idx, ref)))
    # the lowest point is a collision point of its body, at the height reported
    for e, r in enumerate(ref):
        pts = TR.world_points(built.om, r["pos"], r["rot"])
        for b in np.flatnonzero(np.isfinite(r["clearance"])):
            p, rad = pts[b]
            d = np.abs(p - (low[e, b] + [0, 0, 1] * rad[:, None])).max(1).min()
            assert d <= TOL["lowest"] * scale_of(cases[idx[e]]["state"]) * 4, (e, b, d)
    # the sample's qualified states: the query decides as the reference does
    for e, k in enumerate(idx):
        vals = np.array([head[e], ref[e]["cos_tilt"], c[e, thr["body"]] - thr["clear"]])
        assert TR.reason(vals, thr["head_height"], thr["max_tilt"]) == thr["reasons"][k]
    v.close()
    # termination_values: on the state the step launch leaves (the twin's)
    a = actions_for(len(idx), 5, v.model)
    j = judged(cases, idx, collision, a, dict(NEVER, keep_clear={thr["link"]: thr["clear"]}))
    ms = [cases[k]["mass_scale"] for k in idx]
    jref = reference_at(built, j["state_off"].cpu().numpy(), ms)
    cm = thr["clear_min"].astype(np.float32).astype(np.float64)
    want = np.array([TR.values(r, cm) for r in jref])
    sc = np.array([scale_of(s) for s in j["state_off"].cpu().numpy()])
    w["values_head"] = (np.abs(j["values"][:, 0] - want[:, 0]) / sc).max()
    w["cos_tilt"] = np.abs(j["values"][:, 1] - want[:, 1]).max()
    w["margin"] = (np.abs(j["values"][:, 2] - want[:, 2]) / sc).max()
    print("%s K8 deviations at N = %d: %s" % (collision, len(idx), {k: "%.3g" % x for k, x in w.items()}))
    assert w["clearance"] <= TOL["clearance"] and w["lowest"] <= TOL["lowest"] and w["head"] <= TOL["head"]
    assert w["values_head"] <= TOL["head"] and w["cos_tilt"] <= TOL["cos_tilt"] and w["margin"] <= TOL["margin"]


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collision", ("hulls", "primitives"))
def test_decisions_on_every_case(collision):
    """every state of the case list in ONE batch, one step with the qualified thresholds: the reason bits are the reference's at the
    judged state, for every env; no judged state is within the tolerance of a threshold; all three reasons and none occur"""
    built, cases = TC.states(collision)
    thr = TC.search(collision)
    n = len(cases)
    idx = np.arange(n)
    a = actions_for(n, 9, make_model())
    j = judged(cases, idx, collision, a, thr_kwargs(thr, penalty=2.5))
    st = j["state_off"].cpu().numpy()
    jref = reference_at(built, st, [c["mass_scale"] for c in cases])
    cm = thr["clear_min"].astype(np.float32).astype(np.float64)
    hh, tilt = float(np.float32(thr["head_height"])), float(np.float32(thr["max_tilt"]))
    want_v = np.array([TR.values(r, cm) for r in jref])
    want = np.array([TR.reason(x, hh, tilt) for x in want_v])
    sc = np.array([scale_of(s) for s in st])
    ended = j["done_off"].cpu().numpy()
    near = np.minimum(np.minimum(np.abs(want_v[:, 0] - hh) / sc, np.abs(want_v[:, 1] - np.cos(tilt))), np.abs(want_v[:, 2]) / sc)
    print("%s: %d judged states, the closest %.3g from a threshold; reasons %s" % (collision, n, near.min(), TC.counts(want)))
    assert not ended.any()
    assert near.min() > max(TOL.values()), "a judged state sits within the tolerance of a threshold"
    assert np.array_equal(j["reason"], want)
    cnt = TC.counts(want)
    assert min(cnt["head"], cnt["tilt"], cnt["clearance"], cnt["two"], cnt["none"]) >= 1
    # done, reward and the terminal observation of every env
    fired = torch.tensor(want != 0, device=DEV)
    assert torch.equal(j["done_on"], fired) and torch.equal(j["rows_on"][:, 3 * J + 1] != 0, fired)
    assert torch.equal(j["rows_on"][:, 3 * J], torch.where(fired, j["rows_off"][:, 3 * J] - 2.5, j["rows_off"][:, 3 * J]))
    assert torch.equal(j["tobs"][fired], j["rows_off"][fired][:, :3 * J])
    assert torch.equal(j["rows_on"][~fired], j["rows_off"][~fired]) and torch.equal(j["state_on"][~fired], j["state_off"][~fired])


_MODEL = {}


def make_model():
    from trex_gym import _capi
    if "m" not in _MODEL:
        _MODEL["m"] = _capi.Model(ASSET_URDF)
    return _MODEL["m"]


# 3 ------------------------------------------------------------------------------------------------------------------------
def fallen_idx(n, offset=0):
    """n fallen hull states, spread over the `hulls` group"""
    total = len(TC.ec.group("hulls")["cases"])
    return (np.round(np.linspace(0, total - 1, n)).astype(int) + offset) % total


def snapshot(v, sensor):
    steps = torch.zeros(v.num_envs, dtype=torch.int32, device=DEV)
    v.batch.get_episode_steps(steps)
    cnt = torch.zeros(v.num_envs, dtype=torch.int32, device=DEV)
    imp = torch.zeros(v.num_envs, device=DEV)
    v.batch.contact_stats(cnt, imp)
    out = [v.get_state().clone(), v.rows.clone(), v.done.clone(), v.penalties.clone(), steps, cnt, imp]
    if sensor:
        out.append(v.contact_wrench().clone())
    return out


MIXES = {
    "plain1": (1, {}), "plain2": (2, {}), "plain3": (3, {}), "plain67": (67, {}),
    "warm2": (2, dict(params=dict(warmstart=0.85))), "wrench3": (3, dict(wrench=True)), "sensor67": (67, dict(sensor=True)),
    "velocity1": (1, dict(control_mode="velocity")), "domain67": (67, dict(domain=True)), "limit3": (3, dict(max_episode_steps=7)),
}


def build_mix(n, kw, idx):
    _, cases = TC.states("hulls")
    kw = dict(kw)
    wrench, sensor, domain = kw.pop("wrench", False), kw.pop("sensor", False), kw.pop("domain", False)
    v = make_vec(n, **kw)
    load(v, cases, idx)
    rng = np.random.default_rng(3)
    if domain:
        v.set_domain(torch.tensor(rng.uniform(0.8, 1.2, (n, NB)).astype(np.float32)), torch.tensor(rng.uniform(0.5, 1.25, n).astype(np.float32)))
    if wrench:
        w = np.zeros((n, NB, 6), np.float32)
        w[:, 0, :3] = rng.uniform(-3e3, 3e3, (n, 3))
        v.set_external_wrench(torch.tensor(w))
    if sensor:
        v.enable_contact_sensor(True)
    return v, sensor


@pytest.mark.parametrize("mix", list(MIXES))
def test_mechanism_bitwise(mix):
    """run A: termination on; run B: off, and after each step_rows a reset_rows with the mask A reported, reward and done patched
    as the header says. 12 steps from fallen states + 1 more (the warm record's effect): states, rows, done bytes, penalties, episode
    steps, contact stats and the contact sensor are identical after every step"""
    n, kw = MIXES[mix]
    thr = TC.search("hulls")
    idx = fallen_idx(n, offset=5)
    T, pen = 13, 1.5
    acts = [actions_for(n, 100 + t, make_model()) for t in range(T)]
    if kw.get("control_mode") == "velocity":
        acts = [torch.tanh(a) * 2.0 for a in acts]
    A, sensor = build_mix(n, kw, idx)
    A.set_termination(**thr_kwargs(thr, pen))
    snaps, masks = [], []
    for a in acts:
        A.step_tensor(a)
        masks.append((A.termination_reason != 0).clone())
        snaps.append(snapshot(A, sensor))
    A.close()
    assert torch.stack(masks).any(), "no env fell: the test would show nothing"
    B, _ = build_mix(n, kw, idx)
    for t, a in enumerate(acts):
        B.step_tensor(a)
        m = masks[t]
        rew, done_f, done, pens = B.rew.clone(), B.done_f.clone(), B.done.clone(), B.penalties.clone()
        B.batch.reset_rows(B.rows, m.to(torch.uint8))
        B.rew.copy_(torch.where(m, rew - pen, rew))
        B.done_f.copy_(torch.where(m, torch.ones_like(done_f), done_f))
        B.done.copy_(done | m)
        got = snapshot(B, sensor)
        got[3] = pens                                                # (reset_rows leaves the penalties tensor alone, as the sequence does)
        for k, (x, y) in enumerate(zip(snaps[t], got)):
            assert torch.equal(x, y), (mix, t, k)
    B.close()


def test_never_firing_and_switched_off_equal_plain_stepping():
    n = 6
    _, cases = TC.states("hulls")
    idx = fallen_idx(n, offset=2)
    acts = [actions_for(n, 40 + t, make_model()) for t in range(4)]
    runs = []
    for mode in ("plain", "never", "off_again"):
        v = make_vec(n)
        load(v, cases, idx)
        if mode == "never":
            v.set_termination(**NEVER, keep_clear={0: -1.0e3}, penalty=3.0)
        if mode == "off_again":
            v.set_termination(head_height=100.0, penalty=3.0)
            v.set_termination()
            assert not v._term_on
        out = []
        for a in acts:
            v.step_tensor(a)
            out += snapshot(v, False)
        if mode == "never":
            assert not v.termination_reason.any()
        runs.append(out)
        v.close()
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert torch.equal(x, y)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_interplay_with_the_episode_limit_and_containment():
    """thresholds that fire for every env; env 0 reaches the episode limit in the same step, env 1 is contained (a NaN state): both
    have reason 0, done 1 and the plain step's reward; the others are penalised exactly once; the terminal observation is the
    observation the same step writes with termination off"""
    n = 5
    _, cases = TC.states("hulls")
    idx = fallen_idx(n, offset=11)
    a = actions_for(n, 77, make_model())
    res = {}
    for on in (False, True):
        v = make_vec(n, max_episode_steps=10)
        load(v, cases, idx)
        st = v.get_state()
        st[1, 13 + 4] = float("nan")
        v.set_state(st)
        v.set_episode_steps(torch.tensor([9, 0, 0, 3, 0]))
        if on:
            v.set_termination(head_height=100.0, penalty=4.0)
        v.step_tensor(a)
        res[on] = (v.rows.clone(), v.done.clone(), v.episode_steps.clone(), v.get_state().clone())
        if on:
            reason, tobs = v.termination_reason.clone(), v.terminal_obs.clone()
            v.step_tensor(a)                                          # the penalty is not taken again from a later reward
            rew2, reason2 = v.rew.clone(), v.termination_reason.clone()
        else:
            v.batch.reset_rows(v.rows, torch.tensor([0, 0, 1, 1, 1], dtype=torch.uint8, device=DEV))
            v.step_tensor(a)
            rew2_plain = v.rew.clone()
        v.close()
    (rows_off, done_off, _, _), (rows_on, done_on, steps_on, _) = res[False], res[True]
    assert reason.tolist() == [0, 0, 1, 1, 1]
    assert done_off.tolist() == [True, True, False, False, False] and done_on.all() and (rows_on[:, 3 * J + 1] == 1).all()
    assert torch.equal(rows_on[:2], rows_off[:2])                    # not judged: reward, done and observation untouched
    assert torch.equal(rows_on[2:, 3 * J], rows_off[2:, 3 * J] - 4.0)
    assert torch.equal(tobs[2:], rows_off[2:, :3 * J]) and (tobs[:2] == 0).all()
    assert steps_on.tolist() == [0, 0, 0, 0, 0]
    assert reason2.tolist() == [1, 1, 1, 1, 1] and torch.equal(rew2[2:], rew2_plain[2:] - 4.0)


def test_step_with_separate_arrays():
    """trex_batch_step (obs, reward, done as arrays of their own) takes the same three launches: its outputs are step_rows'; without
    a done or reward buffer the envs still fall and are reset"""
    n = 5
    thr = TC.search("hulls")
    _, cases = TC.states("hulls")
    idx = fallen_idx(n, offset=5)
    acts = [actions_for(n, 100 + t, make_model()) for t in range(6)]
    ref = make_vec(n)
    load(ref, cases, idx)
    ref.set_termination(**thr_kwargs(thr, 1.5))
    full, bare = make_vec(n), make_vec(n)
    for v in (full, bare):
        load(v, cases, idx)
        v.set_termination(**thr_kwargs(thr, 1.5))
    obs, rew = torch.zeros(n, 3 * J, device=DEV), torch.zeros(n, device=DEV)
    done, pen = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, 3, device=DEV)
    obs2 = torch.zeros(n, 3 * J, device=DEV)
    fell = False
    for a in acts:
        ref.step_tensor(a)
        full.batch.step(a, obs, rew, done, pen)
        bare.batch.step(a, obs2, None, None)
        assert torch.equal(obs, ref.obs) and torch.equal(rew, ref.rew) and torch.equal(done.bool(), ref.done) and torch.equal(pen, ref.penalties)
        assert torch.equal(obs2, ref.obs) and torch.equal(bare.get_state(), ref.get_state()) and torch.equal(full.get_state(), ref.get_state())
        assert torch.equal(bare.termination_reason, ref.termination_reason) and torch.equal(bare.terminal_obs, ref.terminal_obs)
        fell |= bool(ref.termination_reason.any())
    assert fell
    for v in (ref, full, bare):
        v.close()


def test_termination_info_writes_only_its_outputs():
    """reason, values and terminal observations into buffers with guard words on either side, one at a time and all at once"""
    n, g = 5, 64
    _, cases = TC.states("hulls")
    v = make_vec(n)
    load(v, cases, fallen_idx(n, offset=11))
    v.set_termination(head_height=100.0, penalty=1.0)
    v.step_tensor(actions_for(n, 77, make_model()))
    want = (v.termination_reason.clone(), v.termination_values.clone(), v.terminal_obs.clone())
    assert (want[0] == 1).all() and torch.equal(want[2], v._term_buf[2]) and want[2].abs().sum() > 0
    wr = torch.full((n + 2 * g,), 7, dtype=torch.int32, device=DEV)
    (wv, vals), (wt, tobs) = guarded((n, 3), g), guarded((n, 3 * J), g)
    reason = wr[g:g + n]
    for args in ((reason, None, None), (None, vals, None), (None, None, tobs), (reason, vals, tobs)):
        v.batch.termination_info(*args)
        torch.cuda.synchronize()
        assert (wr[:g] == 7).all() and (wr[g + n:] == 7).all() and guards_intact(wv, (n, 3), g) and guards_intact(wt, (n, 3 * J), g)
    assert torch.equal(reason, want[0]) and torch.equal(vals, want[1]) and torch.equal(tobs, want[2])
    v.close()


def test_step_many_is_four_step_rows():
    n, S = 4, 4
    thr = TC.search("hulls")
    _, cases = TC.states("hulls")
    idx = fallen_idx(n, offset=5)
    acts = torch.stack([actions_for(n, 100 + t, make_model()) for t in range(S)])
    v = make_vec(n)
    load(v, cases, idx)
    v.set_termination(**thr_kwargs(thr, 1.5))
    rows, dones, reasons = [], [], []
    for s in range(S):
        v.step_tensor(acts[s])
        rows.append(v.rows.clone()); dones.append(v.done.clone()); reasons.append(v.termination_reason.clone())
    state = v.get_state().clone()
    v.close()
    assert torch.stack(reasons).any()
    m = make_vec(n)
    load(m, cases, idx)
    m.set_termination(**thr_kwargs(thr, 1.5))
    got = m.step_many_tensor(acts)
    done = torch.zeros(S, n, dtype=torch.bool, device=DEV)
    m2 = make_vec(n)
    load(m2, cases, idx)
    m2.set_termination(**thr_kwargs(thr, 1.5))
    rows2 = torch.empty(S, n, 3 * J + 2, device=DEV)
    m2.batch.step_many(acts, rows2, None, done)
    assert torch.equal(got, torch.stack(rows)) and torch.equal(rows2, got) and torch.equal(done, torch.stack(dones))
    assert torch.equal(m.get_state(), state) and torch.equal(m.done, dones[-1]) and torch.equal(m.termination_reason, reasons[-1])
    m.close()
    m2.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
SYNTHETIC = ("deep_chain", "big_body", "many_hulls")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    import synthetic_models as sm
    out = built_models(SYNTHETIC, tmp_path_factory)
    # a root with a hull, a link without a collision point, a link with ONE
    b = sm.Builder(tmp_path_factory.mktemp("few_points"), "few_points")
    rng = np.random.default_rng(4)
    b.link("root", 3.0, (0.2, 0.1, 0.05), hulls=[(sm.box_verts(rng, (0.2, 0.1, 0.05)), (0, 0, 0), (0, 0, 0))])
    b.link("bare", 1.0, (0.1, 0.02, 0.02))
    b.link("tip", 1.0, (0.1, 0.02, 0.02), hulls=[(np.array([[0.21, 0.01, -0.03]]), (0, 0, 0), (0, 0, 0))])
    b.joint("j_bare", "root", "bare", xyz=(0.2, 0, 0))
    b.joint("j_tip", "bare", "tip", xyz=(0.2, 0, 0), axis=(0, 0.6, 0.8))
    from oracle import trex_model as tm
    path = b.write()
    out["few_points"] = dict(path=path, props=dict(params=sm.SMALL_PARAMS), om=tm.compile_model(path))
    return out


@pytest.mark.parametrize("name", SYNTHETIC + ("few_points",))
def test_generated_models(name, built):
    """depth 6 (deep_chain, with a body without collision points), the big swept body, per-body scan units (many_hulls) and a
    model with a body of zero and of one collision point, at N = 3, one env 64 m from the origin: clearance and lowest point"""
    import dynamics_ref as DR
    from oracle import oracle as O
    m = built[name]
    om = m["om"]
    states, _ = DR.random_states(om, 3, seed=31)
    states[1][0:2] = [64.0, -64.0]
    states[2][2] = 1.0
    v = make_vec(3, urdf=m["path"], params=m["props"]["params"])
    v.reset()
    v.set_state(torch.tensor(np.array(states, np.float32)))
    orc = O.Oracle(om, params=m["props"]["params"])
    ref = [TR.evaluate(orc, om, s) for s in states]
    hs = np.diff(om["hull_start"])
    if name == "few_points":
        assert sorted(hs.tolist())[:2] == [0, 1]
    if name == "deep_chain":
        assert (hs == 0).any() and om["depth"].max() == 6
    c, low = query(v)
    w = clearance_dev(c, low, ref, states)
    print("%s K8 deviations: %s" % (name, {k: "%.3g" % x for k, x in w.items()}))
    assert w["clearance"] <= TOL["clearance"] and w["lowest"] <= TOL["lowest"]
    # a watched set of one body and of all bodies: values[2] on the judged state of one step
    with_pts = [int(b) for b in np.flatnonzero(hs > 0)]
    first_link = {int(b): l for l, b in reversed(list(enumerate(om["link_body"])))}
    for watched in ([with_pts[-1]], list(range(om["nb"]))):
        keep = {first_link[b]: 0.05 for b in watched}
        res = {}
        for on in (False, True):
            t = make_vec(3, urdf=m["path"], params=m["props"]["params"])
            t.reset()
            t.set_state(torch.tensor(np.array(states, np.float32)))
            if on:
                t.set_termination(keep_clear=keep)
            t.step_tensor(torch.zeros(3, om["nb"] - 1, device=DEV))
            res[on] = t.get_state().cpu().numpy() if not on else (t.termination_values.cpu().numpy().astype(np.float64), t.termination_reason.cpu().numpy())
            t.close()
        cm = np.full(om["nb"], np.nan)
        cm[watched] = np.float32(0.05)
        want = np.array([TR.margin(TR.evaluate(orc, om, s.astype(np.float64))["clearance"], cm) for s in res[False]])
        got, reason = res[True]
        dev = (np.abs(got[:, 2] - want) / np.array([scale_of(s) for s in res[False]])).max()
        print("%s margin deviation, %d watched: %.3g" % (name, len(watched), dev))
        assert dev <= TOL["margin"] and np.isfinite(want).all()
        assert (np.abs(want) > TOL["margin"] * 64).all() and np.array_equal(reason, np.where(want < 0, 4, 0))
    v.close()


def test_floor_height_and_no_watched_body():
    """floor_z = 0.3: every clearance 0.2995 lower than at the default 0.0005, against the reference; with no body watched
    values[2] is +inf and the head criterion still works"""
    built_, cases = TC.states("hulls")
    idx = TC.sample("hulls", 5)
    from oracle import oracle as O
    orc = O.Oracle(built_.om, params=dict(floor_z=0.3))
    v = make_vec(len(idx), params=dict(floor_z=0.3))
    load(v, cases, idx)
    c, low = query(v)
    ref = [TR.evaluate(orc, built_.om, cases[k]["state"].astype(np.float64)) for k in idx]
    w = clearance_dev(c, low, ref, [cases[k]["state"] for k in idx])
    assert w["clearance"] <= TOL["clearance"] and w["lowest"] <= TOL["lowest"]
    base = np.array([TC.reference("hulls")[k]["clearance"] for k in idx])
    fin = np.isfinite(base)
    assert np.abs(c[fin] - base[fin] + 0.2995).max() < 1e-5
    v.close()
    v = make_vec(len(idx))
    load(v, cases, idx)
    v.set_termination(head_height=50.0)
    v.step_tensor(actions_for(len(idx), 1, v.model))
    vals = v.termination_values.cpu().numpy()
    assert np.isinf(vals[:, 2]).all() and (vals[:, 2] > 0).all() and (v.termination_reason == 1).all()
    v.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from trex_gym import _capi
    n = 4
    env = make_vec(n)
    env.reset_tensor()
    b = env.batch
    E = _capi.E_INVALID
    refused = functools.partial(gpu_support.refused, E)
    clr = torch.full((n, NB), 7.0, device=DEV)
    low = torch.full((n, NB, 3), 7.0, device=DEV)
    refused(b.body_clearance, clr.cpu())
    refused(b.body_clearance, clr, low.cpu())
    refused(b.body_clearance, clr.double())
    refused(b.body_clearance, torch.empty(n, NB - 1, device=DEV))
    refused(b.body_clearance, clr, torch.empty(n, NB, 2, device=DEV))
    raw = _capi.lib.trex_batch_body_clearance
    assert raw(b.h, None, None, None) == E
    host = np.zeros(n * NB, np.float32)
    assert raw(b.h, C.c_void_p(host.ctypes.data), None, None) == E
    if torch.cuda.device_count() > 1:
        refused(b.body_clearance, torch.empty(n, NB, device="cuda:1"))
    # the raw C-ABI refuses short buffers by itself (the binding's check bypassed). On 65 536 envs the outputs are 6.8 MB and more
    # - more than the allocation a small tensor lives in, whatever the allocator pooled around it
    NBIG = 65536
    big = make_vec(NBIG)
    big.reset_tensor()
    good = torch.empty(NBIG, NB, device=DEV)
    short = torch.full((100,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert raw(big.batch.h, p(short), None, None) == E and raw(big.batch.h, p(good), p(short), None) == E
    # termination_info: never enabled; then short / host buffers
    info = _capi.lib.trex_batch_termination_info
    hp = C.c_void_p(host.ctypes.data)
    assert info(big.batch.h, None, None, None, None) == E
    big.batch.set_termination(head_height=0.1)
    assert info(big.batch.h, None, None, p(short), None) == E
    assert info(big.batch.h, hp, None, None, None) == E and info(big.batch.h, None, hp, None, None) == E
    assert info(big.batch.h, None, None, hp, None) == E
    big.close()
    torch.cuda.synchronize()
    assert (clr == 7.0).all() and (low == 7.0).all() and (short == 7.0).all()          # nothing was launched
    # bad arguments leave the setting as it was
    b.set_termination(head_height=0.2, penalty=1.0)
    nan = float("nan")
    st = _capi.lib.trex_batch_set_termination
    for args in ((float("inf"), nan, None, 0.0), (-float("inf"), nan, None, 0.0), (nan, 0.0, None, 0.0), (nan, -0.5, None, 0.0),
                 (nan, 3.2, None, 0.0), (nan, float("inf"), None, 0.0), (0.2, nan, None, nan), (0.2, nan, None, float("inf"))):
        assert st(b.h, *args) == E, args
    refused(b.set_termination, clear_min=[0.0] * (NB - 1))
    a = torch.zeros(n, J, device=DEV)
    obs, rew, done = torch.zeros(n, 3 * J, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    refused(b.time_steps, a, obs, rew, done, 2)
    refused(b.debug_step, a, obs, torch.zeros(4096, device=DEV))
    env.step_tensor(a)
    assert env.batch is b and not env._term_on                      # (set through the batch: the env's flag is its own)
    reason = torch.zeros(n, dtype=torch.int32, device=DEV)
    b.termination_info(reason)
    assert (reason == 0).all()                                       # the standing T-rex's head is above 0.2 m
    assert st(b.h, nan, np.pi, None, 0.0) == 0                        # pi itself is accepted
    b.set_termination()
    assert b.time_steps(a, obs, rew, done, 2) > 0
    env.close()


def test_stream_capture():
    """three steps with termination on inside torch.cuda.graph (linear, one stream), after eager warm-up calls; replayed twice
    from the same state: bitwise the eager run"""
    n = 8
    thr = TC.search("hulls")
    _, cases = TC.states("hulls")
    idx = fallen_idx(n, offset=5)
    acts = [actions_for(n, 100 + t, make_model()) for t in range(3)]
    start = torch.tensor(np.array([cases[k]["state"] for k in idx], np.float32), device=DEV)

    def run(v):
        for a in acts:
            v.step_tensor(a)
        return v.termination_reason, v.terminal_obs

    e = make_vec(n)
    load(e, cases, idx)
    e.set_termination(**thr_kwargs(thr, 1.5))
    r, t = run(e)
    want = [e.rows.clone(), e.done.clone(), e.get_state().clone(), r.clone(), t.clone()]
    e.close()
    v = make_vec(n)
    load(v, cases, idx)
    v.set_termination(**thr_kwargs(thr, 1.5))
    run(v)                                                           # the first calls: learn the buffers
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    v.batch.set_state(start)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run(v)
    for _ in range(2):
        v.batch.set_state(start)
        v.rows.zero_(); v.done.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [v.rows, v.done, v.get_state(), v._term_buf[0], v._term_buf[2]]
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    del graph
    v.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_python_surface():
    """step_wait's infos, support_bodies, body_clearance by link, the constructor argument"""
    from trex_gym import termination as T
    thr = TC.search("hulls")
    built_, cases = TC.states("hulls")
    n = 6
    idx = fallen_idx(n, offset=5)
    v = make_vec(n, terminate=thr_kwargs(thr, 2.0))
    assert v._term_on
    load(v, cases, idx)
    feet = T.support_bodies(v)
    names = [built_.om["body_names"][b] for b in feet]
    assert feet and all(("toe" in nm or "tarsometatarsus" in nm) for nm in names), names
    assert {("left" in nm) for nm in names} == {True, False}         # both feet
    whole = [built_.om["body_names"][b] for b in T.foot_bodies(v)]
    assert set(names) <= set(whole) and len(whole) == 14 and all(("toe" in nm or "tarsometatarsus" in nm) for nm in whole), whole
    fall = T.fall_bodies(v)
    lb = built_.om["link_body"]
    assert not set(int(lb[l]) for l in fall) & set(T.foot_bodies(v))
    assert len(fall) + len(whole) == int((np.diff(built_.om["hull_start"]) > 0).sum())
    assert {"link_cranium", "link_vertebrae_sacral"} <= {built_.om["body_names"][int(lb[l])] for l in fall}
    c_all = v.body_clearance()
    one = v.body_clearance("link_cranium")
    body = int(lb[list(built_.om["link_names"]).index("link_cranium")])
    assert tuple(c_all.shape) == (n, NB) and torch.equal(one, c_all[:, body])
    two, low = v.body_clearance(["link_cranium", 0], lowest=True)
    assert tuple(two.shape) == (n, 2) and tuple(low.shape) == (n, 2, 3) and torch.equal(two[:, 0], one)
    fired_any = False
    for t in range(6):
        obs, rew, done, infos = v.step(actions_for(n, 100 + t, v.model).cpu().numpy())
        reason = v.termination_reason.cpu().numpy()
        for i in range(n):
            if reason[i]:
                fired_any = True
                assert done[i] and infos[i]["termination"] == int(reason[i]) and "episode" in infos[i]
                assert infos[i]["terminal_observation"].shape == (3 * J,) and not np.array_equal(infos[i]["terminal_observation"], obs[i])
                assert T.reason_names(reason[i])
            else:
                assert "termination" not in infos[i] and "terminal_observation" not in infos[i]
    assert fired_any
    v.close()


def test_trainer_flags_with_graphs():
    """the --terminate_* flags build an env whose rollout the trainer replays as HIP graphs: envs fall, every figure stays finite,
    and the first rollout's reward is the eager trainer's"""
    import math
    from trex_gym import trex_train
    flags = ["--num_envs", "256", "--max_episode_steps", "200", "--terminate_head_height", "2.0", "--terminate_tilt", "1.0",
             "--terminate_contact", "auto", "--fall_penalty", "50"]
    hists = {}
    for graphs in (True, False):
        args = trex_train.parse_args(flags + (["--graphs"] if graphs else []))
        env = trex_train.environment_from_args(args)
        assert env._term_on
        _, hist = trex_train.train(env, 256 * 32 * (3 if graphs else 1), 0, nsteps=32, noptepochs=2, log=lambda s: None,
                                   use_graphs=graphs, preset="throughput")
        hists[graphs] = hist
        assert all(math.isfinite(h[k]) for h in hist for k in ("policy_loss", "value_loss", "entropy", "mean_step_reward"))
        if graphs:
            fallen_now = int((env.termination_reason != 0).sum())
            assert (env.terminal_obs.abs().sum(1) > 0).sum() >= max(fallen_now, 1)      # envs fell during the rollouts
            assert torch.isfinite(env.terminal_obs).all()
        env.close()
    a, b = hists[True][0]["mean_step_reward"], hists[False][0]["mean_step_reward"]
    assert abs(a - b) <= 2e-3 * abs(b)


def test_facade():
    from trex_gym.trex_env import TrexBulletEnv
    env = TrexBulletEnv(urdf_path=ASSET_URDF)
    env.reset()
    a = np.zeros(J, np.float32)
    assert env.step(a)[2] is False and env.should_terminate() is False
    c = env.body_clearance()
    assert c.shape == (NB,) and isinstance(env.body_clearance("link_cranium"), float)
    env.close()
    head = TrexBulletEnv(urdf_path=ASSET_URDF, terminate=dict(head_height=100.0, penalty=1.0))
    first = head.reset()
    obs, rew, done, info = head.step(a)
    assert done is True and head.should_terminate() is True and info == {"termination": 1}
    assert len(obs) == 3 * J and obs != first
    assert np.allclose(head.model.get_observations()[:J], first[:J], atol=1e-3)      # the env is on its next episode
    head.reset()
    assert head.should_terminate() is False
    head.close()
