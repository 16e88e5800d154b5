"""The step kernel, the chain walk and the kernels around them on the generated models of tests/synthetic_models.py: the branches
that depend on the compiled model and that the T-rex asset never takes - the sixth tree level, swept bodies (over 1024 vertices, or
no mask words left), the per-body scan units, oblique joint axes, 4 children below the base - against the f64 oracle.

Tolerances: those stated at the top of tests/test_gpu_parity.py (parity_helpers.assert_step_close). The generated bodies weigh
kilograms and their motors are limited to 40 N m, so the T-rex's absolute torque floor (+1 N m) is replaced by 3 x the deviation of
the oracle's own f32 build on the same state (the rule of test_k_steps_through_contact...); the relative part stays. Contact
wrench: the rule of test_sensor_matches_the_oracle (4 x the f32 oracle's spread, floor 1e-3 M g). Dynamics queries: 4 x the largest
deviation measured on these states (MEASURED below, profiles/r14_synthetic_models.txt), never above the caps of
tests/test_gpu_dynamics.py."""
import numpy as np
import pytest
import torch

import dynamics_ref as R
import gpu_support
import synthetic_models as sm
from dynamics_model_cases import cent_dev
from gpu_support import DEV
from parity_helpers import assert_step_close, oracle_wrench
from state_sets import query_states

pytestmark = pytest.mark.gpu
G = 9.81

# largest deviations on an MI355X over the states of test_queries_outside_the_step (profiles/r14_synthetic_models.txt)
MEASURED = dict(deep_chain=dict(id_zero=6.93e-7, mass=7.75e-7, jac=2.63e-7, cent=3.71e-7, link=4.33e-7),
                bushy=dict(id_zero=3.55e-7, mass=6.06e-7, jac=1.15e-7, cent=2.78e-7, link=5.29e-7))
CAPS = dict(id_zero=1e-4, mass=1e-5, jac=1e-4, cent=1e-4, link=1e-5)
REST_MEASURED = 4.52e-8     # |sum F_z - M g| / M g of the resting slab after 60 env-steps, kernel


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> dict(path, props, om, params, states, actions, o64, o32): built once, shared, never changed"""
    from oracle import oracle as O
    out = {}
    for n in sm.MODELS:
        path, props, om = sm.compile_both(n, tmp_path_factory.mktemp(n))
        ss = sm.state_set(n, om, props["params"])
        out[n] = dict(path=path, props=props, om=om, params=props["params"], states=ss["states"], actions=ss["actions"],
                      o64=O.Oracle(om, params=props["params"]), o32=O.Oracle(om, params=props["params"], precision="f32"))
    return out


def make_vec(m, n, **kw):
    params = dict(m["params"], **kw.pop("params", {}))
    return gpu_support.make_vec(n, m["path"], params=params, **kw)


def loaded(m, n=None, **kw):
    """n envs holding the model's states, cycled"""
    n = len(m["states"]) if n is None else n
    v = make_vec(m, n, **kw)
    v.reset()
    idx = np.arange(n) % len(m["states"])
    v.set_state(torch.tensor(m["states"][idx]))
    return v, torch.tensor(m["actions"][idx], device=DEV)


# ---------------------------------------------------------------- 1. one step, contact count, sensor against the oracle
@pytest.mark.parametrize("name", list(sm.MODELS))
def test_one_step_and_contacts_match_the_oracle(name, built):
    m = built[name]
    om, o64, o32 = m["om"], m["o64"], m["o32"]
    J, nb = om["nb"] - 1, om["nb"]
    fmax = float(m["params"]["motor_max_force"])
    v, acts = loaded(m)
    v.enable_contact_sensor()
    obs, rew, _ = v.step_tensor(acts)
    obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
    cnt = torch.zeros(v.num_envs, dtype=torch.int32, device=DEV)
    v.batch.contact_stats(cnt, None)
    cnt = cnt.cpu().numpy()
    gw = v.contact_wrench().cpu().numpy().astype(np.float64)
    Mg = om["mass"].sum() * G
    worst = dict(dq=0.0, dqd=0.0, dtau=0.0, drew=0.0, wrench=0.0, spread=0.0)
    werr, wspread, in_contact = [], [], 0
    for k, (s, a) in enumerate(zip(m["states"], m["actions"])):
        o, r, c = sm.oracle_step_contacts(o64, s, a)
        o3, _, _ = sm.oracle_step_contacts(o32, s, a)
        ot = o[2 * J:]
        unsat = np.abs(ot) < 0.999 * fmax
        extra = 3.0 * np.abs(o3[2 * J:] - ot)[unsat].max() if unsat.any() else 0.0
        worst["dq"] = max(worst["dq"], np.abs(obs[k, :J] - o[:J]).max())
        worst["dqd"] = max(worst["dqd"], np.abs(obs[k, J:2 * J] - o[J:2 * J]).max() / max(1.0, np.abs(o[J:2 * J]).max()))
        if unsat.any():
            worst["dtau"] = max(worst["dtau"], np.abs(obs[k, 2 * J:] - ot)[unsat].max())
        worst["drew"] = max(worst["drew"], abs(rew[k] - r) / max(abs(r), 1e-9))
        w64, _ = oracle_wrench(o64, om, s, a)
        w32, _ = oracle_wrench(o32, om, s, a)
        werr.append(np.abs(gw[k] - w64).max() / Mg)
        wspread.append(np.abs(w32 - w64).max() / Mg)
        print("%s state %2d: contacts gpu %2d oracle %2d; dq %.1e dqd %.1e; wrench/Mg gpu-f64 %.1e f32-f64 %.1e"
              % (name, k, cnt[k], len(c[0]), np.abs(obs[k, :J] - o[:J]).max(), np.abs(obs[k, J:2 * J] - o[J:2 * J]).max(),
                 werr[-1], wspread[-1]))
        assert_step_close(obs[k], o, rew[k], r, "%s state %d" % (name, k), J=J, max_force=fmax, tau_floor=0.0, tau_extra=extra)
        assert cnt[k] == len(c[0]), (name, k)
        assert set(np.flatnonzero(np.abs(gw[k]).max(1) > 0)) == set(np.flatnonzero(np.abs(w64).max(1) > 0)), (name, k)
        in_contact += len(c[0]) > 0
    tol = max(4 * max(wspread), 1e-3)
    print("%s: max dq %.2e dqd/scale %.2e dtau %.2e N m drew %.2e; wrench/Mg gpu-f64 %.2e f32-f64 %.2e tol %.2e; %d of %d in contact"
          % (name, worst["dq"], worst["dqd"], worst["dtau"], worst["drew"], max(werr), max(wspread), tol, in_contact, len(werr)))
    assert in_contact >= len(werr) // 2
    assert max(werr) <= tol
    v.close()


@pytest.mark.parametrize("name", ["big_body", "full_masks", "deep_chain", "many_hulls", "bushy"])
def test_contact_points_of_the_debug_dump(name, built):
    """Every touching state alone in env 0 through trex_batch_debug_step with ONE substep: the points of the dump at [960 + 16 c ..)
    against Oracle.contacts - body and order exact (ties go to the lowest vertex index on both sides; the generated hulls are
    jittered so that there are none), position and distance to 1e-5 m."""
    from oracle import oracle as O
    from trex_gym import _capi
    m = built[name]
    om = m["om"]
    J = om["nb"] - 1
    params = dict(m["params"], substeps=1)
    orc = O.Oracle(om, params=params)
    cm = _capi.Model(m["path"])
    for k, val in params.items():
        cm.set_param(k, val)
    b = _capi.Batch(cm, 1)
    touching = [k for k in range(len(m["states"])) if len(sm.oracle_step_contacts(orc, m["states"][k], m["actions"][k])[2][0])]
    seen = set()
    for k in touching:
        s, a = m["states"][k], m["actions"][k]
        b.set_state(torch.tensor(s[None], device=DEV))
        b.set_motors_enabled(1)
        obs, dbg = torch.zeros(1, 3 * J, device=DEV), torch.zeros(4096, device=DEV)
        b.debug_step(torch.tensor(a[None], device=DEV), obs, dbg)
        D = dbg.cpu().numpy().astype(np.float64)
        _, _, (cb, lam, pos, dist) = sm.oracle_step_contacts(orc, s, a)
        nc = int(D[128])
        assert nc == len(cb), (name, k, nc, len(cb))
        gb = D[960 + 16 * np.arange(nc)].astype(int)
        gx = np.stack([D[960 + 16 * c + 1:960 + 16 * c + 4] for c in range(nc)]) + s[:3].astype(np.float64)
        gd = D[960 + 16 * np.arange(nc) + 4]
        assert list(gb) == list(cb), (name, k, gb, cb)
        print("%s state %2d: %2d points, position %.1e distance %.1e" % (name, k, nc, np.abs(gx - pos).max(), np.abs(gd - dist).max()))
        assert np.abs(gx - pos).max() <= 1e-5 and np.abs(gd - dist).max() <= 1e-5, (name, k)
        seen |= set(gb)
    for body in m["props"].get("swept", []):
        assert body in seen, (name, body)
    b.close()


# ---------------------------------------------------------------- 2. launch forms, bitwise
def _outputs(v):
    cnt, imp = torch.zeros(v.num_envs, dtype=torch.int32, device=DEV), torch.zeros(v.num_envs, device=DEV)
    v.batch.contact_stats(cnt, imp)
    return [v.rows.clone(), v.get_state(), cnt, imp]


@pytest.mark.parametrize("feature", ["plain", "warmstart", "sensor", "wrench"])
@pytest.mark.parametrize("name", ["big_body", "full_masks", "deep_chain"])
def test_launch_forms_agree_bitwise(name, feature, built):
    """pair form (64 envs) = single form (65 envs, the first 64) = step_many, over 4 steps from the model's states: plain, with the
    PGS warm start (the record's key is the hull vertex - of a swept body too), with the sensor on, with a zero external wrench."""
    m = built[name]
    S = 4

    def prepare(n):
        v, acts = loaded(m, n, params={"warmstart": 0.8} if feature == "warmstart" else {})
        if feature == "sensor":
            v.enable_contact_sensor()
        if feature == "wrench":
            v.set_external_wrench(torch.zeros(n, m["om"]["nb"], 6))
        return v, acts
    a, acts = prepare(64)
    if feature == "plain":
        assert a.batch.launch_info()["block"] == 128
    b, acts65 = prepare(65)
    assert b.batch.launch_info()["block"] == 64
    per_step = []
    for _ in range(S):
        a.step_tensor(acts)
        b.step_tensor(acts65)
        per_step.append(a.rows.clone())
        for x, y in zip(_outputs(a), _outputs(b)):
            assert torch.equal(x, y[:64]), (name, feature)
        if feature == "sensor":
            assert torch.equal(a.contact_wrench(), b.contact_wrench()[:64])
    c, _ = prepare(64)
    rows = c.step_many_tensor(acts.unsqueeze(0).expand(S, -1, -1).contiguous())
    for s_ in range(S):
        assert torch.equal(rows[s_], per_step[s_]), (name, feature, s_)
    assert torch.equal(c.get_state(), a.get_state())
    if feature == "sensor":
        assert torch.equal(c.contact_wrench(), a.contact_wrench())
    assert int(_outputs(a)[2].max()) >= 8
    if feature == "plain":       # the envs hold different states: the outputs differ, and a feature that must not change them does not
        assert not torch.equal(a.rows[0], a.rows[3])
    for v in (a, b, c):
        v.close()


@pytest.mark.parametrize("name", ["big_body", "full_masks", "deep_chain"])
def test_features_leave_the_physics_bitwise_unchanged(name, built):
    m = built[name]
    ref = None
    for feature in ("plain", "sensor", "wrench"):
        v, acts = loaded(m, 64)
        if feature == "sensor":
            v.enable_contact_sensor()
        if feature == "wrench":
            v.set_external_wrench(torch.zeros(64, m["om"]["nb"], 6))
        for _ in range(3):
            v.step_tensor(acts)
        out = _outputs(v)
        if ref is None:
            ref = out
        for x, y in zip(ref, out):
            assert torch.equal(x, y), (name, feature)
        v.close()


# ---------------------------------------------------------------- 3. kernels outside the step
@pytest.mark.parametrize("name", ["deep_chain", "bushy"])
def test_queries_outside_the_step(name, built):
    """link_transforms and head_position against the oracle's body poses; inverse_dynamics, mass_matrix, jacobian (the deepest link,
    at its origin and at an offset point) and centroidal against tests/dynamics_ref.py, at random airborne states. Scales as in
    tests/test_gpu_dynamics.py."""
    from oracle import trex_model as tm
    m = built[name]
    om, o64 = m["om"], m["o64"]
    states = query_states(om)
    v = make_vec(m, len(states))
    v.reset()
    v.set_state(torch.tensor(np.array(states, np.float32)))
    lt = v.link_transforms().cpu().numpy().astype(np.float64)
    head = v.head_position().cpu().numpy().astype(np.float64)
    h_gpu = v.inverse_dynamics().cpu().numpy().astype(np.float64)
    M_gpu = v.mass_matrix()
    assert torch.equal(M_gpu, M_gpu.transpose(1, 2).contiguous())
    M_gpu = M_gpu.cpu().numpy().astype(np.float64)
    c_gpu = v.centroidal().data.cpu().numpy().astype(np.float64)
    deep = int(np.argmax(om["depth"]))
    link = [l for l in range(len(om["link_names"])) if om["link_body"][l] == deep][0]
    assert om["depth"][deep] == 6
    loc = (0.07, -0.02, 0.03)
    jac = [v.jacobian(link, p).cpu().numpy().astype(np.float64) for p in (None, loc)]
    dev = dict(id_zero=0.0, mass=0.0, jac=0.0, cent=0.0, link=0.0)
    for e, s in enumerate(states):
        os_ = o64.new_state()
        o64.set_state(os_, s)
        pos, rot = o64.body_poses(os_)
        for l in range(len(om["link_names"])):
            bb, tf = om["link_body"][l], om["link_tf"][l]
            Rl, pl = rot[bb] @ tf[:9].reshape(3, 3), pos[bb] + rot[bb] @ tf[9:12]
            dev["link"] = max(dev["link"], np.abs(lt[e, l, :3] - pl).max(), np.abs(tm.quat_to_matrix(lt[e, l, 3:]) - Rl).max())
        dev["link"] = max(dev["link"], np.abs(head[e] - o64.head_position(os_)).max())
        h = R.inverse_dynamics(om, s, None, None, G)
        dev["id_zero"] = max(dev["id_zero"], R.block_dev(h_gpu[e], h, np.abs(h[:6]).max(), np.abs(h[6:]).max()))
        M = R.mass_matrix(om, s)
        dg = np.sqrt(np.diag(M))
        dev["mass"] = max(dev["mass"], (np.abs(M_gpu[e] - M) / np.outer(dg, dg)).max())
        for Jg, p in zip(jac, ((0.0, 0.0, 0.0), loc)):
            Jr = R.jacobian(om, s, link, p)
            dev["jac"] = max(dev["jac"], np.abs(Jg[e] - Jr).max() / np.abs(Jr).max())
        dev["cent"] = max(dev["cent"], cent_dev(c_gpu[e], R.centroidal(om, s, None, G)))
    print("%s queries, largest deviations: %s" % (name, {k: "%.3g" % x for k, x in dev.items()}))
    for k, x in dev.items():
        assert x <= min(4 * MEASURED[name][k], CAPS[k]), (name, k, x)
    v.close()


def test_render_of_many_hulls(built):
    """depth and segmentation of the 36-hull model against tests/render_ref.py at one small frame, resting on the floor"""
    import render_ref as rr
    from trex_gym.render import Camera
    from gpu_render_support import render_compare
    m = built["many_hulls"]
    v, _ = loaded(m, 2)
    v.set_state(torch.tensor(m["states"][[-1, len(m["states"]) // 2]]))
    scene = rr.Scene.from_model(v.model)
    cam = Camera(distance=1.6, yaw=40.0, pitch=-35.0, fov=55.0, near=0.1, far=10.0)
    W, H = 64, 48
    rgb, dep, seg = v.render_tensor(None, W, H, cam, depth=True, segmentation=True)
    rgb, dep, seg = rgb.cpu().numpy(), dep.cpu().numpy(), seg.cpu().numpy()
    lt, st = v.link_transforms().cpu().numpy(), v.get_state().cpu().numpy()
    lb, ltf = v.model.array("link_body"), v.model.array("link_tf")
    for e in range(2):
        Rb, pb = rr.body_poses(lt[e], lb, ltf, v.model.num_bodies)
        eye, dirs, _ = rr.camera_rays(cam.distance, cam.yaw, cam.pitch, cam.fov, W, H, st[e, :3])
        render_compare((rgb[e], dep[e], seg[e]), rr.render(scene, Rb, pb, eye, dirs, cam.near, cam.far), ("many_hulls", e))
        assert len(set(seg[e][seg[e] >= 0])) >= 4 and (seg[e] == -1).sum() > 100
    v.close()


# ---------------------------------------------------------------- 4. two anchors that do not use the oracle's results
def _slab_rest_residual(step, weight, steps=60):
    """relative residual of the carried weight after `steps` steps at rest; step() -> summed normal force of the last step"""
    f = 0.0
    for _ in range(steps):
        f = step()
    return abs(f - weight) / weight


def _oracle_slab(m, margin):
    from oracle import oracle as O
    return O.Oracle(m["om"], params=dict(m["params"], contact_margin=margin))


@pytest.mark.parametrize("margin", [0.02, 0.005])
def test_slab_at_rest_carries_its_weight(margin, built):
    """motors at zero force; the sensor's summed normal force = M g. The oracle's own residual is computed first (from its
    contact impulses); the kernel is allowed twice that."""
    m = built["slab"]
    om = m["om"]
    W = om["mass"].sum() * G
    orc = _oracle_slab(m, margin)
    start = sm.flat_state(om, 0.0506)
    s = orc.new_state()
    orc.set_state(s, start)
    orc.set_motors_on(s, 1)

    def ostep():
        return oracle_wrench(orc, om, None, np.zeros(1), oracle_state=s)[0][:, 2].sum()
    res_o = _slab_rest_residual(ostep, W)
    v = make_vec(m, 2, params=dict(contact_margin=margin))
    v.reset()
    v.set_state(torch.tensor(np.tile(start.astype(np.float32), (2, 1))))
    v.enable_contact_sensor()
    a = torch.zeros(2, 1, device=DEV)

    def gstep():
        v.step_tensor(a)
        return float(v.contact_wrench()[0, :, 2].double().sum())
    res_g = _slab_rest_residual(gstep, W)
    print("slab at rest, margin %.3f: residual of M g oracle %.2e kernel %.2e" % (margin, res_o, res_g))
    assert res_o < 1e-2                       # the oracle itself carries the weight
    # (the f64 oracle's residual is at 1e-14, below what f32 impulses can hold; the floor is 4 x the kernel's residual as measured
    # on an MI355X, REST_MEASURED, profiles/r14_synthetic_models.txt)
    assert res_g <= 2 * res_o + 4 * REST_MEASURED
    v.close()


@pytest.mark.parametrize("margin", [0.02, 0.005])
def test_sliding_slab_decelerates_at_friction_times_g(margin, built):
    """launched along +x at 0.8 m/s with motors at zero force: the base decelerates at friction x g until it stops. Measured as the
    velocity lost over 10 env-steps (0.1 s) in the sliding phase, oracle first; the kernel is allowed twice the oracle's residual."""
    m = built["slab"]
    om = m["om"]
    orc = _oracle_slab(m, margin)
    mu, dt_env = orc.params["friction"], orc.params["dt"] * orc.params["substeps"]
    start = sm.flat_state(om, 0.0506, v=(0.8, 0, 0))
    settle, span = 5, 10

    def residual(vx):
        decel = (vx[settle] - vx[settle + span]) / (span * dt_env)
        return abs(decel - mu * G) / (mu * G)
    s = orc.new_state()
    orc.set_state(s, start)
    orc.set_motors_on(s, 1)
    vx_o = []
    for t in range(60):
        vx_o.append(orc.get_state(s)[7])
        orc.step(s, np.zeros(1))
    v = make_vec(m, 2, params=dict(contact_margin=margin))
    v.reset()
    v.set_state(torch.tensor(np.tile(start.astype(np.float32), (2, 1))))
    a = torch.zeros(2, 1, device=DEV)
    vx_g = []
    for t in range(60):
        vx_g.append(float(v.get_state()[0, 7]))
        v.step_tensor(a)
    res_o, res_g = residual(vx_o), residual(vx_g)
    print("sliding slab, margin %.3f: residual of mu g oracle %.2e kernel %.2e; final vx oracle %.1e kernel %.1e"
          % (margin, res_o, res_g, vx_o[-1], vx_g[-1]))
    assert vx_o[settle + span] > 0.2 and res_o < 2e-2      # still sliding over the window; the oracle itself decelerates at mu g
    assert res_g <= 2 * res_o
    # ... until it stops (0.8 / (mu g) = 0.33 s): below 1 % of the launch speed at the same env-step as the oracle, and from then on
    stop_o = min(t for t in range(60) if abs(vx_o[t]) < 8e-3)
    stop_g = min(t for t in range(60) if abs(vx_g[t]) < 8e-3)
    assert abs(stop_g - stop_o) <= 1 and max(abs(x) for x in vx_g[stop_g:]) < 8e-3 and max(abs(x) for x in vx_o[stop_o:]) < 8e-3
    v.close()
