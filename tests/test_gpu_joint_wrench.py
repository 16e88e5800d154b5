"""The joint force/torque sensor on the device (include/trex_joint_wrench.h): trex_batch_joint_wrench against the f64 reference of
tests/joint_wrench_ref.py on the T-rex and the four generated models of tests/dynamics_model_cases.py, identities on the device's
outputs alone, the batch shapes where the tiling can go wrong, robustness, trex_batch_generalized_velocity bitwise against the
torch expression, and the attached sensor of trex_gym.joint_sensor.

Every bound comes from the reference, none from the device (tests/joint_wrench_cases.py): min(1e-4, max(DYNAMICS_TOL["id_zero"],
4 x d32)), d32 the deviation of the reference's own f32 run from its f64 run on the model's cases; the identities likewise from the
f32 run's own residual. tests/test_joint_wrench_ref.py shows the cap never binds and the bound tells four mistakes by 10 x."""
import ctypes as C

import numpy as np
import pytest
import torch

import joint_wrench_cases as JC
from gpu_support import DEV, guarded, guards_intact, loaded_vec, make_vec, random_actions, replay_equals_eager, same_bits

pytestmark = pytest.mark.gpu


def api_of(v):
    from trex_gym.joint_wrench_capi import BatchJointWrench
    return BatchJointWrench(v.batch)


def env_of(m, cases, n=None):
    kw = {} if m["path"] is None else dict(urdf=m["path"], params=m["props"]["params"])
    return loaded_vec(cases, n=n, nb=m["om"]["nb"], **kw)


def dev_inputs(inp, n):
    """(acc, wa, wb) of the first n envs on the device, env e holding case e % 12"""
    idx = np.arange(n) % JC.N
    return tuple(torch.tensor(inp[k][idx]).to(DEV) for k in ("acc", "wa", "wb"))


def device_outputs(v, inp):
    """{(variant, axes): (rows [n, J, 6], base [n, 6])} device tensors, as joint_wrench_cases.reference_outputs lays them out"""
    api, n = api_of(v), v.num_envs
    acc, wa, wb = dev_inputs(inp, n)
    out = {}
    for name, (ua, uwa, uwb) in JC.VARIANTS.items():
        for ax in JC.AXES:
            base = torch.zeros(n, 6, device=DEV)
            rows = api.joint_wrench(acc if ua else None, wa if uwa else None, wb if uwb else None, ax, None, base)
            out[name, ax] = (rows, base)
    return out


def as_numpy(out):
    return {k: (r.cpu().numpy(), b.cpu().numpy()) for k, (r, b) in out.items()}


@pytest.fixture(scope="module")
def built(tmp_path_factory, model):
    return JC.built(tmp_path_factory, model)


@pytest.fixture(scope="module")
def runs(built):
    """name -> (case, the env of 12, its device outputs, the same as numpy), made on first use; the envs are closed at the end"""
    made = {}

    def get(name):
        if name not in made:
            c = JC.case(name, built[name]["om"])
            v = env_of(built[name], c["inp"]["cases"])
            out = device_outputs(v, c["inp"])
            made[name] = (c, v, out, as_numpy(out))
        return made[name]
    yield get
    for _, v, _, _ in made.values():
        v.close()


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", JC.MODELS)
def test_against_reference_n12(name, runs):
    """12 states - three full workgroups, the last two with a per-body mass scale -, every variant of accel / wrench_a / wrench_b
    NULL and given, world and link axes, the joint rows and the base row: within the bound the reference's f32 run sets"""
    c, v, out, got = runs(name)
    assert tuple(out["all", "link"][0].shape) == (JC.N, v.J, 6) and v.J == c["om"]["nb"] - 1
    assert all(torch.isfinite(r).all() and torch.isfinite(b).all() for r, b in out.values())
    devs = {key: float(JC.deviation(*got[key], *c["ref"][key], c["inp"]["weight"]).max()) for key in c["ref"]}
    print("%s: largest deviation %.3g of %s (d32 %.3g, bound %.3g)" % (name, max(devs.values()), max(devs, key=devs.get), c["d32"], c["bound"]))
    for key, d in devs.items():
        assert d <= c["bound"], (name, key, d, c["bound"])


@pytest.mark.parametrize("name", ("trex", "mount_first"))
def test_two_wrenches_are_their_sum(name, runs):
    """wrench_a + wrench_b is bitwise their f32 sum passed as one, in either place"""
    c, v, out, _ = runs(name)
    api = api_of(v)
    acc, wa, wb = dev_inputs(c["inp"], JC.N)
    for ax in JC.AXES:
        rows, base = out["all", ax]
        for a, b in ((wa + wb, None), (None, wa + wb), (wb, wa)):
            base1 = torch.zeros(JC.N, 6, device=DEV)
            rows1 = api.joint_wrench(acc, a, b, ax, None, base1)
            assert same_bits(rows1, rows) and same_bits(base1, base), (name, ax)
    assert not torch.equal(out["all", "world"][0], out["accel", "world"][0])


# ---------------------------------------------------------------- 2. identities on the device's outputs alone
@pytest.mark.parametrize("name", JC.MODELS)
def test_identities(name, runs):
    """no reference: the moment's component along the joint axis - in link axes the model's constant axis - is the joint entry of
    trex_batch_inverse_dynamics, base_out its base rows; with accel = forward_dynamics(force) they return the force"""
    c, v, out, got = runs(name)
    inp, om = c["inp"], c["om"]
    acc = torch.tensor(inp["acc"]).to(DEV)
    res_id = JC.axis_residual(om, inp, *got["accel", "link"], v.inverse_dynamics(acc).cpu().numpy())
    res_h = JC.axis_residual(om, inp, *got["static", "link"], v.inverse_dynamics().cpu().numpy())
    force = torch.tensor(c["forces"]).to(DEV)
    base = torch.zeros(JC.N, 6, device=DEV)
    rows = api_of(v).joint_wrench(v.forward_dynamics(force), None, None, "link", None, base)
    res_fd = JC.axis_residual(om, inp, rows.cpu().numpy(), base.cpu().numpy(), c["forces"])
    print("%s identities: id %.3g, bias %.3g (f32 run %.3g, bound %.3g); fd %.3g (f32 run %.3g, bound %.3g)"
          % (name, res_id, res_h, c["res32"][0], c["id_bound"][0], res_fd, c["res32"][1], c["id_bound"][1]))
    assert res_id <= c["id_bound"][0] and res_h <= c["id_bound"][0], (name, res_id, res_h, c["id_bound"][0])
    assert res_fd <= c["id_bound"][1], (name, res_fd, c["id_bound"][1])


# ---------------------------------------------------------------- 3. shapes where the tiling can go wrong
@pytest.mark.parametrize("name", ("trex", "slab"))
@pytest.mark.parametrize("n", [1, 4, 5, 67])
def test_batch_shapes(n, name, built, runs):
    """N = 1, 4 (one full workgroup), 5 (a last workgroup of one env), 67: env e holds case e % 12, and its rows are bitwise those of
    the N = 12 call - a row does not depend on the batch around it. N = 67: env 66 also against its state ALONE in a batch of one.
    N = 5: both outputs into guarded buffers, on and 4 bytes off the 16-byte grid: guards intact, the same bits."""
    c, _, full, _ = runs(name)
    inp = c["inp"]
    v = env_of(built[name], inp["cases"], n)
    out = device_outputs(v, inp)
    idx = torch.arange(n) % JC.N
    for key, (rows, base) in out.items():
        assert same_bits(rows, full[key][0][idx]) and same_bits(base, full[key][1][idx]), (name, n, key)
    if n == 67:
        alone = env_of(built[name], inp["cases"][66 % JC.N:][:1])
        acc, wa, wb = (t[66 % JC.N:][:1].contiguous() for t in dev_inputs(inp, JC.N))
        base = torch.zeros(1, 6, device=DEV)
        rows = api_of(alone).joint_wrench(acc, wa, wb, "link", None, base)
        assert same_bits(rows, out["all", "link"][0][66:67]) and same_bits(base, out["all", "link"][1][66:67])
        alone.close()
    if n == 5:
        api = api_of(v)
        acc, wa, wb = dev_inputs(inp, n)
        for guard, rest in ((64, 0), (65, 4)):
            whole_r, rows = guarded((n, v.J, 6), guard)
            whole_b, base = guarded((n, 6), guard)
            assert rows.data_ptr() % 16 == rest and base.data_ptr() % 16 == rest
            api.joint_wrench(acc, wa, wb, "link", rows, base)
            torch.cuda.synchronize()
            assert guards_intact(whole_r, (n, v.J, 6), guard) and guards_intact(whole_b, (n, 6), guard), (name, guard)
            assert same_bits(rows, out["all", "link"][0]) and same_bits(base, out["all", "link"][1]), (name, guard)
    v.close()


# ---------------------------------------------------------------- 4. robustness
def test_nan_env_stays_in_its_rows(built, runs):
    """a NaN state in env 5: its own rows are not finite, every other env's are bitwise what they were"""
    c, _, full, _ = runs("trex")
    v = env_of(built["trex"], c["inp"]["cases"])
    st = v.get_state()
    st[5, 13 + 3] = float("nan")
    v.set_state(st)
    out = device_outputs(v, c["inp"])
    keep = torch.tensor([e for e in range(JC.N) if e != 5])
    for key, (rows, base) in out.items():
        assert same_bits(rows[keep], full[key][0][keep]) and same_bits(base[keep], full[key][1][keep]), key
        assert not torch.isfinite(rows[5]).all()
    v.close()


def test_the_calls_write_their_outputs_only(model):
    """state, rows and the contact sensor's record are bitwise unchanged by both calls; an env that is queried steps as one that is not"""
    n = 6
    pair = []
    for probe in (False, True):
        v = make_vec(n)
        v.enable_contact_sensor(True)
        v.reset_tensor()
        gen = torch.Generator(device=DEV).manual_seed(3)
        api = api_of(v)
        latch = torch.zeros(n, 6 + v.J, device=DEV)
        for _ in range(4):
            v.step_tensor(random_actions(model, n, gen))
            if probe:
                before = (v.get_state(), v.rows.clone(), v.contact_wrench().clone())
                acc = torch.zeros(n, 6 + v.J, device=DEV)
                api.generalized_velocity(latch, latch, 50.0, v.rows, 3 * v.J + 1, acc)
                rows = api.joint_wrench(acc, v.contact_wrench(), None)
                assert torch.isfinite(rows).all()
                for x, y in zip(before, (v.get_state(), v.rows, v.contact_wrench())):
                    assert same_bits(x, y)
        pair.append((v.get_state(), v.rows.clone(), v.contact_wrench().clone()))
        v.close()
    for x, y in zip(*pair):
        assert same_bits(x, y)


def test_refusals():
    """BASE axes, out NULL, host memory, a buffer one float short - each TREX_E_INVALID with nothing launched"""
    from trex_gym import _capi as capi
    from trex_gym import joint_wrench_capi as M
    n = 5
    v = make_vec(n)
    v.reset_tensor()
    b, lib = v.batch, capi.lib
    J, D, nb = v.J, 6 + v.J, v.model.num_bodies
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    SENT = 7.0
    out, base = torch.full((n, J, 6), SENT, device=DEV), torch.full((n, 6), SENT, device=DEV)
    vel, acc = torch.full((n, D), SENT, device=DEV), torch.full((n, D), SENT, device=DEV)
    wr, prev = torch.zeros(n, nb, 6, device=DEV), torch.zeros(n, D, device=DEV)
    done = torch.zeros(n, device=DEV)
    jw = lambda a, wa, wb, axes, o, bo: lib.trex_batch_joint_wrench(b.h, a, wa, wb, axes, o, bo, s)
    gv = lambda ve, pr, dn, st, ac: lib.trex_batch_generalized_velocity(b.h, ve, pr, 50.0, dn, st, ac, s)
    assert jw(ptr(prev), ptr(wr), ptr(wr), 1, ptr(out), ptr(base)) == 0 and gv(ptr(vel), ptr(prev), ptr(done), 1, ptr(acc)) == 0   # the calls work at all
    torch.cuda.synchronize()
    for t in (out, base, vel, acc):
        t.fill_(SENT)
    assert jw(None, None, None, 2, ptr(out), None) == capi.E_INVALID                 # TREX_AXES_BASE
    assert jw(None, None, None, 3, ptr(out), None) == capi.E_INVALID and jw(None, None, None, -1, ptr(out), None) == capi.E_INVALID
    assert jw(None, None, None, 1, None, ptr(base)) == capi.E_INVALID                # out NULL
    assert gv(None, None, None, 0, None) == capi.E_INVALID                           # nothing asked for
    assert gv(ptr(vel), ptr(prev), None, 0, None) == capi.E_INVALID                  # prev without accel
    assert gv(ptr(vel), None, None, 0, ptr(acc)) == capi.E_INVALID                   # accel without prev
    assert gv(ptr(vel), ptr(prev), ptr(done), 0, ptr(acc)) == capi.E_INVALID         # done with a stride of 0
    assert gv(ptr(vel), ptr(prev), None, 0, ptr(vel)) == capi.E_INVALID              # accel on top of vel
    assert gv(C.c_void_p(vel.data_ptr() + 4), ptr(vel), None, 0, ptr(acc)) == capi.E_INVALID   # vel overlaps prev and is not prev
    host = np.zeros(n * nb * 6, np.float32)
    hp = C.c_void_p(host.ctypes.data)
    for call in (lambda p: jw(p, None, None, 1, ptr(out), None), lambda p: jw(None, p, None, 1, ptr(out), None),
                 lambda p: jw(None, None, p, 1, ptr(out), None), lambda p: jw(None, None, None, 1, p, None),
                 lambda p: jw(None, None, None, 1, ptr(out), p), lambda p: gv(p, None, None, 0, None),
                 lambda p: gv(ptr(vel), p, None, 0, ptr(acc)), lambda p: gv(ptr(vel), ptr(prev), p, 1, ptr(acc)),
                 lambda p: gv(ptr(vel), ptr(prev), None, 0, p)):
        assert call(hp) == capi.E_INVALID
    hip = C.CDLL("libamdhip64.so")
    for floats, call in ((n * D, lambda p: jw(p, None, None, 1, ptr(out), None)), (n * nb * 6, lambda p: jw(None, p, None, 1, ptr(out), None)),
                         (n * nb * 6, lambda p: jw(None, None, p, 1, ptr(out), None)), (n * J * 6, lambda p: jw(None, None, None, 1, p, None)),
                         (n * 6, lambda p: jw(None, None, None, 1, ptr(out), p)), (n * D, lambda p: gv(p, None, None, 0, None)),
                         (n * D, lambda p: gv(ptr(vel), p, None, 0, ptr(acc))), (n * D, lambda p: gv(ptr(vel), ptr(prev), None, 0, p)),
                         ((n - 1) * 3 + 1, lambda p: gv(ptr(vel), ptr(prev), p, 3, ptr(acc)))):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(4 * floats - 4)) == 0           # one float short
        try:
            assert call(p) == capi.E_INVALID
        finally:
            hip.hipFree(p)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in (out, base, vel, acc))             # nothing was launched
    assert np.all(host == 0)
    api = M.BatchJointWrench(b)
    with pytest.raises(capi.TrexError):
        api.joint_wrench(torch.zeros(n, D))                                        # the Python layer: a host tensor
    with pytest.raises(capi.TrexError):
        api.joint_wrench(axes="base")
    with pytest.raises(capi.TrexError):
        api.joint_wrench(out=torch.zeros(n, J, 5, device=DEV))
    v.close()


def test_stream_capture(runs):
    """the SECOND call of both captured on one stream, one linear chain: the replay is bitwise the eager result at the new state"""
    c, v, _, _ = runs("trex")
    api, n, D = api_of(v), JC.N, 6 + v.J
    _, wa, wb = dev_inputs(c["inp"], n)
    prev = torch.zeros(n, D, device=DEV)
    outs = [torch.zeros(n, D, device=DEV), torch.zeros(n, D, device=DEV), torch.zeros(n, v.J, 6, device=DEV), torch.zeros(n, 6, device=DEV)]

    def call(o):
        api.generalized_velocity(o[0], prev, 50.0, None, 0, o[1])
        api.joint_wrench(o[1], wa, wb, "link", o[2], o[3])
    st = v.get_state()
    moved = st.clone()
    moved[:, 7:13] += 0.25
    moved[:, 13 + v.J:] *= 0.5
    try:
        replay_equals_eager(call, outs, lambda: v.set_state(moved))
    finally:
        v.set_state(st)


# ---------------------------------------------------------------- 5. trex_batch_generalized_velocity
def test_generalized_velocity_is_the_torch_expression(runs):
    """vel is the state's velocity part; accel is bitwise (vel - prev) * inv_dt in f32; vel aliased to prev latches; the done column
    - read with its stride - zeroes its rows"""
    c, v, _, _ = runs("deep_chain")
    api, n, J = api_of(v), JC.N, v.J
    D = 6 + J
    st = v.get_state()
    want = torch.cat([st[:, 7:13], st[:, 13 + J:13 + 2 * J]], 1).contiguous()
    vel, _ = api.generalized_velocity(torch.zeros(n, D, device=DEV))
    assert same_bits(vel, want)
    gen = torch.Generator(device=DEV).manual_seed(11)
    prev = torch.randn(n, D, generator=gen, device=DEV)
    inv_dt = 1.0 / 0.03
    expect = (want - prev) * torch.tensor(inv_dt, dtype=torch.float32, device=DEV)
    whole_v, vel = guarded((n, D), 65)
    whole_a, acc = guarded((n, D), 65)
    api.generalized_velocity(vel, prev, inv_dt, None, 0, acc)
    torch.cuda.synchronize()
    assert same_bits(vel, want) and same_bits(acc, expect)
    assert guards_intact(whole_v, (n, D), 65) and guards_intact(whole_a, (n, D), 65)
    latch, acc2 = prev.clone(), torch.zeros(n, D, device=DEV)
    api.generalized_velocity(latch, latch, inv_dt, None, 0, acc2)                  # vel IS prev
    assert same_bits(latch, want) and same_bits(acc2, expect)
    rows = torch.zeros(n, 5, device=DEV)
    rows[[1, 4, 11], 3] = torch.tensor([1.0, -2.0, 0.5], device=DEV)
    rows[:, 2] = 1.0                                                               # (another column: not the one read)
    acc3 = torch.full((n, D), 9.0, device=DEV)
    api.generalized_velocity(None, prev, inv_dt, rows, 3, acc3)
    zeroed = expect.clone()
    zeroed[[1, 4, 11]] = 0.0
    assert same_bits(acc3, zeroed) and bool((acc3[[1, 4, 11]] == 0).all())


# ---------------------------------------------------------------- 6. the attached sensor
def test_attached_sensor_is_the_bare_query(model):
    """6 envs, a few steps with an external wrench held: joint_reaction is bitwise the bare query fed with the get_state differences,
    contact_wrench() and the external wrench; TrexRobot.get_joint_states returns the reference's four keys - zeros before attach,
    the sensor's rows after; an env without attach steps bitwise as before; detach takes it all off"""
    from trex_gym import joint_sensor
    from trex_gym.trex_robot import TrexRobot
    n = 6
    v, plain = make_vec(n, max_episode_steps=3), make_vec(n, max_episode_steps=3)
    J, D = v.J, 6 + v.J
    gen = torch.Generator(device=DEV).manual_seed(2)
    w = 40 * torch.randn(n, v.model.num_bodies, 6, generator=gen, device=DEV)
    for e in (v, plain):
        e.enable_contact_sensor(True)
        e.set_external_wrench(w)
    robot = TrexRobot(v, 2)
    idx = robot._revolute_joint_indices
    assert robot._get_joint_state_names() == ["jointPosition", "jointVelocity", "jointReactionForces", "appliedJointMotorTorque"]
    v.reset_tensor()
    plain.reset_tensor()
    before = robot.get_joint_states(idx)
    assert list(before) == robot._get_joint_state_names() and all(len(x) == J for x in before.values())
    assert before["jointReactionForces"] == [(0.0,) * 6] * J                       # no sensor: zeros, as pybullet gives
    joint_sensor.attach(v)
    assert tuple(v.joint_reaction.shape) == (n, J, 6) and tuple(v.joint_base_residual.shape) == (n, 6)
    reaction, api = v.joint_reaction, api_of(plain)
    gv = lambda st: torch.cat([st[:, 7:13], st[:, 13 + J:13 + 2 * J]], 1)
    inv_dt = torch.tensor(1.0 / (v.model.get_param("dt") * v.model.get_param("substeps")), dtype=torch.float32, device=DEV)
    last = gv(plain.get_state())
    zero = torch.zeros(n, D, device=DEV)
    assert same_bits(reaction, api.joint_wrench(zero, plain.contact_wrench(), w))  # the reading attach() took, at the reset state
    some_done = False
    for t in range(5):
        a = random_actions(model, n, gen)
        v.step_tensor(a)
        plain.step_tensor(a)
        assert same_bits(v.rows, plain.rows) and same_bits(v.get_state(), plain.get_state())   # the sensor changes no step
        now = gv(plain.get_state())
        acc = (now - last) * inv_dt
        acc[plain.done] = 0.0                                                      # an episode ended: a reset, not a motion
        some_done |= bool(plain.done.any())
        last = now
        base = torch.zeros(n, 6, device=DEV)
        want = api.joint_wrench(acc, plain.contact_wrench(), w, "link", None, base)
        assert v.joint_reaction is reaction                                        # refreshed in place
        assert same_bits(reaction, want) and same_bits(v.joint_base_residual, base), t
    assert some_done and float(reaction.abs().max()) > 0
    after = robot.get_joint_states(idx)
    assert list(after) == robot._get_joint_state_names()
    got = np.array(after["jointReactionForces"])
    assert got.shape == (J, 6) and np.array_equal(got.astype(np.float32), reaction[2].cpu().numpy())
    o = v.obs[2].cpu().numpy().astype(np.float64)
    assert after["jointPosition"] == o[:J].tolist() and after["jointVelocity"] == o[J:2 * J].tolist()
    assert after["appliedJointMotorTorque"] == o[2 * J:3 * J].tolist()
    one = robot.get_joint_state(idx[3])
    assert one == {k: x[3] for k, x in after.items()} and len(one["jointReactionForces"]) == 6
    fixed = [i for i in range(v.model.num_urdf_joints) if i not in idx]
    for bad in (fixed[0], -1, v.model.num_urdf_joints):
        with pytest.raises(ValueError):
            robot.get_joint_state(bad)
    load = joint_sensor.joint_load(v, [0, v.model.joint_names[5]])
    assert tuple(load.shape) == (n, 2, 2)
    assert torch.equal(load[:, 1, 0], reaction[:, 5, :3].norm(dim=-1)) and torch.equal(load[:, 0, 1], reaction[:, 0, 3:].norm(dim=-1))
    v.reset_tensor()
    plain.reset_tensor()
    assert same_bits(reaction, api.joint_wrench(zero, plain.contact_wrench(), w))  # after a reset: zero acceleration
    joint_sensor.detach(v)
    assert v.joint_reaction is None and v.joint_api is None and v._joint_fill is None
    a = random_actions(model, n, gen)
    v.step_tensor(a)
    plain.step_tensor(a)
    assert same_bits(v.rows, plain.rows) and same_bits(v.contact_wrench(), plain.contact_wrench())
    assert robot.get_joint_state(idx[0])["jointReactionForces"] == (0.0,) * 6
    v.close()
    plain.close()


def test_attached_sensor_replays_in_a_captured_step(model):
    """a step with the sensor attached, captured on one stream, replays: the readings are bitwise those of the same steps made eagerly"""
    from trex_gym import joint_sensor
    n = 6
    gen = torch.Generator(device=DEV).manual_seed(4)
    acts = [random_actions(model, n, gen) for _ in range(4)]
    eager = joint_sensor.attach(make_vec(n))
    eager.reset_tensor()
    want = []
    for a in acts:
        eager.step_tensor(a)
        want.append((eager.joint_reaction.clone(), eager.joint_base_residual.clone()))
    eager.close()
    v = joint_sensor.attach(make_vec(n))
    v.reset_tensor()
    a_in = acts[0].clone()
    v.step_tensor(a_in)                                                            # the warm-up call learns the buffers
    assert same_bits(v.joint_reaction, want[0][0])
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            v.step_tensor(a_in)
    for k in (1, 2, 3):
        a_in.copy_(acts[k])
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(v.joint_reaction, want[k][0]) and same_bits(v.joint_base_residual, want[k][1]), k
    del graph
    v.close()
