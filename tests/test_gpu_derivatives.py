"""The derivatives of the rigid-body dynamics on the device (include/trex_dynamics_derivatives.h, trex_gym.derivatives):
trex_batch_inverse_dynamics_derivatives against the f64 reference of tests/dynamics_derivatives_ref.py on the T-rex and the four
generated models of tests/dynamics_model_cases.py, the exact zeros, the batch shapes where the tiling can go wrong, bitwise
independence of a direction from what else is asked for, robustness, and forward_dynamics_derivatives / gravity_stiffness.

Every bound comes from the reference, none from the device (tests/derivatives_cases.py): min(2e-4, max(DYNAMICS_TOL["id_zero"],
4 x d32)), d32 the deviation of the reference's own f32 run from its f64 run on the model's cases, in the per-row metric; the
identity's likewise from the f32 run's own residual. tests/test_derivatives_ref.py shows the cap never binds and that five
mistakes lie beyond 10 x the cap."""
import ctypes as C

import numpy as np
import pytest
import torch

import derivatives_cases as DC
from gpu_support import DEV, guarded, guards_intact, loaded_vec, make_vec, random_actions, replay_equals_eager, same_bits

pytestmark = pytest.mark.gpu


def api_of(v):
    from trex_gym.derivatives_capi import BatchDerivatives
    return BatchDerivatives(v.batch)


def env_of(m, cases, n=None):
    kw = {} if m["path"] is None else dict(urdf=m["path"], params=m["props"]["params"])
    return loaded_vec(cases, n=n, nb=m["om"]["nb"], **kw)


def dev_accel(inp, n):
    return torch.tensor(inp["acc"][np.arange(n) % DC.N]).to(DEV)


def device_outputs(v, inp):
    """{(variant, layout): (dfdq, dfdv)} device tensors [n, D, D]; layout "jac" out[e, i, j] or "dir" out[e, j, i]"""
    from trex_gym import derivatives
    acc = dev_accel(inp, v.num_envs)
    return {(name, lay): derivatives.inverse_dynamics_derivatives(v, acc if name == "accel" else None, by_direction=lay == "dir")
            for name in DC.VARIANTS for lay in ("jac", "dir")}


@pytest.fixture(scope="module")
def built(tmp_path_factory, model):
    return DC.built(tmp_path_factory, model)


@pytest.fixture(scope="module")
def runs(built):
    """name -> (case, the env of 12, its device outputs), made on first use; the envs are closed at the end"""
    made = {}

    def get(name):
        if name not in made:
            c = DC.case(name, built[name]["om"])
            v = env_of(built[name], c["inp"]["cases"])
            made[name] = (c, v, device_outputs(v, c["inp"]))
        return made[name]
    yield get
    for _, v, _ in made.values():
        v.close()


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", DC.MODELS)
def test_against_reference_n12(name, runs):
    """12 states - three full workgroups, the last two with a per-body mass scale -, accel given and NULL, both layouts, both
    matrices: within the bound the reference's f32 run sets, per row; the by-direction layout is bitwise the transpose"""
    c, v, out = runs(name)
    D = 6 + v.J
    assert v.J == c["om"]["nb"] - 1
    devs = {}
    for (variant, lay), (dq, dv) in out.items():
        assert tuple(dq.shape) == tuple(dv.shape) == (DC.N, D, D) and torch.isfinite(dq).all() and torch.isfinite(dv).all()
        if lay == "dir":
            assert same_bits(dq.transpose(1, 2).contiguous(), out[variant, "jac"][0]), (name, variant)
            assert same_bits(dv.transpose(1, 2).contiguous(), out[variant, "jac"][1]), (name, variant)
            dq, dv = dq.transpose(1, 2), dv.transpose(1, 2)
        devs[variant, lay, "dfdq"] = DC.row_deviation(dq.cpu().numpy(), c["ref"][variant][1])
        devs[variant, lay, "dfdv"] = DC.row_deviation(dv.cpu().numpy(), c["ref"][variant][2])
    print("%s: largest deviation %.3g of %s (d32 %.3g, bound %.3g)" % (name, max(devs.values()), max(devs, key=devs.get), c["d32"], c["bound"]))
    for key, d in devs.items():
        assert d <= c["bound"], (name, key, d, c["bound"])


@pytest.mark.parametrize("name", DC.MODELS)
def test_exact_zeros(name, runs):
    """the translation columns of both matrices and the joint pairs on different branches are == 0, in both layouts"""
    c, _, out = runs(name)
    zero = torch.tensor(c["zero"]).to(DEV)
    for (variant, lay), pair in out.items():
        for m in pair:
            m = m.transpose(1, 2) if lay == "dir" else m
            assert bool((m[:, :, 0:3] == 0).all()), (name, variant, lay)
            assert bool((m[:, zero] == 0).all()), (name, variant, lay)
            assert bool((m[:, :, 3:6] != 0).any()) and bool((m[:, 6:, 6:] != 0).any())


@pytest.mark.parametrize("name", ("trex", "mount_first"))
def test_dfdv_does_not_depend_on_the_accelerations(name, runs):
    """M a has no velocity in it: dfdv at the accelerations against dfdv without, within the bound"""
    c, _, out = runs(name)
    d = DC.row_deviation(out["accel", "jac"][1].cpu().numpy(), out["bias", "jac"][1].cpu().numpy(), c["ref"]["bias"][2])
    assert d <= c["bound"], (name, d)


@pytest.mark.parametrize("name", DC.MODELS)
def test_dfdq_is_affine_in_the_accelerations(name, runs):
    """no reference: dfdq(2a) - dfdq(0) = 2 (dfdq(a) - dfdq(0)), within the bound the f32 run's own residual sets"""
    from trex_gym import derivatives
    c, v, out = runs(name)
    dq2, _ = derivatives.inverse_dynamics_derivatives(v, 2 * dev_accel(c["inp"], DC.N), "q")
    res = DC.linearity_residual(dq2.cpu().numpy(), out["accel", "jac"][0].cpu().numpy(), out["bias", "jac"][0].cpu().numpy(), c["ref"])
    print("%s: affine in a: %.3g (f32 run %.3g, bound %.3g)" % (name, res, c["lin32"], c["lin_bound"]))
    assert res <= c["lin_bound"], (name, res, c["lin_bound"])


# ---------------------------------------------------------------- 2. shapes, and what a direction may depend on
@pytest.mark.parametrize("name", ("trex", "deep_chain", "slab"))
@pytest.mark.parametrize("n", [1, 5])
def test_batch_shapes(n, name, built, runs):
    """N = 1 and N = 5 (a last workgroup of one env): env e holds case e % 12, and its blocks are bitwise those of the N = 12 call.
    N = 5: both outputs into guarded buffers, on and 4 bytes off the 16-byte grid: guards intact, the same bits."""
    from trex_gym import derivatives
    c, _, full = runs(name)
    inp = c["inp"]
    v = env_of(built[name], inp["cases"], n)
    out = device_outputs(v, inp)
    idx = torch.arange(n) % DC.N
    for key, (dq, dv) in out.items():
        assert same_bits(dq, full[key][0][idx]) and same_bits(dv, full[key][1][idx]), (name, n, key)
    if n == 5:
        D, acc = 6 + v.J, dev_accel(inp, n)
        for guard, rest in ((64, 0), (65, 4)):
            whole_q, dq = guarded((n, D, D), guard)
            whole_v, dv = guarded((n, D, D), guard)
            assert dq.data_ptr() % 16 == rest and dv.data_ptr() % 16 == rest
            derivatives.inverse_dynamics_derivatives(v, acc, out_q=dq, out_v=dv)
            torch.cuda.synchronize()
            assert guards_intact(whole_q, (n, D, D), guard) and guards_intact(whole_v, (n, D, D), guard), (name, guard)
            assert same_bits(dq, out["accel", "jac"][0]) and same_bits(dv, out["accel", "jac"][1]), (name, guard)
    v.close()


@pytest.mark.parametrize("name", ("trex", "deep_chain", "slab"))
def test_one_output_or_both_same_bits_and_repeatable(name, runs):
    """only dfdq, only dfdv and both give the same bits, in both layouts, and a second call repeats them"""
    from trex_gym import derivatives
    c, v, out = runs(name)
    acc = dev_accel(c["inp"], DC.N)
    for lay in ("jac", "dir"):
        both = out["accel", lay]
        dq, none = derivatives.inverse_dynamics_derivatives(v, acc, "q", lay == "dir")
        assert none is None and same_bits(dq, both[0]), (name, lay)
        none, dv = derivatives.inverse_dynamics_derivatives(v, acc, ("v",), lay == "dir")
        assert none is None and same_bits(dv, both[1]), (name, lay)
        again = derivatives.inverse_dynamics_derivatives(v, acc, by_direction=lay == "dir")
        assert same_bits(again[0], both[0]) and same_bits(again[1], both[1]), (name, lay)


# ---------------------------------------------------------------- 3. robustness
def test_nan_env_stays_in_its_block(built, runs):
    """a NaN state in env 5: its own block is not finite, every other env's is bitwise what it was"""
    c, _, full = runs("trex")
    v = env_of(built["trex"], c["inp"]["cases"])
    st = v.get_state()
    st[5, 13 + 3] = float("nan")
    v.set_state(st)
    out = device_outputs(v, c["inp"])
    keep = torch.tensor([e for e in range(DC.N) if e != 5])
    for key, (dq, dv) in out.items():
        assert same_bits(dq[keep], full[key][0][keep]) and same_bits(dv[keep], full[key][1][keep]), key
        assert not torch.isfinite(dq[5]).all()
    v.close()


def test_the_call_writes_its_outputs_only(model):
    """state, rows, the contact sensor's record and the episode steps are bitwise unchanged by the call; an env that is queried steps
    as one that is not"""
    from trex_gym import derivatives
    n = 6
    pair = []
    for probe in (False, True):
        v = make_vec(n, max_episode_steps=50)
        v.enable_contact_sensor(True)
        v.reset_tensor()
        gen = torch.Generator(device=DEV).manual_seed(3)
        steps = torch.zeros(n, dtype=torch.int32, device=DEV)
        for _ in range(4):
            v.step_tensor(random_actions(model, n, gen))
            if probe:
                v.batch.get_episode_steps(steps)
                before = (v.get_state(), v.rows.clone(), v.contact_wrench().clone(), steps.clone())
                dq, dv = derivatives.inverse_dynamics_derivatives(v, torch.ones(n, 6 + v.J, device=DEV))
                assert torch.isfinite(dq).all() and torch.isfinite(dv).all()
                v.batch.get_episode_steps(steps)
                for x, y in zip(before, (v.get_state(), v.rows, v.contact_wrench(), steps)):
                    assert same_bits(x, y)
        v.batch.get_episode_steps(steps)
        pair.append((v.get_state(), v.rows.clone(), v.contact_wrench().clone(), steps.clone()))
        v.close()
    for x, y in zip(*pair):
        assert same_bits(x, y)


def test_refusals():
    """both outputs NULL, unknown flags, an output on top of accel, host memory, a buffer one float short - each TREX_E_INVALID with
    nothing launched"""
    from trex_gym import _capi as capi
    from trex_gym import derivatives
    n = 5
    v = make_vec(n)
    v.reset_tensor()
    b, lib = v.batch, capi.lib
    D = 6 + v.J
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    SENT = 7.0
    dq, dv = torch.full((n, D, D), SENT, device=DEV), torch.full((n, D, D), SENT, device=DEV)
    acc = torch.zeros(n, D, device=DEV)
    call = lambda a, q, w, flags: lib.trex_batch_inverse_dynamics_derivatives(b.h, a, q, w, flags, s)
    assert call(ptr(acc), ptr(dq), ptr(dv), 1) == 0                                  # the call works at all
    torch.cuda.synchronize()
    assert not bool((dq == SENT).any()) and not bool((dv == SENT).any())
    dq.fill_(SENT)
    dv.fill_(SENT)
    assert call(ptr(acc), None, None, 0) == capi.E_INVALID                           # nothing asked for
    assert call(ptr(acc), ptr(dq), ptr(dv), 2) == capi.E_INVALID and call(None, ptr(dq), None, 0x80000001) == capi.E_INVALID
    assert call(ptr(dq), ptr(dq), None, 0) == capi.E_INVALID                         # an output on top of accel
    assert call(None, ptr(dq), C.c_void_p(dq.data_ptr() + 4 * D), 0) == capi.E_INVALID   # the outputs overlap
    host = np.zeros(n * D * D, np.float32)
    hp = C.c_void_p(host.ctypes.data)
    for bad in (lambda p: call(p, ptr(dq), None, 0), lambda p: call(None, p, None, 0), lambda p: call(None, ptr(dq), p, 0)):
        assert bad(hp) == capi.E_INVALID
    hip = C.CDLL("libamdhip64.so")
    for floats, bad in ((n * D, lambda p: call(p, ptr(dq), None, 0)), (n * D * D, lambda p: call(None, p, None, 0)),
                        (n * D * D, lambda p: call(None, ptr(dq), p, 0))):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(4 * floats - 4)) == 0           # one float short
        try:
            assert bad(p) == capi.E_INVALID
        finally:
            hip.hipFree(p)
    torch.cuda.synchronize()
    assert bool((dq == SENT).all()) and bool((dv == SENT).all())                   # nothing was launched
    assert np.all(host == 0)
    with pytest.raises(capi.TrexError):
        api_of(v).inverse_dynamics_derivatives(torch.zeros(n, D))                  # the Python layer: a host tensor
    with pytest.raises(capi.TrexError):
        api_of(v).inverse_dynamics_derivatives(None, None, None)
    with pytest.raises(capi.TrexError):
        derivatives.inverse_dynamics_derivatives(v, out_q=torch.zeros(n, D, D - 1, device=DEV))
    with pytest.raises(ValueError):
        derivatives.inverse_dynamics_derivatives(v, wrt=("q", "a"))
    v.close()


def test_stream_capture(runs):
    """the SECOND call captured on one stream: the replay is bitwise the eager result at the new state; so is the whole of
    forward_dynamics_derivatives"""
    from trex_gym import derivatives
    c, v, _ = runs("trex")
    n, D = DC.N, 6 + v.J
    acc = dev_accel(c["inp"], n)
    force = torch.tensor(c["ref"]["accel"][0].astype(np.float32)).to(DEV)
    outs = [torch.zeros(n, D, D, device=DEV) for _ in range(2)] + [torch.zeros(n, D, device=DEV)] + [torch.zeros(n, D, D, device=DEV) for _ in range(3)]

    def call(o):
        derivatives.inverse_dynamics_derivatives(v, acc, by_direction=True, out_q=o[0], out_v=o[1])
        derivatives.forward_dynamics_derivatives(v, force, out=o[2:])
    st = v.get_state()
    moved = st.clone()
    moved[:, 7:13] += 0.25
    moved[:, 13:13 + v.J] += 0.05
    moved[:, 13 + v.J:] *= 0.5
    try:
        replay_equals_eager(call, outs, lambda: v.set_state(moved))
    finally:
        v.set_state(st)


# ---------------------------------------------------------------- 4. forward dynamics, gravity stiffness
@pytest.mark.parametrize("name", DC.MODELS)
def test_forward_dynamics_derivatives(name, runs):
    """force = the reference's inverse dynamics of the drawn accelerations: accel returns them, minv is inverse_mass_matrix();
    dadq and dadv against -M_ref^-1 dfdx_ref in the residual metric, and M_ref dadx + dfdx = 0 on the device's own outputs"""
    from trex_gym import derivatives
    c, v, _ = runs(name)
    ref, (Ms, _, _) = c["ref"], c["fwd"]
    force = torch.tensor(ref["accel"][0].astype(np.float32)).to(DEV)
    accel, dadq, dadv, minv = derivatives.forward_dynamics_derivatives(v, force)
    D = 6 + v.J
    assert tuple(accel.shape) == (DC.N, D) and all(tuple(t.shape) == (DC.N, D, D) and t.is_contiguous() for t in (dadq, dadv, minv))
    assert same_bits(accel, v.forward_dynamics(force)) and same_bits(minv, v.inverse_mass_matrix())
    dev = DC.forward_deviation(dadq.cpu().numpy(), dadv.cpu().numpy(), c["fwd"], ref)
    dfdq, dfdv = derivatives.inverse_dynamics_derivatives(v, accel)
    f8 = lambda t: t.cpu().numpy().astype(np.float64)
    own = max(DC.row_deviation(Ms @ f8(dadq), -f8(dfdq), ref["accel"][1]), DC.row_deviation(Ms @ f8(dadv), -f8(dfdv), ref["accel"][2]))
    print("%s: forward dynamics derivatives %.3g, M dadx + dfdx %.3g (f32 run %.3g, bound %.3g)" % (name, dev, own, c["fwd_d32"], c["fwd_bound"]))
    assert dev <= c["fwd_bound"] and own <= c["fwd_bound"], (name, dev, own, c["fwd_bound"])


@pytest.mark.parametrize("name", ("trex", "slab"))
def test_gravity_stiffness(name, runs):
    """the joint block of dfdq at zero acceleration, against the reference per row (the row's scale is the whole row's)"""
    from trex_gym import derivatives
    c, v, out = runs(name)
    K = derivatives.gravity_stiffness(v)
    assert tuple(K.shape) == (DC.N, v.J, v.J) and same_bits(K, out["bias", "jac"][0][:, 6:, 6:].contiguous())
    want = c["ref"]["bias"][1]
    d = DC.row_deviation(K.cpu().numpy(), want[:, 6:, 6:], want[:, 6:, :])
    assert d <= c["bound"], (name, d, c["bound"])


def test_a_single_env_is_taken_too():
    """a TrexBulletEnv: its one env, n = 1"""
    from trex_gym import derivatives
    from trex_gym.trex_env import TrexBulletEnv
    env = TrexBulletEnv(device=DEV)
    env.reset()
    dq, dv = derivatives.inverse_dynamics_derivatives(env)
    D = 6 + env._vec.J
    assert tuple(dq.shape) == tuple(dv.shape) == (1, D, D) and torch.isfinite(dq).all()
    assert tuple(derivatives.gravity_stiffness(env).shape) == (1, D - 6, D - 6)
    assert same_bits(derivatives.forward_dynamics_derivatives(env)[0], env._vec.forward_dynamics())
    env.close()
