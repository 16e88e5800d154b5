"""The first four dynamics queries (trex_batch_inverse_dynamics / _mass_matrix / _jacobian / _centroidal) on the generated models of
tests/dynamics_model_cases.py - six tree levels, four children on two bodies at different depths, welded links behind turned
frames, URDF link 0 in a moving body, scattered observation slots, D = 7, 10, 12 and 31, a last workgroup of one env, per-body
mass scales with fewer than 26 bodies: what the T-rex tree of tests/test_gpu_dynamics.py never exercises.

Every bound comes from the reference, none from the device (dynamics_model_cases, module docstring): for model m and metric k
min(CAPS[k], max(TOL[k], 4 x d32[m][k])), d32 the deviation of the reference's own f32 run from its f64 run on the same 12 states;
the identities likewise from the residual of the f32 run's outputs. tests/test_dynamics_model_cases_host.py shows that these
bounds tell a wrong table from a right one by a factor of at least 100. The Jacobian is taken at EVERY URDF link, at the link
origin and at (0.3, -0.2, 0.1). Each model's env of 12 is built once per module; the outputs are read-only."""
import numpy as np
import pytest
import torch

import dynamics_model_cases as DC
from gpu_support import guarded, guards_intact, loaded_vec, same_bits
from state_sets import built_models

pytestmark = pytest.mark.gpu
KEYS = ("id_zero", "id_acc", "mass", "jac", "cent", "vel")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return built_models(DC.MODELS, tmp_path_factory)


def env_of(m, cases):
    return loaded_vec(cases, urdf=m["path"], params=m["props"]["params"], nb=m["om"]["nb"])


def probe_points(om):
    """(links [2 L], points [2 L, 3]): every URDF link at each of DC.POINTS, link-major"""
    nl = len(om["link_names"])
    return [l for l in range(nl) for _ in DC.POINTS], np.tile(np.array(DC.POINTS), (nl, 1))


def device_outputs(v, om, acc):
    """the outputs dict of dynamics_model_cases as device tensors: the four queries - the Jacobian of every link at both points -
    and the link-state query's linear velocity of the same points"""
    n, nl = v.num_envs, len(om["link_names"])
    out = dict(id_zero=v.inverse_dynamics(), id_acc=v.inverse_dynamics(torch.tensor(acc[:n])), mass=v.mass_matrix(),
               jac=torch.stack([torch.stack([v.jacobian(l, p) for p in DC.POINTS], 1) for l in range(nl)], 1),
               cent=v.centroidal().data.clone())
    h = v.link_probes(*probe_points(om))
    out["vel"] = v.link_state(h).linear_velocity.reshape(n, nl, len(DC.POINTS), 3).clone()
    h.close()
    return out


def as_numpy(out):
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.fixture(scope="module")
def runs(built):
    """name -> (case, the env of 12, its device outputs, the same as numpy), made on first use; the envs are closed at the end"""
    made = {}

    def get(name):
        if name not in made:
            c = DC.case(name, built[name])
            v = env_of(built[name], c["cases"])
            out = device_outputs(v, c["om"], c["acc"])
            made[name] = (c, v, out, as_numpy(out))
        return made[name]
    yield get
    for _, v, _, _ in made.values():
        v.close()


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", DC.MODELS)
def test_against_reference_n12(name, runs):
    """12 states - three full workgroups, the last two states with a per-body mass scale - in the metrics of
    tests/test_gpu_dynamics.py, each within the bound the reference's f32 run sets; the mass matrix bitwise symmetric"""
    c, v, out, got = runs(name)
    assert v.num_envs == DC.N and tuple(out["mass"].shape) == (DC.N, 6 + v.J, 6 + v.J) and v.J == c["om"]["nb"] - 1
    assert all(torch.isfinite(t).all() for t in out.values())
    dev = DC.metric_devs(c["taus"], got, c["ref"])
    print("%s deviations: %s" % (name, {k: "%.3g (d32 %.3g, bound %.3g)" % (dev[k], c["d32"][k], c["bound"][k]) for k in DC.METRICS}))
    assert torch.equal(out["mass"], out["mass"].transpose(1, 2).contiguous())
    for k in DC.METRICS:
        assert dev[k] <= c["bound"][k], (name, k, dev[k], c["bound"][k])


# ---------------------------------------------------------------- 2. exact structure
@pytest.mark.parametrize("name", DC.MODELS)
def test_structure_is_exact(name, runs):
    """on the device outputs, for every link and both points: Jacobian columns of joints off the link's chain == 0.0, the base block
    exactly [[1, ex], [0, 1]] with ex antisymmetric; mass-matrix entries of joint pairs on different branches == 0.0;
    M[:3, :3] exactly mass x 1"""
    c, _, _, got = runs(name)
    assert DC.structure_faults(c["om"], got) == []
    # ... and every joint ON a link's chain does move it: no column is 0 that the tree says may differ from 0
    for l, cols in enumerate(DC.chain_columns(c["om"])):
        assert np.all(np.abs(got["jac"][:, l][..., cols]).max(axis=-2) > 0), (name, l)


# ---------------------------------------------------------------- 3. the queries agree with each other
@pytest.mark.parametrize("name", DC.MODELS)
def test_queries_agree_with_each_other(name, runs):
    """no reference: ID(a) - ID(0) = M a; M[0:3] gv, M[3:6] gv and 0.5 gv M gv are the centroidal query's momentum, angular momentum
    (shifted to the base origin) and kinetic energy; J(link, p) gv is the link-state query's velocity of that point. Bounds from
    the residuals of the reference's f32 run in the same identities (dynamics_model_cases)"""
    c, _, _, got = runs(name)
    res = DC.identity_devs(c["om"], c["cases"], c["acc"], got)
    print("%s identities: %s" % (name, {k: "%.3g (f32 run %.3g, bound %.3g)" % (res[k], c["res32"][k], c["id_bound"][k]) for k in DC.IDENTITIES}))
    for k in DC.IDENTITIES:
        assert res[k] <= c["id_bound"][k], (name, k, res[k], c["id_bound"][k])


# ---------------------------------------------------------------- 4. batch shapes
@pytest.mark.parametrize("name", DC.MODELS)
@pytest.mark.parametrize("n", [5, 1])
def test_batch_shapes(n, name, built, runs):
    """N = 5: one full workgroup and one holding a single env; N = 1: a single env. The first states; bitwise the matching rows of the
    N = 12 outputs. At N = 5 every output also goes into a guarded buffer, aligned and 4 bytes off the 16-byte grid (the scalar
    stores): guards intact, the two bitwise equal - on slab [5, 7], [5, 7, 7], [5, 6, 7] and [5, 16]."""
    c, _, full, _ = runs(name)
    om = c["om"]
    D, nl = 6 + om["nb"] - 1, len(om["link_names"])
    v = env_of(built[name], c["cases"][:n])
    out = device_outputs(v, om, c["acc"])
    for k in KEYS:
        assert out[k].shape[0] == n and same_bits(out[k], full[k][:n]), (name, n, k)
    if n == 5:
        acc = torch.tensor(c["acc"][:n]).to(v.device)
        pt = DC.POINTS[1]
        calls = [((D,), lambda o: v.batch.inverse_dynamics(acc, o), full["id_acc"][:n]),
                 ((D, D), lambda o: v.batch.mass_matrix(o), full["mass"][:n]),
                 ((6, D), lambda o: v.batch.jacobian(nl - 1, pt, o), full["jac"][:n, nl - 1, 1]),
                 ((6, D), lambda o: v.batch.jacobian(0, pt, o), full["jac"][:n, 0, 1]),
                 ((16,), lambda o: v.batch.centroidal(o), full["cent"][:n])]
        if name == "slab":
            assert [(n,) + s for s, _, _ in calls] == [(5, 7), (5, 7, 7), (5, 6, 7), (5, 6, 7), (5, 16)]
        for shape, call, want in calls:
            for guard, rest in ((64, 0), (65, 4)):
                whole, view = guarded((n,) + shape, guard)
                assert view.data_ptr() % 16 == rest and view.is_contiguous()
                call(view)
                torch.cuda.synchronize()
                assert guards_intact(whole, (n,) + shape, guard), (name, shape, guard)
                assert same_bits(view, want), (name, shape, guard)
    v.close()


# ---------------------------------------------------------------- 5. mass scale
@pytest.mark.parametrize("name", DC.MODELS)
def test_mass_scale(name, built, runs):
    """set_domain with nb < 26 (and nb = 26 on bushy): the two scaled states differ from the same states unscaled in id_zero, mass and
    cent - by more than the bound, in the metric - while the Jacobian and the link velocities, kinematics, stay bitwise; each
    scaled state's total mass is sum(mass x scale)"""
    c, _, full, got = runs(name)
    om = c["om"]
    scaled = c["cases"][-2:]
    assert all(ms is not None and len(ms) == om["nb"] for _, ms in scaled)
    v = env_of(built[name], [(s, None) for s, _ in scaled])
    plain = device_outputs(v, om, c["acc"][-2:])
    v.close()
    for k in ("id_zero", "id_acc", "mass", "cent"):
        assert not torch.equal(plain[k], full[k][-2:]), (name, k)
    for k in ("jac", "vel"):
        assert same_bits(plain[k], full[k][-2:]), (name, k)
    ref = {k: x[-2:] for k, x in c["ref"].items()}
    moved = DC.metric_devs(c["taus"][-2:], as_numpy(plain), ref)
    for k in ("id_zero", "mass", "cent"):
        assert moved[k] > 100 * c["bound"][k], (name, k, moved[k])
    for e, (_, ms) in enumerate(scaled):
        total = float((np.asarray(om["mass"], np.float64) * ms).sum())
        row = got["cent"][DC.N - 2 + e]
        assert abs(float(row[14]) - total) <= c["bound"]["cent"] * total
        assert abs(float(got["mass"][DC.N - 2 + e, 0, 0]) - total) <= c["bound"]["mass"] * total
        assert abs(float(plain["cent"][e, 14]) - float(np.sum(om["mass"]))) <= c["bound"]["cent"] * float(np.sum(om["mass"]))
