"""Inverse kinematics on the GPU (trex_batch_inverse_kinematics, include/trex_batch.h) against the f64 restatement tests/ik_ref.py
- itself pinned by tests/test_ik_ref.py - one iteration element by element, and its convergence judged by the independent
forward kinematics of tests/link_state_ref.py alone; the cases are those of tests/ik_cases.py, qualified on the reference by
tests/test_ik_cases_host.py. Then limits, mask, aliasing, early stop, the tiling's edges, read-only, refusals, containment, stream
capture, the generated models and the facades.

Tolerances (TOL): 4 x the largest deviation measured on these very cases on an MI355X (scripts/ik_bench.py prints them;
profiles/r20_inverse_kinematics.txt records them), never above the caps: 1e-4 rad for q after one iteration, 1e-5 m / rad for the
residuals of `info` against the f64 evaluation of q_out, 1 % for the final error norm of the unreachable cases. The convergence
bound is fixed: 1e-4 m / rad, ten times what the reference leaves on the same cases."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dynamics_ref as R
import gpu_support
import ik_cases as IC
import ik_ref as IK
import link_state_ref as L
from gpu_support import DEV, case_env as make_env, guarded, guards_intact, random_steps, replay_equals_eager

pytestmark = pytest.mark.gpu
N = 67
FRAMES = {"world": 0, "base": 2}
FORMS = ["pos4", "head_ori", "three_ori", "k1", "k8", "same_body", "one_leg", "one_leg_ori"]
ONE_ITER = dict(iterations=1, damping=0.05)
CONVERGED = 1e-4

# Largest deviations measured on an MI355X (profiles/r20_inverse_kinematics.txt): q after one iteration (every form, both frames,
# with and without q_init and a mask, N = 67), the two residuals of info against the f64 evaluation of q_out after 30 iterations,
# the final error norm of the unreachable cases relative to the reference's, and one iteration on the generated models (N = 3).
MEASURED = dict(one_iter=4.16e-6, info=7.53e-7, unreachable=1.84e-7, deep_chain=1.1e-6, bushy=5.04e-7)
CAPS = dict(one_iter=1e-4, info=1e-5, unreachable=1e-2, deep_chain=1e-4, bushy=1e-4)
TOL = {k: min(4 * v, CAPS[k]) for k, v in MEASURED.items()}


def bits(joints, J):
    return (1 << J) - 1 if joints is None else sum(1 << int(k) for k in joints)


def run_ik(v, slot, form, targets, frame="world", q_init=None, joints=None, info=True, guard=64, alias=False, **prm):
    """trex_batch_inverse_kinematics through _capi.Batch into NaN-filled buffers with `guard` floats around each output: (q [n, J],
    info [n, 4] or None) as numpy; the guards must still be NaN. alias: q_out IS q_init."""
    n, J, K = v.num_envs, v.J, len(form.links)
    t = torch.tensor(np.asarray(targets, np.float32).reshape(n, K, 7), device=DEV)
    (qb, qo), (ib, io) = guarded((n, J), guard, float("nan")), guarded((n, 4), guard, float("nan"))
    qi = None if q_init is None else torch.tensor(np.asarray(q_init, np.float32).reshape(n, J), device=DEV)
    if alias:
        qo.copy_(qi)
        qi = qo
    v.batch.inverse_kinematics(slot, form.modes, t, qo, FRAMES[frame], qi, bits(joints, J), io if info else None, **prm)
    torch.cuda.synchronize()
    assert guards_intact(qb, (n, J), guard, float("nan")), "the call wrote outside q_out"
    assert guards_intact(ib, (n, 4), guard, float("nan")) if info else torch.isnan(ib).all(), "the call wrote outside info"
    return qo.cpu().numpy(), (io.cpu().numpy() if info else None)


def targets_of(cases, frame):
    return np.array([c.targets[frame] for c in cases])


def independent_residuals(model, state, q, form, target, frame):
    """(largest position error, largest orientation error) of the joint angles q against `target` [K, 7] given in `frame`, by
    link_state_ref alone: the probes' poses in that frame; the angle of R_target R_link^T from |R - 1|_F = 2 sqrt(2) sin(angle / 2)"""
    r = L.link_state(model, IK.with_q(model, state, q), form.links, form.points, axes=frame)
    rp = ro = 0.0
    for k, m in enumerate(form.modes):
        if m & 1:
            rp = max(rp, np.linalg.norm(target[k, :3] - r["position"][k]))
        if m & 2:
            qt = target[k, 3:] / np.linalg.norm(target[k, 3:])
            E = R.quat_to_mat(qt) @ r["rotation"][k].T - np.eye(3)
            ro = max(ro, 2 * np.arcsin(min(1.0, np.linalg.norm(E) / (2 * np.sqrt(2)))))
    return rp, ro


def other_mask(model):
    """a mask for the forms that have none of their own: two joints of three may move"""
    return [k for k in range(model["nb"] - 1) if k % 3]


def one_iteration_deviation(model, form, n=N, key="trex", make=None):
    """largest |q_gpu - q_ref| after ONE iteration at damping 0.05 over both frames, with and without q_init, with and without a
    mask, every env a draw of its own"""
    cases = IC.reachable(model, form, n, key)
    J = model["nb"] - 1
    make = make or (lambda cs, q=None: make_env(model, cs, q))
    worst = 0.0
    for with_init in (False, True):
        # with q_init the envs stand at q*, which the solve must not look at; q_init = q_start, a fifth of the joints far outside
        # the limits: clamped before the first iteration where they may move
        q0 = np.array([c.q_start for c in cases])
        if with_init:
            q0 = IC.f32(q0 + np.where(np.arange(J) % 5 == 0, 10.0, 0.0))
        v = make(cases, np.array([c.q_star for c in cases]) if with_init else None)
        v.batch.set_link_probes(0, form.links, np.array(form.points))
        for frame in FRAMES:
            for joints in (None, form.joints if form.joints is not None else other_mask(model)):
                if form.joints is not None and joints is None:
                    continue            # (the draws of a masked form are reachable with its mask; without it is another task,
                                        # covered by the forms that have none)
                q, _ = run_ik(v, 0, form, targets_of(cases, frame), frame, q0 if with_init else None, joints, **ONE_ITER)
                assert np.isfinite(q).all()
                for e, c in enumerate(cases):
                    r = IK.solve(model, c.state, form.links, form.points, form.modes, c.targets[frame], frame, q0[e], joints,
                                 **ONE_ITER)
                    worst = max(worst, np.abs(q[e] - r["q"]).max())
        v.close()
    return worst


def converged(model, form, n=N, frame="world", iterations=30, key="trex", make=None):
    """(cases, q, info, [(rp, ro) by link_state_ref]) of the reachable draws after `iterations` at the defaults"""
    cases = IC.reachable(model, form, n, key)
    v = (make or (lambda cs: make_env(model, cs)))(cases)
    v.batch.set_link_probes(0, form.links, np.array(form.points))
    q, info = run_ik(v, 0, form, targets_of(cases, frame), frame, None, form.joints, iterations=iterations)
    v.close()
    res = [independent_residuals(model, c.state, q[e], form, c.targets[frame], frame) for e, c in enumerate(cases)]
    return cases, q, info, res


def unreachable_run(model, n=16):
    form, cases = IC.unreachable(model, n)
    v = make_env(model, cases)
    v.batch.set_link_probes(0, form.links, np.array(form.points))
    q, info = run_ik(v, 0, form, targets_of(cases, "world"), iterations=30)
    v.close()
    return form, cases, q, info


def deviations(model):
    """the figures TOL is set from (module docstring)"""
    d = dict(one_iter=0.0, info=0.0)
    for name in FORMS:
        form = IC.form_of(model, name)
        d["one_iter"] = max(d["one_iter"], one_iteration_deviation(model, form))
        for frame in FRAMES:
            _, _, info, res = converged(model, form, frame=frame)
            d["info"] = max(d["info"], np.abs(info[:, :2] - np.array(res)).max())
    form, cases, q, _ = unreachable_run(model)
    d["unreachable"] = max(abs(IK.residuals(model, c.state, q[e], form.links, form.points, form.modes, c.targets["world"])[2]
                               / IC.reference(model, form, c, iterations=30)["norms"][-1] - 1) for e, c in enumerate(cases))
    return d


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORMS)
def test_one_iteration_against_reference(name, model):
    """q_out element by element after one iteration, damping 0.05 (a well-conditioned solve), N = 67, every env its own draw."""
    assert TOL["one_iter"] <= CAPS["one_iter"]
    w = one_iteration_deviation(model, IC.form_of(model, name))
    print("%s: one iteration, largest |q - q_ref| %.3g rad" % (name, w))
    assert w <= TOL["one_iter"], (name, w)


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", FORMS)
def test_convergence_judged_by_link_state_ref(name, frame, model):
    """30 iterations at the defaults: every residual of q_out, evaluated in f64 by link_state_ref and not by the kernel, is at or
    below 1e-4 m / rad - no case excluded - and info's residuals agree with that evaluation."""
    form = IC.form_of(model, name)
    cases, q, info, res = converged(model, form, frame=frame)
    res = np.array(res)
    print("%s %s: largest residual %.3g m, %.3g rad; info off by %.3g" % (name, frame, res[:, 0].max(), res[:, 1].max(),
                                                                         np.abs(info[:, :2] - res).max()))
    assert np.isfinite(q).all() and (info[:, 2] == 30).all()
    assert res[:, 0].max() <= CONVERGED and res[:, 1].max() <= CONVERGED, (name, frame, res.max(0))
    assert np.abs(info[:, :2] - res).max() <= TOL["info"]
    for e, c in enumerate(cases[:8]):      # the norm at the start is the reference's
        assert abs(info[e, 3] - IC.reference(model, form, c, frame, **ONE_ITER)["initial_error"]) <= 1e-5 * max(1.0, info[e, 3])


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_unreachable_targets(model):
    """finite, inside the limits, and at the reference's final error norm (the Euclidean norm: the largest entry may end above
    its start)"""
    form, cases, q, info = unreachable_run(model)
    lo, hi = IK.limits(model)
    assert np.isfinite(q).all() and np.isfinite(info).all()
    assert (q >= lo.astype(np.float32)).all() and (q <= hi.astype(np.float32)).all()
    for e, c in enumerate(cases):
        ref = IC.reference(model, form, c, iterations=30)
        got = IK.residuals(model, c.state, q[e], form.links, form.points, form.modes, c.targets["world"])[2]
        print("unreachable %d: |e| %.5f, reference %.5f" % (e, got, ref["norms"][-1]))
        assert abs(got / ref["norms"][-1] - 1) <= TOL["unreachable"], (e, got, ref["norms"][-1])
        assert got < info[e, 3]


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORMS)
def test_limits_mask_and_aliasing(name, model):
    form = IC.form_of(model, name)
    n, J = 9, model["nb"] - 1
    cases = IC.reachable(model, form, n)
    v = make_env(model, cases)
    v.batch.set_link_probes(0, form.links, np.array(form.points))
    lo32, hi32 = v.model.lower.astype(np.float32), v.model.upper.astype(np.float32)
    joints = form.joints if form.joints is not None else other_mask(model)
    move = IK.joint_mask(model, joints)
    q0 = (np.array([c.q_start for c in cases]) + np.where(np.arange(J) % 4 == 0, -7.0, 0.0)).astype(np.float32)
    t = targets_of(cases, "world")
    for its in (1, 30):
        q, _ = run_ik(v, 0, form, t, "world", q0, joints, iterations=its)
        assert (q[:, move] >= lo32[move]).all() and (q[:, move] <= hi32[move]).all()
        assert q[:, ~move].tobytes() == q0[:, ~move].tobytes()
        qa, _ = run_ik(v, 0, form, t, "world", q0, joints, iterations=its, alias=True)
        assert qa.tobytes() == q.tobytes()
    q, _ = run_ik(v, 0, form, t, "world", None, None, iterations=30)
    assert (q >= lo32).all() and (q <= hi32).all()
    v.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_early_stop(model):
    tol = (1e-3, 1e-3)
    for name in FORMS:
        form = IC.form_of(model, name)
        cases = IC.reachable(model, form, 12)
        v = make_env(model, cases)
        v.batch.set_link_probes(0, form.links, np.array(form.points))
        q, info = run_ik(v, 0, form, targets_of(cases, "world"), "world", None, form.joints, iterations=30, tol_pos=tol[0], tol_ori=tol[1])
        v.close()
        assert (info[:, 2] < 30).all() and (info[:, 2] >= 1).all(), (name, info[:, 2])
        assert (info[:, 0] <= tol[0]).all() and (info[:, 1] <= tol[1]).all()
        for e, c in enumerate(cases):
            rp, ro = independent_residuals(model, c.state, q[e], form, c.targets["world"], "world")
            assert rp <= tol[0] + TOL["info"] and ro <= tol[1] + TOL["info"]
    # an env does not care when the other three of its workgroup stop: they stop at once (their targets are met at the start) or
    # run all 30 iterations (out of reach)
    form, hard = IC.unreachable(model, 3)
    mine = IC.reachable(model, form, 1)[0]
    easy = [IC.Case(c.state, c.q_start, c.q_start, IC.poses(model, c.state, c.q_start, form)) for c in hard]
    rows = []
    for others in (easy, hard):
        for place in (0, 2):
            cases = list(others)
            cases.insert(place, mine)
            v = make_env(model, cases)
            v.batch.set_link_probes(0, form.links, np.array(form.points))
            q, info = run_ik(v, 0, form, targets_of(cases, "world"), iterations=30, tol_pos=tol[0], tol_ori=tol[1])
            v.close()
            its = np.delete(info[:, 2], place)
            assert (its == (0 if others is easy else 30)).all(), its
            rows.append(q[place].tobytes() + info[place].tobytes())
    assert len(set(rows)) == 1


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_tiling_edges(model):
    """N on both sides of the four envs of a workgroup; NaN guards behind both outputs (run_ik); env i of the N = 5 batch bitwise
    the same inputs at another place of the N = 67 batch; two calls bitwise alike"""
    form = IC.form_of(model, "head_ori")
    all67 = IC.reachable(model, form, 67)
    out = {}
    for n in (1, 3, 4, 5, 67):
        cases = all67[62:62 + n] if n < 67 else all67
        v = make_env(model, cases)
        v.batch.set_link_probes(0, form.links, np.array(form.points))
        q, info = run_ik(v, 0, form, targets_of(cases, "base"), "base", iterations=7)
        q2, info2 = run_ik(v, 0, form, targets_of(cases, "base"), "base", iterations=7)
        v.close()
        assert np.isfinite(q).all() and np.isfinite(info).all()
        assert q.tobytes() == q2.tobytes() and info.tobytes() == info2.tobytes()
        out[n] = (q, info)
    for n in (1, 3, 4, 5):
        assert out[n][0].tobytes() == out[67][0][62:62 + n].tobytes() and out[n][1].tobytes() == out[67][1][62:62 + n].tobytes()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_read_only(model):
    """state, observations, episode steps and the next steps' rows are bitwise those of a batch that never made the call (the
    warm-start record is private: the next steps agree only if it was left alone); the mass scale does not enter"""
    from trex_gym.vec_env import TrexVecEnv
    n = 33
    envs = [TrexVecEnv(n, device=DEV, params={"warmstart": 0.85}, max_episode_steps=100) for _ in range(2)]
    for e in envs:
        e.reset_tensor()
        random_steps(e, 5, seed=1)
    before, obs = envs[0].get_state().clone(), envs[0].obs.clone()
    form = IC.form_of(model, "three_ori")
    h = envs[0].link_probes(form.links, form.points)
    want = envs[0].link_state(h, velocity=False)
    pos = want.position + 0.05
    q, info = envs[0].inverse_kinematics(h, pos, want.orientation, iterations=12)
    qb, _ = envs[0].inverse_kinematics(h, pos, want.orientation, frame="base", joints=[0, 3, 4], iterations=3)
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(qb).all() and torch.isfinite(info.position_error).all()
    assert envs[0].get_state().cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    assert envs[0].obs.cpu().numpy().tobytes() == obs.cpu().numpy().tobytes()
    assert (envs[0].episode_steps == envs[1].episode_steps).all()
    envs[0].set_domain(mass_scale=torch.full((n, model["nb"]), 1.7))
    q2, _ = envs[0].inverse_kinematics(h, pos, want.orientation, iterations=12)
    assert q2.cpu().numpy().tobytes() == q.cpu().numpy().tobytes()
    envs[0].set_domain(mass_scale=torch.ones(n, model["nb"]))
    envs[1].set_domain(mass_scale=torch.ones(n, model["nb"]))
    rows = []
    for e in envs:
        random_steps(e, 2, seed=2)
        rows.append(e.rows.cpu().numpy())
    assert rows[0].tobytes() == rows[1].tobytes()
    for e in envs:
        e.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(model):
    """every TREX_E_INVALID case of the header, nothing launched: the outputs keep what they held"""
    from trex_gym import _capi
    from trex_gym.vec_env import TrexVecEnv
    n, E = 4, _capi.E_INVALID
    env = TrexVecEnv(n, device=DEV)
    env.reset_tensor()
    b, J = env.batch, env.J
    form = IC.form_of(model, "head_ori")
    K = len(form.links)
    b.set_link_probes(0, form.links, np.array(form.points))
    b.set_link_probes(1, [1] * 9, np.zeros((9, 3)))                     # K = 9
    b.set_link_probes(2, [1] * 5, np.zeros((5, 3)))                     # five targets of mode 3: M = 30
    t = torch.zeros(n, K, 7, device=DEV)
    t[..., 6] = 1
    q = torch.full((n, J), float("nan"), device=DEV)
    info = torch.full((n, 4), float("nan"), device=DEV)
    ok = dict(set=0, modes=form.modes, target=t, q_out=q, frame=0, info=info)

    def attempt(**kw):
        a = dict(ok, **kw)
        b.inverse_kinematics(a.pop("set"), a.pop("modes"), a.pop("target"), a.pop("q_out"), **a)

    refused = functools.partial(gpu_support.refused, E, attempt)

    refused(set=3)                                                      # never set
    refused(set=8)
    refused(set=-1)
    refused(set=1, modes=[1] * 9, target=torch.zeros(n, 9, 7, device=DEV))
    refused(set=2, modes=[3] * 5, target=torch.zeros(n, 5, 7, device=DEV))
    refused(modes=[3, 1, 0, 1])
    refused(modes=[3, 1, 4, 1])
    refused(frame=1)                                                    # TREX_AXES_LINK is no frame for targets
    refused(frame=3)
    refused(frame=-1)
    refused(joint_mask=0)
    refused(joint_mask=1 << J)                                          # no bit among the J joints
    refused(iterations=0)
    refused(iterations=257)
    for name in ("damping", "gain", "max_step", "tol_pos", "tol_ori"):
        for bad in (-1e-3, float("nan"), float("inf")):
            refused(**{name: bad})
    refused(target=t.cpu())
    refused(q_out=q.cpu())
    refused(info=info.cpu())
    refused(q_init=torch.zeros(n, J))
    refused(target=t.double())
    refused(target=torch.zeros(n, K, 6, device=DEV))
    refused(q_out=torch.empty(n, J - 1, device=DEV))
    refused(q_init=torch.empty(n, J + 1, device=DEV))
    refused(info=torch.empty(n * 4 - 1, device=DEV))
    b.set_link_probes(2, [])                                            # freed
    refused(set=2, modes=[1] * 5, target=torch.zeros(n, 5, 7, device=DEV))
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and torch.isnan(info).all()             # nothing was launched
    # the raw C-ABI refuses NULL arguments, host memory and short buffers by itself (the binding's checks bypassed). On 32 768
    # envs q_out is 3 MB and the targets 3.6 MB: more than the allocation a small tensor lives in (info, 0.5 MB, is not: its
    # length is the binding's check above)
    big = TrexVecEnv(32768, device=DEV)
    big.reset_tensor()
    big.batch.set_link_probes(0, form.links, np.array(form.points))
    raw = _capi.lib.trex_batch_inverse_kinematics
    modes = (C.c_int32 * K)(*form.modes)
    p = lambda x: C.c_void_p(x.data_ptr())
    short = torch.full((100,), 7.0, device=DEV)
    tb = torch.zeros(32768, K, 7, device=DEV)
    qb = torch.full((32768, J), 7.0, device=DEV)
    mask = (1 << J) - 1
    assert raw(big.batch.h, 0, modes, 0, p(tb), None, mask, None, None, None, None) == E          # q_out NULL
    assert raw(big.batch.h, 0, modes, 0, None, None, mask, None, p(qb), None, None) == E          # target NULL
    assert raw(big.batch.h, 0, None, 0, p(tb), None, mask, None, p(qb), None, None) == E          # modes NULL
    assert raw(big.batch.h, 0, modes, 0, p(short), None, mask, None, p(qb), None, None) == E
    assert raw(big.batch.h, 0, modes, 0, p(tb), p(short), mask, None, p(qb), None, None) == E
    assert raw(big.batch.h, 0, modes, 0, p(tb), None, mask, None, p(short), None, None) == E
    host = np.zeros(32768 * K * 7, np.float32)
    assert raw(big.batch.h, 0, modes, 0, C.c_void_p(host.ctypes.data), None, mask, None, p(qb), None, None) == E
    torch.cuda.synchronize()
    assert (short == 7.0).all() and (qb == 7.0).all()
    big.close()
    # the batch keeps answering and stepping
    b.inverse_kinematics(0, form.modes, t, q, info=info)
    env.step_tensor(torch.zeros(n, J, device=DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(info).all() and torch.isfinite(env.obs).all()
    env.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["target", "q_init"])
def test_non_finite_inputs_stay_in_their_env(where, model):
    form = IC.form_of(model, "three_ori")
    n = 11
    cases = IC.reachable(model, form, n)
    v = make_env(model, cases)
    v.batch.set_link_probes(0, form.links, np.array(form.points))
    t = targets_of(cases, "world")
    q0 = np.array([c.q_start for c in cases])
    good = run_ik(v, 0, form, t, "world", q0, iterations=9)
    if where == "target":
        t = t.copy()
        t[5, 1, 2] = np.nan
    else:
        q0 = q0.copy()
        q0[5, IC.chain_joints(model, form.links[1])[0]] = np.nan       # a joint that carries a probe
    bad = run_ik(v, 0, form, t, "world", q0, iterations=9)
    v.close()
    keep = [e for e in range(n) if e != 5]
    assert not np.isfinite(bad[0][5]).any() and not np.isfinite(bad[1][5, [0, 1, 3]]).any()
    for g, b in zip(good, bad):
        assert g[keep].tobytes() == b[keep].tobytes()


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_stream_capture(model):
    """after a warm-up call a graph of the single launch - one stream, no branches - replays twice to the eager result, bitwise"""
    form = IC.form_of(model, "k8")
    n = 8
    cases = IC.reachable(model, form, 2 * n)
    v = make_env(model, cases[:n])
    v.batch.set_link_probes(0, form.links, np.array(form.points))
    J, K = v.J, len(form.links)
    t = torch.tensor(targets_of(cases[:n], "world").astype(np.float32), device=DEV)
    q, info = torch.empty(n, J, device=DEV), torch.empty(n, 4, device=DEV)
    call = lambda o: v.batch.inverse_kinematics(0, form.modes, t, o[0], 0, None, None, o[1], iterations=30)

    def change():
        t.copy_(torch.tensor(targets_of(cases[n:], "world").astype(np.float32)))
        v.set_state(torch.tensor(np.array([c.state for c in cases[n:]], np.float32)))

    replay_equals_eager(call, [q, info], change, replays=2, changed=[0])
    v.close()


# 11 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep_chain", "bushy"])
def test_generated_models(name, tmp_path_factory):
    """depth 6 and oblique axes (deep_chain), four children and merged links (bushy) at N = 3: the one-iteration parity and the
    convergence check, on the forms the model's tree allows"""
    import synthetic_models as sm
    path, props, om = sm.compile_both(name, tmp_path_factory.mktemp(name))
    assert om["depth"].max() == 6
    make = lambda cs, q=None: make_env(om, cs, q, path, props["params"])
    worst, qualified = 0.0, 0
    for fname in ("pos4", "head_ori", "same_body", "one_leg"):
        form = IC.form_of(om, fname)
        worst = max(worst, one_iteration_deviation(om, form, 3, name, make))
        cases, q, info, res = converged(om, form, 3, "base", 30, name, make)
        refs = [IC.reference(om, form, c, "base", name, iterations=30) for c in cases]
        print("%s %s: residuals %s, reference %s" % (name, fname, np.array(res).max(0), [max(r["position_error"], r["orientation_error"]) for r in refs]))
        for (rp, ro), r in zip(res, refs):
            if max(r["position_error"], r["orientation_error"]) <= 1e-5:      # (a draw qualified like the T-rex draws: the
                qualified += 1                                                # reference leaves a tenth of the bound at most)
                assert rp <= CONVERGED and ro <= CONVERGED, (name, fname, rp, ro)
    print("%s: one iteration, largest |q - q_ref| %.3g rad; %d draws qualified for the convergence check" % (name, worst, qualified))
    assert qualified >= 6
    assert worst <= TOL[name], (name, worst)


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_facades(model):
    from trex_gym.trex_env import TrexBulletEnv
    from trex_gym.vec_env import TrexVecEnv
    form = IC.form_of(model, "head_ori")
    n, J = 5, model["nb"] - 1
    cases = IC.reachable(model, form, n)
    v = make_env(model, cases)
    h = v.link_probes(form.links, form.points)
    t = torch.tensor(targets_of(cases, "world").astype(np.float32))
    # a NaN row: "not constrained" - the head's orientation is, the others' are not
    ori = torch.full((n, len(form.links), 4), float("nan"))
    ori[:, 0] = t[:, 0, 3:]
    q, info = v.inverse_kinematics(h, t[..., :3], ori, iterations=30)
    want, winfo = run_ik(v, h.slot, form, t.numpy(), iterations=30)
    assert q.cpu().numpy().tobytes() == want.tobytes()
    assert info.position_error.cpu().numpy().tobytes() == winfo[:, 0].tobytes() and (info.iterations == 30).all()
    assert info.initial_error.cpu().numpy().tobytes() == winfo[:, 3].tobytes()
    names = v.model.joint_names
    qm, _ = v.inverse_kinematics(h, t[..., :3], ori, joints=[names[3], 5, names[7]], iterations=4)
    start = v.get_state()[:, 13:13 + J]
    moved = (qm != start).any(0).cpu().numpy()
    assert set(np.nonzero(moved)[0]) <= {3, 5, 7} and moved.any()
    with pytest.raises(ValueError):
        v.inverse_kinematics(h, None, None)
    with pytest.raises(ValueError):
        v.inverse_kinematics(h, t[..., :3], frame="link")
    # joint_targets_to_actions: the inverse of the action scaling - stepping with it commands q; a target outside the limits is clipped
    a = v.joint_targets_to_actions(q)
    assert tuple(a.shape) == (n, v.A) and torch.equal(a, q)
    far = q.clone()
    far[:, 2] = 100.0
    assert float(v.joint_targets_to_actions(far)[:, 2].max()) == float(np.float32(v.model.upper[2]))
    for _ in range(60):
        v.step_tensor(a)
    assert torch.isfinite(v.obs).all()
    v.close()
    # the single env: pybullet's call against the reference at the env's own state
    env = TrexBulletEnv()
    env.reset()
    body_link, link_of = env._pybullet_links()
    idx = body_link[int(model["link_body"][form.links[1]])]       # pybullet's index of the toe's body; its link: the body's own
    toe = link_of[idx]
    s = env._vec.get_state()[0].cpu().numpy().astype(np.float64)
    cur = L.link_state(model, s, [toe])
    tp, tq = IC.f32(cur["position"][0] + [0.05, -0.03, 0.04]), IC.f32(cur["orientation"][0])
    order = np.argsort(env._vec.model.urdf_joint_indices, kind="stable")
    for tori, modes in ((None, [1]), (tq, [3])):
        got = env.calculateInverseKinematics(idx, tp, tori, maxNumIterations=1)
        assert isinstance(got, list) and len(got) == J and all(isinstance(x, float) for x in got)
        # One iteration at the defaults: lambda2 = 1e-4 + 0.1 |e|^2 = 6e-4 here, the Gram matrix of a toe's three joints has
        # entries of order 1 (levers under 1 m), so its condition is at most ~ 3 / 6e-4 = 5e3 and an f32 solve carries
        # 5e3 x 2^-23 of the step, itself at most 0.2 rad: 1.2e-4. The cap of test 1 is that size.
        ref = IK.solve(model, s, [toe], None, modes, np.concatenate([tp, tq]), iterations=1)
        assert np.abs(np.array(got) - ref["q"][order]).max() <= CAPS["one_iter"]
    assert env.calculateInverseKinematics2([idx], [tp], None, 20) == env.calculateInverseKinematics(idx, tp, None, 20)
    with pytest.raises(ValueError):
        env.calculateInverseKinematics(-1, tp)
    env.close()
