"""Observation channels on the GPU (trex_batch_set_observation / trex_batch_compose_rows, include/trex_batch.h) against the f64
restatement tests/observation_ref.py - itself pinned by tests/test_observation_ref.py - and against what the batch already offers
(link_state, contact_wrench); the 8-env workgroups' edges, pass-through and read-only, the copied channels, what is written and
what is not, refusals, stream capture, and the trainer on the extended row.

States: those of state_sets.case_states - landing and airborne, every env with a state of its own - and the reset state.

Tolerances: those of tests/test_gpu_link_state.py (tolerances.LINK_TOL), applied as there - TOL['pose'] for the gravity vector, positions and heights,
over max(1, the channel's largest |entry|); TOL['velocity'] for velocities, likewise - times the channel's |scale|. The copied
channels (contact force, previous action, external columns) and the pass-through columns are compared bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import observation_ref as OR
from conftest import ASSET_URDF
from gpu_support import DEV, loaded_vec, make_vec
from state_sets import case_states
from tolerances import LINK_TOL as TOL

pytestmark = pytest.mark.gpu
NB, J = 26, 25
Z = (0.0, 0.0, 0.0)
POSE_KINDS = (OR.GRAVITY, OR.BASE_HEIGHT, OR.POINT_POS, OR.POINT_HEIGHT)
VEL_KINDS = (OR.BASE_LIN, OR.BASE_ANG, OR.POINT_VEL)


def pick(model):
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    toe = [l for l in range(len(names)) if "toe" in names[l]][0]
    deepest = [l for l in range(len(names)) if lb[l] == int(np.argmax(model["depth"]))][0]
    head = [l for l in range(len(names)) if lb[l] == int(model["head_body"])][0]
    return toe, deepest, head


def full_spec(model):
    """every kind; position, velocity, height and contact force on one body (the toe's); a point on the deepest link; scales that
    are not 1; two EXTERNAL channels that split the caller's columns"""
    toe, deepest, head = pick(model)
    p = (0.1, -0.2, 0.3)
    return [(OR.GRAVITY, 0, Z, 1.0), (OR.EXTERNAL, 3, Z, 1.0), (OR.BASE_LIN, 0, Z, 0.5), (OR.BASE_ANG, 0, Z, -0.25),
            (OR.BASE_HEIGHT, 0, Z, 1.0), (OR.POINT_POS, toe, p, 1.0), (OR.POINT_VEL, toe, p, 2.0), (OR.POINT_HEIGHT, toe, p, 1.0),
            (OR.CONTACT, toe, Z, 1.0), (OR.PREV_ACTION, 0, Z, 1.0), (OR.POINT_POS, deepest, (0.05, 0.0, -0.02), -3.0),
            (OR.POINT_VEL, deepest, Z, 1.0), (OR.POINT_HEIGHT, head, (0.3, 0.0, 0.1), 1.0), (OR.EXTERNAL, 4, Z, 1.0)]


def inputs(n, seed, ext_cols=7, ext_stride=9, J=J):
    """actions far outside the joint limits and external columns in a buffer wider than the channels read"""
    gen = torch.Generator().manual_seed(seed)
    act = (10.0 * torch.randn(n, J, generator=gen)).to(DEV)
    ext = torch.randn(n, ext_stride, generator=gen).to(DEV)
    return act, ext


def compose(v, rows, act, ext, extra, pad=0, guard_rows=0, fill=float("nan"), J=J):
    """compose_rows into a fresh buffer prefilled with `fill`, `pad` columns wider than the row and `guard_rows` longer -> tensor"""
    tail = 5 if v._pen_in_rows else 2
    out = torch.full((v.num_envs + guard_rows, 3 * J + extra + tail + pad), fill, device=DEV)
    v.batch.compose_rows(rows, out[:v.num_envs] if guard_rows else out, act, ext)
    torch.cuda.synchronize()
    return out


def check_rows(model, spec, out, rows, state, act, ext, fz, envs=None, factor=1.0, J=J, floor_z=OR.FLOOR_Z):
    """every env of `envs` (all): pass-through bitwise, copied channels bitwise, computed channels within the tolerances"""
    n = rows.shape[0]
    out, rows, state = out.cpu().numpy(), rows.cpu().numpy(), state.cpu().numpy().astype(np.float64)
    act = None if act is None else act.cpu().numpy()
    ext, fz = ext.cpu().numpy(), fz.cpu().numpy()
    E = OR.extra_dim(spec, J)
    tail = out.shape[1] - 3 * J - E
    assert out[:, :3 * J].tobytes() == rows[:, :3 * J].tobytes() and out[:, 3 * J + E:].tobytes() == rows[:, 3 * J:3 * J + tail].tobytes()
    worst = dict(pose=0.0, velocity=0.0)
    for e in (range(n) if envs is None else envs):
        want = OR.channels(model, state[e], spec, action=None if act is None else act[e], extern=ext[e], contact_fz=fz[e],
                           done=rows[e, 3 * J + 1], floor_z=floor_z)
        got = out[e, 3 * J:3 * J + E]
        assert np.isfinite(got).all()
        for (kind, _, _, scale), (c0, w) in zip(spec, OR.columns(spec, J)):
            g, r = got[c0:c0 + w].astype(np.float64), want[c0:c0 + w]
            if kind in POSE_KINDS or kind in VEL_KINDS:
                name = "pose" if kind in POSE_KINDS else "velocity"
                dev = np.abs(g - r).max() / (abs(scale) * max(1.0, np.abs(r).max() / abs(scale)))
                worst[name] = max(worst[name], dev)
                assert dev <= factor * TOL[name], (e, kind, dev, g, r)
            else:
                assert g.astype(np.float32).tobytes() == r.astype(np.float32).tobytes(), (e, kind, g, r)
    return worst


def sensed(n, **kw):
    v = make_vec(n, **kw)
    v.enable_contact_sensor(True)
    v.reset_tensor()
    return v


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 67])
def test_values_against_reference(n, oracle64, model):
    """n on both sides of the 8-env workgroup; after reset, and on the landing / airborne states. Largest deviations measured on
    an MI355X at n = 67 (profiles/r21_observations.txt): pose 3.33e-7 against TOL 8.24e-7, velocity 5.44e-7 against 1.73e-6."""
    spec = full_spec(model)
    v = sensed(n)
    E = v.batch.set_observation(spec)
    assert E == OR.extra_dim(spec, J) == v.batch.observation_dim() - 3 * J
    act, ext = inputs(n, seed=n)
    worst = []
    for fallen in (False, True):
        if fallen:
            cases = case_states(oracle64, model, n)
            v.set_state(torch.tensor(np.array([c[0] for c in cases], np.float32)))
        out = compose(v, v.rows, act, ext, E)
        worst.append(check_rows(model, spec, out, v.rows, v.get_state(), act, ext, v.contact_wrench()[:, :, 2]))
    print("observation deviations N=%d: reset %s, states %s" % (n, worst[0], worst[1]))
    v.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pen", [False, True])
def test_pass_through_and_read_only(pen, model):
    """twin envs on the same actions, one with observations: the 3J columns, reward, done and penalties of every step, the state
    and the episode counts at the end are bitwise the same - the compose launch reads only, through resets inside the step"""
    from trex_gym import observations as O
    from trex_gym.vec_env import TrexVecEnv
    n = 9
    toe, deepest, _ = pick(model)
    spec = O.gravity() + O.base_velocity() + O.base_height() + O.point(toe, (0.1, 0, 0), velocity=True, height=True) + \
        O.contact_force(toe) + O.prev_action() + O.external(3) + O.point(deepest)
    ext = torch.randn(n, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    kw = dict(urdf_path=ASSET_URDF, device=DEV, max_episode_steps=16, penalties_in_rows=pen, params={"warmstart": 0.85})
    plain, wide = TrexVecEnv(n, **kw), TrexVecEnv(n, observations=spec, external=ext, **kw)
    D = wide.obs_dim
    assert D == 3 * J + 3 + 6 + 1 + 7 + 1 + J + 3 + 3 == wide.observation_space.shape[0] and plain.obs_dim == 3 * J
    assert wide.rows.shape == (n, D + (5 if pen else 2)) and plain.rows.shape == (n, 3 * J + (5 if pen else 2))
    for e in (plain, wide):
        e.reset_tensor()
    gen = torch.Generator().manual_seed(2)
    lo, hi = torch.tensor(model["q_lower"][model["obs_order"]], dtype=torch.float32), torch.tensor(model["q_upper"][model["obs_order"]], dtype=torch.float32)
    ends = 0
    for t in range(40):
        a = (lo + (hi - lo) * torch.rand(n, J, generator=gen)).to(DEV)
        for e in (plain, wide):
            e.step_tensor(a)
        same = lambda x, y: x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert same(plain.obs, wide.obs[:, :3 * J].contiguous()), t
        assert same(plain.rew, wide.rew) and same(plain.done_f, wide.done_f) and same(plain.done, wide.done), t
        assert same(plain.penalties.contiguous(), wide.penalties.contiguous()), t
        assert torch.isfinite(wide.obs).all()
        ends += int(wide.done.sum())
    assert ends == 2 * n                                            # steps 16 and 32: every env twice
    assert plain.get_state().cpu().numpy().tobytes() == wide.get_state().cpu().numpy().tobytes()
    assert torch.equal(plain.episode_steps, wide.episode_steps)
    with pytest.raises(ValueError, match="step_many_tensor"):
        wide.step_many_tensor(torch.zeros(2, n, J, device=DEV))
    assert wide.all_gather_obs().shape == (n, D)
    for e in (plain, wide):
        e.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_copied_channels_are_bitwise(model):
    """CONTACT_FORCE = contact_wrench()[:, body, 2] once the robot stands on the floor; EXTERNAL = the source columns; PREV_ACTION
    = the actions as passed, beyond the joint limits, 0 for the envs whose episode ended with the step and after reset_tensor"""
    from trex_gym import observations as O
    from trex_gym.vec_env import TrexVecEnv
    n = 9
    toe, _, _ = pick(model)
    bodies = sorted(set(int(b) for b in model["link_body"]) - {0})
    first_link = {int(b): l for l, b in reversed(list(enumerate(model["link_body"])))}
    spec = [c for b in bodies for c in O.contact_force(first_link[b])] + O.external(2) + O.prev_action() + O.external(1)
    ext = torch.randn(n, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    v = TrexVecEnv(n, urdf_path=ASSET_URDF, device=DEV, observations=spec, external=lambda env: ext, max_episode_steps=45)
    nc = len(bodies)
    v.reset_tensor()
    v.set_episode_steps(torch.arange(n) * 5)                        # the episodes end at different steps
    assert (v.obs[:, 3 * J + nc + 2:3 * J + nc + 2 + J] == 0).all()
    gen = torch.Generator().manual_seed(4)
    seen_done = seen_contact = 0
    for t in range(44):
        a = (3.0 * torch.randn(n, J, generator=gen)).to(DEV)        # far outside the limits
        v.step_tensor(a)
        ch = v.obs[:, 3 * J:]
        fz = v.contact_wrench()[:, bodies, 2]
        assert ch[:, :nc].contiguous().cpu().numpy().tobytes() == fz.contiguous().cpu().numpy().tobytes(), t
        assert torch.equal(ch[:, nc:nc + 2], ext[:, :2]) and torch.equal(ch[:, nc + 2 + J], ext[:, 2])
        prev = ch[:, nc + 2:nc + 2 + J]
        done = v.done
        assert torch.equal(prev[~done], a[~done]) and (prev[done] == 0).all(), t
        seen_done += int(done.sum())
        seen_contact += int((fz != 0).sum())
    assert seen_done >= n - 1 and seen_contact > 0
    v.reset_tensor()
    assert (v.obs[:, 3 * J + nc + 2:3 * J + nc + 2 + J] == 0).all() and torch.equal(v.obs[:, 3 * J + nc:3 * J + nc + 2], ext[:, :2])
    v.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_point_channels_agree_with_link_state(oracle64, model):
    """POINT_POSITION and POINT_VELOCITY against link_state(axes='base') of the same batch, within 2 x TOL"""
    n = 9
    cases = case_states(oracle64, model, n)
    v = loaded_vec(cases)
    links = list(pick(model)) + [0]
    pts = np.array([[0.1, -0.2, 0.3], [0.05, 0.0, -0.02], [0.0, 0.0, 0.0], [0.25, 0.5, -0.125]], np.float32)
    spec = [c for l, p in zip(links, pts) for c in ((OR.POINT_POS, l, tuple(p), 1.0), (OR.POINT_VEL, l, tuple(p), 1.0))]
    E = v.batch.set_observation(spec)
    out = compose(v, v.rows, None, None, E)[:, 3 * J:3 * J + E].reshape(n, len(links), 6).cpu().numpy().astype(np.float64)
    ls = v.link_state(v.link_probes(links, pts.astype(np.float64)), axes="base")
    pos, vel = ls.position.cpu().numpy().astype(np.float64), ls.linear_velocity.cpu().numpy().astype(np.float64)
    for e in range(n):
        assert np.abs(out[e, :, :3] - pos[e]).max() <= 2 * TOL["pose"] * max(1.0, np.abs(pos[e]).max()), e
        assert np.abs(out[e, :, 3:] - vel[e]).max() <= 2 * TOL["velocity"] * max(1.0, np.abs(vel[e]).max()), e
    v.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("pen", [False, True])
def test_every_element_written_nothing_else(n, pen, model):
    spec = full_spec(model)
    v = sensed(n, penalties_in_rows=pen)
    E = v.batch.set_observation(spec)
    act, ext = inputs(n, seed=5)
    W = 3 * J + E + (5 if pen else 2)
    out = compose(v, v.rows, act, ext, E, pad=5, guard_rows=1)
    assert out.shape == (n + 1, W + 5)
    assert torch.isfinite(out[:n, :W]).all()
    assert torch.isnan(out[:n, W:]).all() and torch.isnan(out[n]).all()
    v.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(model):
    """every TREX_E_INVALID case of the header, before any launch: the out buffer keeps its fill"""
    from trex_gym import _capi
    E_INV = _capi.E_INVALID
    toe, _, _ = pick(model)
    n = 4096                                # (rows of 4096 envs: larger than the allocation a small tensor lives in)
    v = make_vec(n)
    v.reset_tensor()
    b = v.batch
    raw = _capi.lib.trex_batch_compose_rows
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rows, act = v.rows, torch.zeros(n, J, device=DEV)
    assert raw(b.h, p(rows), rows.shape[1], None, None, 0, p(rows), 600, None) == E_INV          # no channels set
    with pytest.raises(_capi.TrexError):
        b.set_observation([(OR.KINDS, 0, Z, 1.0)])
    with pytest.raises(_capi.TrexError):
        b.set_observation([(OR.POINT_POS, len(model["link_names"]), Z, 1.0)])
    assert b.observation_dim() == 3 * J
    # a contact channel while the sensor is off
    E = b.set_observation([(OR.CONTACT, toe, Z, 1.0)])
    out = torch.full((n, 3 * J + E + 2), 7.0, device=DEV)
    assert raw(b.h, p(rows), rows.shape[1], None, None, 0, p(out), out.shape[1], None) == E_INV
    assert "sensor is off" in _capi.lib.trex_last_error().decode()
    # EXTERNAL: no extern, a stride below the channels' columns, a short buffer
    E = b.set_observation([(OR.EXTERNAL, 300, Z, 1.0), (OR.GRAVITY, 0, Z, 1.0), (OR.EXTERNAL, 100, Z, 1.0)])
    assert E == 403 and b.observation_dim() == 3 * J + 403
    W = 3 * J + E + 2
    out = torch.full((n, W), 7.0, device=DEV)
    ext = torch.zeros(n, 400, device=DEV)
    short = torch.full((100,), 7.0, device=DEV)
    host = np.zeros(n * W, np.float32)
    ok = lambda *a: raw(b.h, *a, None)
    assert ok(p(rows), rows.shape[1], None, None, 0, p(out), W) == E_INV                           # extern NULL
    assert ok(p(rows), rows.shape[1], None, p(ext), 399, p(out), W) == E_INV                       # extern_stride < 400
    assert ok(p(rows), rows.shape[1], None, p(short), 400, p(out), W) == E_INV                     # extern short
    assert ok(p(rows), rows.shape[1], None, p(ext), 400, p(short), W) == E_INV                     # out short
    assert ok(p(rows), rows.shape[1], None, p(ext), 400, C.c_void_p(host.ctypes.data), W) == E_INV  # out in host memory
    assert ok(C.c_void_p(host.ctypes.data), rows.shape[1], None, p(ext), 400, p(out), W) == E_INV  # rows in host memory
    assert ok(p(rows), rows.shape[1], None, p(ext), 400, p(out), W - 1) == E_INV                   # out_stride too small
    assert ok(p(rows), 3 * J + 1, None, p(ext), 400, p(out), W) == E_INV                           # row_stride too small
    assert ok(p(out), W, None, p(ext), 400, p(out), W) == E_INV                                    # out is rows
    assert ok(p(out), W, None, p(ext), 400, C.c_void_p(out.data_ptr() + 4 * (n - 1) * W), W) == E_INV   # out overlaps rows' last row
    assert "overlaps" in _capi.lib.trex_last_error().decode()
    assert ok(None, rows.shape[1], None, p(ext), 400, p(out), W) == E_INV and ok(p(rows), rows.shape[1], None, p(ext), 400, None, W) == E_INV
    with pytest.raises(_capi.TrexError):
        b.compose_rows(rows, out.cpu(), None, ext)
    with pytest.raises(_capi.TrexError):
        b.compose_rows(rows, out[:, :W - 1].contiguous(), None, ext)
    # PREV_ACTION: actions in host memory, and too few of them
    b.set_observation([(OR.PREV_ACTION, 0, Z, 1.0)])
    out2 = torch.full((n, 3 * J + J + 2), 7.0, device=DEV)
    assert ok(p(rows), rows.shape[1], C.c_void_p(host.ctypes.data), None, 0, p(out2), out2.shape[1]) == E_INV
    with pytest.raises(_capi.TrexError):
        b.compose_rows(rows, out2, short, None)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (out2 == 7.0).all() and (short == 7.0).all()
    # the batch keeps answering: the same call with good buffers, and clearing
    assert ok(p(rows), rows.shape[1], p(act), None, 0, p(out2), out2.shape[1]) == 0
    torch.cuda.synchronize()
    assert torch.equal(out2[:, :3 * J], rows[:, :3 * J]) and (out2[:, 3 * J:3 * J + J] == 0).all()
    assert b.set_observation([]) == 0 and b.observation_dim() == 3 * J
    v.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_stream_capture(model):
    """6 steps of step + compose inside torch.cuda.graph on one stream, replayed from the reset state, are bitwise the eager run"""
    from trex_gym import observations as O
    from trex_gym.vec_env import TrexVecEnv
    n, T = 8, 6
    toe, deepest, _ = pick(model)
    spec = O.gravity() + O.base_velocity() + O.base_height() + O.contact_force(toe) + O.point(toe, velocity=True) + O.prev_action() + \
        O.external(2) + O.point(deepest, height=True)
    ext = torch.randn(n, 2, generator=torch.Generator().manual_seed(6)).to(DEV)
    v = TrexVecEnv(n, urdf_path=ASSET_URDF, device=DEV, observations=spec, external=ext)
    acts = (0.3 * torch.randn(T, n, J, generator=torch.Generator().manual_seed(7))).to(DEV)
    log = torch.zeros(T, *v.rows.shape, device=DEV)

    def run():
        for t in range(T):
            v.step_tensor(acts[t])
            log[t].copy_(v.rows)

    v.reset_tensor()
    run()                                                           # the first calls: the batch learns the buffers
    v.reset_tensor()
    run()
    torch.cuda.synchronize()
    eager = log.clone()
    assert torch.isfinite(eager).all() and not torch.equal(eager[0], eager[-1])
    v.reset_tensor()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run()
    log.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert log.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()
    del graph
    v.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_trainer_end_to_end(model):
    """the on-device trainer reads the extended row in place: D = 93 with the locomotion preset, two rollouts and updates with the
    native learner; a specification too wide for the learner is refused when the trainer is made"""
    from trex_gym import _capi, observations as O
    from trex_gym.ppo import PPO
    from trex_gym.vec_env import TrexVecEnv
    n = 64
    loco = O.locomotion(_capi.Model(ASSET_URDF), DEV)
    assert sum(O.width(c, J) for c in loco) == 18
    env = TrexVecEnv(n, urdf_path=ASSET_URDF, device=DEV, observations=loco, terminate=dict(max_tilt=1.0, penalty=1.0),
                     max_episode_steps=200)
    assert env.observation_space.shape == (93,) and env.rows.shape == (n, 95)
    agent = PPO(env, nsteps=8, nminibatches=2, noptepochs=1, seed=0)
    assert agent.kern.D == 93 and agent.native_learner
    theta0 = agent.policy.theta.detach().clone()
    for _ in range(2):                                             # (steps 8 .. 15, the second rollout: the dropped robot meets the floor)
        agent.update(agent.collect())
    torch.cuda.synchronize()
    assert torch.isfinite(agent.b_obs).all() and torch.isfinite(agent.policy.theta).all()
    spread = agent.b_obs[:, :, 75:].std(dim=1)                     # over the envs, per step and column
    assert (spread.max(dim=0).values > 0).all(), spread.max(dim=0).values
    assert not torch.equal(agent.policy.theta.detach(), theta0)
    env.close()
    wide = TrexVecEnv(n, urdf_path=ASSET_URDF, device=DEV, observations=loco + O.prev_action())
    assert wide.observation_space.shape == (118,)
    with pytest.raises(ValueError, match="96"):
        PPO(wide, nsteps=8, nminibatches=2, noptepochs=1)
    wide.close()
    wider = TrexVecEnv(4, urdf_path=ASSET_URDF, device=DEV, observations=loco + O.external(40), external=torch.zeros(4, 40, device=DEV))
    with pytest.raises(ValueError, match="126"):
        PPO(wider, nsteps=8, nminibatches=2, noptepochs=1, native_learner=False)
    wider.close()


def test_training_script_stores_the_specification(tmp_path):
    """--observations locomotion selects the preset; the checkpoint carries the channels, and load_agent rebuilds the same row"""
    from trex_gym import trex_train
    args = trex_train.parse_args(["--observations", "locomotion", "--num_envs", "64"])
    assert args.observations == "locomotion" and trex_train.parse_args([]).observations is None
    env = trex_train.build_environment(64, device=DEV, observations=args.observations)
    assert env.obs_dim == 93 and len(env.observations) == 8
    path = str(tmp_path / "policy.pt")
    agent, hist = trex_train.train(env, 64 * 32, 0, nsteps=32, noptepochs=1, save_path=path, log=lambda *a: None)
    assert len(hist) == 1 and agent.kern.D == 93
    env.close()
    again = trex_train.load_agent(path, num_envs=4, device=DEV)
    assert again.env.observations == env.observations and again.env.obs_dim == 93 and again.kern.D == 93
    assert torch.equal(again.policy.theta.detach(), agent.policy.theta.detach())
    _, rewards = trex_train.play(again, 3, log=lambda *a: None)
    assert rewards.shape == (3,) and np.isfinite(rewards).all()
    again.env.close()
    with pytest.raises(ValueError, match="--observations"):
        trex_train.build_environment(4, device=DEV, observations="no_such_preset")


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_many_workgroups(oracle64, model):
    """one compose at n = 4096 - 512 workgroups: 64 sampled envs (first, last, a spread) against the reference"""
    n = 4096
    spec = full_spec(model)
    cases = case_states(oracle64, model, 67)
    v = sensed(n)
    v.set_state(torch.tensor(np.array([c[0] for c in cases], np.float32)[np.arange(n) % len(cases)]))
    E = v.batch.set_observation(spec)
    act, ext = inputs(n, seed=9)
    out = compose(v, v.rows, act, ext, E)
    assert torch.isfinite(out).all()
    envs = sorted(set(np.linspace(0, n - 1, 64).astype(int).tolist()))
    w = check_rows(model, spec, out, v.rows, v.get_state(), act, ext, v.contact_wrench()[:, :, 2], envs=envs)
    print("observation deviations N=4096 (64 envs):", w)
    v.close()
