"""Shared by the GPU tests and by scripts/*_bench.py: envs on the device, random actions, guard-padded output buffers, the refusal
check and the skeleton of the stream-capture tests. Needs torch and a device; the states themselves are tests/state_sets.py (numpy
and the oracle only). A helper, not a conftest: plain functions."""
import numpy as np
import pytest
import torch

from conftest import ASSET_URDF

DEV = "cuda:0"
NB, J = 26, 25


def make_vec(n, urdf=ASSET_URDF, **kw):
    from trex_gym.vec_env import TrexVecEnv
    return TrexVecEnv(n, urdf_path=urdf, device=DEV, **kw)


def loaded_vec(cases, n=None, urdf=ASSET_URDF, params=None, nb=NB, **kw):
    """a TrexVecEnv of n envs holding cases[e % len(cases)] of state_sets.case_states (mass scales included); of the model at `urdf`
    with `nb` bodies, under the engine parameters `params` (the T-rex asset and the defaults)"""
    n = len(cases) if n is None else n
    v = make_vec(n, urdf=urdf, params=params, **kw)
    v.reset()
    idx = np.arange(n) % len(cases)
    ms = np.array([np.ones(nb) if c[1] is None else c[1] for c in cases], np.float32)
    if any(c[1] is not None for c in cases):
        v.set_domain(torch.tensor(ms[idx]))
    v.set_state(torch.tensor(np.array([c[0] for c in cases], np.float32)[idx]))
    return v


def case_env(model, cases, q=None, path=None, params=None):
    """a TrexVecEnv (of the generated model at `path`) holding cases[e].state of ik_cases, or with the joint angles q [n, J] instead"""
    from trex_gym.vec_env import TrexVecEnv
    kw = {} if path is None else dict(urdf_path=path, params=params)
    v = TrexVecEnv(len(cases), device=DEV, **kw)
    v.reset()
    nj = model["nb"] - 1
    st = np.array([c.state for c in cases])
    if q is not None:
        st[:, 13:13 + nj] = q
    v.set_state(torch.tensor(st.astype(np.float32)))
    return v


def random_steps(env, steps, seed=0):
    """`steps` env-steps under uniform random actions within the joint limits, drawn on the host from `seed`"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(env.model.lower, dtype=torch.float32), torch.tensor(env.model.upper, dtype=torch.float32)
    for _ in range(steps):
        a = lo + (hi - lo) * torch.rand(env.num_envs, env.J, generator=g)
        env.step_tensor(a.to(env.device))


def action_limits(model):
    """(lower, upper) joint limits of the oracle model dict in observation order, f32 on the device"""
    oo = model["obs_order"]
    return (torch.tensor(model["q_lower"][oo], dtype=torch.float32, device=DEV),
            torch.tensor(model["q_upper"][oo], dtype=torch.float32, device=DEV))


def random_actions(model, n, gen):
    """[n, J] uniform within the joint limits: ONE draw from the device generator `gen` per call"""
    lo, hi = action_limits(model)
    return lo + (hi - lo) * torch.rand(n, J, generator=gen, device=DEV)


def random_action_steps(model, steps, n, seed):
    """[steps, n, J] uniform within the joint limits in one draw from a device generator seeded `seed` (not the numbers of
    `steps` calls of random_actions)"""
    lo, hi = action_limits(model)
    g = torch.Generator(device=DEV).manual_seed(seed)
    return lo + (hi - lo) * torch.rand(steps, n, J, device=DEV, generator=g)


def contact_counts(v):
    cnt = torch.zeros(v.num_envs, dtype=torch.int32, device=DEV)
    v.batch.contact_stats(cnt, None)
    return cnt


def dynamics_queries(v, link):
    return [v.inverse_dynamics(), v.mass_matrix(), v.jacobian(link, (0.1, 0.2, 0.3)), v.centroidal().data]


def guarded(shape, guard=64, fill=7.0, dtype=torch.float32):
    """a device buffer with `guard` elements of `fill` on either side of the block the kernel may write: (whole, view)"""
    numel = int(np.prod(shape))
    whole = torch.full((numel + 2 * guard,), fill, dtype=dtype, device=DEV)
    return whole, whole[guard:guard + numel].view(*shape)


def guards_intact(whole, shape, guard=64, fill=7.0):
    numel = int(np.prod(shape))
    edges = torch.cat([whole[:guard], whole[guard + numel:]])
    return bool(torch.isnan(edges).all() if fill != fill else (edges == fill).all())


def refused(code, fn, *a, **kw):
    """fn(*a, **kw) raises TrexError with that code"""
    from trex_gym import _capi
    with pytest.raises(_capi.TrexError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, (a, kw)


def same_bits(x, y):
    return x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def replay_equals_eager(call, outs, change_state, replays=1, changed=None):
    """The stream-capture test of a query `call(outs)` that fills the list of tensors `outs`: one warm-up call (it learns the
    buffers), the second call captured on a fresh side stream - one launch, one linear chain -, then `change_state()`, an eager
    call into fresh buffers, and `replays` times: outs zeroed, the graph replayed, outs bitwise the eager results. The outputs
    `changed` (indices; all when None) must differ from what the first state gave: the replay read the new state."""
    call(outs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call(outs)
    first = [o.clone() for o in outs]
    change_state()
    eager = [torch.empty_like(o) for o in outs]
    call(eager)
    torch.cuda.synchronize()
    for _ in range(replays):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, want in zip(outs, eager):
            assert same_bits(o, want)
    for k in range(len(outs)) if changed is None else changed:
        assert not torch.equal(outs[k], first[k])
    del graph
