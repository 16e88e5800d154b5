"""The small caches TrexVecEnv keeps for its queries - the one-off probe set of link_state() / bias_acceleration(), the output
buffers of ray_test() and closest_points() - and the pass-through of step_tensor()'s actions. What each has to do is written in
the docstring of the method that owns it; here it is pinned, on one env of two copies.

Buffers are told apart by data_ptr() while the test still holds every earlier result: a pointer that differs from all of those
is a new allocation, one that equals an earlier one is that buffer again."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from trex_gym.vec_env import TrexVecEnv
    e = TrexVecEnv(2)
    e.reset_tensor()
    lo = torch.as_tensor(e.model.lower, dtype=torch.float32, device=e.device)
    hi = torch.as_tensor(e.model.upper, dtype=torch.float32, device=e.device)
    for t in range(3):      # off the start pose, with velocities
        e.step_tensor((lo + (hi - lo) * (0.3 + 0.1 * t)).repeat(2, 1).contiguous())
    yield e
    e.close()


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_one_off_probe_sets_do_not_pile_up(env):
    """(a) ten different link lists in turn take ONE of the 8 probe-set slots between them; a handle opened before keeps its own."""
    h = env.link_probes([3, 7])
    assert sum(s is not None for s in env._probe_sets) == 1
    for k in range(10, 20):
        env.link_state([k, k + 1])        # (parent and child of a chain or not: any two links)
        assert sum(s is not None for s in env._probe_sets) == 2
    held, direct = env.link_state(h, acceleration=True), env.link_state(list(h.links), acceleration=True)
    assert held.position.shape == (2, 2, 3) and _same(held, direct)
    assert float(held.linear_velocity.abs().max()) > 0.0
    h.close()
    assert sum(s is not None for s in env._probe_sets) == 1


def test_bias_acceleration_and_link_state_share_the_one_off_set(env):
    """(b) alternated, each evicts the other's set and makes its own again: the answers stay bitwise the first ones."""
    link = 9
    first_b, first_s = env.bias_acceleration(link), env.link_state([link], acceleration=True)
    assert first_b.shape == (2, 6) and first_s.linear_acceleration.shape == (2, 1, 3)
    for _ in range(4):
        assert torch.equal(env.bias_acceleration(link), first_b)
        assert _same(env.link_state([link], acceleration=True), first_s)
    assert sum(s is not None for s in env._probe_sets) == 1


def _ptrs(tensors):
    return [t.data_ptr() for t in tensors]


def test_ray_test_keeps_one_shape_of_buffers(env):
    """(c) the same (R, positions, normals): the same buffers; another R: others; back to the first R: allocated again."""
    g = torch.Generator().manual_seed(0)
    rays4 = torch.cat([torch.rand(4, 3, generator=g) + torch.tensor([0.0, 0.0, 3.0]), torch.rand(4, 3, generator=g) - 1.0], 1).to(env.device)
    rays5 = torch.cat([rays4, rays4[:1]], 0).contiguous()
    a = env.ray_test(rays4, positions=True)
    values = [t.clone() for t in a]
    b = env.ray_test(rays4, positions=True)
    assert len(a) == 3 and _ptrs(a) == _ptrs(b) and _same(values, b)
    c = env.ray_test(rays5, positions=True)
    assert c[0].shape == (2, 5) and not set(_ptrs(c)) & set(_ptrs(a))
    d = env.ray_test(rays4, positions=True)
    assert not set(_ptrs(d)) & set(_ptrs(a) + _ptrs(c)), "two shapes were kept"
    assert _same(values, d)
    e = env.ray_test(rays4, positions=True, normals=True)      # (the flags are part of the key)
    assert len(e) == 4 and not set(_ptrs(e)) & set(_ptrs(a) + _ptrs(c) + _ptrs(d))


def test_closest_points_keeps_one_shape_of_buffers(env):
    """(d) as (c): distance alone and distance with points are two shapes, and one is kept."""
    caps = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.1, 0.05]] * 3
    shapes = env.proximity_shapes(capsules=([1, 5, 9], caps), pairs=[(1, 5), (5, 9), (1, 9)])
    assert len(shapes.pairs) == 3
    a = env.closest_points()
    value = a.clone()
    b = env.closest_points()
    assert a.shape == (2, 3) and a.data_ptr() == b.data_ptr() and torch.equal(b, value)
    c = env.closest_points(points=True)
    assert torch.equal(c.distance, value) and c.point_a.shape == (2, 3, 3) and c.capsule.dtype == torch.int32
    assert a.data_ptr() not in _ptrs(c)
    c2 = env.closest_points(points=True)
    assert _ptrs(c2) == _ptrs(c)
    d = env.closest_points()
    assert d.data_ptr() not in [a.data_ptr()] + _ptrs(c), "two shapes were kept"
    assert torch.equal(d, value)
    env.proximity_shapes(capsules=())


def test_step_tensor_passes_ready_actions_through(env):
    """(e) actions that are float32, contiguous and on the env's device reach the library as they are: no copy, no launch."""
    seen = []
    step_rows = env.batch.step_rows

    def record(actions, *args, **kwargs):
        seen.append(actions)
        return step_rows(actions, *args, **kwargs)

    a = torch.zeros(2, env.A, device=env.device)
    env.batch.step_rows = record
    try:
        env.step_tensor(a)
        env.step_tensor(a.double())
    finally:
        del env.batch.step_rows
    assert seen[0] is a and seen[0].data_ptr() == a.data_ptr()
    assert seen[1].dtype == torch.float32 and seen[1].data_ptr() != a.data_ptr()
