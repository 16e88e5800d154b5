"""Host side of the external wrench (no GPU): the exported symbol, trex_gym.perturb.link_wrench against a hand-built case,
RandomPushes on CPU tensors, and the trainer's push flags."""
import numpy as np
import pytest
import torch

from trex_gym import _capi
from trex_gym.perturb import LINK_FRAME, WORLD_FRAME, LinkTable, RandomPushes, link_wrench


def test_symbol_is_exported():
    assert "trex_batch_set_external_wrench" in _capi.SYMBOLS
    assert hasattr(_capi.lib, "trex_batch_set_external_wrench")
    assert hasattr(_capi.Batch, "set_external_wrench")


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _quat(R):   # xyzw of a rotation matrix (trace > 0 here)
    w = 0.5 * np.sqrt(1 + np.trace(R))
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def _case():
    # 3 bodies, 4 links; link 2 belongs to body 1 with a rotated, offset frame
    Rt = _rot([0, 0, 1], 0.4)
    tt = np.array([0.1, -0.2, 0.3])
    tf = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (4, 1))
    tf[2] = np.concatenate([Rt.ravel(), tt])
    com = np.array([[0.0, 0.0, 0.0], [0.05, 0.2, -0.1], [0.0, 0.1, 0.0]])
    table = LinkTable(["a", "b", "head", "c"], [0, 1, 1, 2], tf, com)
    Rb = _rot([1, 2, 3], 0.7)
    pb = np.array([1.0, 2.0, 3.0])
    Rl, pl = Rb @ Rt, pb + Rb @ tt                    # link = body o tf
    poses = np.zeros((2, 4, 7))
    poses[:, :, 6] = 1.0
    poses[:, 2, :3] = pl
    poses[:, 2, 3:] = _quat(Rl)
    return table, torch.tensor(poses), Rb, pb, Rl, pl, com[1]


def test_link_wrench_world_frame_force_at_a_point():
    table, poses, Rb, pb, _, _, comb = _case()
    F = np.array([10.0, -4.0, 2.5])
    P = np.array([1.5, 1.7, 3.2])
    w = link_wrench(table, poses, "head", torch.tensor(F), torch.tensor(P), WORLD_FRAME).numpy()
    c = pb + Rb @ comb
    assert w.shape == (2, 3, 6)
    np.testing.assert_allclose(w[:, 1, :3], np.tile(F, (2, 1)), atol=1e-12)
    np.testing.assert_allclose(w[:, 1, 3:], np.tile(np.cross(P - c, F), (2, 1)), atol=1e-9)
    assert (w[:, [0, 2]] == 0).all()
    # no point: at the COM, no moment; by index the same as by name
    w2 = link_wrench(table, poses, 2, torch.tensor(F)).numpy()
    np.testing.assert_allclose(w2[:, 1, :3], np.tile(F, (2, 1)))
    assert (w2[:, 1, 3:] == 0).all()


def test_link_wrench_link_frame_is_rotated_into_world():
    table, poses, Rb, pb, Rl, pl, comb = _case()
    F = np.array([0.0, 5.0, -1.0])
    Pl = np.array([0.2, 0.0, -0.1])                   # in the link frame
    w = link_wrench(table, poses, "head", torch.tensor(F), torch.tensor(Pl), LINK_FRAME).numpy()
    Fw, Pw = Rl @ F, pl + Rl @ Pl
    c = pb + Rb @ comb
    np.testing.assert_allclose(w[0, 1, :3], Fw, atol=1e-12)
    np.testing.assert_allclose(w[0, 1, 3:], np.cross(Pw - c, Fw), atol=1e-9)
    # accumulates into a given wrench
    acc = link_wrench(table, poses, "head", torch.tensor(F), torch.tensor(Pl), LINK_FRAME, wrench=torch.tensor(w))
    np.testing.assert_allclose(acc.numpy(), 2 * w)
    with pytest.raises(KeyError):
        link_wrench(table, poses, "tail", torch.tensor(F))
    with pytest.raises(ValueError):
        link_wrench(table, poses, 2, torch.tensor(F), frame="body")


def test_random_pushes_rate_direction_and_magnitude():
    n, steps = 2000, 40
    gen = torch.Generator().manual_seed(0)
    p = RandomPushes(n, body=3, interval=4, probability=0.3, max_force=500.0, duration=1, generator=gen)
    starts, draws = 0, 0
    for t in range(steps):
        w = p.wrench(26)
        assert w.shape == (n, 26, 6)
        others = torch.ones(26, dtype=torch.bool)
        others[3] = False
        assert (w[:, others] == 0).all() and (w[:, 3, 2:] == 0).all()      # horizontal, body 3 only, no moment
        f = w[:, 3, :3].norm(dim=-1)
        assert (f <= 500.0 * (1 + 1e-6)).all()
        if t % 4 == 0:
            starts += int((f > 0).sum())
            draws += n
        else:
            assert (f == 0).all()                      # duration 1: a push lasts its own step only
    assert abs(starts / draws - 0.3) < 0.03
    assert f.max() > 0 or starts > 0


def test_random_pushes_duration_and_drop_on_done():
    n = 64
    gen = torch.Generator().manual_seed(1)
    p = RandomPushes(n, body=0, interval=10, probability=1.0, max_force=100.0, duration=3, generator=gen)
    f0 = p.step()
    assert (f0.norm(dim=-1) > 0).all()
    assert torch.equal(p.step(), f0) and torch.equal(p.step(), f0)      # held for 3 env-steps
    assert (p.step() == 0).all()                                         # then gone
    for _ in range(6):
        p.step()
    f1 = p.step()                                                        # step 10: a new draw
    assert (f1.norm(dim=-1) > 0).all()
    done = torch.zeros(n, dtype=torch.bool)
    done[::2] = True
    f2 = p.step(done)
    assert (f2[::2] == 0).all() and torch.equal(f2[1::2], f1[1::2])     # dropped where the episode ended


def test_trainer_parses_the_push_flags():
    from trex_gym import trex_train
    a = trex_train.parse_args(["--push_force", "2000", "--push_interval", "50", "--push_duration", "4"])
    assert (a.push_force, a.push_interval, a.push_duration) == (2000.0, 50, 4)
    d = trex_train.parse_args([])
    assert d.push_force == 0.0
    with pytest.raises(SystemExit):
        trex_train.parse_args(["--push_force", "10", "--graphs"])
