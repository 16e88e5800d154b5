"""Contact sensor without a GPU: the C-ABI symbols, and the torch helpers behind TrexVecEnv.contact_forces / in_contact
(trex_gym.perturb.link_contact_forces, contact_flags) on CPU tensors."""
import numpy as np
import pytest
import torch


def test_symbols_are_exported():
    from trex_gym import _capi
    for name in ("trex_batch_set_contact_sensor", "trex_batch_contact_wrench"):
        assert name in _capi.SYMBOLS
        assert hasattr(_capi.lib, name)
    assert hasattr(_capi.Batch, "set_contact_sensor") and hasattr(_capi.Batch, "contact_wrench")


def table():
    """5 links on 4 bodies: 'foot_L' and its fixed 'toe_L' share body 2."""
    from trex_gym.perturb import LinkTable
    names = ["base", "thigh_L", "foot_L", "toe_L", "foot_R"]
    return LinkTable(names, [0, 1, 2, 2, 3], np.tile(np.r_[np.eye(3).ravel(), 0, 0, 0], (5, 1)), np.zeros((4, 3)))


def test_link_contact_forces_maps_links_to_bodies():
    from trex_gym.perturb import link_contact_forces
    w = torch.arange(2 * 4 * 6, dtype=torch.float32).reshape(2, 4, 6)
    t = table()
    f = link_contact_forces(t, w, ["foot_L", "foot_R"])
    assert f.shape == (2, 2, 3)
    assert torch.equal(f[:, 0], w[:, 2, :3]) and torch.equal(f[:, 1], w[:, 3, :3])
    # links on one body count it once; a group sums distinct bodies; indices work like names
    g = link_contact_forces(t, w, [["foot_L", "toe_L"], ["thigh_L", 4], 3])
    assert torch.equal(g[:, 0], w[:, 2, :3])
    assert torch.equal(g[:, 1], w[:, 1, :3] + w[:, 3, :3])
    assert torch.equal(g[:, 2], w[:, 2, :3])
    with pytest.raises(KeyError):
        link_contact_forces(t, w, ["tail"])


def test_contact_flags_on_cpu_tensors():
    from trex_gym.perturb import contact_flags
    w = torch.zeros(3, 4, 6)
    w[0, 2, 2] = 120.0
    w[1, 3, 2] = 0.5
    w[2, 1, 0] = 50.0          # a tangential value alone is no contact
    f = contact_flags(w)
    assert f.dtype == torch.bool and f.shape == (3, 4) and f.device.type == "cpu"
    assert f.nonzero().tolist() == [[0, 2], [1, 3]]
    assert contact_flags(w, threshold=1.0).nonzero().tolist() == [[0, 2]]
