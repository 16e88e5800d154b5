"""The actuator model without a GPU: exported symbols, the header's declarations, argument handling of the Python layer."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NAMES = ["j%d" % k for k in range(5)]


def test_symbols_are_exported_and_declared():
    from trex_gym import _capi
    header = open(os.path.join(ROOT, "include", "trex_batch.h")).read()
    for s in ("trex_batch_set_control_mode", "trex_batch_set_motor_gains", "trex_batch_set_stiffness_actions"):
        assert hasattr(_capi.lib, s), s
        assert re.search(r"\bint %s\(" % s, header), s
    for k, name in enumerate(("TREX_CTRL_POSITION", "TREX_CTRL_VELOCITY", "TREX_CTRL_TORQUE")):
        assert re.search(r"#define %s\s+%d\b" % (name, k), header)
    assert _capi.Batch.CONTROL_MODES == {"position": 0, "velocity": 1, "torque": 2}


def test_resolve_control_modes():
    from trex_gym.actuators import resolve_control_modes as r
    assert r(None, NAMES) == [0] * 5
    assert r("torque", NAMES) == [2] * 5
    assert r(["position", 1, "torque", 0, 2], NAMES) == [0, 1, 2, 0, 2]
    assert r({"j3": "velocity", "j0": 2}, NAMES) == [2, 0, 0, 1, 0]
    for bad in ("force", [0, 1], {"nope": 1}, [0, 1, 2, 3, 0], [0.5] * 5):
        with pytest.raises((ValueError, KeyError)):
            r(bad, NAMES)


def test_action_bounds():
    from trex_gym.actuators import action_bounds
    lower, upper = -np.arange(1.0, 6.0), np.arange(1.0, 6.0)
    lo, hi = action_bounds([0, 1, 2, 0, 0], lower, upper, 100.0, 3e5)
    np.testing.assert_array_equal(lo, np.float32([-1, -100, -3e5, -4, -5]))
    np.testing.assert_array_equal(hi, np.float32([1, 100, 3e5, 4, 5]))
    lo, hi = action_bounds([0] * 5, lower, upper, 100.0, 3e5, variable_stiffness=True, kp_max=0.5)
    assert lo.shape == hi.shape == (10,) and (lo[5:] == 0).all() and (hi[5:] == 0.5).all() and lo.dtype == np.float32


def test_broadcast_gains():
    from trex_gym.actuators import broadcast_gains as b
    assert b(None, 3, 5) is None
    for v in (0.25, np.full(5, 0.25), torch.full((3, 5), 0.25), [0.25] * 5):
        t = b(v, 3, 5)
        assert t.shape == (3, 5) and t.dtype == torch.float32 and t.is_contiguous() and (t == 0.25).all()
    for bad in (np.zeros(4), np.zeros((2, 5)), np.zeros((3, 5, 1))):
        with pytest.raises(ValueError):
            b(bad, 3, 5)


def test_random_gains_on_cpu_tensors():
    from trex_gym.perturb import RandomGains
    g = RandomGains(6, 25, kp_scale=(0.5, 2.0), kd_scale=(1.0, 1.0), max_force_scale=(0.1, 0.3),
                    generator=torch.Generator().manual_seed(3))
    d = g.draw()
    assert set(d) == {"kp", "kd", "max_force"} and all(t.shape == (6, 25) and t.is_contiguous() for t in d.values())
    assert ((d["kp"] >= 0.5 * 5e-3) & (d["kp"] <= 2.0 * 5e-3)).all() and (d["kd"] == 0.1).all()
    assert ((d["max_force"] >= 0.1 * 3e5) & (d["max_force"] <= 0.3 * 3e5)).all()
    assert (d["kp"] == d["kp"][:, :1]).all() and d["kp"][:, 0].unique().numel() == 6      # one scale per env
    mask = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.uint8)
    d2 = g.draw(mask)
    same = (d2["kp"][:, 0] == d["kp"][:, 0])
    assert same.tolist() == [True, False, True, True, False, True]
    with pytest.raises(ValueError):
        RandomGains(2, 25, kp_scale=(1.2, 0.8))


def test_trainer_flags():
    from trex_gym import trex_train
    a = trex_train.parse_args([])
    assert a.control_mode == "position" and not a.variable_stiffness and a.gain_scale == 0.0
    assert trex_train.parse_args(["--control_mode", "torque", "--gain_scale", "0.2"]).control_mode == "torque"
    for bad in (["--variable_stiffness"], ["--control_mode", "force"], ["--gain_scale", "1.5"]):
        with pytest.raises(SystemExit):
            trex_train.parse_args(bad)
    with pytest.raises(ValueError, match="policy kernel"):
        trex_train.check_action_space("position", True)
    with pytest.raises(ValueError):
        trex_train.check_action_space("force", False)
    trex_train.check_action_space("velocity", False)
