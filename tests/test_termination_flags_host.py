"""CPU: the trainer's --terminate_* flags and the reason names (no device needed)."""
import pytest

from trex_gym import termination, trex_train


def test_flags_make_the_termination_arguments():
    assert trex_train.termination_args(trex_train.parse_args([])) is None
    a = trex_train.parse_args(["--terminate_head_height", "0.6", "--terminate_contact", "link_cranium,link_vertebrae_sacral",
                               "--fall_penalty", "5", "--graphs"])
    assert trex_train.termination_args(a) == dict(head_height=0.6, max_tilt=None, keep_clear=["link_cranium", "link_vertebrae_sacral"],
                                                  penalty=5.0)
    t = trex_train.termination_args(trex_train.parse_args(["--terminate_tilt", "1.2"]))
    assert t == dict(head_height=None, max_tilt=1.2, keep_clear=None, penalty=0.0)
    assert trex_train.termination_args(trex_train.parse_args(["--terminate_contact", "auto"]))["keep_clear"] == ["auto"]


def test_redrawn_gains_are_refused_in_a_graph():
    with pytest.raises(SystemExit):
        trex_train.parse_args(["--terminate_tilt", "1.0", "--graphs", "--gain_scale", "0.1"])
    trex_train.parse_args(["--terminate_tilt", "1.0", "--gain_scale", "0.1"])
    trex_train.parse_args(["--graphs", "--gain_scale", "0.1"])


def test_reason_names():
    assert termination.reason_names(0) == [] and termination.reason_names(5) == ["head", "clearance"]
    assert termination.reason_names(7) == ["head", "tilt", "clearance"]
