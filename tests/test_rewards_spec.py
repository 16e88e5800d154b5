"""trex_gym.rewards without a GPU: what the constructors make and that they add up, names, links / joints / bodies resolved to
indices and mask bits, the plain-data form a checkpoint stores, refusals by name, and the training script's flags."""
import io

import pytest
import torch

import reward_ref as RR

J = 25


def test_constructors_add_up():
    from trex_gym import rewards as R
    assert {R.KINDS[k] for k in R.KINDS} == set(range(RR.KINDS)) and R.MAX_TERMS == RR.MAX_TERMS
    pairs = dict(step=RR.STEP, alive=RR.ALIVE, track_lin_vel=RR.TRACK_LIN, track_ang_vel=RR.TRACK_ANG, lin_vel_z=RR.LIN_VEL_Z,
                 ang_vel_xy=RR.ANG_VEL_XY, orientation=RR.ORIENTATION, base_height=RR.BASE_HEIGHT, point_height=RR.POINT_HEIGHT,
                 torque=RR.TORQUE, joint_vel=RR.JOINT_VEL, joint_acc=RR.JOINT_ACC, action_rate=RR.ACTION_RATE, joint_limit=RR.JOINT_LIMIT,
                 power=RR.POWER, joint_pose=RR.JOINT_POSE, contact_count=RR.CONTACT_COUNT, foot_air_time=RR.FOOT_AIR_TIME,
                 foot_slip=RR.FOOT_SLIP)
    assert R.KINDS == pairs
    spec = R.step(0.5) + R.alive() + R.track_lin_vel(1.0, 0.25) + R.track_ang_vel(0.5, 0.5) + R.lin_vel_z() + R.ang_vel_xy() + \
        R.orientation() + R.base_height(-1.0, 0.6) + R.point_height(1.0, "link_cranium", 0.9, (0.1, 0, 0)) + R.torque(-1e-4) + \
        R.joint_vel(-1e-3, joints=[0, "b"]) + R.joint_acc() + R.action_rate() + R.joint_limit(-1.0, 0.9) + R.power() + \
        R.joint_pose(-0.1, joints=[24]) + R.contact_count(-1.0, ["link_cranium", 3], 2.0) + R.foot_air_time(1.0, 7, 1.0, 0.3) + \
        R.foot_slip(-0.1, 7, 1.0)
    assert [c.kind for c in spec] == list(pairs) and all(isinstance(c, R.Term) for c in spec)
    assert R.names(spec) == ["step", "alive", "track_lin_vel", "track_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "base_height",
                             "point_height[link_cranium]", "torque", "joint_vel", "joint_acc", "action_rate", "joint_limit", "power",
                             "joint_pose", "contact_count", "foot_air_time[7]", "foot_slip[7]"]
    assert R.names(R.torque() + R.torque(joints=[1]) + R.foot_slip(1, 7) + R.foot_slip(1, 7)) == ["torque", "torque#2", "foot_slip[7]", "foot_slip[7]#2"]
    link = lambda l: 43 if l == "link_cranium" else int(l)
    joint = lambda j: 1 if j == "b" else int(j)
    terms, contact, command, actions = R.resolve([spec[:5], spec[5:]], link, joint, lambda l: l // 2)     # (nested lists flatten)
    assert contact and command and actions and len(terms) == 19
    assert [t[0] for t in terms] == list(range(19))
    assert [t[1] for t in terms] == [0] * 8 + [43] + [0] * 8 + [7, 7]
    assert [t[2] for t in terms] == [0] * 10 + [3, 0, 0, 0, 0, 1 << 24, (1 << 21) | (1 << 1), 0, 0]
    assert terms[8][3] == (0.1, 0.0, 0.0) and terms[8][4:] == (1.0, 0.9, 0.0) and terms[17][4:] == (1.0, 1.0, 0.3)
    assert R.resolve(R.alive(), link, joint, int)[1:] == (False, False, False)


def test_refused_by_name():
    from trex_gym import rewards as R
    with pytest.raises(ValueError, match="track_lin_vel: sigma must be positive"):
        R.track_lin_vel(1.0, 0.0)
    with pytest.raises(ValueError, match="track_ang_vel: sigma must be positive"):
        R.track_ang_vel(1.0, -1.0)
    with pytest.raises(ValueError, match="joint_limit: soft must lie in"):
        R.joint_limit(-1.0, 0.0)
    with pytest.raises(ValueError, match="joint_limit: soft must lie in"):
        R.joint_limit(-1.0, 1.5)
    with pytest.raises(ValueError, match="torque: weight, parameters and xyz must be finite"):
        R.torque(float("nan"))
    with pytest.raises(ValueError, match="point_height: xyz must have 3 entries"):
        R.point_height(1.0, 3, xyz=(0.0, 1.0))
    with pytest.raises(ValueError, match="foot_slip: weight, parameters and xyz must be finite"):
        R.foot_slip(1.0, 3, xyz=(0.0, float("inf"), 0.0))
    with pytest.raises(ValueError, match="unknown reward term kind 'tilt'"):
        R.resolve([R.Term("tilt", 0, None, (0, 0, 0), 1.0, 0.0, 0.0)], int, int, int)
    with pytest.raises(ValueError, match="unknown reward term kind 19"):
        R.names([R.Term(19, 0, None, (0, 0, 0), 1.0, 0.0, 0.0)])
    with pytest.raises(ValueError, match="sigma must be positive"):
        R.resolve([R.Term("track_lin_vel", 0, None, (0, 0, 0), 1.0, 0.0, 0.0)], int, int, int)
    with pytest.raises(ValueError, match="33 terms, at most 32"):
        R.resolve(R.alive() * 33, int, int, int)


def test_plain_data_round_trip():
    from trex_gym import rewards as R
    spec = R.step(0.0) + R.torque(-1e-4, joints=["a", 3]) + R.foot_slip(-0.1, "link_toe", 1.0, (0.25, -0.5, 0.125)) + \
        R.contact_count(-1.0, ["link_tail", 2])
    data = R.as_tuples(spec)
    buf = io.BytesIO()
    torch.save({"rewards": data, "command": [0.5, 0.0, 0.0], "none": None}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)
    assert back["rewards"] == data and back["none"] is None and back["command"] == [0.5, 0.0, 0.0]
    assert R.from_tuples(back["rewards"]) == spec
    assert set(R.PRESETS) == {"locomotion"}


def test_training_flags():
    from trex_gym import trex_train
    a = trex_train.parse_args([])
    assert a.rewards is None and a.command is None
    a = trex_train.parse_args(["--rewards", "locomotion", "--command", "0.5", "0", "-0.25"])
    assert a.rewards == "locomotion" and a.command == [0.5, 0.0, -0.25]
    with pytest.raises(SystemExit):
        trex_train.parse_args(["--rewards", "everything"])
    with pytest.raises(SystemExit):
        trex_train.parse_args(["--command", "1", "0", "0"])
