"""trex_gym.observations without a GPU: what the constructors make, their widths against the reference's, link names resolved to
indices, the plain-data form a checkpoint stores, and the training script's flag."""
import io

import pytest
import torch

import observation_ref as OR

J = 25


def test_constructors_and_widths():
    from trex_gym import observations as O
    assert {O.KINDS[k] for k in O.KINDS} == set(range(OR.KINDS)) and O.KINDS["projected_gravity"] == OR.GRAVITY
    assert O.KINDS["contact_force"] == OR.CONTACT and O.KINDS["prev_action"] == OR.PREV_ACTION and O.KINDS["external"] == OR.EXTERNAL
    spec = O.gravity() + O.base_velocity() + O.base_height(2.0) + O.point("link_cranium", (0.1, 0, 0), velocity=True, height=True) + \
        O.contact_force(7) + O.prev_action() + O.external(4)
    assert [c.kind for c in spec] == ["projected_gravity", "base_linear_velocity", "base_angular_velocity", "base_height",
                                      "point_position", "point_velocity", "point_height", "contact_force", "prev_action", "external"]
    assert [O.width(c, J) for c in spec] == [3, 3, 3, 1, 3, 3, 1, 1, J, 4]
    assert O.base_velocity(angular=False)[0].kind == "base_linear_velocity" and len(O.base_velocity(linear=False)) == 1
    assert O.point(3, position=False, height=True) == [O.Channel("point_height", 3, (0.0, 0.0, 0.0), 1.0)]
    with pytest.raises(ValueError):
        O.external(0)
    with pytest.raises(ValueError):
        O.point(3, (0.0, 1.0))
    chans, extra, contact, ext = O.resolve([spec[:4], spec[4:]], lambda l: 43 if l == "link_cranium" else int(l), J)      # (nested lists flatten)
    assert extra == OR.extra_dim(chans, J) == 47 and contact and ext == 4
    assert [c[1] for c in chans] == [0, 0, 0, 0, 43, 43, 43, 7, 0, 4] and chans[3][3] == 2.0
    with pytest.raises(ValueError, match="unknown observation channel kind"):
        O.resolve([O.Channel("tilt", 0, (0, 0, 0), 1.0)], int, J)
    assert (O.MAX_CHANNELS, O.MAX_DIM) == (64, 512)


def test_plain_data_round_trip():
    from trex_gym import observations as O
    spec = O.gravity() + O.point("link_cranium", (0.25, -0.5, 0.125), velocity=True) + O.external(3, scale=0.5)
    data = O.as_tuples(spec)
    buf = io.BytesIO()
    torch.save({"observations": data, "none": None}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)
    assert back["observations"] == data and back["none"] is None
    assert O.from_tuples(back["observations"]) == spec


def test_training_flag():
    from trex_gym import trex_train
    assert trex_train.parse_args([]).observations is None
    assert trex_train.parse_args(["--observations", "locomotion"]).observations == "locomotion"
    with pytest.raises(SystemExit):
        trex_train.parse_args(["--observations", "everything"])
