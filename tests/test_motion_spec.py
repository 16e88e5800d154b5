"""trex_gym.motion without a GPU: clips to and from files, from state rows and from keyframes (the host resampling against the
reference's interpolation), the term constructors, the preset and what a checkpoint stores."""
import numpy as np
import pytest

import motion_cases as MC
import motion_ref as MR

J = 25


def test_clip_files_and_keyframes(tmp_path, model):
    from trex_gym import motion as M
    frames = MC.clip_frames(model, 9, seed=2)
    clip = M.Clip(frames, MC.DT, loop=True)
    path = str(tmp_path / "clip.npz")
    clip.save(path)
    back = M.Clip.load(path)
    assert (back.frames == frames).all() and back.frame_dt == MC.DT and back.loop and back.velocities is None
    assert back.num_frames == 9 and back.num_joints == J and back.duration == 0.25
    key = M.Clip.from_keyframes([0.0, 0.25], frames[[0, 8]], MC.DT)
    tab = MR.device_table(MR.build_table(model, frames[[0, 8]], None, 0.25, False))
    assert key.num_frames == 9
    for k in range(9):
        assert np.abs(key.frames[k, [0, 1, 2] + list(range(7, 7 + J))] - MR.sample(tab, k * MC.DT)[0][[0, 1, 2] + list(range(13, 13 + J))]).max() < 1e-6
        assert abs(abs(key.frames[k, 3:7] @ MR.sample(tab, k * MC.DT)[0][3:7]) - 1) < 1e-6
    spec = M.imitation(None)
    assert M.from_tuples(M.as_tuples(spec)) == spec and [t.weight for t in spec] == [0.65, 0.1, 0.15, 0.1]
    assert [t.scale for t in spec] == [2.0, 0.1, 40.0, 10.0]


def test_constructors_names_and_refusals(model):
    from trex_gym import motion as M
    spec = M.pose(1.0, joints=["tail_joint_that_is_not_resolved_here", 3]) + M.pose(0.5) + M.end_effector() + M.root_velocity(1.0, 2.0, 0.5)
    assert M.names(spec) == ["motion/pose", "motion/pose#2", "motion/end_effector", "motion/root_velocity"]
    out, effectors = M.resolve(spec[1:], int)
    assert effectors and out == [(0, 0, 0.5, 2.0, 0.0), (2, 0, 1.0, 40.0, 0.0), (4, 0, 1.0, 2.0, 0.5)]
    assert M.resolve(M.velocity(1.0, 0.1, joints=[0, 24]), int)[0][0][1] == 1 | 1 << 24
    for bad in (lambda: M.pose(1.0, 0.0), lambda: M.root_pose(1.0, 1.0, -1.0), lambda: M.velocity(float("nan")),
                lambda: M.resolve(M.pose() * 9, int), lambda: M.resolve([M.Term("no_such_kind", None, 1.0, 1.0, 0.0)], int),
                lambda: M.Clip(np.zeros((1, 7 + J)), 0.1), lambda: M.Clip(np.zeros((3, 7 + J)), 0.0),
                lambda: M.Clip(np.zeros((3, 7 + J)), 0.1, velocities=np.zeros((3, 5)))):
        with pytest.raises(ValueError):
            bad()
    s = np.arange(3 * (13 + 2 * J), dtype=np.float64).reshape(3, -1)
    c = M.Clip.from_states(s, 0.02)
    assert (c.frames[:, :7] == s[:, :7]).all() and (c.frames[:, 7:] == s[:, 13:13 + J]).all()
    assert (c.velocities[:, :6] == s[:, 7:13]).all() and (c.velocities[:, 6:] == s[:, 13 + J:]).all()
    c = M.Clip.from_states(s, 0.02, limits=(np.full(J, 20.0), np.full(J, 100.0)))
    assert c.frames[:, 7:].min() == 20.0 and c.frames[:, 7:].max() == 100.0
