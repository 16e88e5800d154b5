"""Robot adapter with the surface of the reference's trex_robot.TrexRobot (trex_robot.py:256-433),
backed by one env of a GPU batch instead of a pybullet body. Only what the env and the training
script read is kept: get_action_limits / get_observation_limits / get_observations /
get_head_position / get_base_position / get_total_joint_power, `_revolute_joint_indices`,
`_total_mass`, `_head_link_index` (trex_train.py:121-123, trex_env.py:93-96,153,187-190) - and
get_joint_state / get_joint_states (trex_robot.py:120-150), whose jointReactionForces the joint
force/torque sensor supplies (trex_gym.joint_sensor)."""
import numpy as np
import torch


class TrexRobot:
    _MAX_JOINT_TORQUE_IN_NM = 300000.0  # trex_robot.py:260

    def __init__(self, vec_env, index=0):
        self._vec = vec_env
        self._index = index
        m = vec_env.model
        # pybullet joint indices of the revolute joints, sorted by joint name (trex_robot.py:311-314)
        self._revolute_joint_indices = list(m.urdf_joint_indices)
        # trex_robot.py:318-320 sums getDynamicsInfo over links 0..n-1, which skips the base link
        self._total_mass = m.total_mass(include_base_link=False)
        self._head_link_index = None  # resolved on the host at model load; kept for attribute parity
        self._starting_configuration = {}

    def _joint_limits(self):
        m = self._vec.model
        return list(m.lower), list(m.upper)

    def get_action_limits(self):
        lo, hi = self._joint_limits()
        return np.array(lo), np.array(hi)

    def get_observation_limits(self):
        lo, hi = self._joint_limits()
        n = len(lo)
        lo.extend([-1.0e12] * 2 * n)
        hi.extend([1.0e12] * 2 * n)
        return np.array(lo), np.array(hi)

    def get_observations(self):
        return self._vec.obs[self._index].cpu().numpy().astype(np.float64).tolist()

    def get_base_position(self):
        return tuple(self._vec.get_state()[self._index, :3].cpu().numpy().astype(np.float64).tolist())

    def get_head_position(self):
        return tuple(self._vec.head_position()[self._index].cpu().numpy().astype(np.float64).tolist())

    def _get_joint_state_names(self):
        return ["jointPosition", "jointVelocity", "jointReactionForces", "appliedJointMotorTorque"]   # trex_robot.py:120-126

    def _joint_slot(self, joint_index):
        """pybullet joint index -> the joint's place in the observation order; ValueError for any other index"""
        try:
            return self._revolute_joint_indices.index(int(joint_index))
        except ValueError:
            if 0 <= int(joint_index) < self._vec.model.num_urdf_joints:
                raise ValueError("joint index %d is a fixed joint: its link is merged into its parent's body and has no joint state"
                                 % joint_index) from None
            raise ValueError("joint index %d outside [0, %d)" % (joint_index, self._vec.model.num_urdf_joints)) from None

    def get_joint_states(self, joint_index_list):
        """pybullet's getJointStates (trex_robot.py:140-150): {name: [value per joint]} for pybullet joint indices. position,
        velocity and the applied motor torque are the observation's three blocks; jointReactionForces is the 6-tuple of the joint
        force/torque sensor (trex_gym.joint_sensor.attach: force, then moment about the joint origin, child link axes) and zeros
        without one, as pybullet gives with no sensor enabled. Sign and frame parity with pybullet is unpinned."""
        slots = [self._joint_slot(j) for j in joint_index_list]
        J = self._vec.J
        o = self._vec.obs[self._index].cpu().numpy().astype(np.float64)
        r = self._vec.joint_reaction
        r = np.zeros((J, 6)) if r is None else r[self._index].cpu().numpy().astype(np.float64)
        cols = [[float(o[s]) for s in slots], [float(o[J + s]) for s in slots], [tuple(r[s].tolist()) for s in slots],
                [float(o[2 * J + s]) for s in slots]]
        return dict(zip(self._get_joint_state_names(), cols))

    def get_joint_state(self, joint_index):
        """pybullet's getJointState (trex_robot.py:128-138): {name: value} of one joint."""
        return {k: v[0] for k, v in self.get_joint_states([joint_index]).items()}

    def get_total_joint_power(self):
        o = self._vec.obs[self._index]
        J = self._vec.J
        return float(torch.sum(torch.abs(o[J:2 * J] * o[2 * J:])).item())

    def reset(self, reload_urdf=False):
        self._vec.reset_tensor()
