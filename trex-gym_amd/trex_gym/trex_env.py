"""TrexBulletEnv with the reference's gym surface (trex_env.py:25-196), one env on the GPU batch.

Same constructor keywords, spaces, old-gym 4-tuple step(), python-list observations. The physics
engine behind it is the HIP kernel (C-ABI include/trex_batch.h), not pybullet. For throughput use
trex_gym.vec_env.TrexVecEnv; this single-env class exists so code written against the reference
(`trex_gym.trex_env.TrexBulletEnv(urdf_path)`) runs unmodified.
"""
import numpy as np
import torch

from . import spaces, trex_robot
from .vec_env import TrexVecEnv

NUM_SUBSTEPS = 5
FLOOR_URDF_FILENAME = 'floor.urdf'
EARTH_GRAVITATIONAL_CONSTANT = 9.81
RENDER_HEIGHT = 720
RENDER_WIDTH = 960


class TrexBulletEnv(spaces.Env):     # gym.Env where gym is importable (trex_env.py:25)
    metadata = {
        "render.modes": ["human", "rgb_array"],
        "video.frames_per_second": 50
    }

    def __init__(self, urdf_path=None, action_repeat=1, distance_weight=1.0, energy_weight=0.005,
                 drift_weight=0.002, render=False, device=None, contact_sensor=False, control_mode=None,
                 variable_stiffness=False, kp_max=1.0, terminate=None, rewards=None, command=None):
        if render:   # (the reference's render=True opens pybullet's GUI; rgb_array frames need no flag: render())
            raise NotImplementedError("render=True asks for a GUI, which this env has not; render('rgb_array') draws frames")
        self._time_step = 0.01 / NUM_SUBSTEPS
        self._urdf_path = urdf_path
        self._action_repeat = action_repeat * NUM_SUBSTEPS
        self._num_bullet_solver_iterations = 300 // NUM_SUBSTEPS
        self._observation = []
        self._env_step_counter = 0
        self._is_render = render
        self._last_base_position = [0.] * 3
        self._weight_distance = distance_weight
        self._weight_energy = energy_weight
        self._weight_drift = drift_weight
        self._action_bound = 1
        # the v1 env spells the joints 'femur_L_joint' (trex_env.py:81-87); the loader accepts both
        self._starting_configuration = {'femur_L_joint': -0.6, 'tibia_L_joint': 0.4,
                                        'tarsometatarsus_L_joint': -1.2, 'femur_R_joint': -0.6,
                                        'tibia_R_joint': 0.4, 'tarsometatarsus_R_joint': -1.2}
        self._vec = TrexVecEnv(1, urdf_path=urdf_path, device=device, action_repeat=action_repeat,
                               distance_weight=distance_weight, energy_weight=energy_weight,
                               drift_weight=drift_weight,
                               starting_configuration=self._starting_configuration, control_mode=control_mode,
                               variable_stiffness=variable_stiffness, kp_max=kp_max, terminate=terminate, rewards=rewards)
        if command is not None and self._vec.commands is None:
            raise ValueError("command: there are no reward terms to track it (rewards=[...])")
        if command is not None:   # (vx, vy, yaw rate) the tracking terms of `rewards` (trex_gym.rewards) compare the base's velocity with
            self._vec.commands[0] = torch.tensor([float(x) for x in command], device=self._vec.device)
        self._terminated = False                 # the last step ended the episode by a fall (terminate=dict(...): TrexVecEnv.set_termination)
        self.model = trex_robot.TrexRobot(self._vec, 0)
        self._ray_links = None
        self._prox_cols = None                   # getClosestPoints: (body pair -> column of the proximity table, body -> pybullet link)
        self._sensor_on = bool(contact_sensor)   # (contact_wrench(); off: the default kernels)
        if self._sensor_on:
            self._vec.enable_contact_sensor(True)
        self.np_random = None
        self.seed()
        self.reset()
        action_low, action_high = self.model.get_action_limits()
        self.action_space = spaces.Box(low=action_low, high=action_high, dtype=np.float32)
        if any(self._vec.control_modes) or self._vec.variable_stiffness:   # what the joints' modes make of an action (TrexVecEnv)
            self.action_space = self._vec.action_space
        observation_low, observation_high = self.model.get_observation_limits()
        self.observation_space = spaces.Box(low=observation_low, high=observation_high, dtype=np.float32)

    def reset(self):
        self._vec.reset_tensor()
        self._env_step_counter = 0
        self._terminated = False
        self._last_base_position = self.model.get_base_position()
        return self.model.get_observations()

    def seed(self, seed=None):
        self.np_random = np.random.RandomState(seed)  # created, never consumed (trex_env.py:124-126)
        return [seed]

    def step(self, action):
        action = np.asarray(action, dtype=np.float32).reshape(-1)
        if action.shape[0] < self._vec.A:
            raise ValueError("The action dimension is not the same as the number of motors.")
        # only the first J entries are joint targets (trex_robot.py:418-421; with variable_stiffness the next J are the
        # stiffnesses, trex_robot.py:420); the kernel clips
        a = torch.from_numpy(action[: self._vec.A].copy()).reshape(1, -1)
        self._vec.step_tensor(a)
        self._env_step_counter += 1
        self._observation = self.model.get_observations()
        info = {}
        if self._vec._term_on:   # a fall: done, with the episode's last observation (the env is already on its next episode)
            reason = int(self._vec.termination_reason[0].item())
            self._terminated = reason != 0
            if self._terminated:
                self._observation = self._vec.terminal_obs[0].cpu().numpy().astype(np.float64).tolist()
                info = {"termination": reason}
                self._env_step_counter = 0
        if self._vec.reward_terms is not None:   # rewards=[...] (trex_gym.rewards): the breakdown of this step's reward, weight x value per term
            info["reward_terms"] = dict(zip(self._vec.reward_names, self._vec.reward_terms[0].cpu().numpy().astype(np.float64).tolist()))
        return self._observation, self.compute_reward(), self.should_terminate(), info

    def render(self, mode='rgb_array', close=False):
        """'rgb_array': uint8 [720, 960, 3] from the reference's camera (distance 10, yaw 90, pitch -30, fov 60, following the
        base: trex_env.py:156-181), ray-cast from the collision hulls (trex_batch_render). 'human' returns np.array([]) as
        the reference's method does without a GUI."""
        if mode != 'rgb_array':
            return np.array([])
        from .render import Camera
        rgb = self._vec.render_tensor([0], RENDER_WIDTH, RENDER_HEIGHT, Camera())
        return rgb[0].cpu().numpy()

    def set_motor_gains(self, kp=None, kd=None, max_force=None):
        """Motor gains per joint: scalars or [J] in observation order, None = the model parameter (TrexVecEnv.set_motor_gains)."""
        self._vec.set_motor_gains(kp, kd, max_force)

    def contact_wrench(self):
        """[num_bodies, 6] numpy: the floor-contact wrench per body of the last step (force at the body's COM, torque
        about it, world axes; TrexVecEnv.contact_wrench). Construct with contact_sensor=True to record from the first
        reset; otherwise the first call switches the sensor on and reports zeros until the next step or reset."""
        if not self._sensor_on:
            self._vec.enable_contact_sensor(True)
            self._sensor_on = True
        return self._vec.contact_wrench()[0].cpu().numpy()

    # dynamics queries of the one env, as numpy (TrexVecEnv has the batched ones and their conventions)
    def inverse_dynamics(self, accel=None):
        """[6 + J] generalised force M a + h for the accelerations accel [6 + J] (None: zeros) at the current state."""
        if accel is not None:
            accel = np.asarray(accel, np.float32).reshape(1, -1)
        return self._vec.inverse_dynamics(accel)[0].cpu().numpy()

    def gravity_compensation(self):
        """[J] joint torques that hold the current state against gravity (inverse dynamics of zero accelerations)."""
        return self._vec.gravity_compensation()[0].cpu().numpy()

    def mass_matrix(self):
        """[6 + J, 6 + J] joint-space inertia matrix."""
        return self._vec.mass_matrix()[0].cpu().numpy()

    def jacobian(self, link, position=None):
        """[6, 6 + J] Jacobian of a point of a link (index or name; position in the link frame, None: its origin)."""
        return self._vec.jacobian(link, position)[0].cpu().numpy()

    def centroidal(self):
        """COM, COM velocity, momentum, angular momentum about the COM, energies and mass (vec_env.Centroidal of numpy)."""
        from .vec_env import Centroidal
        return Centroidal(self._vec.centroidal().data[0].cpu().numpy())

    def forward_dynamics(self, force=None, tau=None):
        """[6 + J] accelerations that the generalised force `force` [6 + J] (or the joint torques tau [J]; None: zeros)
        produces at the current state: the inverse of inverse_dynamics."""
        if force is not None:
            force = np.asarray(force, np.float32).reshape(1, -1)
        if tau is not None:
            tau = np.asarray(tau, np.float32).reshape(1, -1)
        return self._vec.forward_dynamics(force, tau)[0].cpu().numpy()

    def solve_mass(self, rhs=None):
        """M^-1 applied to rhs: [6 + J] -> [6 + J], [K, 6 + J] -> [K, 6 + J] row by row; None: M^-1 itself."""
        if rhs is not None:
            rhs = np.asarray(rhs, np.float32)[None]
        return self._vec.solve_mass(rhs)[0].cpu().numpy()

    def inverse_mass_matrix(self):
        """[6 + J, 6 + J] inverse of the joint-space inertia matrix."""
        return self._vec.inverse_mass_matrix()[0].cpu().numpy()

    def operational_space_inertia(self, link, position=None):
        """[6, 6] task-space inertia inv(J M^-1 J^T) of a point of a link (as jacobian())."""
        return self._vec.operational_space_inertia(link, position)[0].cpu().numpy()

    def link_state(self, probes, accel=None, axes="world", proper=False, velocity=True, acceleration=False):
        """TrexVecEnv.link_state of the one env, as a LinkState of numpy arrays: position [K, 3], orientation [K, 4] xyzw, and -
        where asked for - linear / angular velocity and acceleration [K, 3]; probes: a link, a list of links, or a handle of
        link_probes(). NOT pybullet's getLinkState tuple: its entries 0..3 are poses of the link's INERTIAL frame, and the model
        keeps no inertial frame for a link merged into its parent across a fixed joint, so they cannot be honoured. The pose here
        is the URDF link frame's (getLinkState's entries 4, 5); the velocities are those of the probe point and the link."""
        from .vec_env import LinkState
        if accel is not None:
            accel = np.asarray(accel, np.float32).reshape(1, -1)
        s = self._vec.link_state(probes, accel, axes, proper, velocity, acceleration)
        return LinkState(*[None if t is None else t[0].cpu().numpy() for t in s])

    def link_probes(self, links, positions=None):
        """A handle for points fixed in links (TrexVecEnv.link_probes), for link_state()."""
        return self._vec.link_probes(links, positions)

    def bias_acceleration(self, link, position=None):
        """[6] = Jdot qd of a point of a link (as jacobian(), in its row order)."""
        return self._vec.bias_acceleration(link, position)[0].cpu().numpy()

    # pybullet's body ids of this world: the robot and the floor (the ids are this env's own - the reference loads the floor first)
    ROBOT_ID, FLOOR_ID = 0, 1

    def _pybullet_links(self):
        """(body -> pybullet link index, pybullet link index -> URDF link): a moving body's pybullet link index is the index of the
        joint that moves it (-1: the base), its link the one whose frame is the body's"""
        m = self._vec.model
        if self._ray_links is None:
            body_link = [-1] * m.num_bodies
            for k, b in enumerate(m.array("obs_order").astype(int)):
                body_link[b] = int(m.urdf_joint_indices[k])
            own = {}
            ltf = m.array("link_tf").reshape(-1, 12)
            for l, (name, b) in enumerate(m.links()):   # the body's own link: the one whose frame is the body's
                off = np.abs(ltf[l, :9] - np.eye(3).reshape(-1)).sum() + np.abs(ltf[l, 9:]).sum()
                if b not in own or off < own[b][0]:
                    own[b] = (off, l)
            self._ray_links = (body_link, {body_link[b]: own[b][1] for b in own})
        return self._ray_links

    def calculateInverseKinematics2(self, endEffectorLinkIndices, targetPositions, targetOrientations=None, maxNumIterations=20):
        """pybullet's calculateInverseKinematics2: joint angles, as a list of J floats in pybullet's joint order (ascending joint
        index), that bring the origins of the links endEffectorLinkIndices (pybullet link indices of moving links, at most 8) to
        targetPositions (world) - and, where given, their frames to targetOrientations (xyzw) - from the current joint angles,
        with the base where it is. All targets are solved together by damped least squares (TrexVecEnv.inverse_kinematics,
        include/trex_batch.h): no null-space or rest-pose terms, no per-joint damping, joint limits by clamping."""
        _, link_of = self._pybullet_links()
        idx = [int(i) for i in endEffectorLinkIndices]
        for i in idx:
            if i == -1 or i not in link_of:
                raise ValueError("endEffectorLinkIndex %r is not a moving link of the robot" % (i,))
        pos = np.asarray(targetPositions, np.float32).reshape(len(idx), 3)
        ori = None if targetOrientations is None else np.asarray(targetOrientations, np.float32).reshape(len(idx), 4)
        probes = self._vec.link_probes([link_of[i] for i in idx])
        try:
            q, _ = self._vec.inverse_kinematics(probes, pos, ori, iterations=int(maxNumIterations))
            q = q[0].cpu().numpy().astype(np.float64)
        finally:
            probes.close()
        return [float(q[k]) for k in np.argsort(self._vec.model.urdf_joint_indices, kind="stable")]

    def calculateInverseKinematics(self, endEffectorLinkIndex, targetPosition, targetOrientation=None, maxNumIterations=20):
        """pybullet's calculateInverseKinematics: calculateInverseKinematics2 of the one link."""
        return self.calculateInverseKinematics2([endEffectorLinkIndex], [targetPosition],
                                                None if targetOrientation is None else [targetOrientation], maxNumIterations)

    def rayTestBatch(self, rayFromPositions, rayToPositions, parentLinkIndex=-1):
        """pybullet's rayTestBatch: one (objectUniqueId, linkIndex, hitFraction, hitPosition, hitNormal) per ray. The rays are in
        world coordinates, or - parentLinkIndex >= 0, pybullet's joint / link index - in the frame of that link. objectUniqueId:
        ROBOT_ID, FLOOR_ID, or -1 on a miss (then linkIndex -1, hitFraction 1.0, zeros); linkIndex: the pybullet index of the
        hit body's own link, -1 for the base. Cast against the collision hulls, not the visual meshes; a shape that contains a
        ray's origin is not hit by it (TrexVecEnv.ray_test, include/trex_batch.h)."""
        frm = np.asarray(rayFromPositions, np.float32).reshape(-1, 3)
        to = np.asarray(rayToPositions, np.float32).reshape(-1, 3)
        if frm.shape != to.shape:
            raise ValueError("rayFromPositions and rayToPositions differ in length")
        if len(frm) == 0:
            return []
        body_link, link_of = self._pybullet_links()
        if parentLinkIndex not in link_of:
            raise ValueError("parentLinkIndex %r is not a link of the robot (-1: world frame)" % (parentLinkIndex,))
        link = None if parentLinkIndex == -1 else link_of[parentLinkIndex]
        rays = torch.from_numpy(np.concatenate([frm, to], 1))
        frac, body, pos, nrm = [x[0].cpu().numpy() for x in self._vec.ray_test(rays, link, positions=True, normals=True)]
        out = []
        for k in range(len(frm)):
            b = int(body[k])
            if b == -2:
                out.append((-1, -1, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
            else:
                out.append((self.FLOOR_ID if b == -1 else self.ROBOT_ID, -1 if b == -1 else body_link[b], float(frac[k]),
                            tuple(float(x) for x in pos[k]), tuple(float(x) for x in nrm[k])))
        return out

    def rayTest(self, rayFromPosition, rayToPosition):
        """pybullet's rayTest: rayTestBatch of the one ray (a list of one tuple)."""
        return self.rayTestBatch([rayFromPosition], [rayToPosition])

    def getClosestPoints(self, bodyA, bodyB):
        """pybullet's getClosestPoints between two bodies of the robot, bodyA and bodyB being body indices of the model (the
        indices of TrexVecEnv.proximity_shapes' pairs; every moving link of the URDF is one): a list of one tuple in pybullet's
        layout - (contactFlag 0, ROBOT_ID, ROBOT_ID, linkIndexA, linkIndexB, positionOnA, positionOnB, contactNormalOnB,
        contactDistance, normalForce 0.0) - or [] when one of the two carries no collision geometry. The link indices are
        pybullet's (-1: the base). No distance threshold: the pair is always reported. Capsules fitted to the hulls, not the
        hulls (TrexVecEnv.closest_points, include/trex_batch.h). The first call sets the env's proximity table to ALL body pairs."""
        m = self._vec.model
        if self._prox_cols is None:
            shapes = self._vec.proximity_shapes(exclude_adjacent=False, exclude_start_overlaps=False)
            body_link = [-1] * m.num_bodies
            for k, b in enumerate(m.array("obs_order").astype(int)):
                body_link[b] = int(m.urdf_joint_indices[k])
            self._prox_cols = ({(int(a), int(b)): k for k, (a, b) in enumerate(shapes.pairs)}, body_link)
        cols, body_link = self._prox_cols
        A, B = int(bodyA), int(bodyB)
        for x in (A, B):
            if not 0 <= x < m.num_bodies:
                raise IndexError("body index %d out of range [0, %d)" % (x, m.num_bodies))
        if A == B:
            raise ValueError("getClosestPoints: bodyA and bodyB are the same body")
        swap = (A, B) not in cols
        if swap and (B, A) not in cols:
            return []
        k = cols[(B, A)] if swap else cols[(A, B)]
        r = self._vec.closest_points(points=True)
        d, pa, pb, n = (x[0, k].cpu().numpy() for x in (r.distance, r.point_a, r.point_b, r.normal))
        if swap:   # the table holds (B, A): the same two points, the normal turned round
            pa, pb, n = pb, pa, -n
        return [(0, self.ROBOT_ID, self.ROBOT_ID, body_link[A], body_link[B], tuple(float(x) for x in pa),
                 tuple(float(x) for x in pb), tuple(float(x) for x in n), float(d), 0.0)]

    def body_clearance(self, link=None):
        """Height of the lowest collision point above the floor (TrexVecEnv.body_clearance), numpy: [num_bodies] for every body,
        or the float of the body of `link` (name or index)."""
        c = self._vec.body_clearance(link)[0].cpu().numpy()
        return c if link is None else float(c)

    def should_terminate(self):
        # constant False in the reference (trex_env.py:183-184), and here unless the env was made with terminate=dict(...):
        # then whether the last step ended the episode by a fall
        return self._terminated

    def compute_reward(self):
        # computed inside the step kernel (trex_env.py:186-196); penalties = the three logged values
        self._last_penalties = dict(zip(("penalty_lifting_com", "penalty_station_keeping", "penalty_energy"),
                                        self._vec.penalties[0].cpu().numpy().astype(np.float64).tolist()))
        return float(self._vec.rew[0].item())

    def close(self):
        self._vec.close()
