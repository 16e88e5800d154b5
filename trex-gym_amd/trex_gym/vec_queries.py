"""The read-only half of TrexVecEnv: the calls that only READ the batch's state - rendering, kinematics, dynamics, contact and
proximity queries, inverse kinematics, ray casts, what the fall predicate left - and the setters of tables that only such calls
read (probe sets, proximity shapes). The same cut as capi_queries.cpp against capi.cpp on the host side: nothing here changes
what a step or reset launch does, and nothing the step path of vec_env.py runs per step lives here but termination_reason.

VecQueries is a mixin without a constructor: TrexVecEnv inherits from it and calls _init_queries() once. It uses the env's
device, batch, model, num_envs, J and _dev().
"""
import collections

import numpy as np
import torch

from . import _capi
from .perturb import LinkTable, contact_flags, link_contact_forces
from .render import RENDER_HEIGHT, RENDER_WIDTH, Camera, tile_images


class Centroidal:
    """Named view of the [n, 16] block of trex_batch_centroidal (include/trex_batch.h); numpy or torch alike."""

    def __init__(self, data):
        self.data = data
        self.com, self.com_velocity = data[..., 0:3], data[..., 3:6]
        self.momentum, self.angular_momentum = data[..., 6:9], data[..., 9:12]
        self.kinetic, self.potential, self.mass = data[..., 12], data[..., 13], data[..., 14]


LinkState = collections.namedtuple("LinkState", "position orientation linear_velocity angular_velocity linear_acceleration "
                                                "angular_acceleration")
AXES = {"world": 0, "link": 1, "base": 2}
IkInfo = collections.namedtuple("IkInfo", "position_error orientation_error iterations initial_error")
ProximityShapes = collections.namedtuple("ProximityShapes", "bodies capsules pairs")
ClosestPoints = collections.namedtuple("ClosestPoints", "distance point_a point_b normal capsule")


class LinkProbes:
    """A set of points fixed in URDF links, held on the device by a TrexVecEnv (TrexVecEnv.link_probes): what link_state()
    evaluates in one launch. links: the link indices [K]; positions: [K, 3] in the link frames. close() gives the env's set slot
    back (an env holds 8)."""

    def __init__(self, env, slot, links, positions):
        self.env, self.slot = env, slot
        self.links, self.positions = links, positions
        self.num_probes = len(links)

    def close(self):
        if self.slot is not None:
            self.env._release_probes(self)
            self.slot = None

    def __len__(self):
        return self.num_probes


class VecQueries:
    def _init_queries(self):
        self._link_table = None                 # trex_gym.perturb.LinkTable of the model, made on first use (_links)
        self._probe_sets = [None] * 8           # the LinkProbes handle in each of the batch's probe-set slots
        self._probe_cache = (None, None)        # (key, handle): the one-off set of the last links given to a query directly
        self._out_bufs = {}                     # query name -> (shape key, output buffers) of its last call (_buffers)
        self._prox = None                       # the ProximityShapes in force

    @property
    def _links(self):
        """the model's LinkTable: link names -> indices -> bodies"""
        if self._link_table is None:
            self._link_table = LinkTable.from_model(self.model)
        return self._link_table

    def _one_off_probes(self, key, make):
        """The LinkProbes handle make() of a query that was given links instead of a handle: kept until another key comes, then
        closed - the one-off sets of link_state() and bias_acceleration() take ONE of the env's 8 slots between them."""
        if self._probe_cache[0] != key:
            if self._probe_cache[1] is not None:
                self._probe_cache[1].close()
            self._probe_cache = (key, make())
        return self._probe_cache[1]

    def _buffers(self, query, key, make):
        """The output buffers make() of `query` for the shapes `key`, kept until the key changes: ONE key per query - a caller
        that sweeps a size does not pile up device memory (the old set is let go before the new one is made)."""
        if self._out_bufs.get(query, (None, None))[0] != key:
            self._out_bufs[query] = (None, None)
            self._out_bufs[query] = (key, make())
        return self._out_bufs[query][1]

    # ---- rendering (trex_batch_render: a ray caster over the collision hulls, include/trex_batch.h)
    def render_tensor(self, env_ids=None, width=84, height=84, camera=None, depth=False, segmentation=False):
        """Pixel observations on the device: rgb [V, H, W, 3] uint8 of the envs env_ids (host sequence, None = all n), plus
        depth [V, H, W] float32 (linear eye-space metres) and / or seg [V, H, W] int32 (body index, -1 floor, -2 nothing)
        when asked - then a tuple (rgb, depth?, seg?). camera: trex_gym.render.Camera (default: the reference's, following
        each env's base). One launch, stream-ordered, no host sync; the state is only read."""
        camera = Camera() if camera is None else camera
        V = self.num_envs if env_ids is None else len(env_ids)
        rgb = torch.empty(V, height, width, 3, dtype=torch.uint8, device=self.device)
        dep = torch.empty(V, height, width, dtype=torch.float32, device=self.device) if depth else None
        seg = torch.empty(V, height, width, dtype=torch.int32, device=self.device) if segmentation else None
        self.batch.render(camera, width, height, env_ids, rgb, dep, seg)
        if not depth and not segmentation:
            return rgb
        return (rgb,) + ((dep,) if depth else ()) + ((seg,) if segmentation else ())

    def get_images(self, width=None, height=None, camera=None, env_ids=None):
        """baselines' VecEnv.get_images: a list of H x W x 3 uint8 numpy frames, one per env (default 720 x 960, the
        reference's frame size: mind the memory for large batches - render_tensor keeps them on the device)."""
        rgb = self.render_tensor(env_ids, width or RENDER_WIDTH, height or RENDER_HEIGHT, camera)
        return list(rgb.cpu().numpy())

    def render(self, mode="rgb_array"):
        """'rgb_array': ONE near-square tile (baselines' tile_images) of the first min(n, 16) envs at 720 x 960 each - not
        of all n: 4 096 full frames would be 8 GB. 'human' raises NotImplementedError (no display)."""
        if mode == "human":
            raise NotImplementedError("render('human'): there is no display; use 'rgb_array' or render_tensor()")
        if mode != "rgb_array":
            raise ValueError("render mode must be 'rgb_array' or 'human'")
        return tile_images(np.stack(self.get_images(env_ids=list(range(min(self.num_envs, 16))))))

    # ---- poses
    def head_position(self):
        out = torch.zeros(self.num_envs, 3, device=self.device)
        self.batch.head_position(out)
        return out

    def link_transforms(self):
        """World pose of every URDF link frame, [n, L, 7] = xyz + quaternion xyzw (rollout export for
        rendering, the step after the path: trex_env.py:156-181)."""
        L = len(self.model.links())
        out = torch.empty(self.num_envs, L, 7, device=self.device)
        self.batch.link_transforms(out)
        return out

    def visual_transforms(self):
        """World pose of every <visual> mesh of the URDF, [n, V, 7] = xyz + quaternion xyzw (252 meshes for trex.urdf;
        `model.visuals()` names them): what a renderer places the meshes with - the table pybullet keeps for
        getCameraImage (trex_env.py:164-176)."""
        V = len(self.model.visuals())
        out = torch.empty(self.num_envs, V, 7, device=self.device)
        self.batch.visual_transforms(out)
        return out

    # ---- contact sensor readings (trex_batch_contact_wrench; enable_contact_sensor() switches the recording on; no host sync)
    def contact_wrench(self, out=None):
        """[n, num_bodies, 6] on the device: floor-contact force at each body's COM and torque about it, world axes (N, N m),
        the mean over the substeps of the last step (a reset env: its settle substep; a contained env: zeros)."""
        return self.batch.contact_wrench(out)

    def contact_forces(self, links):
        """[n, K, 3] floor-contact force on URDF links: links = K entries, each a link name / index or a list of them (the
        force summed over their distinct bodies), e.g. contact_forces(["foot_L", "foot_R"])."""
        return link_contact_forces(self._links, self.contact_wrench(), links)

    def in_contact(self, threshold=0.0):
        """[n, num_bodies] bool: the floor pushes the body with more than `threshold` N (normal force)."""
        return contact_flags(self.contact_wrench(), threshold)

    # ---- dynamics queries (trex_batch_inverse_dynamics / _mass_matrix / _jacobian / _centroidal / _forward_dynamics /
    # _solve_mass; no host sync)
    # Generalised velocity [D = 6 + J]: base linear v(3), base angular w(3), world axes, then qd in observation order - the
    # velocity part of get_state(); forces are its duals (base force, base torque about the base origin, joint torques).
    def inverse_dynamics(self, accel=None, out=None):
        """[n, D] generalised force M(q) a + h(q, qd) for the accelerations accel [n, D] (None: zeros) at the current state.
        Rigid-body terms only: no joint damping, link damping, motors, limits or contacts (pybullet's calculateInverseDynamics)."""
        if accel is not None:
            accel = self._dev(torch.as_tensor(accel))
        return self.batch.inverse_dynamics(accel, out)

    def gravity_compensation(self):
        """[n, J] joint torques of inverse_dynamics() with zero accelerations: what holds the joints against gravity (and the
        velocity-product terms of a moving state), ready to add to the actions of TORQUE-mode joints."""
        return self.batch.inverse_dynamics(None, None)[:, 6:]

    def mass_matrix(self, out=None):
        """[n, D, D] joint-space inertia matrix M(q), symmetric (pybullet's calculateMassMatrix)."""
        return self.batch.mass_matrix(out)

    def jacobian(self, link, position=None, out=None):
        """[n, 6, D] Jacobian of the point `position` (link frame; None: the link origin) of link `link` (index or name):
        rows 0..2 its world linear velocity, rows 3..5 the link's world angular velocity (pybullet's calculateJacobian)."""
        return self.batch.jacobian(self._links.index(link), position, out)

    def centroidal(self, out=None):
        """Whole-body quantities as a Centroidal of device tensors: com [n, 3], com_velocity, momentum, angular_momentum (about
        the COM), kinetic [n], potential (sum m g z), mass (the env's mass scale included); `.data` is the [n, 16] block."""
        return Centroidal(self.batch.centroidal(out))

    def forward_dynamics(self, force=None, tau=None, out=None):
        """[n, D] accelerations M(q)^-1 (force - h(q, qd)) that the generalised force `force` [n, D] produces at the current
        state (None: zeros - free motion under gravity): the inverse of inverse_dynamics, rigid-body terms only. tau [n, J] is
        shorthand for a force with a zero base block; giving both is an error."""
        if force is not None and tau is not None:
            raise ValueError("forward_dynamics: give force or tau, not both")
        if tau is not None:
            tau = torch.as_tensor(tau).to(device=self.device, dtype=torch.float32)
            force = torch.cat([torch.zeros(tau.shape[0], 6, dtype=torch.float32, device=self.device), tau], 1)
        elif force is not None:
            force = self._dev(torch.as_tensor(force))
        return self.batch.forward_dynamics(force, out)

    def solve_mass(self, rhs=None, out=None):
        """[n, K, D] = M(q)^-1 applied to the K force-like rows rhs[e, k, :] of every env, K <= 64 ([n, D]: one row, returns
        [n, D]); None: the identity, M^-1 itself. solve_mass(jacobian(link)) is (M^-1 J^T)^T. Depends on q alone."""
        if rhs is not None:
            rhs = self._dev(torch.as_tensor(rhs))
        return self.batch.solve_mass(rhs, out)

    def inverse_mass_matrix(self, out=None):
        """[n, D, D] M(q)^-1 (symmetric up to rounding)."""
        return self.batch.solve_mass(None, out)

    def operational_space_inertia(self, link, position=None):
        """[n, 6, 6] task-space inertia inv(J M^-1 J^T) of the point `position` of link `link` (as jacobian()): one Jacobian
        launch, one solve launch and a batched 6 x 6 inverse."""
        Jm = self.jacobian(link, position)
        return torch.linalg.inv(Jm @ self.batch.solve_mass(Jm).transpose(1, 2))

    # ---- link kinematics (trex_batch_set_link_probes / trex_batch_link_state; one launch for all probes, no host sync)
    def link_probes(self, links, positions=None):
        """A LinkProbes handle for the points `positions` [K, 3] (link frames; None: the link origins) of the links `links` (K
        names or indices, or one). It takes one of the env's 8 probe-set slots until its close(); RuntimeError when none is free."""
        if isinstance(links, (str, int, np.integer)):
            links = [links]
            if positions is not None:
                positions = np.asarray(positions, np.float64).reshape(1, 3)
        idx = [self._links.index(l) for l in links]
        pos = np.zeros((len(idx), 3)) if positions is None else np.asarray(positions, np.float64)
        if pos.shape != (len(idx), 3):
            raise ValueError("positions must have shape (%d, 3), got %s" % (len(idx), pos.shape))
        if not idx:
            raise ValueError("link_probes: no link given")
        free = [k for k, h in enumerate(self._probe_sets) if h is None]
        if not free:
            raise RuntimeError("link_probes: all %d probe sets of this env are in use; close() one first" % len(self._probe_sets))
        self.batch.set_link_probes(free[0], idx, pos)
        h = LinkProbes(self, free[0], idx, pos)
        self._probe_sets[free[0]] = h
        return h

    def _release_probes(self, h):
        if self._probe_sets[h.slot] is h:
            self.batch.set_link_probes(h.slot, [])
            self._probe_sets[h.slot] = None
        if self._probe_cache[1] is h:
            self._probe_cache = (None, None)

    def link_state(self, probes, accel=None, axes="world", proper=False, velocity=True, acceleration=False):
        """Kinematics of the K probes of `probes` - a LinkProbes handle, or a link / a list of links (their origins; kept as a
        one-off set until other links are given) - at the current state, as a LinkState of device tensors:
        position [n, K, 3] of the points and orientation [n, K, 4] (xyzw, w >= 0) of their link frames; with `velocity`
        linear_velocity of the points and angular_velocity of the links; with `acceleration` linear_acceleration (classical,
        d2p/dt2) and angular_acceleration at the generalised accelerations accel [n, D] (None: zeros - the bias acceleration
        Jdot qd). Parts not asked for are None.
        axes: "world", "link" (each probe's own link frame) or "base" (URDF link 0's frame): the axes the velocities and
        accelerations - still relative to the world - are expressed in; with "base" the pose is relative to that frame too.
        proper: + g z (world) on the linear acceleration: the specific force an accelerometer at the point reads."""
        if axes not in AXES:
            raise ValueError("axes must be one of %s" % sorted(AXES))
        if not isinstance(probes, LinkProbes):
            key = tuple(probes) if isinstance(probes, (list, tuple)) else (probes,)
            probes = self._one_off_probes(key, lambda: self.link_probes(list(key)))
        if probes.env is not self or probes.slot is None:
            raise ValueError("link_state: the probes are closed or belong to another env")
        n, K = self.num_envs, probes.num_probes
        if accel is not None:
            accel = self._dev(torch.as_tensor(accel))
        pose = torch.empty(n, K, 7, device=self.device)
        vel = torch.empty(n, K, 6, device=self.device) if velocity else None
        acc = torch.empty(n, K, 6, device=self.device) if acceleration else None
        self.batch.link_state(probes.slot, AXES[axes], proper, accel, pose, vel, acc, probes=K)
        return LinkState(pose[..., :3], pose[..., 3:], None if vel is None else vel[..., :3], None if vel is None else vel[..., 3:],
                         None if acc is None else acc[..., :3], None if acc is None else acc[..., 3:])

    def bias_acceleration(self, link, position=None):
        """[n, 6] = Jdot qd of the point `position` of link `link` (as jacobian(), and in its row order: linear, angular; world
        axes): the point's acceleration at zero generalised accelerations - with operational_space_inertia(), jacobian() and
        inverse_dynamics() what a task-space controller needs."""
        key = ("bias", link, None if position is None else tuple(float(x) for x in position))
        h = self._one_off_probes(key, lambda: self.link_probes(link, position))
        acc = torch.empty(self.num_envs, 1, 6, device=self.device)
        self.batch.link_state(h.slot, 0, False, None, None, None, acc, probes=1)
        return acc[:, 0]

    # ---- inverse kinematics (trex_batch_inverse_kinematics: pybullet's calculateInverseKinematics; one launch for every env, all
    # targets and all iterations, no host sync)
    def inverse_kinematics(self, probes, positions=None, orientations=None, frame="world", q_init=None, joints=None,
                           iterations=20, damping=0.01, gain=0.1, max_step=0.2, tol=(0.0, 0.0)):
        """Joint angles that bring the K <= 8 probes of `probes` (a LinkProbes of link_probes()) to per-env targets, by damped
        least squares at the envs' current base poses: (q [n, J] in observation order, IkInfo of device tensors).
        positions [n, K, 3] (or [K, 3], every env alike): where the probe points are to be; orientations [n, K, 4] (xyzw): the
        orientations of their link frames; either may be None, and a row with a NaN in it means "not constrained" - rows are
        read on the host once to find them, so every env constrains the same parts. frame: "world", or "base": targets relative
        to URDF link 0's frame, as link_state(axes="base") reports poses. q_init [n, J]: where the solve starts (None: the
        current joint angles). joints: the names or observation indices of the joints that may move (None: all); the others
        come back as they went in. tol = (metres, radians): stop an env early once both residuals are at or below them.
        info: position_error [n] and orientation_error [n] (the largest residuals at q), iterations [n], initial_error [n]
        (the norm of the stacked error at the start). step(joint_targets_to_actions(q)) commands the result."""
        if frame not in ("world", "base"):
            raise ValueError("frame must be 'world' or 'base'")
        if not isinstance(probes, LinkProbes) or probes.env is not self or probes.slot is None:
            raise ValueError("inverse_kinematics: probes must be an open LinkProbes of this env")
        n, J, K = self.num_envs, self.J, probes.num_probes
        if positions is None and orientations is None:
            raise ValueError("inverse_kinematics: give positions, orientations or both")

        def rows(t, width, what):
            if t is None:
                return None, np.zeros(K, bool)
            t = torch.as_tensor(t, dtype=torch.float32)
            if t.dim() == 2:
                t = t.unsqueeze(0).expand(n, K, width)
            if tuple(t.shape) != (n, K, width):
                raise ValueError("%s must have shape (%d, %d, %d) or (%d, %d), got %s" % (what, n, K, width, K, width, tuple(t.shape)))
            t = t.to(self.device)
            return t, (~torch.isnan(t).any(2).any(0)).cpu().numpy()

        pos, has_p = rows(positions, 3, "positions")
        ori, has_o = rows(orientations, 4, "orientations")
        modes = has_p * 1 + has_o * 2
        if (modes == 0).any():
            raise ValueError("inverse_kinematics: probe %d is not constrained at all" % int(np.argmin(modes)))
        target = torch.zeros(n, K, 7, device=self.device)
        target[..., 6] = 1.0
        if pos is not None:
            target[..., :3] = pos
        if ori is not None:
            target[..., 3:] = ori
        if joints is None:
            mask = (1 << J) - 1
        else:
            names = self.model.joint_names
            mask = 0
            for j in ([joints] if isinstance(joints, (str, int, np.integer)) else joints):
                k = names.index(j) if isinstance(j, str) else int(j)
                if not 0 <= k < J:
                    raise IndexError("joint index %d out of range [0, %d)" % (k, J))
                mask |= 1 << k
        if q_init is not None:
            q_init = torch.as_tensor(q_init, dtype=torch.float32).to(self.device).expand(n, J).contiguous()
        q, info = torch.empty(n, J, device=self.device), torch.empty(n, 4, device=self.device)
        self.batch.inverse_kinematics(probes.slot, modes, target.contiguous(), q, AXES[frame], q_init, mask, info, iterations, damping,
                                      gain, max_step, tol[0], tol[1])
        return q, IkInfo(info[:, 0], info[:, 1], info[:, 2].to(torch.int32), info[:, 3])

    def joint_targets_to_actions(self, q):
        """Action rows [n, A] that command the joint angles q [n, J] (observation order; e.g. inverse_kinematics()' result): the
        inverse of the env's action scaling. A POSITION-mode joint's action IS its target angle, clipped by the step to the
        joint's limits as it is here; a VELOCITY- or TORQUE-mode joint has no position target: its column is 0. With stiffness
        actions the J stiffness columns carry the model's motor_kp, clipped to kp_max."""
        q = torch.as_tensor(q, dtype=torch.float32).to(self.device)
        lo = torch.as_tensor(self.model.lower.astype(np.float32), device=self.device)
        hi = torch.as_tensor(self.model.upper.astype(np.float32), device=self.device)
        position = torch.as_tensor(np.asarray(self.control_modes) == 0, device=self.device)
        a = torch.where(position, torch.minimum(torch.maximum(q, lo), hi), torch.zeros_like(q))
        if self.variable_stiffness:
            kp = min(float(self.model.get_param("motor_kp")), self.kp_max)
            a = torch.cat([a, torch.full_like(a, kp)], -1)
        return a

    # ---- proximity between bodies (trex_batch_set_proximity_shapes / trex_batch_proximity: pybullet's getClosestPoints between
    # links of the robot; one launch for all pairs, no host sync)
    def proximity_shapes(self, capsules=None, pairs=None, max_radius=0.2, max_divisions=3, min_points=4, exclude_adjacent=True,
                         exclude_start_overlaps=True):
        """Set the env's proximity table and return what it holds, as ProximityShapes(bodies [C], capsules [C, 7], pairs [P, 2]).
        capsules: (bodies [C], [C, 7] = p0 xyz, p1 xyz, radius in the body frames); None: every convex hull fitted with
        Model.fit_hull_primitives(max_radius, max_divisions, min_points) - or, with collision="primitives", the model's spheres
        as capsules of length 0: what the physics collides with (the cylinder between a capsule's ends is absent there too).
        pairs: [P, 2] body pairs (A, B); None: all pairs of bodies with geometry, minus parent-child pairs (exclude_adjacent),
        minus the pairs that already overlap at the start pose (exclude_start_overlaps; found with one query on a reset batch of
        one env). capsules=() frees the table."""
        m = self.model
        if capsules is None:
            hs = m.array("hull_start").astype(int)
            if self.collision == "primitives":
                xyz, rad = m.array("hull_xyz").reshape(-1, 3), m.array("hull_radius")
                bodies = np.repeat(np.arange(m.num_bodies), np.diff(hs)).astype(np.int32)
                caps = np.concatenate([xyz, xyz, rad[:, None]], 1)
            else:
                gs = m.array("hull_group_start").astype(int)
                bodies, caps = [], []
                for b in range(m.num_bodies):
                    for g in range(len(gs) - 1):
                        if hs[b] <= gs[g] < hs[b + 1] and gs[g + 1] > gs[g]:
                            for p0, p1, r in m.fit_hull_primitives(g, max_radius, max_divisions, min_points):
                                bodies.append(b)
                                caps.append(np.concatenate([p0, p1, [r]]))
                bodies, caps = np.array(bodies, np.int32), np.array(caps, np.float64).reshape(-1, 7)
        else:
            bodies, caps = capsules if len(capsules) else ((), ())
            bodies, caps = np.asarray(bodies, np.int32).reshape(-1), np.asarray(caps, np.float64).reshape(-1, 7)
        self._out_bufs.pop("closest_points", None)
        if len(bodies) == 0:
            self.batch.set_proximity_shapes([])
            self._prox = None
            return None
        if pairs is None:
            have = sorted(set(int(b) for b in bodies))
            parent = m.array("parent").astype(int)
            pairs = [(a, b) for i, a in enumerate(have) for b in have[i + 1:]
                     if not (exclude_adjacent and (parent[b] == a or parent[a] == b))]
            if exclude_start_overlaps and pairs:
                probe = _capi.Batch(m, 1, self.device.index)
                try:
                    probe.reset()
                    probe.set_proximity_shapes(bodies, caps, pairs)
                    d = torch.empty(1, len(pairs), device=self.device)
                    probe.proximity(d, pairs=len(pairs))
                    keep = (~(d[0] < 0)).cpu().numpy()
                finally:
                    probe.forget_buffers()
                    probe.close()
                pairs = [p for p, k in zip(pairs, keep) if k]
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        self.batch.set_proximity_shapes(bodies, caps, pairs)
        self._prox = ProximityShapes(bodies, caps, pairs)
        return self._prox

    def closest_points(self, points=False):
        """Signed distance [n, P] between the bodies of every pair of proximity_shapes() (made with its defaults on first use) at
        the current state: the smallest over the capsules of the two bodies, negative = overlap depth. points: a ClosestPoints
        instead, adding point_a, point_b [n, P, 3] (world; on the surfaces of A and B), normal [n, P, 3] (unit, from B to A:
        pybullet's contactNormalOnB) and capsule [n, P, 2] int32 (table indices of the two winning capsules). The tensors are
        buffers of the env, reused by the next call."""
        if self._prox is None:
            self.proximity_shapes()
        n, P = self.num_envs, len(self._prox.pairs)
        f = lambda *s: torch.empty(*s, device=self.device)
        out = self._buffers("closest_points", (P, bool(points)), lambda: (f(n, P),) + (
            (f(n, P, 3), f(n, P, 3), f(n, P, 3), torch.empty(n, P, 2, dtype=torch.int32, device=self.device)) if points else (None,) * 4))
        self.batch.proximity(*out, pairs=P)
        return ClosestPoints(*out) if points else out[0]

    def self_collision_distance(self):
        """[n]: the smallest distance over the pairs of proximity_shapes(); negative: two bodies of the env overlap by that much."""
        return self.closest_points().min(dim=1).values

    def in_self_collision(self, margin=0.0):
        """[n] bool: some pair of proximity_shapes() is closer than `margin`."""
        return self.self_collision_distance() < margin

    # ---- floor clearance, and what the fall predicate of set_termination() left (trex_batch_body_clearance /
    # trex_batch_termination_info; no host sync)
    def _link_bodies(self, links):
        """links: names or indices of URDF links -> their bodies [K] (numpy int64)"""
        return np.array([self._links.link_body[self._links.index(l)] for l in links], np.int64)

    def body_clearance(self, links=None, lowest=False):
        """Height of the lowest collision point above the floor, exact over the collision geometry of the physics, at the
        current state: [n, num_bodies] for every body (links=None), or [n, K] for the bodies of the links `links` (names or
        indices; one link: [n]). +inf for a body without collision geometry; negative: that deep in the floor. lowest: a tuple
        (clearance, point [..., 3]) with the world position of that lowest point. One launch, device tensors."""
        n, nb = self.num_envs, self.model.num_bodies
        clr = torch.empty(n, nb, device=self.device)
        low = torch.empty(n, nb, 3, device=self.device) if lowest else None
        self.batch.body_clearance(clr, low)
        if links is not None:
            one = isinstance(links, (str, int, np.integer))
            idx = torch.as_tensor(self._link_bodies([links] if one else list(links)), device=self.device)
            clr = clr[:, idx[0]] if one else clr[:, idx]
            if lowest:
                low = low[:, idx[0]] if one else low[:, idx]
        return (clr, low) if lowest else clr

    def _term_info(self, k):
        if self._term_buf is None:
            raise RuntimeError("termination is not enabled (set_termination)")
        out = self._term_buf[k]
        self.batch.termination_info(*[out if i == k else None for i in range(3)])
        return out

    @property
    def termination_reason(self):
        """[n] int32 on the device: why each env fell in the last step - bits 1 head height, 2 tilt, 4 clearance; 0: it did not.
        A buffer of the env, rewritten by the next read."""
        return self._term_info(0)

    @property
    def termination_values(self):
        """[n, 3] on the device, what the last step's decision compared: head height above the floor, cos of the base's tilt,
        least (clearance - allowed) over the watched bodies (+inf: none watched)."""
        return self._term_info(1)

    @property
    def terminal_obs(self):
        """[n, 3J] on the device: for an env that fell, the last observation of that episode (the row of an env that did not
        fall in the last step holds the one of its most recent fall, zeros before the first). With observations it stays the 3J
        base columns: the channels of the state that fell are not kept."""
        return self._term_info(2)

    # ---- ray casts (trex_batch_ray_test: pybullet's rayTestBatch; no host sync; trex_gym.sensors builds patterns)
    def ray_test(self, rays, link=None, positions=False, normals=False, bodies=None, floor=True):
        """Cast rays [n, R, 6] (or [R, 6]: one pattern for every env) - from xyz, to xyz, in the frame of link `link` (name or
        index; None: the world) - against the collision geometry render_tensor() draws, at the current state. bodies: an
        iterable of body indices that may be hit (None: all); floor: whether the floor may be.
        -> (fraction [n, R], body [n, R] int32[, position [n, R, 3]][, normal [n, R, 3]]) on the device: fraction of the
        segment at the nearest hit (1.0: none), body index (-1 the floor, -2 a miss), world hit point (a miss: the segment's
        end) and unit normal (a miss: zeros). The tensors are buffers of the env, reused by the next call of the same shape."""
        k = -1 if link is None else self._links.index(link)
        rays = self._dev(torch.as_tensor(rays))
        if rays.dim() not in (2, 3) or rays.shape[-1] != 6:
            raise ValueError("rays must have shape (%d, R, 6) or (R, 6), got %s" % (self.num_envs, tuple(rays.shape)))
        mask = 0xFFFFFFFF
        if bodies is not None:
            mask = 0
            for b in bodies:
                if not 0 <= int(b) < self.model.num_bodies:
                    raise IndexError("body index %d out of range [0, %d)" % (int(b), self.model.num_bodies))
                mask |= 1 << int(b)
        n, R = self.num_envs, int(rays.shape[-2])
        frac, body, pos, nrm = self._buffers("ray_test", (R, bool(positions), bool(normals)), lambda: (
            torch.empty(n, R, device=self.device), torch.empty(n, R, dtype=torch.int32, device=self.device),
            torch.empty(n, R, 3, device=self.device) if positions else None,
            torch.empty(n, R, 3, device=self.device) if normals else None))
        self.batch.ray_test(rays, k, None, mask, floor, frac, body, pos, nrm)
        return (frac, body) + ((pos,) if positions else ()) + ((nrm,) if normals else ())
