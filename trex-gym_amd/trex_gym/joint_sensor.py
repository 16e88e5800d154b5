"""The joint force/torque sensor of a TrexVecEnv (include/trex_joint_wrench.h): the 6-D wrench every joint transmits - pybullet's
enableJointForceTorqueSensor / getJointState(...)[2], the `jointReactionForces` of the reference's TrexRobot.get_joint_state.

    joint_wrench(env, accel=None, wrench=None, axes="link", out=None)   the bare query: one launch, reads the state
    attach(env, external=True)      the sensor on every joint: the env gets `joint_api`, `joint_reaction` [n, J, 6] (link axes)
                                    and `joint_base_residual` [n, 6], refreshed in place behind every step and reset
    joint_load(env, joints=None)    [n, k, 2]: the norms of the force and of the moment of the attached sensor's rows
    detach(env)                     takes it all off again

Row k is the wrench the parent exerts on the child body of joint k (observation order, env.model.joint_names) through the joint:
force (N), then moment (N m) about the joint origin, in the child link's axes ("link") or in world axes ("world"). Rigid-body
terms only, as for inverse_dynamics(): the motor, the joint limit and the link damping are not inputs; their sum is what the
component of the moment along the joint axis reports.

What the attached sensor measures is a STEP-MEAN ESTIMATE, stated once: the contact sensor's wrench - the mean floor-contact
wrench over the solves of the env-step - and the external wrench of set_external_wrench / apply_external_force, against the mean
acceleration of the env-step, (generalised velocity now - generalised velocity one step ago) / (dt * substeps), evaluated at the
post-step state. An env whose episode ended with the step (its done flag is set) and every env after a reset_tensor() get a zero
acceleration: their velocity jump is a reset, not a motion. `joint_base_residual` - the wrench the free base would still need from
outside, zero for a consistent free-floating body - tells how far the estimate is from closing; scripts/joint_wrench_bench.py
reports it. The wrenches of trex_gym.perturb.RandomPushes and of the pushes of trex_gym.randomize live in the batch and are not
seen by the sensor. Parity with pybullet's sign and frame conventions for jointReactionForces is unpinned.

Feeding the readings on takes no more code. Into the observation: construct the env with observations.external(6 * k) channels
and external=lambda env: env.joint_reaction[:, ankles].reshape(env.num_envs, -1) (ankles: k joint indices), then attach() before
the first reset - the callable reads the attribute when the channels are composed, and the sensor refreshes before that. Into a
privileged critic: after attach(), critic.attach(env, critic.clean() + critic.tensor(env.joint_reaction.view(env.num_envs, -1)))
- joint_reaction is refreshed in place, so the view stays valid, and the critic's row is filled behind the sensor. Nothing
attached: nothing changes - not a launch, not a byte."""
import torch

from . import joint_wrench_capi as JC
from ._capi import TrexError


def joint_wrench(env, accel=None, wrench=None, axes="link", out=None, base_out=None):
    """The bare query at the env's current state -> [n, J, 6]: accel [n, 6 + J] generalised accelerations (None: zeros - the
    static and velocity-product load), wrench [n, num_bodies, 6] what the world applies to the bodies (world axes, force at the
    COM, torque about it: the layout of contact_wrench() and set_external_wrench(); None: nothing), axes "link" or "world".
    base_out [n, 6]: also the whole tree's residual about the base origin, world axes."""
    api = env.joint_api if env.joint_api is not None else JC.BatchJointWrench(env.batch)
    dev = lambda t: None if t is None else env._dev(torch.as_tensor(t))
    return api.joint_wrench(dev(accel), dev(wrench), None, axes, out, base_out)


def attach(env, external=True):
    """pybullet's enableJointForceTorqueSensor for every joint. Enables the contact sensor, allocates the velocity latch, and hooks
    two launches behind every step_tensor and reset_tensor (trex_batch_generalized_velocity, trex_batch_joint_wrench), before the
    channels' compose and the critic's row. external: the env's external wrench, while one is set, enters as the second wrench.
    The env then has `joint_api` (joint_wrench_capi.BatchJointWrench), `joint_reaction` [n, J, 6] in link axes and
    `joint_base_residual` [n, 6], tensors refreshed in place - views and captured graphs stay valid. The first reading is taken
    here, at zero acceleration."""
    if env._joint_fill is not None:
        detach(env)
    api = JC.BatchJointWrench(env.batch)
    n, dev = env.num_envs, env.device
    try:
        env.contact_wrench()
        sensor_was_on = True
    except TrexError:
        sensor_was_on = False
        env.enable_contact_sensor(True)
    inv_dt = 1.0 / (env.model.get_param("dt") * env.model.get_param("substeps"))
    latch, accel = torch.zeros(n, api.D, device=dev), torch.zeros(n, api.D, device=dev)
    contact = torch.zeros(n, api.num_bodies, 6, device=dev)
    reaction, residual = torch.zeros(n, api.J, 6, device=dev), torch.zeros(n, 6, device=dev)
    done_column = 3 * env.J + 1

    def fill(rows):
        """rows: the block the step call wrote (its done column zeroes the rows of the envs that ended an episode); None: a reset"""
        if rows is None:
            api.generalized_velocity(vel=latch)
            accel.zero_()
        else:
            api.generalized_velocity(latch, latch, inv_dt, rows, done_column, accel)
        env.contact_wrench(contact)
        api.joint_wrench(accel, contact, env._wrench if external else None, JC.AXES_LINK, reaction, residual)

    env.joint_api, env.joint_reaction, env.joint_base_residual = api, reaction, residual
    env._joint_fill = fill
    env._joint_sensor = dict(external=bool(external), sensor_was_on=sensor_was_on, inv_dt=inv_dt, latch=latch, accel=accel, contact=contact)
    fill(None)
    return env


def detach(env):
    """Takes the sensor off the env again; the contact sensor goes off where attach() switched it on."""
    if env._joint_fill is None:
        return env
    if not env._joint_sensor["sensor_was_on"]:
        env.enable_contact_sensor(False)
    env.joint_api, env.joint_reaction, env.joint_base_residual, env._joint_fill = None, None, None, None
    del env._joint_sensor
    return env


def joint_index(env, joint):
    """a joint name or an index in observation order -> the index"""
    if isinstance(joint, str):
        return list(env.model.joint_names).index(joint)
    if not 0 <= int(joint) < env.J:
        raise ValueError("joint %r outside [0, %d)" % (joint, env.J))
    return int(joint)


def joint_load(env, joints=None):
    """-> [n, k, 2]: |force| (N) and |moment| (N m) of the attached sensor's rows for `joints` (names or indices in observation
    order; None: all J) - a joint-load penalty, an overload flag, a critic input."""
    if env.joint_reaction is None:
        raise ValueError("the env has no joint sensor (trex_gym.joint_sensor.attach)")
    r = env.joint_reaction
    if joints is not None:
        r = r[:, [joint_index(env, j) for j in joints]]
    return torch.stack([r[..., :3].norm(dim=-1), r[..., 3:].norm(dim=-1)], dim=-1)
