"""The actuator model's host side (include/trex_batch.h: trex_batch_set_control_mode / _set_motor_gains /
_set_stiffness_actions): argument handling shared by TrexVecEnv and TrexBulletEnv. Nothing here touches a device."""
import numpy as np

CONTROL_MODES = {"position": 0, "velocity": 1, "torque": 2}   # TREX_CTRL_*; pybullet's POSITION_ / VELOCITY_ / TORQUE_CONTROL
DEFAULT_KP_MAX = 1.0


def resolve_control_modes(control_mode, joint_names):
    """control_mode: None / a mode name (every joint), a sequence of J names or ints, or {joint_name: mode} (the joints it
    does not name stay position controlled) -> list of J ints in observation order."""
    J = len(joint_names)

    def one(m):
        if isinstance(m, str):
            if m not in CONTROL_MODES:
                raise ValueError("unknown control mode %r (position, velocity, torque)" % (m,))
            return CONTROL_MODES[m]
        if isinstance(m, (bool, float)) or int(m) != m or not 0 <= int(m) <= 2:
            raise ValueError("unknown control mode %r (0 position, 1 velocity, 2 torque)" % (m,))
        return int(m)

    if control_mode is None:
        return [0] * J
    if isinstance(control_mode, str):
        return [one(control_mode)] * J
    if isinstance(control_mode, dict):
        out = [0] * J
        index = {n: k for k, n in enumerate(joint_names)}
        for name, m in control_mode.items():
            if name not in index:
                raise KeyError("control_mode: unknown joint %r" % (name,))
            out[index[name]] = one(m)
        return out
    modes = [one(m) for m in control_mode]
    if len(modes) != J:
        raise ValueError("control_mode: expected %d entries, got %d" % (J, len(modes)))
    return modes


def action_bounds(modes, lower, upper, max_velocity, max_force, variable_stiffness=False, kp_max=DEFAULT_KP_MAX):
    """(low, high) f32 of the action space: per joint its limits (position), +- max_velocity (velocity) or +- max_force
    (torque); with variable_stiffness J more columns [0, kp_max]."""
    modes = np.asarray(modes)
    lo = np.where(modes == 1, -max_velocity, np.where(modes == 2, -max_force, lower)).astype(np.float32)
    hi = np.where(modes == 1, max_velocity, np.where(modes == 2, max_force, upper)).astype(np.float32)
    if variable_stiffness:
        lo = np.concatenate([lo, np.zeros(len(modes), np.float32)])
        hi = np.concatenate([hi, np.full(len(modes), kp_max, np.float32)])
    return lo, hi


def broadcast_gains(value, n, J, name="gain"):
    """A scalar, [J] or [n, J] (numpy, torch or a sequence) -> a torch f32 [n, J] tensor on the value's device (CPU for
    host values); None stays None."""
    import torch
    if value is None:
        return None
    t = value if isinstance(value, torch.Tensor) else torch.as_tensor(np.asarray(value, np.float32))
    t = t.to(torch.float32)
    if t.dim() > 2 or (t.dim() == 2 and tuple(t.shape) != (n, J)) or (t.dim() == 1 and t.shape[0] != J):
        raise ValueError("%s: expected a scalar, [%d] or [%d, %d], got shape %s" % (name, J, n, J, tuple(t.shape)))
    return t.expand(n, J).contiguous()
