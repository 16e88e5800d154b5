"""Tolerance tables that more than one test module reads. A table read by one module stays in that module."""

# ---------------------------------------------------------------- dynamics queries (tests/test_gpu_dynamics.py)
# Largest deviations measured at N = 67 on an MI355X (profiles/r12_dynamics.txt). Tolerance = 4 x measured, never above the cap;
# no cap binds. The round trip and the step-tied check draw their torques with dynamics_ref.random_tau - every joint accelerates
# within 10 rad/s^2 - and compare with [0, tau] itself, the rounding of the accelerations to f32 included. (Torques drawn joint
# by joint, without regard to the coupling, throw the light links at 1e3 .. 1e5 rad/s^2; the body forces that cancel to tau
# are then tens of times larger than tau and the round trip sat at 2.5e-5 .. 4.7e-5, half of it the f32 rounding of the input.)
DYNAMICS_MEASURED = dict(id_zero=4.38e-7, id_roundtrip=7.56e-7, id_step=2.21e-6, mass=1.81e-6, minv=1.82e-7, jac=2.59e-7, cent=1.05e-5)
DYNAMICS_CAPS = dict(id_zero=1e-4, id_roundtrip=1e-4, id_step=1e-4, mass=1e-5, minv=1e-5, jac=1e-4, cent=1e-4)
DYNAMICS_TOL = {k: min(4 * v, DYNAMICS_CAPS[k]) for k, v in DYNAMICS_MEASURED.items()}

# ---------------------------------------------------------------- link kinematics (tests/test_gpu_link_state.py)
# Largest deviations measured at N = 67 on an MI355X (profiles/r17_link_state.txt): pose, velocity, the bias acceleration (accel
# NULL) and the acceleration at a random accel (dynamics_ref.random_tau: joints within 10 rad/s^2), each over the three axes and,
# for the accelerations, with and without `proper`. Tolerance = 4 x measured, never above the cap.
LINK_MEASURED = dict(pose=2.06e-7, velocity=4.33e-7, bias=3.43e-7, accel=4.42e-7)
LINK_CAPS = dict(pose=1e-5, velocity=1e-4, bias=1e-4, accel=1e-4)
LINK_TOL = {k: min(4 * v, LINK_CAPS[k]) for k, v in LINK_MEASURED.items()}
