/*
 * trex_joint_wrench.h - C-ABI of the joint force/torque sensor of a TrexBatch (include/trex_batch.h, whose conventions hold here:
 * return codes, pointer validation - TREX_E_INVALID with nothing launched and nothing changed -, streams, capturable from the second
 * call with the same buffers on). trex_batch.h includes this header at its end; including either one declares both.
 */
#ifndef TREX_JOINT_WRENCH_H
#define TREX_JOINT_WRENCH_H

#include "trex_batch.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- joint force/torque sensor (pybullet's enableJointForceTorqueSensor / getJointState(...)[2], jointReactionForces; the third
 * field of the reference's TrexRobot.get_joint_state, trex_robot.py:120-150): the 6-D wrench every joint transmits, at the env's
 * current state and the env's mass scale. A read-only query beside the dynamics queries, whose conventions it uses: D = 6 + J, the
 * order and the axes of the generalised velocity, classical accelerations, joints in observation order.
 *
 * out_dev [N, J, 6] f32 device: row k is the wrench the PARENT exerts on the CHILD body of joint k through the joint - force
 *   fx fy fz (N), then moment tx ty tz (N m) about the joint origin, which is the origin of the child body's frame.
 * accel_dev [N, D], nullable: the generalised accelerations the wrench is to hold at (NULL: zeros), as for
 *   trex_batch_inverse_dynamics.
 * wrench_a_dev, wrench_b_dev [N, num_bodies, 6], each nullable: what the world applies to the bodies, in the layout of
 *   trex_batch_set_external_wrench and trex_batch_contact_wrench - world axes, force at the body's COM, torque about it. Their SUM is
 *   what enters (two inputs, so that the contact sensor's buffer and the external wrench go in as they are); each element pair is
 *   added first, so a + b gives the bits of their f32 sum passed as one. With both NULL no wrench is loaded.
 * The definition (ONE). With S(i) the bodies of the subtree of body i (i included), m_b, c_b, Ic_b a body's mass, world COM and
 *   rotational inertia about it, w_b, al_b its angular velocity and acceleration, a_c,b the classical acceleration of its COM PLUS
 *   g z (gravity as the base's upward acceleration), (F_b, T_b) the summed input wrench on it and r_i the origin of joint i:
 *     f_i = sum_{b in S(i)} (m_b a_c,b - F_b)
 *     n_i = sum_{b in S(i)} [ Ic_b al_b + w_b x Ic_b w_b - T_b + (c_b - r_i) x (m_b a_c,b - F_b) ]
 *   Rigid-body terms only, as for trex_batch_inverse_dynamics: link damping, motors and joint limits are not inputs - their sum is
 *   what the component of n_i along the joint axis reports. That component equals the joint's entry of trex_batch_inverse_dynamics
 *   when both wrenches are NULL.
 * axes: TREX_AXES_WORLD, or TREX_AXES_LINK: every row in the axes of its CHILD BODY's frame. That frame is the URDF frame of the
 *   joint's child link - the link the joint carries, whose "link_tf" (trex_model_get_array) is the identity. A link welded to it by
 *   fixed joints shares the body; its frame is the body's composed with its "link_tf" (body <- link), so a row in that link's axes
 *   is the transpose of that rotation times the row's force and moment (the moment still about the joint origin).
 *   TREX_AXES_BASE is refused.
 * base_out_dev [N, 6], nullable: the same sums over the WHOLE tree about the base origin, world axes - the wrench the free base
 *   would still need from outside. It equals the base rows of trex_batch_inverse_dynamics when both wrenches are NULL, and it is
 *   zero when accel and the wrenches are consistent with a free-floating base.
 * Like the dynamics queries: asynchronous on `stream`, nothing allocated or waited for, only the outputs written, from the second
 * call with known buffers ONE plain kernel launch, usable inside a single-stream capture; a non-finite env affects its own rows
 * only. TREX_E_INVALID, nothing launched: out_dev NULL, axes neither WORLD nor LINK, a buffer shorter than stated, host memory or
 * another device's. */
int trex_batch_joint_wrench(TrexBatch *batch, const float *accel_dev, const float *wrench_a_dev, const float *wrench_b_dev, int axes,
                            float *out_dev, float *base_out_dev, void *stream);

/* The generalised velocity of every env in the order of the dynamics queries - base linear v(3), base angular w(3), world axes,
 * then qd(J) in observation order - and its backward difference: ONE launch gives the sensor its acceleration and its memory.
 * vel_dev [N, D], nullable: receives the current generalised velocity.
 * prev_dev [N, D], nullable: with it, accel_dev [N, D] (then required) = (current - prev) * inv_dt, evaluated as exactly that f32
 *   expression. vel_dev may be prev_dev ITSELF (the latch: the difference is taken before the element is replaced); any other
 *   overlap of the three buffers is refused. Without prev_dev, accel_dev must be NULL.
 * done_dev, nullable: a float column, env e's entry at done_dev[e * done_stride] (done_stride >= 1; the done column of the rows,
 *   or any array). An env whose entry is non-zero gets a ZERO accel row: its velocity jump is a reset, not a motion.
 * Asynchronous, one launch, capturable, only vel_dev and accel_dev written. TREX_E_INVALID, nothing launched: vel_dev and prev_dev
 * both NULL, accel_dev missing or unexpected, a non-finite inv_dt, done_stride < 1 with done_dev, overlapping buffers, a short
 * buffer, host memory or another device's. */
int trex_batch_generalized_velocity(TrexBatch *batch, float *vel_dev, const float *prev_dev, float inv_dt, const float *done_dev,
                                    int done_stride, float *accel_dev, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_JOINT_WRENCH_H */
