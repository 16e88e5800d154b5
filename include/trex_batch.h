/*
 * trex_batch.h - C-ABI of the MI355X-native batched physics step for the T-rex gym env.
 *
 * This is the drop-in boundary for ONE path of bingjeff/trex-gym: everything that
 * TrexBulletEnv.step()/reset() delegates to the physics engine and the robot adapter
 * (boundary 3).  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative TREX_E_* code on failure;
 *     trex_last_error() returns a thread-local message for the last failure
 *     (pybullet raises pybullet.error at the same call sites [EXT]).
 *   - a TrexModel is immutable after trex_batch_create() has consumed it and may be
 *     shared by several batches; a TrexBatch is bound to one HIP device, is not re-entrant,
 *     and all of its calls are asynchronous and ordered on the hipStream_t given
 *     (passed as void* so the header needs no HIP include; NULL = the default stream).
 *   - "device" pointers are caller-owned HIP device buffers (e.g. torch tensors' data_ptr()) on the
 *     batch's device. Every batch call validates each distinct ALLOCATION once (hipPointerGetAttributes +
 *     its address range, cached per batch; pointers into a validated allocation are range-checked against it): host memory, another device's memory or a buffer shorter than
 *     the call needs returns TREX_E_INVALID instead of faulting the GPU. The cache is keyed by address: a
 *     buffer that was validated must stay allocated for as long as it is passed to the batch; a caller that
 *     FREES buffers it has passed (and may get the address back for a shorter or foreign allocation) calls
 *     trex_batch_forget_buffers() after freeing.
 *   - joints are always exposed in the reference's observation order: revolute joint names
 *     sorted (trex_robot.py:311-314); J = trex_model_num_joints() (25 for trex.urdf).
 */
#ifndef TREX_BATCH_H
#define TREX_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define TREX_OK 0
#define TREX_E_INVALID (-1)   /* bad argument (null pointer, unknown name, size mismatch) */
#define TREX_E_IO (-2)        /* file missing / unreadable */
#define TREX_E_PARSE (-3)     /* malformed URDF / mesh */
#define TREX_E_UNSUPPORTED (-4) /* model outside what the kernels handle (>26 bodies, joint type) */
#define TREX_E_HIP (-5)       /* HIP runtime error, no device */

typedef struct TrexModel TrexModel;
typedef struct TrexBatch TrexBatch;

const char *trex_last_error(void);
/* Identifies the kernel build (hash of the kernel sources, set by the Makefile): profiles/ records the
 * build its counters were collected on, bench.py quotes them only for a matching build. */
const char *trex_build_id(void);

/* ---- model: replaces loadURDF + the getJointInfo/getDynamicsInfo/getNumJoints introspection
 *      of trex_robot.py:47-56,98-117,158,175-187,294-320 and the floor of trex_env.py:103 ---- */

/* Parse a URDF (fixed + revolute joints), merge fixed joints, attach collision hulls.
 * collisions_dir: NULL -> use the URDF's own <collision><mesh .obj>; otherwise a directory of
 * COL_*_convex_hull.dae hulls placed with the <visual><origin> of the same-named mesh (this is
 * how the reference's own assets/trex.urdf, which has no <collision>, is loaded). */
int trex_model_load(const char *urdf_path, const char *collisions_dir, TrexModel **out);
void trex_model_destroy(TrexModel *model);

int trex_model_num_bodies(const TrexModel *model);      /* 26: moving bodies after the merge */
int trex_model_num_joints(const TrexModel *model);      /* 25: actuated revolute joints */
int trex_model_num_urdf_joints(const TrexModel *model); /* 132 = pybullet getNumJoints (trex_robot.py:158) */
int trex_model_num_hull_vertices(const TrexModel *model);
double trex_model_total_mass(const TrexModel *model, int include_base_link); /* trex_robot.py:318-320 sums without the base link */

/* k-th joint in observation order: name, pybullet joint index (trex_robot.py:314), limits
 * (trex_robot.py:337-346). Any out pointer may be NULL. */
int trex_model_joint_info(const TrexModel *model, int k, const char **name, int *urdf_joint_index,
                          double *lower, double *upper);

/* reset configuration (trex_env.py:81-87, trex_robot.py:305-308). Accepts the URDF joint name
 * or the pre-rename spelling ("femur_L_joint"). Unknown joint -> TREX_E_INVALID (the reference
 * raises KeyError there). Must be called before trex_batch_create. */
int trex_model_set_start_angle(TrexModel *model, const char *joint_name, double angle);
int trex_model_set_start_pose(TrexModel *model, const double xyz[3], const double rpy[3]); /* trex_env.py:105-106 */

/* Collision primitives (the step before the path): replace every convex hull by capsules /
 * spheres fitted as the reference's tools/mesh_primitives.py:323-402 does (PCA box -> capsule, octant
 * subdivision while radius > max_radius). Contacts are then generated from the capsule end spheres
 * (148 points instead of 2 181 vertices for trex.urdf at max_radius 0.2). Call before trex_batch_create. */
int trex_model_use_primitive_collision(TrexModel *model, double max_radius, int max_divisions, int min_points);
/* The fit of ONE convex hull (group g of "hull_group_start", body-frame coordinates) without changing the
 * model: writes up to `capacity` primitives as 7 doubles each (p0 xyz, p1 xyz, radius; p0 == p1 = sphere)
 * and returns their number (MJCF export, tests). */
int trex_model_fit_hull_primitives(const TrexModel *model, int group, double max_radius, int max_divisions,
                                   int min_points, double *out, int capacity);

/* engine parameters: "dt" "substeps" "iterations" "gravity" "motor_kp" "motor_kd" "motor_max_force"
 * "floor_z" "friction" "erp" "contact_erp" "contact_margin" "link_damping"
 * "max_coordinate_velocity" "max_contacts"  (setTimeStep / setPhysicsEngineParameter / setGravity,
 * trex_env.py:115-117; motor gains trex_robot.py:260,401,421). "max_contacts" is the contact-point budget
 * per env: default and upper limit 13 (25 motor rows + 3 x 13 contact rows = the 64 lanes of a wavefront;
 * larger values are clamped by the kernel).
 * "warmstart" (default 0 = off; values outside [0, 1] are refused with TREX_E_INVALID): PGS warm start of the contact rows,
 * Bullet's warmstartingFactor. Read when a batch is created, like every parameter. With warmstart > 0:
 *   - a contact point is identified by its hull vertex (its index into the model's collision points, unique across bodies;
 *     primitive collision keeps its sphere centres and capsule ends in the same array);
 *   - every env keeps a record of the points its last solve used (at most 13): vertex and final normal / friction-x /
 *     friction-y impulses, unscaled. A point found in the record starts the next solve at warmstart x those impulses on
 *     its three rows (the friction pyramid uses world axes, so the rows mean the same from one solve to the next); every
 *     other row - new points, motor rows, joint-limit rows - starts at 0, as with warmstart 0;
 *   - every solve (every substep, the settle substep of a reset included) overwrites the record with its own points;
 *   - the record is emptied for the envs that trex_batch_reset / trex_batch_reset_rows reset (before their settle substep;
 *     the others keep theirs), for an env the step launch resets (episode limit, non-finite containment), and for every
 *     env by trex_batch_set_state;
 *   - it persists across launches (step, step_rows, step_many, time_steps) in a per-env device array of 256 B per env,
 *     allocated at batch creation; trex_batch_debug_step is refused (TREX_E_INVALID): its diagnostics kernel has no record.
 * With warmstart 0 nothing of this exists: the same kernels, rows and memory as without the parameter. */
int trex_model_set_param(TrexModel *model, const char *name, double value);
int trex_model_get_param(const TrexModel *model, const char *name, double *value);

/* Introspection of the compiled model for tests: copies the named array as doubles, returns the
 * element count (or a negative error). Names: "parent" "depth" "joint_axis" "joint_pos" "joint_rot"
 * "q_lower" "q_upper" "joint_damping" "mass" "com" "inertia" "obs_order" "head_body" "head_point"
 * "hull_xyz" "hull_radius" "hull_group_start" "hull_start" "sphere_center" "sphere_radius" "q_start" "base_start_pos"
 * "base_start_quat" "revolute_joint_indices" "link_body" "link_tf" (12 per link: R row-major, t).
 * "hull_plane" / "hull_plane_start": what trex_batch_render draws a hull with - the face planes (nx, ny, nz, d per plane,
 * body frame, unit n, n.x <= d inside) of the convex hull of every hull group's radius-0 points, computed from the VERTICES
 * (coplanar triangles merged; every plane touches at least 3 of them), with a CSR start per group. A group with fewer than
 * 4 non-coplanar such points has no plane and draws nothing. */
int trex_model_get_array(const TrexModel *model, const char *name, double *out, int capacity);

/* ---- batch: N independent env copies resident on one GPU ---- */

int trex_batch_create(const TrexModel *model, int num_envs, int device, TrexBatch **out);
void trex_batch_destroy(TrexBatch *batch);
int trex_batch_num_envs(const TrexBatch *batch);

/* Forget the validated caller pointers (see the conventions above): the next call validates them afresh. */
int trex_batch_forget_buffers(TrexBatch *batch);

/* Row-block calls (trex_batch_step_rows / _reset_rows / _step_many): enabled != 0 -> columns [3J+2, 3J+5) of every row
 * receive the three penalties; 0 (default) -> nothing beyond column 3J + 1 is written. */
int trex_batch_set_penalties_in_rows(TrexBatch *batch, int enabled);

/* Which wave runs which env. All waves of a launch of <= 4096 envs are resident at once and a SIMD is done when
 * its slowest wave is, so the step kernel can rank the envs by the contact count of their previous step and deal
 * them to the SIMDs heaviest-with-lightest (device-side state only; results are bitwise independent of it).
 * mode -1 (default): on for batches of 2048 envs or more - below that most SIMDs hold at most two waves and there is
 * nothing to level -, 0: off (workgroup k runs env k), 1: on for any size. */
int trex_batch_set_wave_balance(TrexBatch *batch, int mode);

/* reward weights (trex_env.py:42-44): distance, energy, drift. Defaults 1.0, 0.005, 0.002. */
int trex_batch_set_reward_weights(TrexBatch *batch, float distance, float energy, float drift);

/* TrexBulletEnv.reset (trex_env.py:98-122): envs with mask[n] != 0 (all if mask == NULL) go to the
 * start pose with motors disabled and take ONE un-actuated substep. obs_out (device, [N, 3J],
 * nullable) receives the observation of every env (reset or not). */
int trex_batch_reset(TrexBatch *batch, const uint8_t *mask_dev, float *obs_out_dev, void *stream);

/* TrexBulletEnv.step (trex_env.py:128-154) for all N envs in ONE kernel launch:
 * clip(actions) -> substeps x [position motors + physics substep] -> obs, reward, done.
 *   actions_dev   [N, J]  f32 device, joint targets in observation order
 *   obs_dev       [N, 3J] f32 device: q, qd, appliedJointMotorTorque (trex_robot.py:365)
 *   reward_dev    [N]     f32 device (trex_env.py:192)
 *   done_dev      [N]     u8 device, 0 (trex_env.py:183-184) - except 1 for an env whose state became
 *                         non-finite (it is put back on the start pose and reports reward 0: containment) and
 *                         for an env that reached the episode limit (trex_batch_set_episode_limit)
 *   penalties_dev [N, 3]  f32 device, nullable: lifting_com, station_keeping, energy
 *                         (the three values logged at trex_env.py:193-195) */
int trex_batch_step(TrexBatch *batch, const float *actions_dev, float *obs_dev, float *reward_dev,
                    uint8_t *done_dev, float *penalties_dev, void *stream);

/* The same two calls writing ONE row block (what the multi-GPU exchange gathers):
 *   rows_dev [N, row_stride] f32 device, row_stride >= 3J + 2:
 *     [0, 3J) observation, [3J] reward, [3J+1] done as 0.0 / 1.0. Columns beyond 3J + 2 are NOT touched, whatever the
 *     stride (rows padded for alignment, or embedded in a wider tensor with columns of the caller's own) - unless the
 *     batch was told to carry the three penalties (lifting_com, station_keeping, energy: trex_env.py:193-195) in the
 *     rows: after trex_batch_set_penalties_in_rows(batch, 1) the row calls need row_stride >= 3J + 5 and write
 *     [3J+2, 3J+5) too (zeros from a reset) - one message for a consumer that wants them. (Until round 3 a stride of
 *     3J + 5 or more switched this on implicitly.)
 * done_dev [N] u8, nullable: the done flags once more as bytes (what a consumer masks with - saves it a
 *   conversion pass over the column). trex_batch_reset_rows writes the observation columns of every env (reset or
 *   not) and, for the envs it resets, reward = 0 and done = 0: the row of a new episode. */
int trex_batch_step_rows(TrexBatch *batch, const float *actions_dev, float *rows_dev, int row_stride,
                         float *penalties_dev, uint8_t *done_dev, void *stream);
int trex_batch_reset_rows(TrexBatch *batch, const uint8_t *mask_dev, float *rows_dev, int row_stride, void *stream);

/* num_steps env-steps of every env in ONE launch, for action sequences that are known in advance (open-loop rollouts:
 * random-action benchmarks, sampling-based planners, replaying recorded actions): step s reads actions_dev[s] and writes
 * the row block rows_dev[s] -
 *   actions_dev [S, N, J] f32, rows_dev [S, N, row_stride] f32 (obs | reward | done per row, as trex_batch_step_rows),
 *   penalties_dev [S, N, 3] and done_dev [S, N] u8 nullable.
 * Results are BITWISE those of num_steps trex_batch_step_rows calls (episode limit and containment included: tested).
 * Why it exists: with one step per launch every SIMD waits for the launch's slowest wave - a fifth of the launch at 4 096
 * envs -, here a wave goes straight on to its env's next step and the env's state stays on the chip between steps. A
 * closed loop (a policy that needs step s's observations for step s + 1's actions) cannot use it. */
int trex_batch_step_many(TrexBatch *batch, const float *actions_dev, float *rows_dev, int row_stride, int num_steps,
                         float *penalties_dev, uint8_t *done_dev, void *stream);

/* Episode limit of the harness. The reference env never terminates (should_terminate() is constant False,
 * trex_env.py:183-184); a training harness cuts episodes (gym's TimeLimit; baselines' VecEnv then resets the env
 * and returns the first observation of the new episode with done = True). With max_episode_steps > 0 the STEP
 * LAUNCH itself does that for the envs whose step count reaches the limit: reward of the finished step, done = 1,
 * then start pose + the reset's settle substep, observation of the new episode - no separate reset launch.
 * episode_steps_dev ([N] i32, nullable = zeros) sets the counts (e.g. to stagger the episodes);
 * max_episode_steps = 0 switches the limit off. trex_batch_reset zeroes the count of the envs it resets. */
int trex_batch_set_episode_limit(TrexBatch *batch, int max_episode_steps, const int32_t *episode_steps_dev, void *stream);
int trex_batch_get_episode_steps(TrexBatch *batch, int32_t *episode_steps_dev, void *stream);

/* env state [N, 13 + 2J] f32 device: base position(3), base orientation quaternion xyzw(4) - both
 * of the base INERTIAL frame as resetBasePositionAndOrientation/getBasePositionAndOrientation
 * (trex_robot.py:63,327) - base linear(3) and angular(3) world velocity, q(J), qd(J). */
int trex_batch_get_state(TrexBatch *batch, float *state_dev, void *stream);
int trex_batch_set_state(TrexBatch *batch, const float *state_dev, void *stream);
/* motors stay disabled after reset until the first step (trex_robot.py:309); set_state keeps the
 * flag, this call forces it (tests). */
int trex_batch_set_motors_enabled(TrexBatch *batch, int enabled, void *stream);

/* world position of the head link COM, [N,3] (trex_robot.py:330-335). */
int trex_batch_head_position(TrexBatch *batch, float *out_dev, void *stream);

/* Rollout export for rendering (the step after the path: trex_env.py:156-181, trex_train.py:126-136):
 * world pose of EVERY URDF link frame (133 for trex.urdf, document order) as [N, L, 7] f32 device =
 * position xyz + quaternion xyzw - what getLinkState(...)[4:6] returns per link [EXT]. A renderer
 * composes it with the <visual><origin> of each mesh. */
int trex_model_num_links(const TrexModel *model);
int trex_model_link_info(const TrexModel *model, int link, const char **name, int *body);
int trex_batch_link_transforms(TrexBatch *batch, float *out_dev, void *stream);

/* The table a renderer needs to place the meshes (trex_env.py:156-181 draws them through pybullet; the reference's
 * parser holds them as UrdfLink.visual_shapes, tools/urdf_parsing.py:93-120,299-307): every <visual> mesh of the URDF
 * in document order (252 for trex.urdf) - mesh file name as written in the URDF, index of its link
 * (trex_model_link_info), and its <origin> in the link frame as position + quaternion xyzw. Any out pointer may be
 * NULL. trex_batch_visual_transforms: world pose of every mesh, [N, V, 7] f32 device = link pose x <origin> -
 * no URDF re-parsing, no composition left to the caller. The mesh FILES are the caller's (not loaded here). */
int trex_model_num_visuals(const TrexModel *model);
int trex_model_visual_info(const TrexModel *model, int visual, const char **mesh_file, int *link, double xyz[3],
                           double quat_xyzw[4]);
int trex_batch_visual_transforms(TrexBatch *batch, float *out_dev, void *stream);

/* ---- rendering (trex_env.py:156-181 getCameraImage; no GUI): a ray caster over the collision geometry the physics holds
 *
 * What is drawn: every body's convex hulls (the planes of "hull_plane" above) or, after trex_model_use_primitive_collision,
 * its collision spheres, and the floor - the plane z = floor_z (model parameter: the floor box's top face), a 1 m
 * checkerboard. Deterministic shading: one colour per body (a fixed palette), Lambert under one fixed directional light
 * plus ambient, a constant sky; one ray per pixel centre - no anti-aliasing, shadows or textures. Pixel parity with
 * pybullet's image is NOT a goal: pybullet draws the visual meshes (not shipped), this draws the collision hulls.
 *
 * Camera (pybullet's computeViewMatrixFromYawPitchRoll with upAxisIndex = 2, roll 0, and computeProjectionMatrixFOV):
 *   eye = target + Rz(yaw) Rx(pitch) (0, -distance, 0), up = Rz(yaw) Rx(pitch) (0, 0, 1), +z up, looking at target;
 *   the reference's camera (distance 10, yaw 90, pitch -30) sits at target + (8.66, 0, 5.0) looking along -x.
 *   NOT CONFIRMED against pybullet (not available here): that is the convention of its source as recalled.
 *   Projection: OpenGL perspective, VERTICAL fov, aspect = width / height; row 0 is the TOP of the image (getCameraImage).
 *   Geometry closer than near_z is cut away; farther than far_z is not drawn. */
typedef struct TrexCamera {
  float distance, yaw_deg, pitch_deg, fov_deg, near_z, far_z;
  int follow_base;        /* != 0: target = each env's base position (trex_env.py:157); else target[] */
  float target[3];
} TrexCamera;

/* Render num_views views: view v shows env env_ids[v] (a HOST array; NULL = all N envs in order, num_views then 0 or N).
 * Outputs per view, each device and nullable (not all three):
 *   rgb_dev   [V, H, W, 3] u8;
 *   depth_dev [V, H, W] f32: linear eye-space z in metres (pybullet's depth buffer is depth_to_zbuffer of it), far_z where
 *             nothing is hit;
 *   seg_dev   [V, H, W] i32: body index in [0, num_bodies), -1 floor, -2 nothing.
 * Every pixel of every non-NULL buffer is written. An env id out of range, a width or height <= 0 or > 4096, more than
 * 65535 views, a non-finite or degenerate camera, all outputs NULL or a buffer shorter than the call needs return
 * TREX_E_INVALID before anything reaches the GPU; a model with more than 512 drawable primitives TREX_E_UNSUPPORTED.
 * Ordered on `stream`. Reads the state and writes nothing else (no state, warm-start record or episode count). The first
 * call computes the hull planes and keeps them in the batch; env ids are copied to a batch-owned device buffer. */
int trex_batch_render(TrexBatch *batch, const TrexCamera *camera, int width, int height, const int32_t *env_ids,
                      int num_views, uint8_t *rgb_dev, float *depth_dev, int32_t *seg_dev, void *stream);

/* ---- ray casts (pybullet's rayTestBatch; no reference counterpart): range sensors - height scanners, lidar fans on a link,
 *      foot clearance, line of sight. R segments per env against the geometry trex_batch_render draws, at the current state.
 *
 * rays_dev [N, R, 6] f32 device, or [R, 6] when shared != 0 (one pattern for every env): from xyz, to xyz of each segment.
 * link: the coordinates are in the frame of URDF link `link` (indices and frames as trex_model_link_info and "link_tf", as in
 *   trex_batch_jacobian), evaluated at each env's current state; -1: the world frame. A HOST value shared by all envs.
 * body_mask: bit b set = body b may be hit (0xFFFFFFFF: every body); hit_floor != 0: the floor half-space z <= floor_z may be
 *   hit. body_mask 0 without hit_floor is legal: everything misses. Masked bodies cost no work.
 * Geometry: exactly what trex_batch_render draws - the hull planes ("hull_plane"), after trex_model_use_primitive_collision the
 *   spheres, the floor plane - from the table the two calls share (made by whichever comes first; more than 512 primitives:
 *   TREX_E_UNSUPPORTED). The hulls are the COLLISION hulls, not pybullet's visual meshes.
 * Outputs, device; fraction_dev is required, the other three are nullable; every element of every non-NULL output is written:
 *   fraction_dev [N, R] f32     t in [0, 1] along from -> to of the hit; 1.0 on a miss (pybullet's value)
 *   body_dev     [N, R] i32     body index, -1 the floor (the renderer's seg code); -2 on a miss
 *   position_dev [N, R, 3] f32  world hit point; the world `to` point on a miss
 *   normal_dev   [N, R, 3] f32  world unit normal - the entered face of a hull, radial for a sphere, (0, 0, 1) for the floor;
 *                               zeros on a miss
 * Hit rule: the nearest ENTRY point with 0 <= t <= 1. A primitive that contains `from` (its entry lies behind the origin,
 *   t_enter < 0) is not hit by that ray - a hull, a sphere, and the floor when from.z < floor_z: a sensor placed inside the head
 *   hull looks out of it. This is Bullet's behaviour AS RECALLED (a ray that starts inside a convex shape does not report it);
 *   it is NOT pinned against pybullet, which is not available here. Ties go to the floor first, then to the lower primitive
 *   index, as in the renderer.
 * Ray values are not validated: a zero-length or non-finite ray is a miss (fraction 1, body -2, zero normal; its position is
 *   whatever its `to` transforms to) and disturbs no other ray.
 * Like the dynamics queries: asynchronous on `stream`; every device buffer validated (host memory, foreign memory or a short
 *   buffer: TREX_E_INVALID before any launch); nothing but the outputs written - state, warm-start record, contact sensor and
 *   episode counts stay bitwise untouched. The first call may allocate the table; from the second call with known buffers it is
 *   one plain kernel launch, usable in a single-stream capture. TREX_E_INVALID also for num_rays outside [1, 16384], link
 *   outside [-1, num_links), rays_dev or fraction_dev NULL. */
int trex_batch_ray_test(TrexBatch *batch, const float *rays_dev, int num_rays, int shared, int link, uint32_t body_mask,
                        int hit_floor, float *fraction_dev, int32_t *body_dev, float *position_dev, float *normal_dev,
                        void *stream);

/* domain randomisation (BASELINE config 5; no reference counterpart): per-env mass scale of each
 * moving body [N, num_bodies] and per-env friction coefficient [N]; either may be NULL. */
int trex_batch_set_domain(TrexBatch *batch, const float *mass_scale_dev, const float *friction_dev,
                          void *stream);

/* External wrench per env and moving body, world frame: wrench_dev [N, num_bodies, 6] f32 = fx fy fz (N) at the
 * body's centre of mass, tx ty tz (N m) about it. NULL clears it. (pybullet's applyExternalForce / applyExternalTorque;
 * no reference counterpart: pushes, perturbations, load cases.)
 *   - the values are COPIED on `stream` into a batch-owned buffer (allocated at the first non-NULL call: a batch that never
 *     sets a wrench allocates nothing) and stay in force until the next call replaces them or NULL clears them; resets,
 *     trex_batch_set_state and trex_batch_set_domain do not clear them;
 *   - they act, held constant, on EVERY SUBSTEP of every env-step of trex_batch_step, _step_rows, _step_many (all S steps) and
 *     _time_steps. pybullet's applyExternalForce lasts one stepSimulation - ONE substep here -: this call holds the wrench
 *     for the whole env-step (substeps x dt seconds);
 *   - they do NOT act on a reset's settle substep: trex_batch_reset / _reset_rows, and the settle substep of an
 *     episode-limit reset inside a step launch - the first observation of an episode never depends on the wrench;
 *   - values are not validated: a non-finite value in an env's wrench makes that env non-finite, and containment handles it
 *     (done = 1, reward 0, start pose - at every step while the value stays); no other env is affected;
 *   - trex_batch_debug_step returns TREX_E_INVALID while a wrench is set;
 *   - a buffer shorter than N * num_bodies * 6 floats, host memory or another device's memory returns TREX_E_INVALID
 *     before anything is launched.
 * While a wrench is set the step launches run separate kernel instantiations; after NULL the default kernels again. */
int trex_batch_set_external_wrench(TrexBatch *batch, const float *wrench_dev, void *stream);

/* Actuator model: per-joint control modes, per-env motor gains, stiffness actions (pybullet's setJointMotorControlArray
 * with POSITION_CONTROL / VELOCITY_CONTROL / TORQUE_CONTROL, its positionGains / velocityGains / forces arguments; the reference's
 * intended action space "a desired joint angle and stiffness", trex_env.py:30, trex_robot.py:399-401, 420). One motor row per joint
 * stays; a row is (target position, target velocity, kp, kd, max_force). With all modes POSITION, no gains and stiffness actions
 * off - the default - nothing of this exists: the kernels, rows and memory are the ones without it.
 *   - POSITION joint: action = target angle, clipped to the joint limits; target velocity 0; kp, kd, max_force from the gains
 *     where set, else the model parameters (motor_kp, motor_kd, motor_max_force);
 *   - VELOCITY joint: action = target velocity (rad/s), clipped to +- max_coordinate_velocity; the row has kp = 0: velocity
 *     error x kd, bounded by max_force. (pybullet's default velocityGain is 1; here the gain stays the joint's kd - set kd = 1
 *     for pybullet's default; unpinned: pybullet is not available to compare against);
 *   - TORQUE joint: action = torque (N m), clipped to +- the joint's max_force, added to the joint force on every substep of the
 *     env-step; the motor row is a null row. The observation's torque column and the energy penalty use the clipped command;
 *   - a reset's settle substep (trex_batch_reset / _reset_rows, the episode-limit reset inside a step launch) applies no motor
 *     and no commanded torque; resets, trex_batch_set_state and trex_batch_set_domain clear neither modes nor gains;
 *   - trex_batch_debug_step returns TREX_E_INVALID while any of the three is active.
 *   - the first call that activates any of the three allocates the batch-owned gains buffer and waits for the device once
 *     (hipDeviceSynchronize: not inside a stream capture); with stiffness actions the step launches also WRITE that buffer
 *     (the env-step's kp, kd), so two step launches of one batch must not run on two streams at the same time;
 *   - a batch with warm start (model parameter warmstart > 0) AND an active actuator model steps through the single-env launch
 *     form at every size (the rows are bitwise those of the pair form); trex_batch_launch_info reports that form.
 * While any of the three is active the step launches run separate kernel instantiations; after clearing all, the default ones. */
#define TREX_CTRL_POSITION 0   /* default */
#define TREX_CTRL_VELOCITY 1
#define TREX_CTRL_TORQUE   2
/* mode_host: J ints in observation order, a HOST array, shared by all envs (NULL = all POSITION). A value outside 0..2 returns
 * TREX_E_INVALID and changes nothing. */
int trex_batch_set_control_mode(TrexBatch *batch, const int32_t *mode_host);
/* Per env and joint, observation order, each [N, J] f32 device, each nullable = "the model parameter"; all three NULL clears.
 * Copied on `stream` into a batch-owned buffer (allocated at the first use of the actuator model: a batch that never uses it
 * allocates nothing). Values are not validated: a negative value is clamped to 0; a non-finite value (an infinite max_force
 * included) makes that env non-finite, and containment handles it (done = 1, reward 0, start pose - at every step while the
 * value stays); no other env is affected. The same holds for a non-finite torque action of a TORQUE joint. A buffer shorter
 * than N * J floats, host memory or another device's memory returns TREX_E_INVALID before anything is launched. */
int trex_batch_set_motor_gains(TrexBatch *batch, const float *kp_dev, const float *kd_dev,
                               const float *max_force_dev, void *stream);
/* enabled != 0: every action row is [2J]: J targets, then J stiffnesses kp, clipped to [0, kp_max]; kd = sqrt(2 kp)
 * (trex_robot.py:399-401: kp = 5e-3 gives the default kd = 0.1). They replace the gains' kp and kd for POSITION joints (max_force
 * stays the gains'); VELOCITY and TORQUE joints ignore their stiffness column. trex_batch_step, _step_rows, _step_many
 * ([S, N, 2J]) and _time_steps then expect action buffers of 2J columns. kp_max non-finite or < 0 returns TREX_E_INVALID. */
int trex_batch_set_stiffness_actions(TrexBatch *batch, int enabled, float kp_max);

/* Contact sensor: the floor-contact wrench per env and moving body (pybullet's getContactPoints(bodyA, linkIndexA) -
 * normalForce, lateralFriction1/2 - summed per link; no reference counterpart: foot-contact flags, contact rewards,
 * ground-reaction forces). enabled != 0: the step and reset launches record it (separate kernel instantiations); 0: they stop
 * (the default kernels again). The first enable allocates the batch-owned buffer, zeroed: a batch that never enables the
 * sensor allocates nothing, and the values are zero until the first launch that records. */
int trex_batch_set_contact_sensor(TrexBatch *batch, int enabled);

/* out_dev [N, num_bodies, 6] f32 device: fx fy fz (N), tx ty tz (N m) - world axes, force at the body's COM, torque about it
 * (the layout of trex_batch_set_external_wrench). TREX_E_INVALID while the sensor has never been enabled or is off.
 *   - the value: for each env and body, the MEAN floor-contact wrench over the solves since the env's last observation. For
 *     every contact point of the body, its final impulses lambda = (lambda_x, lambda_y, lambda_n) of the solve are summed as
 *     the world vector (lambda_x, lambda_y, lambda_n), and the moment (p - c) x lambda about the body's world COM c, p being
 *     the point the contact rows act at; the sums are divided by (number of solves x dt). This is the wrench the solver
 *     applied: with gravity and the external wrench it closes the momentum balance;
 *   - a stepped env averages the `substeps` solves of its env-step; an env that was reset - trex_batch_reset / _reset_rows
 *     (mask honoured: the other envs keep their values) or an episode-limit reset inside a step launch - reports its one
 *     settle substep, the state its observation shows (trex_batch_contact_stats reports the same substep); an env that
 *     containment put back reports zeros;
 *   - trex_batch_step, _step_rows, _time_steps and _step_many record it; _step_many reports the LAST of its S steps;
 *     with or without warmstart, an external wrench, a domain, primitive collision, in either launch form;
 *   - read-only: state, observations, rewards, done, penalties, contact_stats, the warm-start record and the episode counts
 *     are bitwise those of the same launches with the sensor off;
 *   - trex_batch_debug_step returns TREX_E_INVALID while the sensor is on; a buffer shorter than N * num_bodies * 6 floats,
 *     host memory or another device's memory returns TREX_E_INVALID before anything is launched. */
int trex_batch_contact_wrench(TrexBatch *batch, float *out_dev, void *stream);

/* ---- dynamics queries (pybullet's calculateInverseDynamics / calculateMassMatrix / calculateJacobian and what users derive from
 *      getLinkState(computeLinkVelocity=1); no reference counterpart: gravity compensation, computed-torque and operational-space
 *      controllers for TORQUE-mode joints, momentum / energy rewards, privileged critic inputs - without a host round trip)
 *
 * All four are asynchronous and ordered on `stream`, validate every device buffer like the other batch calls (host memory,
 * another device's memory or a short buffer returns TREX_E_INVALID before anything is launched), allocate nothing and never wait
 * for the device. The first call that sees a new caller buffer validates it with runtime queries, like every batch call; from
 * the second call on - once the buffers have been seen - the calls are plain kernel launches, usable inside a stream capture.
 * They read each env's current state and, once trex_batch_set_domain has set one, its per-env mass scale (mass and rotational
 * inertia of a body scale together). They write nothing but their outputs: state, observations, the warm-start record, the
 * contact sensor and the episode counts are untouched.
 *
 * Generalised velocity, D = 6 + J entries (31 for trex.urdf), in the order of the state vector: base linear velocity v(3) - of
 * the base frame origin - and base angular velocity w(3), both in world axes, then qd(J) in observation order. Accelerations are
 * the classical time derivatives of those (dv/dt is the acceleration of the base origin as a point, NOT the linear part of a
 * spatial acceleration). Forces are their duals: force on the base, torque on the base about the base frame origin, joint
 * torques. Relation to the CPU oracle (oracle/trex_oracle.c), checked in tests/test_dynamics_ref.py against oracle_get_state and
 * oracle_minv: the oracle orders its generalised velocity [w(3), v(3), joints in BODY order] about the same point - the base
 * origin, world axes - so the two differ by a permutation only: entries 0..2 <-> 3..5, and joint k here = body obs_order[k]
 * there. oracle_forward_dynamics already returns the classical base acceleration as [dw/dt, dv/dt] and qdd in observation order. */

/* force_dev [N, D] = M(q) a + h(q, qd) at every env's current state: the generalised force that produces the accelerations
 * accel_dev [N, D] (NULL = zeros: h alone). Gravity is the model parameter "gravity". RIGID-BODY terms only: joint damping,
 * "link_damping", motors, joint limits, contacts and external wrenches are NOT in it (pybullet's calculateInverseDynamics ignores
 * them too) - a joint's share of them is the caller's to add. accel NULL on a state at rest is the gravity-compensation force. */
int trex_batch_inverse_dynamics(TrexBatch *batch, const float *accel_dev, float *force_dev, void *stream);

/* M_dev [N, D, D]: the joint-space inertia matrix M(q), full and exactly symmetric (both triangles written, bitwise equal). */
int trex_batch_mass_matrix(TrexBatch *batch, float *M_dev, void *stream);

/* J_dev [N, 6, D]: rows 0..2 map the generalised velocity to the world linear velocity of the point fixed in URDF link `link`
 * at local_xyz (link frame; link indices and frames as trex_model_link_info and "link_tf"), rows 3..5 to the link's world angular
 * velocity. Link and point are HOST values shared by all envs. A link outside [0, num_links) or a non-finite point returns
 * TREX_E_INVALID. */
int trex_batch_jacobian(TrexBatch *batch, int link, const double local_xyz[3], float *J_dev, void *stream);

/* out_dev [N, 16]: [0,3) world position of the centre of mass, [3,6) its velocity, [6,9) linear momentum, [9,12) angular momentum
 * about the centre of mass, [12] kinetic energy, [13] potential energy sum m g z (z = 0 is the world origin), [14] total mass
 * (the env's mass scale included), [15] 0. World axes, SI units. */
int trex_batch_centroidal(TrexBatch *batch, float *out_dev, void *stream);

/* ---- the other direction (articulated-body algorithm, O(bodies) per env and right-hand side). Both calls use the conventions
 *      above - D, the order and the axes of the generalised velocity, classical accelerations, forces as duals, the env's mass
 *      scale, RIGID-BODY terms only - and behave like the four queries above: asynchronous on `stream`, every buffer validated,
 *      nothing allocated or waited for, nothing written but the output, plain launches from the second call on. The output may
 *      alias the input EXACTLY (in place); any other overlap is the caller's error and is not detected. */

/* accel_dev [N, D] = M(q)^-1 (force - h(q, qd)) at every env's current state: the exact inverse of trex_batch_inverse_dynamics.
 * force_dev [N, D] (NULL = zeros: free motion under gravity and the velocity-product forces). */
int trex_batch_forward_dynamics(TrexBatch *batch, const float *force_dev, float *accel_dev, void *stream);

/* x_dev [N, K, D] = M(q)^-1 applied to K right-hand sides per env, rhs_dev [N, K, D] (force-like rows; the layout of
 * trex_batch_jacobian's output, so solve_mass(J) is (M^-1 J^T)^T with K = 6). rhs_dev NULL: the identity, K must be D,
 * x = M^-1 itself. 1 <= K <= 64, otherwise TREX_E_INVALID. No gravity and no velocity terms enter: it depends on q alone. */
int trex_batch_solve_mass(TrexBatch *batch, const float *rhs_dev, int num_rhs, float *x_dev, void *stream);

/* ---- link kinematics (what users take from pybullet's getLinkState(computeLinkVelocity=1), and more: the acceleration of a
 *      task point - at zero generalised accelerations the bias acceleration Jdot qd of an operational-space controller - and the
 *      specific force an accelerometer on a link reads; no reference counterpart: foot velocities for slip penalties, body-frame
 *      foot positions for observations, IMUs - without a host round trip and without one Jacobian launch per link)
 *
 * The query behaves like the dynamics queries above: asynchronous and ordered on `stream`, every device buffer validated (host
 * memory, another device's memory or a short buffer returns TREX_E_INVALID before anything is launched), nothing allocated or
 * waited for, nothing written but the outputs (state, observations, the warm-start record, the contact sensor and the episode
 * counts are untouched), and from the second call with known buffers a plain kernel launch - ONE launch whatever the number of
 * probes - usable inside a single-stream capture. It uses their conventions: D, the order and the axes of the generalised
 * velocity, classical accelerations. The env's mass scale does not enter: this is kinematics. */
#define TREX_AXES_WORLD 0
#define TREX_AXES_LINK  1   /* each probe's own link frame */
#define TREX_AXES_BASE  2   /* URDF link 0's frame */

/* A probe = a point fixed in a URDF link: (link, local_xyz in the link frame; indices and frames as trex_model_link_info /
 * "link_tf", as in trex_batch_jacobian). link_host [num_probes] and local_xyz_host [num_probes, 3] are HOST arrays, shared by all
 * envs, validated here (link outside [0, num_links), non-finite point, set outside [0, 8), num_probes outside [0, 1024]:
 * TREX_E_INVALID, nothing changed) and copied into a batch-owned device table; a batch holds up to 8 sets. num_probes 0 frees the
 * set (the arrays may then be NULL). Synchronous: it waits for the device before it replaces or frees a set's table (not inside
 * a capture), like trex_batch_set_control_mode. */
int trex_batch_set_link_probes(TrexBatch *batch, int set, const int32_t *link_host, const double *local_xyz_host, int num_probes);

/* Kinematics of every probe of `set` at every env's current state. K = the set's size. Outputs f32 device, each nullable, not all:
 *   pose_dev         [N, K, 7]  position of the point xyz + orientation of the link frame, quaternion xyzw (w >= 0)
 *   velocity_dev     [N, K, 6]  linear velocity of the point, angular velocity of the link
 *   acceleration_dev [N, K, 6]  classical linear acceleration of the point (d2p/dt2), angular acceleration of the link,
 *                               at the generalised accelerations accel_dev [N, D] (conventions of the dynamics queries);
 *                               accel_dev NULL = zeros: the bias acceleration Jdot qd. accel_dev is read only when
 *                               acceleration_dev is given.
 * axes: the axes the velocity and acceleration 3-vectors are expressed in. They stay velocities / accelerations relative to
 *   the WORLD; only their components change. pose_dev is the world pose for WORLD and LINK (for a probe at its link's origin,
 *   the link's row of trex_batch_link_transforms); for BASE it is the pose relative to URDF link 0's frame (position in its axes
 *   from its origin, orientation base^-1 o link).
 * proper != 0: the linear acceleration has +g z (world) added before it is expressed in `axes`: the specific force an
 *   accelerometer at the point reads; a body at rest reads (0, 0, g) in world axes. g = the model parameter "gravity".
 * An empty or never-set probe set, a set outside [0, 8), axes outside 0..2 or all three outputs NULL return TREX_E_INVALID.
 * Non-finite state values are not an error: they give non-finite outputs for that env only. The common outputs of a pose-only, a
 * pose + velocity and a full call are bitwise equal (the smaller calls run kernels that read neither qd nor accel_dev). */
int trex_batch_link_state(TrexBatch *batch, int set, int axes, int proper, const float *accel_dev,
                          float *pose_dev, float *velocity_dev, float *acceleration_dev, void *stream);

/* ---- proximity between bodies (what users take from pybullet's getClosestPoints between links of the robot: a self-collision
 *      penalty or termination, leg-to-leg and tail-to-leg clearance as an observation, a filter on sampled poses; the step itself
 *      collides the bodies with the floor only)
 *
 * Geometry: capsules fixed in bodies - the primitive trex_model_fit_hull_primitives fits to the hulls; a sphere is a capsule of
 * length 0. The distance of two capsules is closed-form (segment to segment, minus the radii): no iteration.
 *
 * The table, one per batch: body_host [C] the body of each capsule, capsule_host [C, 7] = p0 xyz, p1 xyz, radius in that body's
 * frame (the layout of trex_model_fit_hull_primitives), pair_host [P, 2] the bodies (A, B) of each pair to report. HOST arrays,
 * shared by all envs, validated here and copied into batch-owned device memory. TREX_E_INVALID with nothing changed: C outside
 * [0, 256] or P outside [1, 1024]; a body outside [0, num_bodies); a non-finite coordinate, a non-finite or negative radius; a
 * pair with A == B; a pair one of whose bodies has no capsule; more than 65536 capsule-pair tests in all (the sum over the pairs
 * of capsules(A) x capsules(B)). A capsule with |p1 - p0|^2 < 1e-12 m^2 is stored as a sphere (p1 = p0); coordinates are rounded
 * to f32. num_capsules 0 frees the table (the arrays may then be NULL). Synchronous: it waits for the device before it replaces
 * or frees the table (not inside a capture), like trex_batch_set_link_probes. */
int trex_batch_set_proximity_shapes(TrexBatch *batch, const int32_t *body_host, const double *capsule_host, int num_capsules,
                                    const int32_t *pair_host, int num_pairs);

/* For every env and pair: the closest capsule of A and capsule of B at the env's current state. With a on the axis of A's capsule
 * and b on the axis of B's realising the smallest segment-to-segment distance:
 *   normal_dev   [N, P, 3]  n = (a - b) / |a - b|: from B to A (pybullet's contactNormalOnB); (0, 0, 1) where |a - b| < 1e-6 m
 *                           (crossing axes, concentric spheres) - the points and the distance follow the same formulas there
 *   distance_dev [N, P]     |a - b| - rA - rB: negative when the capsules overlap, then the depth. Required.
 *   point_a_dev  [N, P, 3]  a - rA n, on A's surface, world coordinates
 *   point_b_dev  [N, P, 3]  b + rB n, on B's surface: (point_a - point_b) . n = distance
 *   capsule_dev  [N, P, 2]  i32: the table index of the winning capsule of A, of B
 * Every output but distance_dev is nullable. Among capsule pairs of equal distance the one earlier in (capsule of A, capsule of B)
 * table order wins; two calls on the same state are bitwise equal; the row of a pair does not depend on which other pairs the
 * table holds, the row of an env not on N. There is no distance threshold: every pair of the table is reported.
 * It behaves like the queries above: asynchronous and ordered on `stream`, every device buffer validated (TREX_E_INVALID before
 * anything is launched), nothing allocated or waited for, nothing written but the outputs, from the second call with known
 * buffers ONE plain kernel launch, usable inside a single-stream capture. TREX_E_INVALID when no table is set or distance_dev is
 * NULL. A non-finite state makes that env's distances, points and normals unspecified - its capsule_dev entries still name
 * capsules of the pair's bodies - and leaves every other env bitwise as without it. */
int trex_batch_proximity(TrexBatch *batch, float *distance_dev, float *point_a_dev, float *point_b_dev, float *normal_dev,
                         int32_t *capsule_dev, void *stream);

/* ---- floor clearance per body, and fall termination inside the step (no reference counterpart: the reference's
 * should_terminate() is constant False, trex_env.py:183-184). One kernel (csrc/termination.hip) serves both.
 *
 * trex_batch_body_clearance: for every env and body b, at the env's current state,
 *   clearance_dev [N, num_bodies]     min over the body's collision points of (world z - support radius) - floor_z, metres:
 *                                     how high the lowest point of the body stands above the floor; negative = it is that deep
 *                                     in it. Required. +inf for a body without collision points.
 *   lowest_dev    [N, num_bodies, 3]  world position of that lowest point, the radius subtracted along z (so that its z - floor_z
 *                                     is the clearance, up to rounding); NaN for a body without points. Nullable.
 * The collision points are what the physics collides with: the hull vertices (radius 0), or after
 * trex_model_use_primitive_collision the sphere centres / capsule ends with their radii. The query is exact over them - every
 * point of every body is evaluated, no bounding volume decides anything; among points of equal height the one earlier in the
 * model's order is reported. It behaves like the dynamics queries: read-only, asynchronous and ordered on `stream`, every device
 * buffer validated (TREX_E_INVALID before anything is launched), nothing allocated or waited for, from the second call with known
 * buffers ONE plain kernel launch, usable inside a single-stream capture. A non-finite state makes that env's row unspecified
 * and leaves every other env bitwise as without it.
 *
 * trex_batch_set_termination: end an env's episode when the robot falls, decided on the device after every env-step.
 *   head_height_min   criterion 1 (TREX_TERM_HEAD): the head point (trex_batch_head_position) is lower than this above floor_z
 *   tilt_max_rad      criterion 2 (TREX_TERM_TILT): the base is tipped further than this from its start orientation, in (0, pi]:
 *                     cos(tilt) = z component of R_base R_start^-1 e_z, 1 at the start orientation, compared with cos(tilt_max_rad)
 *   clear_min_host    criterion 3 (TREX_TERM_CLEARANCE) [num_bodies], host: a watched body's clearance is below its entry. NaN = the
 *                     body is not watched; NULL = none is. With the model's contact_margin as the entry the criterion reads "a body
 *                     that is not a foot touches the floor". Copied.
 *   penalty           subtracted, once, from the reward of the step in which an env terminates
 * A NaN head_height_min / tilt_max_rad switches that criterion off; all three off = the feature off: the step calls are again
 * exactly what they are for a batch that never enabled it (same launches, same results). TREX_E_INVALID, nothing changed: an
 * infinite head_height_min, a tilt_max_rad that is neither NaN nor in (0, pi], a non-finite penalty. Comparisons are strict (<).
 *
 * While a criterion is on, trex_batch_step and trex_batch_step_rows enqueue THREE launches on `stream`:
 *   1. the step launch, exactly as without termination (every feature mix, either launch form; trex_batch_launch_info unchanged);
 *   2. the predicate launch: per env values[0] = head z - floor_z, values[1] = cos(tilt), values[2] = min over the watched bodies of
 *      clearance - clear_min (+inf: none watched); the reason bits of the criteria that fire; for an env with reason != 0: done = 1
 *      in the done bytes and in the done column / array, wherever the step launch wrote them, reward -= penalty, and its
 *      observation row - the last of the episode - copied to the batch's terminal-observation buffer. An env that the step launch
 *      itself ended (done already 1: the episode limit, a contained non-finite env) is on its new episode's state and is NOT judged:
 *      reason 0, reward and done untouched (its values are still written, from the state it is in). A trex_batch_step call
      without obs_dev keeps no terminal observation; one without done_dev has the step launch write its done flags to a buffer
      of the batch's, so that the predicate can tell;
 *   3. the reset launch of trex_batch_reset with reason != 0 as its mask, writing observations only: the env is put to the start
 *      pose, motors off, one un-actuated settle substep, episode count 0, warm-start record emptied, the contact sensor (if on)
 *      recording the settle substep; its observation row is the first of the new episode; reward and done stay as 1 and 2 left
 *      them. (For the other envs it rewrites the q, qd columns with the values they hold, as trex_batch_reset does.)
 * No host decision is made and nothing is waited for: the three launches run whether or not an env terminates, and a linear
 * single-stream capture of step calls may hold them from the second call on. trex_batch_step_many performs num_steps such
 * triplets from the host; its results stay bitwise those of num_steps trex_batch_step_rows calls. trex_batch_time_steps and
 * trex_batch_debug_step return TREX_E_INVALID while termination is on.
 * The first enabling call allocates the batch's buffers (mask, reasons, values, terminal observations) and may wait for the
 * device once: not inside a capture. A batch that never enables termination allocates nothing and launches nothing new.
 * With termination on the step calls WRITE batch-owned memory: two step calls of one batch must not run on two streams at once
 * (as with stiffness actions).
 *
 * trex_batch_termination_info: device-to-device copies, ordered on `stream`, of what the LAST step call left: reason_dev [N] i32,
 * values_dev [N, 3], terminal_obs_dev [N, 3J] - the row of an env is the observation of its most recent termination (zeros
 * before the first). Each nullable. TREX_E_INVALID for a batch that never enabled termination. */
#define TREX_TERM_HEAD 1
#define TREX_TERM_TILT 2
#define TREX_TERM_CLEARANCE 4
int trex_batch_body_clearance(TrexBatch *batch, float *clearance_dev, float *lowest_dev, void *stream);
int trex_batch_set_termination(TrexBatch *batch, float head_height_min, float tilt_max_rad, const float *clear_min_host,
                               float penalty);
int trex_batch_termination_info(TrexBatch *batch, int32_t *reason_dev, float *values_dev, float *terminal_obs_dev, void *stream);

/* ---- inverse kinematics (pybullet's calculateInverseKinematics / calculateInverseKinematics2; no reference counterpart: foot
 *      placement as a task-space action, reference poses for resets and imitation rewards, posing the head or tail)
 *
 * Joint angles that bring the probes of `set` (trex_batch_set_link_probes: K task points, 1 <= K <= 8) to per-env targets, by
 * damped least squares, every env in ONE launch that stays resident for all iterations. The base pose of every env is its current
 * one and stays fixed; only joint angles are solved for. Several targets are solved together.
 *   mode_host  [K]        HOST: 1 = the position of the point, 2 = the orientation of the link frame, 3 = both. Task rows
 *                         M = 3 per position + 3 per orientation, M <= 24, in probe order, a probe's position rows first.
 *   frame                 TREX_AXES_WORLD, or TREX_AXES_BASE: targets relative to URDF link 0's frame, as trex_batch_link_state
 *                         defines its BASE pose (link 0 must belong to the base body, which every root link does).
 *   target_dev [N, K, 7]  xyz + quaternion xyzw per env and target; the quaternion is normalised here, the parts a mode does not
 *                         use are ignored (they may be NaN).
 *   q_init_dev [N, J]     where the solve starts, observation order; NULL = the env's current joint angles.
 *   joint_mask            bit k set: joint k (observation order) may move. The other joints come back bitwise as they went in.
 *   params                NULL = the defaults of TREX_IK_DEFAULTS.
 *   q_out_dev  [N, J]     the result; may be q_init_dev itself (no other overlap).
 *   info_dev   [N, 4]     nullable: [0] the largest position error |p_target - p| over the position targets at q_out, metres;
 *                         [1] the largest orientation error at q_out, radians; [2] the iterations run; [3] the Euclidean norm
 *                         of the stacked error e at the start (q_init with the moving joints clamped to their limits).
 * Per env, with q = q_init, the moving joints clamped to [lower, upper], and then `iterations` times:
 *   forward kinematics at q; the error e [M]: p_target - p for a position, 2 sign(w) (x, y, z) of quat_target o quat_link^-1
 *   for an orientation (sign(0) = +1; the rotation vector for small angles), world axes; the residuals: the largest |p_target - p|
 *   and the largest 2 asin(min(1, |(x, y, z)|)); stop if a tolerance is positive and both residuals are at or below theirs;
 *   A [M, J]: the joint columns of the point Jacobians (a_j x (p - r_j) and a_j for the joints on the probe's chain, zero
 *   elsewhere and for joints that may not move); lambda2 = damping^2 + gain |e|^2; (A A^T + lambda2 I) x = e by Cholesky, a
 *   pivot that is not positive replaced by lambda2; dq = A^T x, scaled as a whole so that max |dq| <= max_step;
 *   q = clamp(q + dq, lower, upper) for the moving joints.
 * The residuals of info_dev are evaluated at q_out by one more pass of kinematics.
 * It behaves like the link kinematics query: read-only (state, observations, the warm-start record, the contact sensor and the
 * episode counts are untouched; the env's mass scale does not enter), asynchronous and ordered on `stream`, every device buffer
 * validated before anything is launched, nothing allocated or waited for, from the second call with known buffers ONE plain
 * kernel launch whatever K and `iterations` are, usable inside a single-stream capture. An env's arithmetic does not depend on N,
 * on its place in the batch or on the other envs: the same inputs give bitwise the same row. TREX_E_INVALID, nothing launched: a
 * set outside [0, 8), empty or larger than 8 probes; a mode outside 1..3; M > 24; a frame other than the two; a joint_mask
 * without a bit among the J joints; iterations outside 1..256; a negative or non-finite parameter; a NULL target or output.
 * A non-finite target or q_init value gives non-finite q_out (the moving joints) and info for that env only. */
#define TREX_IK_POSITION 1
#define TREX_IK_ORIENTATION 2
#define TREX_IK_MAXPROBES 8
#define TREX_IK_MAXROWS 24
typedef struct TrexIkParams {
  int32_t iterations;   /* 1..256 */
  float damping;        /* lambda2 = damping^2 + gain |e|^2 */
  float gain;
  float max_step;       /* largest joint step of one iteration, rad */
  float tol_pos;        /* metres; 0 with tol_ori 0: never stop early */
  float tol_ori;        /* radians */
} TrexIkParams;
#define TREX_IK_DEFAULTS {20, 0.01f, 0.1f, 0.2f, 0.0f, 0.0f}
int trex_batch_inverse_kinematics(TrexBatch *batch, int set, const int32_t *mode_host, int frame, const float *target_dev,
                                  const float *q_init_dev, uint32_t joint_mask, const TrexIkParams *params, float *q_out_dev,
                                  float *info_dev, void *stream);

/* ---- observation channels (no reference counterpart: the reference's observation is [q | qd | torque] alone): what the base does
 * - its tilt, velocity and height -, where points of the robot are and whether a foot presses on the floor, as extra columns of
 * the row a policy reads. The step and reset calls keep writing their own rows; ONE more launch composes the extended row
 *   out row e = rows row e [0, 3J) | the E channel columns | rows row e [3J, 3J + tail)
 * with tail = 2 (reward, done), or 5 with trex_batch_set_penalties_in_rows. Every channel is evaluated at the batch's CURRENT state:
 * after a step the post-step state, and for an env the launch reset the new episode's - the instant of the 3J columns beside them.
 *
 * A channel: kind, link (URDF link index where the kind names one), local_xyz (a point in that link's frame) and scale - every
 * value of the channel is multiplied by it. "Base axes" are TREX_AXES_BASE of the link kinematics: URDF link 0's frame.
 *   PROJECTED_GRAVITY      3  world (0, 0, -1) in base axes
 *   BASE_LINEAR_VELOCITY   3  of the origin of URDF link 0, in base axes
 *   BASE_ANGULAR_VELOCITY  3  in base axes
 *   BASE_HEIGHT            1  world z of the origin of URDF link 0 - floor_z
 *   POINT_POSITION         3  the point local_xyz of `link` relative to the origin of URDF link 0, in base axes: the pose xyz of
 *                             the link kinematics query with TREX_AXES_BASE
 *   POINT_VELOCITY         3  its linear velocity in base axes, as that query reports it
 *   POINT_HEIGHT           1  its world z - floor_z
 *   CONTACT_FORCE          1  fz of the contact sensor for the body of `link` (needs trex_batch_set_contact_sensor on)
 *   PREV_ACTION            A  the env's row of actions_dev as passed (not clipped); zeros when actions_dev is NULL and for an env
 *                             whose done column in `rows` is non-zero: a new episode has no previous action
 *   EXTERNAL        link = k  the next k >= 1 columns of the env's row of extern_dev, copied: ray fractions, distances, anything
 *                             the caller computed joins the row in the same launch
 * At most 64 channels, and 3J + E <= 512. */
#define TREX_OBS_PROJECTED_GRAVITY 0
#define TREX_OBS_BASE_LINEAR_VELOCITY 1
#define TREX_OBS_BASE_ANGULAR_VELOCITY 2
#define TREX_OBS_BASE_HEIGHT 3
#define TREX_OBS_POINT_POSITION 4
#define TREX_OBS_POINT_VELOCITY 5
#define TREX_OBS_POINT_HEIGHT 6
#define TREX_OBS_CONTACT_FORCE 7
#define TREX_OBS_PREV_ACTION 8
#define TREX_OBS_EXTERNAL 9
#define TREX_OBS_KINDS 10
typedef struct TrexObsChannel {
  int32_t kind, link;
  float local_xyz[3];
  float scale;
} TrexObsChannel;
/* Set the batch's channels (host values, copied; synchronises the device; replaces the previous set); num_channels 0 clears.
 * extra_dim_out (nullable) <- E. TREX_E_INVALID, nothing changed: an unknown kind, a link out of range, a local_xyz or scale that
 * is not finite, k < 1, more than 64 channels, 3J + E > 512. PREV_ACTION takes the batch's action width of this moment: set the
 * channels after trex_batch_set_stiffness_actions. */
int trex_batch_set_observation(TrexBatch *batch, const TrexObsChannel *channels_host, int num_channels, int *extra_dim_out);
/* 3J + E; 3J while no channels are set */
int trex_batch_observation_dim(const TrexBatch *batch);
/* Compose the extended rows (above) of all N envs into out_rows_dev (row e at + e * out_stride, out_stride >= 3J + E + tail) from
 * rows_dev (what a step or reset call wrote; row_stride >= 3J + tail), actions_dev [N, A] (nullable) and extern_dev (row e at
 * + e * extern_stride; nullable unless an EXTERNAL channel is set, extern_stride >= the sum of their widths). One launch,
 * asynchronous on `stream`, capturable from the second call with the same buffers on. Reads the state, the contact sensor and its
 * arguments; writes the 3J + E + tail columns of every out row and nothing else. TREX_E_INVALID, nothing launched: no channels
 * set, a stride too small, a CONTACT_FORCE channel with the sensor off, a missing or short buffer, host memory, out_rows_dev
 * overlapping rows_dev, an action width that is no longer the one the channels were set with. */
int trex_batch_compose_rows(TrexBatch *batch, const float *rows_dev, int row_stride, const float *actions_dev,
                            const float *extern_dev, int extern_stride, float *out_rows_dev, int out_stride, void *stream);

/* diagnostics of the last substep: contact count per env [N] i32 (nullable), summed normal
 * impulse per env [N] f32 (nullable). */
int trex_batch_contact_stats(TrexBatch *batch, int32_t *count_dev, float *normal_impulse_dev, void *stream);

/* Diagnostics for the parity tests: one step like trex_batch_step, additionally dumping env 0's
 * intermediates of its LAST substep into debug_dev (4096 f32 device): [0,32) qdd per body lane,
 * [32,38) base spatial acceleration, [64,96) generalised velocity before the constraint solve
 * per dof lane, [96,128) its PGS correction, [128] contact count, [129] limit-row mask,
 * [160,960) the 25 joint columns of M^-1, [960+16c ..) per contact body,x,y,z,dist,1/diag(3),rhs(3),
 * lambda(3), [1216+32(3c+a) ..) the contact rows' response vectors. Not part of the product path. */
int trex_batch_debug_step(TrexBatch *batch, const float *actions_dev, float *obs_dev, float *debug_dev, void *stream);

/* Launch geometry + bytes, for bench.py: fills grid, block, lds bytes, algorithmic bytes/env-step. block = 128 means the
 * pair form of the step launch (two envs = two wavefronts per workgroup: even batches of at most 4096 envs), 64 the
 * single-env form. */
int trex_batch_launch_info(const TrexBatch *batch, int *grid, int *block, int *lds_bytes,
                           int *alg_bytes_per_env_step);

/* Times `steps` trex_batch_step launches with hipEvents on `stream` (the stream the kernels run on)
 * and returns the average per-launch duration in milliseconds. */
int trex_batch_time_steps(TrexBatch *batch, const float *actions_dev, float *obs_dev, float *reward_dev,
                          uint8_t *done_dev, int steps, void *stream, float *avg_ms_out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
/* The reward terms of a batch - a specification of terms, one launch per step that composes them into the reward column of
 * the rows a step call wrote - are declared in a header of their own, with the conventions above: */
#include "trex_reward.h"
/* So is the motion clip of a batch - reference poses that depend on time, tracking terms against them, and resets to an instant of
 * the clip: */
#include "trex_motion.h"
/* So is the sensor model of a batch - noise, bias, resolution and latency on the observation columns of the row the policy reads,
 * latency on the actions: */
#include "trex_sensing.h"
/* So is the episode randomisation of a batch - mass scale, friction, motor gains, pushes and the velocity command, redrawn on the
 * device when an episode starts or at an interval inside it: */
#include "trex_randomize.h"
/* So is the start-state randomisation of a batch - the state an episode starts in, perturbed on the device and placed on the
 * floor, the counterpart of the episode randomisation: */
#include "trex_start_state.h"
/* So is the episode monitor of a batch - the return, the length and the end reason of every finished episode, the window of the
 * last W of them and its summary, kept on the device: */
#include "trex_monitor.h"
/* So are the first-order derivatives of the inverse dynamics along the configuration tangent and the generalised velocity, a
 * read-only query beside the dynamics queries: */
#include "trex_dynamics_derivatives.h"
/* So is the joint force/torque sensor - the 6-D wrench every joint transmits, a read-only query beside the dynamics queries - and
 * the generalised velocity with its backward difference: */
#include "trex_joint_wrench.h"

#endif /* TREX_BATCH_H */
