// The tables the kernels read and the layouts of the per-env state they write, as pure host arithmetic: everything the C-ABI computes
// between its argument checks and its HIP calls.
// INCLUDE RULE: this unit includes model.hpp, device_model.h, proximity_limits.h, observation_limits.h, reward_limits.h, motion_limits.h, sensing_limits.h, start_state_limits.h, policy_limits.h, planner_limits.h, symmetry_limits.h and include/trex_batch.h, and nothing of HIP; it makes
// no HIP call and knows no batch. It builds with plain g++ -std=c++17, as model.cpp does, so that tests/host/tables_harness.cpp runs
// it under the sanitizers on a machine without a GPU. A refusal is a thrown Refusal whose text is the C-ABI's message, whole.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/trex_batch.h"
// device_model.h names float4 in one pointer member and includes nothing for it: a unit that has the HIP runtime has the type, a
// plain C++ unit declares the name (such a unit must not include the HIP runtime afterwards)
#ifndef HIP_INCLUDE_HIP_AMD_DETAIL_HIP_VECTOR_TYPES_H
struct float4;
#endif
#include "device_model.h"
#include "model.hpp"
#include "motion_limits.h"
#include "observation_limits.h"
#include "planner_limits.h"
#include "policy_limits.h"
#include "proximity_limits.h"
#include "reward_limits.h"
#include "sensing_limits.h"
#include "start_state_limits.h"
#include "symmetry_limits.h"

namespace trex {

struct Refusal : std::runtime_error {
  int code;
  explicit Refusal(const std::string &msg, int c = TREX_E_INVALID) : std::runtime_error(msg), code(c) {}
};

void fill_device_model(const HostModel &h, TrexDeviceModel &d);

// The byte extent of n rows of `width` floats, `stride` floats apart: the last row ends at its width, not at its stride (n 1:
// width * 4 whatever the stride). Formed in size_t. The caller has refused a stride below the width.
size_t row_block_bytes(size_t n, int stride, int width);
// true when the byte ranges [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb);
// a batch of n envs whose env 0 has the global index env_offset: every global index fits 32 bits. who: the call, for the refusal
void check_env_offset(const std::string &who, uint32_t env_offset, int n_envs);

// The layout of ONE allocation that holds a piece of per-env state: the members in the order they were taken, each at the first
// multiple of its alignment behind the one before, and the bytes of the whole. Every state layout below is built with take(), so
// it lists its own members: what tests/host/layout_check.hpp walks. A layout is computed from counts alone; the HIP units
// allocate `bytes` and point into the allocation once.
struct Layout {
  struct Member { const char *name; size_t at, bytes, align; };
  std::vector<Member> members;
  size_t bytes = 0;
  size_t take(const char *name, size_t member_bytes, size_t align);   // the member's offset
};
// trex_batch_set_reward: the history of the terms - previous actions [n][A] | previous qd [n][J] | timers [n][T] | held values
// [n][T] | valid flags [n]. T 0 gives the empty layout (bytes 0).
struct RewardHistLayout : Layout { size_t prev_act = 0, prev_qd = 0, timer = 0, held = 0, valid = 0; };
RewardHistLayout reward_hist_layout(int n, int A, int J, int T);
// trex_batch_set_motion: the clocks - start times [n] f32 | step counts [n] i32
struct MotionClockLayout : Layout { size_t t0 = 0, k = 0; };
MotionClockLayout motion_clock_layout(int n);
// trex_batch_set_motion_reward: the held values [n][T]. T 0 gives the empty layout.
Layout motion_held_layout(int n, int T);
// trex_batch_set_sensing: the counters - episode counts [n] u32 | row counts [n] u32 | started flags [n] u32 | drawn delays [n][G]
// i32. trex_batch_set_action_delay: the same with G = 1. G 0 gives the empty layout.
struct SenseCounterLayout : Layout { size_t ep = 0, k = 0, started = 0, delay = 0; };
SenseCounterLayout sense_counter_layout(int n, int G);
// the history of the delayed columns [TREX_SENSE_SLOTS][n][cols] f32: cols is the table's `delayed` (sensing) or the action
// width (action delay). cols 0 gives the empty layout.
Layout sense_hist_layout(int n, int cols);
// trex_batch_set_randomization: the state, in the order of TrexRandState (randomize.h), each member [n] outermost - ep | k |
// started | off [P] | push_left [P] | push_force [P][3] | push_base [P][6] | values [T][TREX_TL]. T 0 gives the empty layout.
struct RandStateLayout : Layout { size_t ep = 0, k = 0, started = 0, off = 0, push_left = 0, push_force = 0, push_base = 0, values = 0; };
RandStateLayout rand_state_layout(int n, int T, int P);
// trex_batch_set_start_state: the state, in the order of TrexStartState (start_state.h), each member [n] outermost - ep | started |
// shift | lowest | values [T][TREX_TL]. T 0 gives the empty layout.
struct StartStateLayout : Layout { size_t ep = 0, started = 0, shift = 0, lowest = 0, values = 0; };
StartStateLayout start_state_layout(int n, int T);

// rotation row-major (9) | translation (3): the [12] layout of every transform a kernel reads
void tf12(const Tf &t, float out[12]);

// every URDF link: the body it was merged into and its frame in that body's frame (HostModel::link_body / link_tf)
struct Links { std::vector<int> body; std::vector<Tf> tf; };
// a point given in a link's frame, in the frame of the link's body
struct LinkPoint { int body; float point[3]; };
LinkPoint link_point(const Links &links, int link, const double local_xyz[3]);

// trex_batch_set_link_probes: body [K], and body <- link rotation (9) | the point in the body frame (3) [K][12]
struct ProbeTable { std::vector<int32_t> body; std::vector<float> tf; };
ProbeTable build_probe_table(const Links &links, const int32_t *link, const double *local_xyz, int num_probes);

// trex_batch_set_proximity_shapes: ONE blob, every part at a multiple of 16 bytes - capsules [C][8] at 0, their bodies [C] at
// o_body, the TREX_PROX_TEST words [T] in (pair, capsule of A, capsule of B) order at o_test, each pair's first test [P] at o_first.
// num_capsules 0 gives the empty table.
struct ProxTable {
  int caps = 0, pairs = 0, tests = 0;
  size_t o_body = 0, o_test = 0, o_first = 0;
  std::vector<char> blob;
};
ProxTable build_prox_table(int nb, const int32_t *body, const double *capsule, int num_capsules, const int32_t *pair, int num_pairs);

// trex_batch_inverse_kinematics: per probe its body, mode, first task row and chain mask (bit b: body b is the probe's body or an
// ancestor of it, the base excluded); the joints that may move, by body lane; the parameters, checked, damping squared
struct IkTask {
  uint8_t body[TREX_IK_MAXPROBES] = {}, mode[TREX_IK_MAXPROBES] = {}, row0[TREX_IK_MAXPROBES] = {};
  uint32_t chain[TREX_IK_MAXPROBES] = {};
  uint32_t move_mask = 0u;
  int rows = 0, iterations = 0;
  float damping2 = 0.f, gain = 0.f, max_step = 0.f, tol_pos = 0.f, tol_ori = 0.f;
};
IkTask build_ik_task(const std::vector<int32_t> &probe_body, const std::vector<int> &parent, const std::vector<int> &obs_order,
                     const int32_t *mode, uint32_t joint_mask, const TrexIkParams *params);

// trex_batch_set_observation: ONE blob - the channels [C] as TrexObsChan at 0, then at o_col, a multiple of 16 bytes, the channel
// of every extra column [E] as a byte: column 3J + c of the composed row belongs to channel col_chan[c]. nj, action_cols: the
// batch's J and the width of its action rows (what PREV_ACTION copies). num_channels 0 gives the empty table.
struct ObsTable {
  int channels = 0, extra = 0;          // C, E
  int extern_cols = 0;                  // the sum of the EXTERNAL channels' widths: the columns read of a row of extern_dev
  int action_cols = 0;                  // the action width the table was built with
  bool contact = false, actions = false;   // a CONTACT_FORCE / PREV_ACTION channel is set
  uint32_t body_mask = 0u;              // bit b: a channel names body b (the body of URDF link 0 not included)
  size_t o_col = 0;
  std::vector<char> blob;
};
ObsTable build_obs_table(const Links &links, int nj, int action_cols, const TrexObsChannel *channels, int num_channels);

// trex_batch_set_reward: ONE blob - the terms [T] as TrexRewTerm at 0, then at o_joint, a multiple of 16 bytes, the body lane of
// every joint in observation order [32] as int32 (what the kernel's lane j reads the limits and the start angle of joint j by).
// obs_order: observation slot -> body; nb: the body count; action_cols: the width of the batch's action rows (what ACTION_RATE
// sums over). num_terms 0 gives the empty table.
struct RewTable {
  int terms = 0;                        // T
  int action_cols = 0;                  // the action width the table was built with
  bool contact = false, actions = false, command = false;   // a contact kind / ACTION_RATE / a tracking term is set
  uint32_t body_mask = 0u;              // bit b: a term names body b (the body of URDF link 0 not included)
  size_t o_joint = 0;
  std::vector<char> blob;
};
RewTable build_reward_table(const Links &links, const std::vector<int> &obs_order, int nb, int action_cols, const TrexRewardTerm *terms,
                            int num_terms);

// trex_batch_set_motion: the clip as the kernels read it - F rows of TREX_MOT_STRIDE(J) floats, the state layout of
// trex_batch_get_state in f32 (quaternions normalised and brought into one hemisphere frame after frame, velocities as given or
// derived in f64: include/trex_motion.h) - and the f32 constants of the time mapping. q_lower, q_upper: by body; obs_order:
// observation slot -> body. num_frames 0 gives the empty table.
struct MotionTable {
  int frames = 0, nj = 0, stride = 0;
  bool loop = false;
  float frame_dt = 0.f, inv_dt = 0.f, duration = 0.f, inv_duration = 0.f;   // dt, 1 / dt, T = (F - 1) dt, 1 / T
  float disp[2] = {0.f, 0.f};                                               // pos[F-1] - pos[0], x and y
  std::vector<float> rows;
};
MotionTable build_motion_table(const std::vector<double> &q_lower, const std::vector<double> &q_upper, const std::vector<int> &obs_order,
                               const double *frames, const double *velocities, int num_frames, double frame_dt, int loop);
// trex_batch_set_motion_reward: the terms checked and as the kernel reads them (a mask of 0 as all J bits). has_probes: the clip
// names end effectors.
std::vector<TrexMotTerm> build_motion_terms(int nj, bool has_probes, const TrexMotionTerm *terms, int num_terms, float step_weight);

// trex_batch_set_sensing: the groups checked and as the kernel reads them, the column -> group map and the packing of the delayed
// columns (those of a group with delay_max > 0, in column order: the rows of the history), and the blob the device holds, laid out
// as sensing_limits.h says. obs_dim: 3J + E, the columns a group may cover. num_groups 0 gives the empty table.
struct SenseTable {
  int groups = 0, obs_dim = 0, delayed = 0;
  std::vector<TrexSenseGrp> group;
  std::vector<int16_t> col_group, col_hist;
  size_t o_col_group = 0, o_col_hist = 0;
  std::vector<char> blob;
};
SenseTable build_sense_table(int obs_dim, const TrexSenseGroup *groups, int num_groups);
// trex_batch_set_action_delay, and the delays of a group: the range checked
void check_sense_delay(const std::string &who, int delay_min, int delay_max);

// trex_batch_set_randomization: the terms checked and as the kernel reads them - a mask of 0 as all the model's bodies (MASS) or
// joints (KP, KD, MAX_FORCE), FRICTION and COMMAND as element 0 alone, PUSH as no element -, push_slot[t]: the index of term t
// among the PUSH terms, -1 for another kind; what the terms need of the batch. nb, nj: the model's bodies and joints; stiffness:
// stiffness actions are on. num_terms 0 gives the empty table.
struct RandTable {
  int terms = 0, pushes = 0;
  std::vector<TrexRandomTerm> term;
  int push_slot[TREX_RAND_MAXTERMS];
  bool mass = false, friction = false, gains = false, command = false;
};
RandTable build_random_table(int nb, int nj, bool stiffness, const TrexRandomTerm *terms, int num_terms);

// trex_batch_set_start_state: the terms checked and as the kernel reads them (TrexStartTable, start_state_limits.h) - a joint mask
// of 0 as all the model's joints, a base kind and FLOOR_CLEARANCE as element 0 alone, shared as 0 / 1 -, whether a BASE_RPY term
// is among them and which term is the FLOOR_CLEARANCE one (-1: none). nj: the model's joints. num_terms 0 gives the empty table.
TrexStartTable build_start_table(int nj, const TrexStartTerm *terms, int num_terms);
// trex_batch_apply_start_state: the arguments against the table and the row's width; the pointers as "is it there" flags
void check_start_apply(int num_terms, bool done, int done_stride, bool rows, int row_stride, int nj, bool pen_in_rows);

// trex_batch_set_monitor: the shape checked, the team of lanes an env takes in the accumulate launch (the smallest power of two
// that holds the C columns, at least 1), the workgroups of that launch, and the layout of the ONE allocation that is the
// monitor's state - byte offsets, 8-byte members first, in the order of TrexMonState (monitor.h). block: the lanes of an
// accumulate workgroup. window 0 gives the empty layout (bytes 0).
struct MonitorLayout : Layout {
  int window = 0, cols_a = 0, cols_b = 0, cols = 0, team = 1, groups = 0;
  size_t ret = 0, col = 0, total = 0, by_reason = 0, len = 0, episodes = 0, fin = 0, last_return = 0, last_length = 0, last_reason = 0,
         last_t = 0, last_cols = 0, t = 0, ring_return = 0, ring_length = 0, ring_reason = 0, ring_env = 0, ring_t = 0, ring_cols = 0,
         counts = 0;
};
MonitorLayout monitor_layout(int n_envs, int window, int cols_a, int cols_b, uint32_t env_offset, int block);
// trex_batch_monitor_apply: the strides against the widths; the pointers as "is it there" flags
void check_monitor_apply(const MonitorLayout &m, bool reward, int reward_stride, bool done, int done_stride, bool block_a, int stride_a,
                         bool block_b, int stride_b);

// The trainer (include/trex_policy.h, trex_policy_critic.h, trex_policy_distill.h): what its C-ABI refuses before any HIP call, as
// functions of sizes, strides and of which pointers are there (a bool per pointer, or one for "all that the call requires").
// PolicyShape is the policy as the checks see it - env count, widths (Dv 0: no critic), parameter layout -; a null one is refused
// by every check that takes it, with the call's own words. The first refusal of a call that is wrong twice is the one listed first.
struct PolicyShape { int n = 0, D = 0, A = 0, Dv = 0; trex_policy::PolicyLayout lay{}; };
void check_policy_create(int num_envs, int obs_dim, int act_dim, int hidden);
void check_policy_set_critic(const PolicyShape *p, int critic_dim);
// a call of trex_policy_critic.h that needs a critic: the policy and `arg`, the call's one required pointer, then the width
void check_policy_has_critic(const char *who, const PolicyShape *p, bool arg);
void check_policy_observe(const PolicyShape *p, bool rows, int row_stride, bool with_reward);
void check_policy_critic_observe(const PolicyShape *p, bool rows_v, int stride_v);
struct PolicyActCall { bool theta, rows, rows_v, noise, actions, value_out, obs_v_out; int row_stride, stride_v; bool value_only; };
void check_policy_act(const PolicyShape *p, const PolicyActCall &c);          // (rows_v, obs_v_out, stride_v: not looked at)
void check_policy_critic_act(const PolicyShape *p, const PolicyActCall &c);
void check_policy_gae(const PolicyShape *p, bool buffers, int T);
void check_policy_minibatch_stats(const PolicyShape *p, bool buffers, int num_minibatches, int mb, int64_t num_samples);
// one of the six minibatch entry points. critic: an entry point of trex_policy_critic.h (it passes obs_v); distill: one of
// trex_policy_distill.h, whose kind, teacher_logstd, teacher_value and vf_coef are looked at for it alone
struct PolicyMinibatchCall {
  const char *who;
  bool distill, critic, buffers;
  int mb, first;
  int64_t num_samples;
  int kind;
  bool teacher_logstd, teacher_value;
  float vf_coef;
};
void check_policy_minibatch(const PolicyShape *p, const PolicyMinibatchCall &c);

// The planner (include/trex_planner.h): its sizes checked, its tap tables - the interpolation table, one tap set per step, and the
// shift table of a `steps`, one per new knot -, the discount table of a gamma, the noise as the kernel reads it, and what the
// calls refuse before any HIP call (the pointers as "is it there" flags).
struct PlannerShape { int G = 0, K = 0, S = 0, P = 0, A = 0, kind = 0, N = 0; };
PlannerShape check_planner_create(int groups, int samples, int horizon, int knots, int act_dim, int interpolation);
// the four taps of the knot coordinate num / den (den 0: the constant), as the header defines them
TrexPlanTap plan_tap(int kind, int P, int64_t num, int64_t den);
std::vector<TrexPlanTap> build_plan_taps(const PlannerShape &p);
// steps as the table is kept by: min(steps, S - 1)
int plan_shift_key(const PlannerShape &p, int steps);
std::vector<TrexPlanTap> build_plan_shift(const PlannerShape &p, int steps);
std::vector<float> build_plan_discount(int S, float gamma);
TrexPlanNoise build_plan_noise(const PlannerShape &p, const float *sigma, const float *lo, const float *hi, uint32_t env_offset);
void check_plan_update(const PlannerShape &p, bool noise_set, bool reward, int64_t step_stride, int64_t env_stride, float gamma,
                       float temperature);
// the bytes a strided [S, N] column reaches: its last element ends it
size_t plan_column_bytes(const PlannerShape &p, int64_t step_stride, int64_t env_stride);

// The mirror maps (include/trex_symmetry.h): a table checked and as the kernels read it - word c is src[c], with TREX_MIRROR_NEG set
// where sign[c] < 0 -, whether it is an involution, and what the two row launches refuse before any HIP call. The pointers are
// looked at as addresses only (null, overlap).
struct MirrorWords { std::vector<uint32_t> word; bool involution = false; };
MirrorWords build_mirror_words(const int32_t *src, const int8_t *sign, int width);
void check_mirror_rows(int table_width, const void *in, int in_stride, const void *out, int out_stride, int n, int width);
// widths: the tables' (critic 0: none); has_critic_table, obs_v: what was given; buffers: every required pointer is there
void check_mirror_augment(int obs_width, int act_width, int critic_width, bool has_critic_table, bool buffers, bool obs_v,
                          int64_t num_samples, int D, int A, int Dv);

// trex_model_mirror_table: the bodies paired by the reflection of their joint origins at q = 0 in the plane through URDF link 0's
// origin whose normal is link 0's axis `lateral` (-1: searched), the joints' pairs and signs in observation order, and what of
// the model is NOT symmetric (include/trex_symmetry.h lists the five residuals). Refuses what the header says.
struct ModelMirror {
  int lateral = 0;
  std::vector<int32_t> pair, body_pair;     // [J] observation slots, [B] bodies
  std::vector<int8_t> sign;                 // [J]
  double residual[5] = {0, 0, 0, 0, 0};
};
ModelMirror build_model_mirror(const HostModel &h, int lateral, double tol_pos);
// trex_model_mirror_row_table: the table of a composed row [q J | qd J | torque J | the E channel columns | tail] - the rules of
// include/trex_symmetry.h. action_cols: J or 2 J (what PREV_ACTION copies); extern_src / extern_sign: the caller's table of the
// EXTERNAL columns, concatenated in channel order (nullable where no such channel is set).
struct RowMirror { std::vector<int32_t> src; std::vector<int8_t> sign; };
RowMirror build_mirror_row_table(const HostModel &h, const ModelMirror &mm, double tol_pos, const TrexObsChannel *channels, int num_channels,
                                 int action_cols, int tail, const int32_t *extern_src, const int8_t *extern_sign);
// the action table [A] of a joint table [J]: the joint table, and with stiffness actions (A = 2 J) a second block of the same
// permutation with sign +1
void build_mirror_action_table(const int32_t *pair, const int8_t *sign, int nj, bool stiffness, int32_t *src_out, int8_t *sign_out);
// the table of a velocity command (vx, vy, wz) in base axes: the lateral component and wz change sign
void build_mirror_command_table(int lateral, int32_t src_out[3], int8_t sign_out[3]);

// trex_batch_render: the camera of include/trex_batch.h, checked, as the renderer's basis
struct CameraBasis { float offset[3], fwd[3], right[3], up[3], tan_x, tan_y; };
CameraBasis camera_basis(const TrexCamera &cam, int width, int height);

}  // namespace trex
