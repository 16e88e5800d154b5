// What capi.cpp and capi_queries.cpp share: the two handles of include/trex_batch.h (the owner of device memory and the error
// plumbing: internal.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/trex_batch.h"
#include "host_tables.hpp"
#include "internal.hpp"
#include "link_state.h"
#include "monitor.h"
#include "randomize.h"
#include "start_state.h"

using DeviceGuard = TrexDeviceGuard;

struct TrexModel {
  trex::HostModel host;
};

struct TrexBatch {
  int n = 0, device = 0, nb = 0, nj = 0;
  // the model, the state arrays, the hull points and the link / visual tables: made by trex_batch_create, `dmodel` and `arr` point into them
  std::vector<DeviceBuf> state;
  TrexDeviceModel *dmodel = nullptr;
  TrexBatchArrays arr{};
  DeviceBuf warm;                              // PGS warm-start records [n][TREX_WARM_WORDS] (device_model.h); warmstart > 0 only
  DeviceBuf ext;                               // external wrench [n][6][TREX_TL] (trex_batch_set_external_wrench); first non-NULL call on
  bool ext_on = false;                         // set: the step launches take the EXT kernels
  const float *wrench() const { return ext_on ? ext.as<float>() : nullptr; }
  DeviceBuf sens;                              // contact sensor [n][TREX_SENS_FLOATS] (trex_batch_set_contact_sensor); first enable
  bool sens_on = false;                        // on: every step and reset launch takes the SENS kernels
  float *sensor() const { return sens_on ? sens.as<float>() : nullptr; }
  // actuator model (trex_batch_set_control_mode / _set_motor_gains / _set_stiffness_actions): while any of the three is active the
  // step launches take the ACT kernels; the gains buffer [n][TREX_ACT_FLOATS] exists from the first use of any of them and
  // then always holds what the launches are to read - the caller's gains, or the model parameters
  std::vector<int> obs_order;                  // observation slot -> body lane
  std::vector<int> parent;                     // body -> parent body (trex_batch_inverse_kinematics: which joints carry a probe)
  uint32_t vel_mask = 0u, tor_mask = 0u;       // joints under VELOCITY / TORQUE control, bit b = body lane b
  float kp_max = 0.f;                          // upper clip of an action's stiffness
  DeviceBuf gains;
  bool gains_set = false, stiff = false;
  bool act_on() const { return (vel_mask | tor_mask) != 0u || gains_set || stiff; }
  int action_cols() const { return stiff ? 2 * nj : nj; }
  float wd = 1.0f, we = 0.005f, wk = 0.002f;  // trex_env.py:42-44
  bool pen_in_rows = false;                    // trex_batch_set_penalties_in_rows
  int balance_mode = -1;                       // trex_batch_set_wave_balance: -1 auto, 0 off, 1 on
  bool balance() const { return balance_mode < 0 ? n >= 2048 : balance_mode != 0; }
  // renderer (trex_batch_render): the model's hull data, its primitive / plane table made on the first render call
  std::vector<trex::Vec3> hull_xyz;
  std::vector<double> hull_radius;
  std::vector<int> hull_start, hull_group_start;
  double floor_z = 0;
  double step_seconds = 0;                // dt * substeps: what an env-step advances time by (the reward terms' Ts)
  int render_nprim = 0;
  DeviceBuf render_prim, render_plane;   // TrexRenderPrim [], float4 []: both or neither
  DeviceBuf render_ids;                  // device copy of the env ids of the last call
  // dynamics queries (trex_batch_jacobian): body and body<-link transform of every URDF link, host side
  trex::Links links;
  // link kinematics (trex_batch_set_link_probes): per set the device table of its probes - body [K], then body<-link rotation and
  // the point in the body frame [K][12]; freed by num_probes 0 and with the batch
  // (host_body: the bodies again, host side, for the chain masks of trex_batch_inverse_kinematics)
  struct ProbeSet { int n = 0; DeviceBuf body, tf; std::vector<int32_t> host_body; };
  ProbeSet probes[TREX_LINK_SETS];
  // proximity queries (trex_batch_set_proximity_shapes): ONE device allocation laid out as trex::ProxTable says (`table`: its counts
  // and offsets, the host blob dropped); freed by num_capsules 0 and with the batch
  struct Prox { trex::ProxTable table; DeviceBuf blob; } prox;
  // observation channels (trex_batch_set_observation): ONE device allocation laid out as trex::ObsTable says (`table`: its counts
  // and offsets, the host blob dropped); freed by num_channels 0 and with the batch
  struct Observation { trex::ObsTable table; DeviceBuf blob; } observation;
  // reward terms (trex_batch_set_reward): the term table, ONE device allocation laid out as trex::RewTable says, and the history
  // of its terms, ONE more, zeroed by every set and laid out by trex::reward_hist_layout, as `st` points into it; both freed by
  // num_terms 0 and with the batch
  struct Reward {
    trex::RewTable table;
    DeviceBuf blob, hist;
    struct Hist { float *prev_act, *prev_qd, *timer, *held; int32_t *valid; } st{};
  } reward;
  // motion clip (trex_batch_set_motion, include/trex_motion.h): the clip table, ONE device allocation laid out as
  // trex::MotionTable says (`table`: its counts and constants, the host rows dropped); the clocks, ONE more, zeroed by every set
  // and laid out by trex::motion_clock_layout, as `st` points into it; the terms of trex_batch_set_motion_reward, host side - they
  // travel in the launch arguments - and their held values (trex::motion_held_layout). q_lower, q_upper: the joint limits by
  // body, what the builder checks a clip against. probe_set, probes: the end effectors' set and its size when the clip was set
  // (-1, 0: none)
  struct Motion {
    trex::MotionTable table;
    DeviceBuf blob, clock, held;
    struct Clock { float *t0; int32_t *k; } st{};
    std::vector<TrexMotTerm> terms;
    float step_weight = 1.f;
    int probe_set = -1, probes = 0;
    std::vector<double> q_lower, q_upper;
  } motion;
  // sensor model (trex_batch_set_sensing, include/trex_sensing.h): the group table, ONE device allocation laid out as
  // sensing_limits.h says (`table`: its counts and maps, the blob dropped); the counters, ONE more, zeroed by every set and laid
  // out by trex::sense_counter_layout, as `st` points into it; the history (trex::sense_hist_layout), only while a group can be
  // late. seed, env_offset: of the last set, kept by a clear. The action delay (trex_batch_set_action_delay): its range, the
  // action width it was set for, its counters (the same layout with one group, `act_st`) and its history
  struct Sensing {
    trex::SenseTable table;
    DeviceBuf blob, state, hist;
    uint64_t seed = 0;
    uint32_t env_offset = 0;
    int act_min = 0, act_max = 0, act_cols = 0;
    DeviceBuf act_state, act_hist;
    struct Counters { uint32_t *ep, *k, *started; int32_t *delay; } st{}, act_st{};
  } sensing;
  // episode randomisation (trex_batch_set_randomization, include/trex_randomize.h): the term table (`table`: host side; `blob`: the
  // TrexRandTable of randomize.h on the device); the state, ONE allocation zeroed by every set, laid out by
  // trex::rand_state_layout, as `st` points into it (TrexRandState); the snapshots taken at the set - the gains buffer (`nominal`, with a KP / KD / MAX_FORCE term), the mass
  // scale and the friction (with a term of that kind) - and the switches as they stood then: what a clear puts back
  struct Randomization {
    trex::RandTable table;
    DeviceBuf blob, state, nominal, mass0, friction0;
    TrexRandState st{};
    uint64_t seed = 0;
    uint32_t env_offset = 0;
    bool was_domain = false, was_gains_set = false, was_ext_on = false;
  } random;
  // start-state randomisation (trex_batch_set_start_state, include/trex_start_state.h): the term table (`table`: host side, num_terms
  // 0 = nothing set; `blob`: the same on the device); the state, ONE allocation zeroed by every set - the lowest points then set to
  // -1 -, laid out by trex::start_state_layout, as `st` points into it (TrexStartState); seed and env_offset of the last set, kept
  // by a clear
  struct StartStates {
    TrexStartTable table{};
    DeviceBuf blob, state;
    TrexStartState st{};
    uint64_t seed = 0;
    uint32_t env_offset = 0;
  } start;
  // episode monitor (trex_batch_set_monitor, include/trex_monitor.h): its shape and the layout of its state (`layout`: host side,
  // window 0 = no monitor), the state itself, ONE allocation zeroed by every set, as `st` points into it (TrexMonState), and the
  // global index of env 0; all freed by window 0 and with the batch
  struct Monitor {
    trex::MonitorLayout layout;
    DeviceBuf state;
    TrexMonState st{};
    uint32_t env_offset = 0;
  } monitor;
  // fall termination (trex_batch_set_termination): the thresholds in force - a NaN is a criterion that is off - and the batch-owned
  // buffers of the predicate launch, ONE device allocation made by the first enabling call: terminal observations [n][3J], values
  // [n][3], reasons [n], reset mask [n], and done bytes [n] for a trex_batch_step call that passes no done buffer
  struct Termination {
    bool on = false, watch_any = false;
    float head_min = NAN, cos_tilt = NAN, penalty = 0.f;
    float clear_min[TREX_TL];
    DeviceBuf blob;
    float *tobs = nullptr, *values = nullptr;
    int32_t *reason = nullptr;
    uint8_t *mask = nullptr, *done = nullptr;
  } term;
  // caller allocations already validated as memory of this device (base address, bytes known to be good):
  // the hot path pays one hash-free scan of a handful of entries, hipPointerGetAttributes only on a new one
  std::vector<TrexSeen> seen;
};

// the gains buffer of a batch whose actuator model is about to be used: allocated on first use, holding the model parameters (capi.cpp)
int ensure_gains(TrexBatch *b);

inline int check_batch(const TrexBatch *b) { return b ? TREX_OK : fail(TREX_E_INVALID, "null batch"); }

// URDF link 0's frame in its body, into the launch arguments that carry it; returns the body's bit of a body mask
template <class A> uint32_t fill_base(const TrexBatch *b, A &a) {
  a.base_body = b->links.body[0];
  trex::tf12(b->links.tf[0], a.base_tf);
  return 1u << a.base_body;
}

// One output of an *_info call: `bytes` of the batch's state at `src` for the caller's `dst` (NULL: not asked for). A NULL src is
// state that is not set: asking for it is refused as "<who><asked> asked for and <unset>" (asked NULL: the name).
struct InfoCopy { void *dst; const void *src; size_t bytes; const char *name, *unset, *asked; };
// refuses what is asked for and not set, validates every output as memory of the batch's device, then issues the copies on `stream`
template <size_t N> int info_copies(const TrexBatch *b, const std::string &who, const InfoCopy (&copies)[N], void *stream) {
  for (const InfoCopy &c : copies)
    if (c.dst && !c.src) return fail(TREX_E_INVALID, who + (c.asked ? c.asked : c.name) + " asked for and " + c.unset);
  DeviceGuard guard(b->device);
  TrexBatch *mb = const_cast<TrexBatch *>(b);   // (the cache of validated buffers is the batch's)
  for (const InfoCopy &c : copies)
    if (c.dst)
      if (int code = trex_check_device_buffer(mb->device, mb->seen, c.dst, c.bytes, (who + c.name).c_str())) return code;
  for (const InfoCopy &c : copies)
    if (c.dst && c.bytes) HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TREX_OK;
}
