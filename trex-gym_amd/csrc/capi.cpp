// C-ABI of include/trex_batch.h: model handle, batch handle, stream-ordered launches.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/trex_batch.h"
#include "device_model.h"
#include "dynamics.h"
#include "internal.hpp"
#include "inverse_kinematics.h"
#include "link_state.h"
#include "model.hpp"
#include "proximity.h"
#include "raycast.h"
#include "render.h"
#include "step_launch.h"
#include "termination.h"

struct TrexModel {
  trex::HostModel host;
};

struct TrexBatch {
  int n = 0, device = 0, nb = 0, nj = 0;
  TrexDeviceModel *dmodel = nullptr;
  TrexBatchArrays arr{};
  float *warm = nullptr;                       // PGS warm-start records [n][TREX_WARM_WORDS] (device_model.h); warmstart > 0 only
  float *ext = nullptr;                        // external wrench [n][6][TREX_TL] (trex_batch_set_external_wrench); first non-NULL call on
  bool ext_on = false;                         // set: the step launches take the EXT kernels
  const float *wrench() const { return ext_on ? ext : nullptr; }
  float *sens = nullptr;                       // contact sensor [n][TREX_SENS_FLOATS] (trex_batch_set_contact_sensor); first enable
  bool sens_on = false;                        // on: every step and reset launch takes the SENS kernels
  float *sensor() const { return sens_on ? sens : nullptr; }
  // actuator model (trex_batch_set_control_mode / _set_motor_gains / _set_stiffness_actions): while any of the three is active the
  // step launches take the ACT kernels; the gains buffer [n][TREX_ACT_FLOATS] exists from the first use of any of them and
  // then always holds what the launches are to read - the caller's gains, or the model parameters
  std::vector<int> obs_order;                  // observation slot -> body lane
  std::vector<int> parent;                     // body -> parent body (trex_batch_inverse_kinematics: which joints carry a probe)
  uint32_t vel_mask = 0u, tor_mask = 0u;       // joints under VELOCITY / TORQUE control, bit b = body lane b
  float kp_max = 0.f;                          // upper clip of an action's stiffness
  float *gains = nullptr;
  bool gains_set = false, stiff = false;
  bool act_on() const { return (vel_mask | tor_mask) != 0u || gains_set || stiff; }
  int action_cols() const { return stiff ? 2 * nj : nj; }
  float wd = 1.0f, we = 0.005f, wk = 0.002f;  // trex_env.py:42-44
  bool pen_in_rows = false;                    // trex_batch_set_penalties_in_rows
  int balance_mode = -1;                       // trex_batch_set_wave_balance: -1 auto, 0 off, 1 on
  bool balance() const { return balance_mode < 0 ? n >= 2048 : balance_mode != 0; }
  std::vector<void *> allocs;
  // renderer (trex_batch_render): the model's hull data, its primitive / plane table made on the first render call
  std::vector<trex::Vec3> hull_xyz;
  std::vector<double> hull_radius;
  std::vector<int> hull_start, hull_group_start;
  double floor_z = 0;
  bool render_ready = false;
  int render_nprim = 0;
  TrexRenderPrim *render_prim = nullptr;
  float4 *render_plane = nullptr;
  int32_t *render_ids = nullptr;     // device copy of the env ids of the last call
  size_t render_ids_cap = 0;
  // dynamics queries (trex_batch_jacobian): body and body<-link transform of every URDF link, host side
  std::vector<int> link_body;
  std::vector<trex::Tf> link_tf;
  // link kinematics (trex_batch_set_link_probes): per set the device table of its probes - body [K], then body<-link rotation and
  // the point in the body frame [K][12]; freed by num_probes 0 and with the batch
  // (host_body: the bodies again, host side, for the chain masks of trex_batch_inverse_kinematics)
  struct ProbeSet { int n = 0; int32_t *body = nullptr; float *tf = nullptr; std::vector<int32_t> host_body; };
  ProbeSet probes[TREX_LINK_SETS];
  // proximity queries (trex_batch_set_proximity_shapes): ONE device allocation holding the capsules [C][8], their bodies [C], the
  // capsule-pair tests [T] and each pair's first test [P]; freed by num_capsules 0 and with the batch
  struct ProxTable {
    int caps = 0, pairs = 0, tests = 0;
    void *blob = nullptr;
    const float *cap = nullptr; const int32_t *cap_body = nullptr; const uint32_t *test = nullptr; const int32_t *pair_first = nullptr;
  } prox;
  // fall termination (trex_batch_set_termination): the thresholds in force - a NaN is a criterion that is off - and the batch-owned
  // buffers of the predicate launch, ONE device allocation made by the first enabling call: terminal observations [n][3J], values
  // [n][3], reasons [n], reset mask [n], and done bytes [n] for a trex_batch_step call that passes no done buffer
  struct Termination {
    bool on = false, watch_any = false;
    float head_min = NAN, cos_tilt = NAN, penalty = 0.f;
    float clear_min[TREX_TL];
    void *blob = nullptr;
    float *tobs = nullptr, *values = nullptr;
    int32_t *reason = nullptr;
    uint8_t *mask = nullptr, *done = nullptr;
  } term;
  // caller allocations already validated as memory of this device (base address, bytes known to be good):
  // the hot path pays one hash-free scan of a handful of entries, hipPointerGetAttributes only on a new one
  std::vector<TrexSeen> seen;
};

namespace {

thread_local std::string g_error;

int fail(int code, const std::string &msg) {
  g_error = msg;
  return code;
}
int hip_fail(hipError_t e, const char *what) {
  return fail(TREX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return hip_fail(_e, #expr);  \
  } while (0)

using DeviceGuard = TrexDeviceGuard;

void fill_device_model(const trex::HostModel &h, TrexDeviceModel &d) {
  std::memset(&d, 0, sizeof d);
  d.nb = h.nb;
  d.head_body = h.head_body;
  d.nv = (int)h.hull_xyz.size();
  const trex::Params &p = h.prm;
  const double prm[TP_COUNT] = {p.dt, p.substeps, p.iterations, p.gravity, p.motor_kp, p.motor_kd, p.motor_max_force,
                                p.floor_z, p.friction, p.erp, p.contact_erp, p.contact_margin, p.link_damping,
                                p.max_coordinate_velocity, p.max_contacts, p.warmstart};
  for (int i = 0; i < TP_COUNT; i++) d.prm[i] = (float)prm[i];
  d.n_substeps = (int)p.substeps; d.n_iterations = (int)p.iterations; d.max_contacts = (int)p.max_contacts;
  d.inv_dt = 1.0f / (float)p.dt;
  d.motor_max_impulse = (float)p.motor_max_force * (float)p.dt;
  d.head_point[0] = (float)h.head_point.x; d.head_point[1] = (float)h.head_point.y; d.head_point[2] = (float)h.head_point.z;
  d.base_pos0[0] = (float)h.base_start_pos.x; d.base_pos0[1] = (float)h.base_start_pos.y; d.base_pos0[2] = (float)h.base_start_pos.z;
  for (int c = 0; c < 4; c++) d.base_quat0[c] = (float)h.base_start_quat[c];
  int maxdepth = 0;
  for (int l = 0; l < TREX_TL; l++) {
    d.parent[l] = -1; d.depth[l] = -1; d.obs_slot[l] = -1;
    for (int k = 0; k < TREX_MAXD; k++) d.anc[k][l] = -1;
    for (int k = 0; k < TREX_MAXCH; k++) d.child[k][l] = -1;
    d.mass[l] = 1.0f;
    d.jrot[0][l] = d.jrot[4][l] = d.jrot[8][l] = 1.0f;
    d.axis[2][l] = 1.0f;
    d.inertia[0][l] = d.inertia[3][l] = d.inertia[5][l] = 1.0f;
  }
  for (int b = 0; b < h.nb; b++) {
    d.parent[b] = h.parent[b];
    d.depth[b] = h.depth[b];
    maxdepth = std::max(maxdepth, h.depth[b]);
    for (int i = b; i > 0; i = h.parent[i]) d.anc[h.depth[i] - 1][b] = i;
    if (b > 0) {
      int p = h.parent[b];
      for (int k = 0; k < TREX_MAXCH; k++)
        if (d.child[k][p] < 0) { d.child[k][p] = b; break; }
    }
    const trex::Vec3 &a = h.joint_axis[b], &jp = h.joint_pos[b], &c = h.com[b], &sc = h.sphere_center[b];
    d.axis[0][b] = (float)a.x; d.axis[1][b] = (float)a.y; d.axis[2][b] = (float)a.z;
    d.jpos[0][b] = (float)jp.x; d.jpos[1][b] = (float)jp.y; d.jpos[2][b] = (float)jp.z;
    d.com[0][b] = (float)c.x; d.com[1][b] = (float)c.y; d.com[2][b] = (float)c.z;
    for (int k = 0; k < 9; k++) d.jrot[k][b] = (float)h.joint_rot[b].m[k];
    for (int k = 0; k < 6; k++) d.inertia[k][b] = (float)h.inertia[b][k];
    d.mass[b] = (float)h.mass[b];
    d.lower[b] = (float)h.q_lower[b]; d.upper[b] = (float)h.q_upper[b]; d.damp[b] = (float)h.joint_damping[b];
    d.q_start[b] = (float)h.q_start[b];
    d.sphere[0][b] = (float)sc.x; d.sphere[1][b] = (float)sc.y; d.sphere[2][b] = (float)sc.z;
    d.sphere[3][b] = (float)h.sphere_radius[b];
    // round the half extents up one ulp-ish: the bound must stay conservative in f32
    d.box_half[0][b] = (float)(h.box_half[b].x * (1 + 1e-6) + 1e-7); d.box_half[1][b] = (float)(h.box_half[b].y * (1 + 1e-6) + 1e-7);
    d.box_half[2][b] = (float)(h.box_half[b].z * (1 + 1e-6) + 1e-7);
    d.hull_start[b] = h.hull_start[b];
  }
  for (int b = h.nb; b <= TREX_TL; b++) d.hull_start[b] = h.hull_start[h.nb];
  {
    int off = 0;
    for (int b = 0; b < TREX_TL; b++) {
      const int nv = b < h.nb ? h.hull_start[b + 1] - h.hull_start[b] : 0;
      int lg = nv == 0 ? 0 : (nv <= 256 ? 3 : (nv <= 1024 ? 5 : 0));
      if (lg && off + (1 << lg) > TREX_CM_WORDS) lg = 0;          // no room left: this body is swept, not masked
      d.cm_pack[b] = (off << 8) | lg;
      if (lg) off += 1 << lg;
    }
  }
  {
    // scan units: the hull groups if they nest in the bodies' vertex ranges and are at most 32, else one per body
    std::vector<std::array<int, 3>> units;   // body, v0, v1
    bool ok = h.hull_group_start.size() >= 2;
    if (ok)
      for (size_t g = 0; g + 1 < h.hull_group_start.size() && ok; g++) {
        const int g0 = h.hull_group_start[g], g1 = h.hull_group_start[g + 1];
        if (g1 <= g0) continue;
        int body = -1;
        for (int b = 0; b < h.nb; b++)
          if (h.hull_start[b] <= g0 && g1 <= h.hull_start[b + 1]) body = b;
        if (body < 0) ok = false;
        else units.push_back({body, g0, g1});
      }
    if (!ok || units.size() > TREX_TL) {
      units.clear();
      for (int b = 0; b < h.nb; b++)
        if (h.hull_start[b + 1] > h.hull_start[b]) units.push_back({b, h.hull_start[b], h.hull_start[b + 1]});
    }
    d.nchunk = (int)units.size();
    for (int k = 0; k < TREX_TL; k++) { d.chunk_body[k] = 0; d.chunk_v0[k] = 0; d.chunk_v1[k] = 0; }
    for (size_t k = 0; k < units.size(); k++) {
      const int v0 = units[k][1], v1 = units[k][2];
      trex::Vec3 lo{1e300, 1e300, 1e300}, hi{-1e300, -1e300, -1e300};
      for (int v = v0; v < v1; v++) {
        const trex::Vec3 &p = h.hull_xyz[v];
        const double r = h.hull_radius[v];
        lo = {std::min(lo.x, p.x - r), std::min(lo.y, p.y - r), std::min(lo.z, p.z - r)};
        hi = {std::max(hi.x, p.x + r), std::max(hi.y, p.y + r), std::max(hi.z, p.z + r)};
      }
      d.chunk_body[k] = units[k][0]; d.chunk_v0[k] = v0; d.chunk_v1[k] = v1;
      d.chunk_c[0][k] = (float)(0.5 * (lo.x + hi.x)); d.chunk_c[1][k] = (float)(0.5 * (lo.y + hi.y)); d.chunk_c[2][k] = (float)(0.5 * (lo.z + hi.z));
      // half extents rounded up: the bound must stay conservative in f32 (centre rounding included)
      d.chunk_h[0][k] = (float)(0.5 * (hi.x - lo.x) * (1 + 1e-6) + 1e-6); d.chunk_h[1][k] = (float)(0.5 * (hi.y - lo.y) * (1 + 1e-6) + 1e-6);
      d.chunk_h[2][k] = (float)(0.5 * (hi.z - lo.z) * (1 + 1e-6) + 1e-6);
    }
  }
  d.maxdepth = maxdepth;
  for (size_t k = 0; k < h.obs_order.size(); k++) d.obs_slot[h.obs_order[k]] = (int)k;
  // dof lane l in chain of body b?  joint lanes: b is l or a descendant of l; base dof lanes: every body
  for (int l = 0; l < TREX_TL; l++) {
    unsigned m = 0;
    if (l >= 1 && l < h.nb) {
      for (int b = 0; b < h.nb; b++)
        for (int i = b; i > 0; i = h.parent[i])
          if (i == l) { m |= 1u << b; break; }
    } else if (l >= h.nb && l < h.nb + 6) {
      m = (h.nb >= 32) ? 0xffffffffu : ((1u << h.nb) - 1u);
    }
    d.desc_mask[l] = m;
  }
}

int check_batch(const TrexBatch *b) { return b ? TREX_OK : fail(TREX_E_INVALID, "null batch"); }

// the gains buffer of a batch whose actuator model is about to be used: allocated on first use, holding the model parameters
int ensure_gains(TrexBatch *b) {
  if (b->gains) return TREX_OK;
  DeviceGuard guard(b->device);
  void *p = nullptr;
  HIP_TRY(hipMalloc(&p, (size_t)b->n * TREX_ACT_FLOATS * sizeof(float)));
  b->allocs.push_back(p);
  HIP_TRY(trex_launch_copy_gains(b->dmodel, nullptr, nullptr, nullptr, (float *)p, b->n, nullptr));
  HIP_TRY(hipDeviceSynchronize());   // (in place before a launch on any stream)
  b->gains = (float *)p;
  return TREX_OK;
}

// What every launch of the batch's step kernels is given: the model, the state, the reward weights and the record / buffer of each
// feature that is switched on - a non-null pointer IS the switch (step_launch.h). A reset takes no actions: no wave balance, no
// external wrench, no actuator model. The caller adds the outputs and their strides.
TrexStepArgs step_args(const TrexBatch *b, TrexStepKind kind) {
  TrexStepArgs a{};
  a.model = b->dmodel; a.arr = b->arr; a.n_envs = b->n;
  a.w_distance = b->wd; a.w_energy = b->we; a.w_drift = b->wk;
  a.obs_stride = 3 * b->nj; a.scal_stride = 1; a.n_steps = 1;
  a.warm = b->warm; a.sens = b->sensor();
  if (kind == TREX_KIND_RESET) return a;
  a.bal = b->balance() ? b->arr.balance : nullptr;
  a.ext = b->wrench();
  if (b->act_on()) {
    a.act = b->gains; a.act_vel = b->vel_mask; a.act_tor = b->tor_mask;
    a.act_cols = b->action_cols(); a.act_kp_max = b->kp_max;
  }
  return a;
}
// the outputs as ONE row block: row e = obs | reward | done (| the three penalties) at rows + e * row_stride
void rows_out(const TrexBatch *b, TrexStepArgs &a, float *rows, int row_stride) {
  a.obs = rows; a.reward = rows + 3 * b->nj; a.done_f = a.reward + 1;
  a.obs_stride = a.scal_stride = row_stride;
  a.pen_in_rows = b->pen_in_rows ? 1 : 0;
}

// the state and the collision points of a K8 launch (termination.hip)
TrexTermArgs term_args(const TrexBatch *b) {
  TrexTermArgs t{};
  t.model = b->dmodel; t.base = b->arr.base; t.q = b->arr.q; t.hull = b->arr.hull; t.n_envs = b->n;
  return t;
}
// The two launches that follow the step launch `a` of a batch with termination on: the K8 predicate on the outputs `a` names, then
// the RESET launch with the K8 mask - observation into the caller's rows, no reward, no done, so that what the step and K8 wrote
// there survives. Nothing is decided on the host: both run whether or not an env terminates.
hipError_t termination_tail(const TrexBatch *b, const TrexStepArgs &a, hipStream_t stream) {
  const TrexBatch::Termination &tm = b->term;
  TrexTermArgs t = term_args(b);
  t.watch_any = tm.watch_any ? 1 : 0;
  t.head_min = tm.head_min; t.cos_tilt = tm.cos_tilt; t.penalty = tm.penalty;
  std::memcpy(t.clear_min, tm.clear_min, sizeof t.clear_min);
  t.mask = tm.mask; t.reason = tm.reason; t.values = tm.values; t.terminal_obs = tm.tobs;
  t.obs = a.obs; t.reward = a.reward; t.done_f = a.done_f; t.done = a.done;
  t.obs_stride = a.obs_stride; t.scal_stride = a.scal_stride; t.obs_cols = 3 * b->nj;
  hipError_t e = trex_launch_termination(t, 1, stream);
  if (e != hipSuccess) return e;
  TrexStepArgs r = step_args(b, TREX_KIND_RESET);
  r.reset_mask = tm.mask; r.obs = a.obs; r.obs_stride = a.obs_stride;
  return trex_launch_step(&r, TREX_KIND_RESET, stream);
}

int check_device_buffer(TrexBatch *b, const void *p, size_t bytes, const char *what) {
  return trex_check_device_buffer(b->device, b->seen, p, bytes, what);
}
#define BUF_TRY(p, bytes, what)                                                  \
  do {                                                                           \
    if (int _c = check_device_buffer(b, (p), (size_t)(bytes), (what))) return _c; \
  } while (0)

}  // namespace

int trex_fail(int code, const std::string &msg) { return fail(code, msg); }

// A caller-owned buffer must be HIP device (or managed) memory of the given device and at least `bytes`
// long: a host pointer or a short buffer would make the kernel fault the GPU. NULL is accepted where the
// header says nullable (the caller checks non-nullable arguments first).
int trex_check_device_buffer(int device, std::vector<TrexSeen> &seen, const void *p, size_t bytes, const char *what) {
  if (!p) return TREX_OK;
  // validated ALLOCATIONS of this device: any pointer into one of them with enough room behind it passes without a
  // runtime query (a caller that walks through one large tensor - a [T, N, J] action pool - presents a new pointer
  // every step; hipPointerGetAttributes + hipMemGetAddressRange cost about 20 us)
  for (const auto &s : seen) {
    const char *lo = (const char *)s.p, *q = (const char *)p;
    if (q >= lo && q + bytes <= lo + s.bytes) return TREX_OK;
  }
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof at);
  hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();   // unregistered host memory reports an error: clear it
    return fail(TREX_E_INVALID, std::string(what) + ": not a HIP device pointer (host memory?)");
  }
  if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)
    return fail(TREX_E_INVALID, std::string(what) + ": pointer is not device memory");
  if (at.type == hipMemoryTypeDevice && at.device != device)
    return fail(TREX_E_INVALID, std::string(what) + ": buffer lives on device " + std::to_string(at.device) +
                                    ", the batch on device " + std::to_string(device));
  void *base = nullptr;
  size_t size = 0;
  const void *lo = p;
  size_t known = bytes;
  if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)p) == hipSuccess && base) {
    const size_t left = size - (size_t)((const char *)p - (const char *)base);
    if (left < bytes)
      return fail(TREX_E_INVALID, std::string(what) + ": buffer too small (" + std::to_string(left) + " bytes, need " +
                                      std::to_string(bytes) + ")");
    lo = base; known = size;   // the whole allocation is good
  } else {
    (void)hipGetLastError();
  }
  if (seen.size() >= 64) seen.erase(seen.begin());
  seen.push_back({lo, known});
  return TREX_OK;
}

extern "C" {

const char *trex_last_error(void) { return g_error.c_str(); }

#ifndef TREX_BUILD_ID
#define TREX_BUILD_ID "unknown"
#endif
const char *trex_build_id(void) { return TREX_BUILD_ID; }

int trex_model_load(const char *urdf_path, const char *collisions_dir, TrexModel **out) {
  if (!urdf_path || !out) return fail(TREX_E_INVALID, "trex_model_load: null argument");
  *out = nullptr;
  int code = TREX_OK;
  try {
    auto m = std::make_unique<TrexModel>();
    m->host = trex::load_model(urdf_path, collisions_dir, &code);
    *out = m.release();
    return TREX_OK;
  } catch (const std::exception &e) {
    return fail(code ? code : TREX_E_PARSE, e.what());
  }
}

void trex_model_destroy(TrexModel *m) { delete m; }

int trex_model_num_bodies(const TrexModel *m) { return m ? m->host.nb : fail(TREX_E_INVALID, "null model"); }
int trex_model_num_joints(const TrexModel *m) { return m ? m->host.nb - 1 : fail(TREX_E_INVALID, "null model"); }
int trex_model_num_urdf_joints(const TrexModel *m) { return m ? m->host.num_urdf_joints : fail(TREX_E_INVALID, "null model"); }
int trex_model_num_hull_vertices(const TrexModel *m) { return m ? (int)m->host.hull_xyz.size() : fail(TREX_E_INVALID, "null model"); }
double trex_model_total_mass(const TrexModel *m, int include_base_link) {
  if (!m) return -1.0;
  return include_base_link ? m->host.total_mass : m->host.total_mass_excluding_base;
}

int trex_model_joint_info(const TrexModel *m, int k, const char **name, int *urdf_joint_index, double *lower, double *upper) {
  if (!m) return fail(TREX_E_INVALID, "null model");
  if (k < 0 || k >= m->host.nb - 1) return fail(TREX_E_INVALID, "joint index out of range");
  int b = m->host.obs_order[k];
  if (name) *name = m->host.obs_joint_names[k].c_str();
  if (urdf_joint_index) *urdf_joint_index = m->host.revolute_joint_indices[k];
  if (lower) *lower = m->host.q_lower[b];
  if (upper) *upper = m->host.q_upper[b];
  return TREX_OK;
}

int trex_model_set_start_angle(TrexModel *m, const char *joint_name, double angle) {
  if (!m || !joint_name) return fail(TREX_E_INVALID, "null argument");
  std::string n = trex::rename_v0_name(joint_name);
  for (int i = 1; i < m->host.nb; i++)
    if (m->host.joint_names[i] == n) { m->host.q_start[i] = angle; return TREX_OK; }
  return fail(TREX_E_INVALID, std::string("unknown joint '") + joint_name + "'");
}

int trex_model_set_start_pose(TrexModel *m, const double xyz[3], const double rpy[3]) {
  if (!m || !xyz || !rpy) return fail(TREX_E_INVALID, "null argument");
  m->host.base_start_pos = {xyz[0], xyz[1], xyz[2]};
  trex::matrix_to_quat(trex::rpy_to_matrix(rpy[0], rpy[1], rpy[2]), m->host.base_start_quat);
  return TREX_OK;
}

int trex_model_use_primitive_collision(TrexModel *m, double max_radius, int max_divisions, int min_points) {
  if (!m) return fail(TREX_E_INVALID, "null model");
  if (!(max_radius > 0) || max_divisions < 0 || min_points < 1) return fail(TREX_E_INVALID, "bad primitive-fitting arguments");
  trex::use_primitive_collision(m->host, max_radius, max_divisions, min_points);
  return TREX_OK;
}

int trex_model_fit_hull_primitives(const TrexModel *m, int group, double max_radius, int max_divisions, int min_points,
                                   double *out, int capacity) {
  if (!m) return fail(TREX_E_INVALID, "null model");
  const auto &gs = m->host.hull_group_start;
  if (group < 0 || group + 1 >= (int)gs.size()) return fail(TREX_E_INVALID, "hull group out of range");
  if (!(max_radius > 0) || max_divisions < 0 || min_points < 1) return fail(TREX_E_INVALID, "bad primitive-fitting arguments");
  std::vector<trex::Vec3> pts(m->host.hull_xyz.begin() + gs[group], m->host.hull_xyz.begin() + gs[group + 1]);
  auto prims = trex::fit_primitives(pts, max_radius, max_divisions, min_points);
  if (out) {
    if (capacity < (int)prims.size()) return fail(TREX_E_INVALID, "capacity too small");
    for (size_t i = 0; i < prims.size(); i++) {
      double *o = out + 7 * i;
      o[0] = prims[i].p0.x; o[1] = prims[i].p0.y; o[2] = prims[i].p0.z;
      o[3] = prims[i].p1.x; o[4] = prims[i].p1.y; o[5] = prims[i].p1.z; o[6] = prims[i].radius;
    }
  }
  return (int)prims.size();
}

int trex_model_set_param(TrexModel *m, const char *name, double value) {
  if (!m || !name) return fail(TREX_E_INVALID, "null argument");
  double *p = m->host.prm.find(name);
  if (!p) return fail(TREX_E_INVALID, std::string("unknown parameter '") + name + "'");
  if (!std::isfinite(value)) return fail(TREX_E_INVALID, "parameter value is not finite");
  if (std::strcmp(name, "warmstart") == 0 && !(value >= 0.0 && value <= 1.0))
    return fail(TREX_E_INVALID, "warmstart must lie in [0, 1] (0 = off)");
  *p = value;
  return TREX_OK;
}
int trex_model_get_param(const TrexModel *m, const char *name, double *value) {
  if (!m || !name || !value) return fail(TREX_E_INVALID, "null argument");
  double *p = const_cast<TrexModel *>(m)->host.prm.find(name);
  if (!p) return fail(TREX_E_INVALID, std::string("unknown parameter '") + name + "'");
  *value = *p;
  return TREX_OK;
}

int trex_model_get_array(const TrexModel *m, const char *name, double *out, int capacity) {
  if (!m || !name) return fail(TREX_E_INVALID, "null argument");
  const trex::HostModel &h = m->host;
  std::vector<double> v;
  std::string n = name;
  auto push3 = [&](const std::vector<trex::Vec3> &a) { for (auto &p : a) { v.push_back(p.x); v.push_back(p.y); v.push_back(p.z); } };
  if (n == "parent") v.assign(h.parent.begin(), h.parent.end());
  else if (n == "depth") v.assign(h.depth.begin(), h.depth.end());
  else if (n == "joint_axis") push3(h.joint_axis);
  else if (n == "joint_pos") push3(h.joint_pos);
  else if (n == "joint_rot") { for (auto &r : h.joint_rot) v.insert(v.end(), r.m, r.m + 9); }
  else if (n == "q_lower") v = h.q_lower;
  else if (n == "q_upper") v = h.q_upper;
  else if (n == "joint_damping") v = h.joint_damping;
  else if (n == "mass") v = h.mass;
  else if (n == "com") push3(h.com);
  else if (n == "inertia") { for (auto &a : h.inertia) v.insert(v.end(), a.begin(), a.end()); }
  else if (n == "obs_order") v.assign(h.obs_order.begin(), h.obs_order.end());
  else if (n == "revolute_joint_indices") v.assign(h.revolute_joint_indices.begin(), h.revolute_joint_indices.end());
  else if (n == "head_body") v = {(double)h.head_body};
  else if (n == "link_body") v.assign(h.link_body.begin(), h.link_body.end());
  else if (n == "link_tf") { for (auto &t : h.link_tf) { v.insert(v.end(), t.R.m, t.R.m + 9); v.push_back(t.t.x); v.push_back(t.t.y); v.push_back(t.t.z); } }
  else if (n == "head_point") v = {h.head_point.x, h.head_point.y, h.head_point.z};
  else if (n == "hull_xyz") push3(h.hull_xyz);
  else if (n == "hull_start") v.assign(h.hull_start.begin(), h.hull_start.end());
  else if (n == "hull_radius") v = h.hull_radius;
  else if (n == "hull_group_start") v.assign(h.hull_group_start.begin(), h.hull_group_start.end());
  else if (n == "sphere_center") push3(h.sphere_center);
  else if (n == "sphere_radius") v = h.sphere_radius;
  else if (n == "q_start") v = h.q_start;
  else if (n == "base_start_pos") v = {h.base_start_pos.x, h.base_start_pos.y, h.base_start_pos.z};
  else if (n == "base_start_quat") v.assign(h.base_start_quat, h.base_start_quat + 4);
  else if (n == "hull_plane" || n == "hull_plane_start") {
    std::vector<int> start;
    trex::hull_group_planes(h, v, start);
    if (n == "hull_plane_start") v.assign(start.begin(), start.end());
  }
  else return fail(TREX_E_INVALID, "unknown array '" + n + "'");
  if (out) {
    if (capacity < (int)v.size()) return fail(TREX_E_INVALID, "capacity too small for '" + n + "'");
    std::memcpy(out, v.data(), v.size() * sizeof(double));
  }
  return (int)v.size();
}

// ------------------------------------------------------------------ batch
int trex_batch_create(const TrexModel *model, int num_envs, int device, TrexBatch **out) {
  if (!model || !out) return fail(TREX_E_INVALID, "trex_batch_create: null argument");
  *out = nullptr;
  if (num_envs <= 0) return fail(TREX_E_INVALID, "num_envs must be positive");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return fail(TREX_E_HIP, "no HIP device available (the physics step has no CPU fallback)");
  if (device < 0 || device >= count) return fail(TREX_E_INVALID, "device index out of range");
  DeviceGuard guard(device);
  if (!guard.ok) return fail(TREX_E_HIP, "hipSetDevice failed");
  auto b = std::make_unique<TrexBatch>();
  b->n = num_envs; b->device = device; b->nb = model->host.nb; b->nj = b->nb - 1;
  b->obs_order = model->host.obs_order; b->parent = model->host.parent;
  auto alloc = [&](size_t bytes, void **p) -> hipError_t {
    hipError_t r = hipMalloc(p, bytes);
    if (r == hipSuccess) { b->allocs.push_back(*p); r = hipMemset(*p, 0, bytes); }
    return r;
  };
  auto cleanup = [&]() { for (void *p : b->allocs) (void)hipFree(p); };
  TrexDeviceModel dm;
  fill_device_model(model->host, dm);
  size_t n = (size_t)num_envs;
  hipError_t r = hipSuccess;
  auto A = [&](size_t bytes, void **p) { if (r == hipSuccess) r = alloc(bytes, p); };
  A(sizeof(TrexDeviceModel), (void **)&b->dmodel);
  A(n * 16 * sizeof(float), (void **)&b->arr.base);
  A(n * TREX_TL * sizeof(float), (void **)&b->arr.q);
  A(n * TREX_TL * sizeof(float), (void **)&b->arr.qd);
  A(n * TREX_TL * sizeof(float), (void **)&b->arr.mass_scale);
  A(n * sizeof(float), (void **)&b->arr.friction);
  A(TREX_BAL_WORDS(n) * sizeof(int32_t), (void **)&b->arr.balance);
  // the warm-start records exist only for a model with warmstart > 0 (zeroed by alloc: every record empty)
  if (model->host.prm.warmstart > 0) A(n * TREX_WARM_WORDS * sizeof(float), (void **)&b->warm);
  b->arr.max_episode_steps = 0;
  b->arr.domain = 0;
  b->floor_z = model->host.prm.floor_z;
  b->hull_xyz = model->host.hull_xyz; b->hull_radius = model->host.hull_radius;
  b->hull_start = model->host.hull_start; b->hull_group_start = model->host.hull_group_start;
  size_t nv = model->host.hull_xyz.size();
  A((nv ? nv : 1) * sizeof(float4), (void **)&b->arr.hull);
  const size_t nl = model->host.link_names.size();
  int *link_body_dev = nullptr;
  float *link_tf_dev = nullptr;
  A(nl * sizeof(int), (void **)&link_body_dev);
  A(nl * 12 * sizeof(float), (void **)&link_tf_dev);
  const size_t nvis = model->host.visual_file.size();
  int *vis_body_dev = nullptr;
  float *vis_tf_dev = nullptr;
  A((nvis ? nvis : 1) * sizeof(int), (void **)&vis_body_dev);
  A((nvis ? nvis : 1) * 12 * sizeof(float), (void **)&vis_tf_dev);
  if (r != hipSuccess) { cleanup(); return hip_fail(r, "hipMalloc"); }
  {
    std::vector<int> vb(nvis);
    std::vector<float> vtf(nvis * 12);
    for (size_t v = 0; v < nvis; v++) {
      vb[v] = model->host.link_body[model->host.visual_link[v]];
      const trex::Tf &t = model->host.visual_body_tf[v];
      for (int k = 0; k < 9; k++) vtf[12 * v + k] = (float)t.R.m[k];
      vtf[12 * v + 9] = (float)t.t.x; vtf[12 * v + 10] = (float)t.t.y; vtf[12 * v + 11] = (float)t.t.z;
    }
    b->arr.num_visuals = (int)nvis; b->arr.visual_body = vis_body_dev; b->arr.visual_tf = vis_tf_dev;
    if (nvis) {
      r = hipMemcpy(vis_body_dev, vb.data(), nvis * sizeof(int), hipMemcpyHostToDevice);
      if (r == hipSuccess) r = hipMemcpy(vis_tf_dev, vtf.data(), vtf.size() * sizeof(float), hipMemcpyHostToDevice);
      if (r != hipSuccess) { cleanup(); return hip_fail(r, "hipMemcpy (visual table)"); }
    }
  }
  std::vector<float4> hull(nv ? nv : 1);
  for (size_t i = 0; i < nv; i++) hull[i] = make_float4((float)model->host.hull_xyz[i].x, (float)model->host.hull_xyz[i].y, (float)model->host.hull_xyz[i].z, (float)model->host.hull_radius[i]);
  std::vector<float> ltf(nl * 12);
  for (size_t l = 0; l < nl; l++) {
    for (int k = 0; k < 9; k++) ltf[12 * l + k] = (float)model->host.link_tf[l].R.m[k];
    ltf[12 * l + 9] = (float)model->host.link_tf[l].t.x; ltf[12 * l + 10] = (float)model->host.link_tf[l].t.y; ltf[12 * l + 11] = (float)model->host.link_tf[l].t.z;
  }
  b->link_body = model->host.link_body; b->link_tf = model->host.link_tf;
  b->arr.num_links = (int)nl; b->arr.link_body = link_body_dev; b->arr.link_tf = link_tf_dev;
  r = hipMemcpy(link_body_dev, model->host.link_body.data(), nl * sizeof(int), hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(link_tf_dev, ltf.data(), ltf.size() * sizeof(float), hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(b->dmodel, &dm, sizeof dm, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(b->arr.hull, hull.data(), hull.size() * sizeof(float4), hipMemcpyHostToDevice);
  {   // wave balance: before the first step launch every env is filed under contact count 0, in env order
    std::vector<int32_t> bal(TREX_BAL_LISTS + n, 0);
    bal[TREX_BAL_COUNTS + 0] = (int32_t)n;
    for (size_t i = 0; i < n; i++) bal[TREX_BAL_LISTS + i] = (int32_t)i;
    if (r == hipSuccess) r = hipMemcpy(b->arr.balance, bal.data(), bal.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  }
  if (r == hipSuccess) r = trex_launch_fill(b->arr.mass_scale, 1.0f, num_envs * TREX_TL, nullptr);
  if (r == hipSuccess) r = trex_launch_fill(b->arr.friction, (float)model->host.prm.friction, num_envs, nullptr);
  if (r == hipSuccess) r = hipDeviceSynchronize();
  if (r != hipSuccess) { cleanup(); return hip_fail(r, "batch initialisation"); }
  *out = b.release();
  return TREX_OK;
}

void trex_batch_destroy(TrexBatch *b) {
  if (!b) return;
  DeviceGuard guard(b->device);
  (void)hipDeviceSynchronize();
  for (void *p : b->allocs) (void)hipFree(p);
  if (b->render_ids) (void)hipFree(b->render_ids);
  for (auto &ps : b->probes) {
    if (ps.body) (void)hipFree(ps.body);
    if (ps.tf) (void)hipFree(ps.tf);
  }
  if (b->prox.blob) (void)hipFree(b->prox.blob);
  if (b->term.blob) (void)hipFree(b->term.blob);
  delete b;
}

int trex_batch_num_envs(const TrexBatch *b) { return b ? b->n : fail(TREX_E_INVALID, "null batch"); }

int trex_batch_set_reward_weights(TrexBatch *b, float distance, float energy, float drift) {
  if (check_batch(b)) return TREX_E_INVALID;
  b->wd = distance; b->we = energy; b->wk = drift;
  return TREX_OK;
}

int trex_batch_set_wave_balance(TrexBatch *b, int mode) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (mode < -1 || mode > 1) return fail(TREX_E_INVALID, "trex_batch_set_wave_balance: mode must be -1 (auto), 0 (off) or 1 (on)");
  b->balance_mode = mode;
  return TREX_OK;
}

int trex_batch_set_penalties_in_rows(TrexBatch *b, int enabled) {
  if (check_batch(b)) return TREX_E_INVALID;
  b->pen_in_rows = enabled != 0;
  return TREX_OK;
}

int trex_batch_forget_buffers(TrexBatch *b) {
  if (check_batch(b)) return TREX_E_INVALID;
  b->seen.clear();
  return TREX_OK;
}

int trex_batch_reset(TrexBatch *b, const uint8_t *mask_dev, float *obs_out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(mask_dev, n, "trex_batch_reset: mask");
  BUF_TRY(obs_out_dev, n * 3 * b->nj * sizeof(float), "trex_batch_reset: obs_out");
  TrexStepArgs a = step_args(b, TREX_KIND_RESET);
  a.reset_mask = mask_dev; a.obs = obs_out_dev;
  HIP_TRY(trex_launch_step(&a, TREX_KIND_RESET, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_reset_rows(TrexBatch *b, const uint8_t *mask_dev, float *rows_dev, int row_stride, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!rows_dev) return fail(TREX_E_INVALID, "trex_batch_reset_rows: rows is null");
  if (row_stride < 3 * b->nj + (b->pen_in_rows ? 5 : 2)) return fail(TREX_E_INVALID, "trex_batch_reset_rows: row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(mask_dev, n, "trex_batch_reset_rows: mask");
  BUF_TRY(rows_dev, ((n - 1) * row_stride + 3 * b->nj + (b->pen_in_rows ? 5 : 2)) * sizeof(float), "trex_batch_reset_rows: rows");
  TrexStepArgs a = step_args(b, TREX_KIND_RESET);
  a.reset_mask = mask_dev;
  rows_out(b, a, rows_dev, row_stride);
  HIP_TRY(trex_launch_step(&a, TREX_KIND_RESET, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_step(TrexBatch *b, const float *actions_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
                    float *penalties_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!actions_dev) return fail(TREX_E_INVALID, "trex_batch_step: actions is null");
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(actions_dev, n * b->action_cols() * sizeof(float), "trex_batch_step: actions");
  BUF_TRY(obs_dev, n * 3 * b->nj * sizeof(float), "trex_batch_step: obs");
  BUF_TRY(reward_dev, n * sizeof(float), "trex_batch_step: reward");
  BUF_TRY(done_dev, n, "trex_batch_step: done");
  BUF_TRY(penalties_dev, n * 3 * sizeof(float), "trex_batch_step: penalties");
  TrexStepArgs a = step_args(b, TREX_KIND_STEP);
  a.actions = actions_dev; a.obs = obs_dev; a.reward = reward_dev; a.done = done_dev; a.penalties = penalties_dev;
  if (b->term.on && !a.done) a.done = b->term.done;   // (the predicate has to see which envs the step launch ended)
  HIP_TRY(trex_launch_step(&a, TREX_KIND_STEP, (hipStream_t)stream));
  if (b->term.on) HIP_TRY(termination_tail(b, a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_step_rows(TrexBatch *b, const float *actions_dev, float *rows_dev, int row_stride, float *penalties_dev,
                         uint8_t *done_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!actions_dev || !rows_dev) return fail(TREX_E_INVALID, "trex_batch_step_rows: null argument");
  if (row_stride < 3 * b->nj + (b->pen_in_rows ? 5 : 2)) return fail(TREX_E_INVALID, "trex_batch_step_rows: row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(actions_dev, n * b->action_cols() * sizeof(float), "trex_batch_step_rows: actions");
  BUF_TRY(rows_dev, ((n - 1) * row_stride + 3 * b->nj + (b->pen_in_rows ? 5 : 2)) * sizeof(float), "trex_batch_step_rows: rows");
  BUF_TRY(penalties_dev, n * 3 * sizeof(float), "trex_batch_step_rows: penalties");
  BUF_TRY(done_dev, n, "trex_batch_step_rows: done");
  TrexStepArgs a = step_args(b, TREX_KIND_STEP);
  a.actions = actions_dev; a.done = done_dev; a.penalties = penalties_dev;
  rows_out(b, a, rows_dev, row_stride);
  HIP_TRY(trex_launch_step(&a, TREX_KIND_STEP, (hipStream_t)stream));
  if (b->term.on) HIP_TRY(termination_tail(b, a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_step_many(TrexBatch *b, const float *actions_dev, float *rows_dev, int row_stride, int num_steps,
                         float *penalties_dev, uint8_t *done_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!actions_dev || !rows_dev) return fail(TREX_E_INVALID, "trex_batch_step_many: null argument");
  if (num_steps < 1) return fail(TREX_E_INVALID, "trex_batch_step_many: num_steps must be >= 1");
  if (row_stride < 3 * b->nj + (b->pen_in_rows ? 5 : 2)) return fail(TREX_E_INVALID, "trex_batch_step_many: row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n, S = (size_t)num_steps;
  BUF_TRY(actions_dev, S * n * b->action_cols() * sizeof(float), "trex_batch_step_many: actions");
  BUF_TRY(rows_dev, ((S * n - 1) * row_stride + 3 * b->nj + (b->pen_in_rows ? 5 : 2)) * sizeof(float), "trex_batch_step_many: rows");
  BUF_TRY(penalties_dev, S * n * 3 * sizeof(float), "trex_batch_step_many: penalties");
  BUF_TRY(done_dev, S * n, "trex_batch_step_many: done");
  if (b->term.on) {   // S triplets step, predicate, reset from the host: what S trex_batch_step_rows calls enqueue
    for (size_t s = 0; s < S; s++) {
      TrexStepArgs a = step_args(b, TREX_KIND_STEP);
      a.actions = actions_dev + s * n * b->action_cols();
      a.done = done_dev ? done_dev + s * n : nullptr;
      a.penalties = penalties_dev ? penalties_dev + s * n * 3 : nullptr;
      rows_out(b, a, rows_dev + s * n * (size_t)row_stride, row_stride);
      HIP_TRY(trex_launch_step(&a, TREX_KIND_STEP, (hipStream_t)stream));
      HIP_TRY(termination_tail(b, a, (hipStream_t)stream));
    }
    return TREX_OK;
  }
  TrexStepArgs a = step_args(b, TREX_KIND_STEP_MANY);
  a.actions = actions_dev; a.done = done_dev; a.penalties = penalties_dev;
  rows_out(b, a, rows_dev, row_stride);
  a.n_steps = num_steps; a.step_rows = (long long)b->n * row_stride;
  HIP_TRY(trex_launch_step(&a, TREX_KIND_STEP_MANY, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_debug_step(TrexBatch *b, const float *actions_dev, float *obs_dev, float *debug_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!actions_dev || !debug_dev) return fail(TREX_E_INVALID, "trex_batch_debug_step: null argument");
  DeviceGuard guard(b->device);
  BUF_TRY(actions_dev, (size_t)b->n * b->nj * sizeof(float), "trex_batch_debug_step: actions");
  BUF_TRY(obs_dev, (size_t)b->n * 3 * b->nj * sizeof(float), "trex_batch_debug_step: obs");
  BUF_TRY(debug_dev, 4096 * sizeof(float), "trex_batch_debug_step: debug");   // (diagnostic builds: 4096 + 16 N)
  if (b->warm)   // (the diagnostics instantiation has no warm-start record: it would step cold without saying so)
    return fail(TREX_E_INVALID, "trex_batch_debug_step: not available for a batch with warmstart > 0");
  if (b->ext_on)   // (nor an external wrench)
    return fail(TREX_E_INVALID, "trex_batch_debug_step: not available while an external wrench is set");
  if (b->sens_on)   // (nor the contact sensor)
    return fail(TREX_E_INVALID, "trex_batch_debug_step: not available while the contact sensor is on");
  if (b->act_on())   // (nor the actuator model)
    return fail(TREX_E_INVALID, "trex_batch_debug_step: not available while control modes, motor gains or stiffness actions are set");
  if (b->term.on)   // (nor the predicate and reset launches of fall termination)
    return fail(TREX_E_INVALID, "trex_batch_debug_step: not available while termination is on (trex_batch_set_termination)");
  TrexStepArgs a = step_args(b, TREX_KIND_STEP_DEBUG);
  a.actions = actions_dev; a.obs = obs_dev; a.debug = debug_dev;
  HIP_TRY(trex_launch_step(&a, TREX_KIND_STEP_DEBUG, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_set_episode_limit(TrexBatch *b, int max_episode_steps, const int32_t *episode_steps_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (max_episode_steps < 0) return fail(TREX_E_INVALID, "max_episode_steps must be >= 0 (0 = no limit)");
  DeviceGuard guard(b->device);
  BUF_TRY(episode_steps_dev, (size_t)b->n * sizeof(int32_t), "trex_batch_set_episode_limit: episode_steps");
  b->arr.max_episode_steps = max_episode_steps;
  HIP_TRY(trex_launch_scalars_set(b->arr, b->n, episode_steps_dev, 1, -1, (hipStream_t)stream));
  return TREX_OK;
}
int trex_batch_get_episode_steps(TrexBatch *b, int32_t *episode_steps_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!episode_steps_dev) return fail(TREX_E_INVALID, "episode_steps is null");
  DeviceGuard guard(b->device);
  BUF_TRY(episode_steps_dev, (size_t)b->n * sizeof(int32_t), "trex_batch_get_episode_steps: episode_steps");
  HIP_TRY(trex_launch_scalars_get(b->arr, b->n, nullptr, nullptr, episode_steps_dev, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_get_state(TrexBatch *b, float *state_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!state_dev) return fail(TREX_E_INVALID, "state is null");
  DeviceGuard guard(b->device);
  BUF_TRY(state_dev, (size_t)b->n * (13 + 2 * b->nj) * sizeof(float), "trex_batch_get_state: state");
  HIP_TRY(trex_launch_pack_state(b->dmodel, b->arr, b->n, state_dev, 1, (hipStream_t)stream));
  return TREX_OK;
}
int trex_batch_set_state(TrexBatch *b, const float *state_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!state_dev) return fail(TREX_E_INVALID, "state is null");
  DeviceGuard guard(b->device);
  BUF_TRY(state_dev, (size_t)b->n * (13 + 2 * b->nj) * sizeof(float), "trex_batch_set_state: state");
  HIP_TRY(trex_launch_pack_state(b->dmodel, b->arr, b->n, const_cast<float *>(state_dev), 0, (hipStream_t)stream));
  if (b->warm)   // the recorded impulses belong to the states just replaced: every record is emptied
    HIP_TRY(hipMemsetAsync(b->warm, 0, (size_t)b->n * TREX_WARM_WORDS * sizeof(float), (hipStream_t)stream));
  return TREX_OK;
}
int trex_batch_set_motors_enabled(TrexBatch *b, int enabled, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  HIP_TRY(trex_launch_scalars_set(b->arr, b->n, nullptr, 0, enabled ? 1 : 0, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_head_position(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(out_dev, (size_t)b->n * 3 * sizeof(float), "trex_batch_head_position: out");
  HIP_TRY(trex_launch_head(b->dmodel, b->arr, b->n, out_dev, (hipStream_t)stream));
  return TREX_OK;
}

int trex_model_num_links(const TrexModel *m) { return m ? (int)m->host.link_names.size() : fail(TREX_E_INVALID, "null model"); }
int trex_model_link_info(const TrexModel *m, int link, const char **name, int *body) {
  if (!m) return fail(TREX_E_INVALID, "null model");
  if (link < 0 || link >= (int)m->host.link_names.size()) return fail(TREX_E_INVALID, "link index out of range");
  if (name) *name = m->host.link_names[link].c_str();
  if (body) *body = m->host.link_body[link];
  return TREX_OK;
}
int trex_batch_link_transforms(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(out_dev, (size_t)b->n * b->arr.num_links * 7 * sizeof(float), "trex_batch_link_transforms: out");
  HIP_TRY(trex_launch_link_transforms(b->dmodel, b->arr, b->n, out_dev, (hipStream_t)stream, 0));
  return TREX_OK;
}

int trex_model_num_visuals(const TrexModel *m) { return m ? (int)m->host.visual_file.size() : fail(TREX_E_INVALID, "null model"); }
int trex_model_visual_info(const TrexModel *m, int visual, const char **mesh_file, int *link, double xyz[3], double quat_xyzw[4]) {
  if (!m) return fail(TREX_E_INVALID, "null model");
  if (visual < 0 || visual >= (int)m->host.visual_file.size()) return fail(TREX_E_INVALID, "visual index out of range");
  if (mesh_file) *mesh_file = m->host.visual_file[visual].c_str();
  if (link) *link = m->host.visual_link[visual];
  const trex::Tf &t = m->host.visual_origin[visual];
  if (xyz) { xyz[0] = t.t.x; xyz[1] = t.t.y; xyz[2] = t.t.z; }
  if (quat_xyzw) trex::matrix_to_quat(t.R, quat_xyzw);
  return TREX_OK;
}
int trex_batch_visual_transforms(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "out is null");
  if (b->arr.num_visuals == 0) return fail(TREX_E_INVALID, "the model has no <visual> meshes");
  DeviceGuard guard(b->device);
  BUF_TRY(out_dev, (size_t)b->n * b->arr.num_visuals * 7 * sizeof(float), "trex_batch_visual_transforms: out");
  HIP_TRY(trex_launch_link_transforms(b->dmodel, b->arr, b->n, out_dev, (hipStream_t)stream, 1));
  return TREX_OK;
}

int trex_batch_set_domain(TrexBatch *b, const float *mass_scale_dev, const float *friction_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  BUF_TRY(mass_scale_dev, (size_t)b->n * b->nb * sizeof(float), "trex_batch_set_domain: mass_scale");
  BUF_TRY(friction_dev, (size_t)b->n * sizeof(float), "trex_batch_set_domain: friction");
  if (mass_scale_dev) HIP_TRY(trex_launch_copy_mass_scale(mass_scale_dev, b->arr.mass_scale, b->n, b->nb, (hipStream_t)stream));
  if (friction_dev) HIP_TRY(hipMemcpyAsync(b->arr.friction, friction_dev, b->n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (mass_scale_dev || friction_dev) b->arr.domain = 1;   // from now on the step launches read the per-env arrays
  return TREX_OK;
}

int trex_batch_set_external_wrench(TrexBatch *b, const float *wrench_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!wrench_dev) { b->ext_on = false; return TREX_OK; }   // the default kernels again; the buffer stays for the next call
  DeviceGuard guard(b->device);
  BUF_TRY(wrench_dev, (size_t)b->n * b->nb * 6 * sizeof(float), "trex_batch_set_external_wrench: wrench");
  if (!b->ext) {   // first use: a batch that never sets a wrench allocates nothing
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, (size_t)b->n * 6 * TREX_TL * sizeof(float)));
    b->allocs.push_back(p);
    b->ext = (float *)p;
  }
  HIP_TRY(trex_launch_copy_wrench(wrench_dev, b->ext, b->n, b->nb, (hipStream_t)stream));
  b->ext_on = true;
  return TREX_OK;
}

int trex_batch_set_control_mode(TrexBatch *b, const int32_t *mode_host) {
  if (check_batch(b)) return TREX_E_INVALID;
  uint32_t vel = 0u, tor = 0u;
  for (int k = 0; mode_host && k < b->nj; k++) {
    const int32_t m = mode_host[k];
    if (m < TREX_CTRL_POSITION || m > TREX_CTRL_TORQUE)
      return fail(TREX_E_INVALID, "trex_batch_set_control_mode: mode " + std::to_string(m) + " of joint " + std::to_string(k) +
                                      " (0 position, 1 velocity, 2 torque)");
    if (m == TREX_CTRL_VELOCITY) vel |= 1u << b->obs_order[k];
    if (m == TREX_CTRL_TORQUE) tor |= 1u << b->obs_order[k];
  }
  if ((vel | tor) != 0u)
    if (int c = ensure_gains(b)) return c;
  b->vel_mask = vel; b->tor_mask = tor;
  return TREX_OK;
}

int trex_batch_set_motor_gains(TrexBatch *b, const float *kp_dev, const float *kd_dev, const float *max_force_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  const size_t bytes = (size_t)b->n * b->nj * sizeof(float);
  BUF_TRY(kp_dev, bytes, "trex_batch_set_motor_gains: kp");
  BUF_TRY(kd_dev, bytes, "trex_batch_set_motor_gains: kd");
  BUF_TRY(max_force_dev, bytes, "trex_batch_set_motor_gains: max_force");
  const bool any = kp_dev || kd_dev || max_force_dev;
  if (!any && !b->gains) { b->gains_set = false; return TREX_OK; }   // nothing was ever set: nothing to clear, nothing allocated
  if (int c = ensure_gains(b)) return c;
  // (all three NULL: the buffer goes back to the model parameters - control modes and stiffness actions keep reading it)
  HIP_TRY(trex_launch_copy_gains(b->dmodel, kp_dev, kd_dev, max_force_dev, b->gains, b->n, (hipStream_t)stream));
  b->gains_set = any;
  return TREX_OK;
}

int trex_batch_set_stiffness_actions(TrexBatch *b, int enabled, float kp_max) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!enabled) { b->stiff = false; return TREX_OK; }
  if (!std::isfinite(kp_max) || kp_max < 0.f) return fail(TREX_E_INVALID, "trex_batch_set_stiffness_actions: kp_max must be finite and >= 0");
  if (int c = ensure_gains(b)) return c;
  b->stiff = true; b->kp_max = kp_max;
  return TREX_OK;
}

int trex_batch_set_contact_sensor(TrexBatch *b, int enabled) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!enabled) { b->sens_on = false; return TREX_OK; }   // the default kernels again; the buffer stays for the next enable
  if (!b->sens) {   // first enable: a batch that never enables the sensor allocates nothing; zeros until a launch records
    DeviceGuard guard(b->device);
    const size_t bytes = (size_t)b->n * TREX_SENS_FLOATS * sizeof(float);
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    b->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, bytes));
    HIP_TRY(hipDeviceSynchronize());   // (the zeros are in place before a launch on any stream)
    b->sens = (float *)p;
  }
  b->sens_on = true;
  return TREX_OK;
}

int trex_batch_contact_wrench(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!b->sens_on) return fail(TREX_E_INVALID, "trex_batch_contact_wrench: the contact sensor is off (trex_batch_set_contact_sensor)");
  if (!out_dev) return fail(TREX_E_INVALID, "trex_batch_contact_wrench: out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(out_dev, (size_t)b->n * b->nb * 6 * sizeof(float), "trex_batch_contact_wrench: out");
  HIP_TRY(trex_launch_contact_wrench(b->sens, out_dev, b->n, b->nb, (hipStream_t)stream));
  return TREX_OK;
}

// ---- dynamics queries (dynamics.hip): read the state, write only their outputs; nothing allocated, nothing waited for
static TrexDynArgs dyn_args(const TrexBatch *b, float *out) {
  TrexDynArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q; a.qd = b->arr.qd;
  a.mass_scale = b->arr.domain ? b->arr.mass_scale : nullptr;
  a.n_envs = b->n; a.nb = b->nb; a.out = out;
  return a;
}

int trex_batch_inverse_dynamics(TrexBatch *b, const float *accel_dev, float *force_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!force_dev) return fail(TREX_E_INVALID, "trex_batch_inverse_dynamics: force is null");
  DeviceGuard guard(b->device);
  const size_t bytes = (size_t)b->n * (6 + b->nj) * sizeof(float);
  BUF_TRY(accel_dev, bytes, "trex_batch_inverse_dynamics: accel");
  BUF_TRY(force_dev, bytes, "trex_batch_inverse_dynamics: force");
  TrexDynArgs a = dyn_args(b, force_dev);
  a.accel = accel_dev;
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_INVERSE_DYNAMICS, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_mass_matrix(TrexBatch *b, float *M_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!M_dev) return fail(TREX_E_INVALID, "trex_batch_mass_matrix: M is null");
  DeviceGuard guard(b->device);
  const size_t D = 6 + (size_t)b->nj;
  BUF_TRY(M_dev, (size_t)b->n * D * D * sizeof(float), "trex_batch_mass_matrix: M");
  HIP_TRY(trex_launch_dynamics(dyn_args(b, M_dev), TREX_DYN_MASS_MATRIX, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_jacobian(TrexBatch *b, int link, const double local_xyz[3], float *J_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!J_dev || !local_xyz) return fail(TREX_E_INVALID, "trex_batch_jacobian: null argument");
  if (link < 0 || link >= (int)b->link_body.size())
    return fail(TREX_E_INVALID, "trex_batch_jacobian: link " + std::to_string(link) + " out of range [0, " +
                                    std::to_string(b->link_body.size()) + ")");
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(local_xyz[c])) return fail(TREX_E_INVALID, "trex_batch_jacobian: local_xyz is not finite");
  DeviceGuard guard(b->device);
  BUF_TRY(J_dev, (size_t)b->n * 6 * (6 + b->nj) * sizeof(float), "trex_batch_jacobian: J");
  TrexDynArgs a = dyn_args(b, J_dev);
  // the point in the frame of the link's body: body<-link transform of "link_tf"
  const trex::Tf &t = b->link_tf[link];
  const double tt[3] = {t.t.x, t.t.y, t.t.z};
  a.jac_body = b->link_body[link];
  for (int r = 0; r < 3; r++)
    a.jac_point[r] = (float)(t.R.m[3 * r] * local_xyz[0] + t.R.m[3 * r + 1] * local_xyz[1] + t.R.m[3 * r + 2] * local_xyz[2] + tt[r]);
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_JACOBIAN, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_centroidal(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "trex_batch_centroidal: out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(out_dev, (size_t)b->n * TREX_DYN_CENT_FLOATS * sizeof(float), "trex_batch_centroidal: out");
  HIP_TRY(trex_launch_dynamics(dyn_args(b, out_dev), TREX_DYN_CENTROIDAL, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_forward_dynamics(TrexBatch *b, const float *force_dev, float *accel_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!accel_dev) return fail(TREX_E_INVALID, "trex_batch_forward_dynamics: accel is null");
  DeviceGuard guard(b->device);
  const size_t bytes = (size_t)b->n * (6 + b->nj) * sizeof(float);
  BUF_TRY(force_dev, bytes, "trex_batch_forward_dynamics: force");
  BUF_TRY(accel_dev, bytes, "trex_batch_forward_dynamics: accel");
  TrexDynArgs a = dyn_args(b, accel_dev);
  a.rhs = force_dev;
  a.num_rhs = 1;
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_FORWARD_DYNAMICS, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_solve_mass(TrexBatch *b, const float *rhs_dev, int num_rhs, float *x_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!x_dev) return fail(TREX_E_INVALID, "trex_batch_solve_mass: x is null");
  if (num_rhs < 1 || num_rhs > TREX_DYN_MAX_RHS)
    return fail(TREX_E_INVALID, "trex_batch_solve_mass: num_rhs " + std::to_string(num_rhs) + " outside 1.." + std::to_string(TREX_DYN_MAX_RHS));
  if (!rhs_dev && num_rhs != 6 + b->nj)
    return fail(TREX_E_INVALID, "trex_batch_solve_mass: a null rhs is the identity, num_rhs must be " + std::to_string(6 + b->nj));
  DeviceGuard guard(b->device);
  const size_t bytes = (size_t)b->n * num_rhs * (6 + b->nj) * sizeof(float);
  BUF_TRY(rhs_dev, bytes, "trex_batch_solve_mass: rhs");
  BUF_TRY(x_dev, bytes, "trex_batch_solve_mass: x");
  TrexDynArgs a = dyn_args(b, x_dev);
  a.rhs = rhs_dev;
  a.num_rhs = num_rhs;
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_SOLVE_MASS, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_contact_stats(TrexBatch *b, int32_t *count_dev, float *normal_impulse_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  BUF_TRY(count_dev, (size_t)b->n * sizeof(int32_t), "trex_batch_contact_stats: count");
  BUF_TRY(normal_impulse_dev, (size_t)b->n * sizeof(float), "trex_batch_contact_stats: normal_impulse");
  if (count_dev || normal_impulse_dev)
    HIP_TRY(trex_launch_scalars_get(b->arr, b->n, count_dev, normal_impulse_dev, nullptr, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_launch_info(const TrexBatch *b, int *grid, int *block, int *lds_bytes, int *alg_bytes_per_env_step) {
  if (!b) return fail(TREX_E_INVALID, "null batch");
  // the shape the step launch of this batch takes (trex_launch_step asks the same function)
  const TrexStepShape shape = trex_step_launch_shape(TREX_KIND_STEP, b->n, trex_step_features(step_args(b, TREX_KIND_STEP)));
  if (grid) *grid = shape.grid;
  if (block) *block = shape.block;
  if (lds_bytes) *lds_bytes = shape.lds_bytes;
  // state in + out (13 + 2J floats each), action in (J), obs out (3J), reward (4 B), done (padded 4 B): SURVEY 8d
  if (alg_bytes_per_env_step) *alg_bytes_per_env_step = 4 * (2 * (13 + 2 * b->nj) + b->nj + 3 * b->nj + 1 + 1);
  return TREX_OK;
}

int trex_batch_time_steps(TrexBatch *b, const float *actions_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
                          int steps, void *stream, float *avg_ms_out) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!actions_dev || !avg_ms_out || steps <= 0) return fail(TREX_E_INVALID, "trex_batch_time_steps: bad argument");
  if (b->term.on)   // (it times the step launch alone: with termination on a step is three launches)
    return fail(TREX_E_INVALID, "trex_batch_time_steps: not available while termination is on (trex_batch_set_termination)");
  DeviceGuard guard(b->device);
  BUF_TRY(actions_dev, (size_t)b->n * b->action_cols() * sizeof(float), "trex_batch_time_steps: actions");
  BUF_TRY(obs_dev, (size_t)b->n * 3 * b->nj * sizeof(float), "trex_batch_time_steps: obs");
  BUF_TRY(reward_dev, (size_t)b->n * sizeof(float), "trex_batch_time_steps: reward");
  BUF_TRY(done_dev, (size_t)b->n, "trex_batch_time_steps: done");
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipEventRecord(e0, s));
  TrexStepArgs a = step_args(b, TREX_KIND_STEP);
  a.actions = actions_dev; a.obs = obs_dev; a.reward = reward_dev; a.done = done_dev;
  for (int i = 0; i < steps; i++) HIP_TRY(trex_launch_step(&a, TREX_KIND_STEP, s));
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms_out = ms / steps;
  return TREX_OK;
}

// The primitive / plane table the renderer and the ray casts share (render.cpp), once per batch and made by whichever call comes
// first (trex_model_load stays as fast as it was). `who`: the calling entry point, for the message.
static int ensure_render_table(TrexBatch *b, const char *who) {
  if (b->render_ready) return TREX_OK;
  trex::HostModel hm;
  hm.nb = b->nb;
  hm.hull_xyz = b->hull_xyz; hm.hull_radius = b->hull_radius; hm.hull_start = b->hull_start; hm.hull_group_start = b->hull_group_start;
  std::vector<TrexRenderPrim> prims;
  std::vector<float> planes;
  const int np = trex::render_table(hm, prims, planes);
  if (np > TREX_RENDER_MAXPRIM)
    return fail(TREX_E_UNSUPPORTED, std::string(who) + ": the model has " + std::to_string(np) + " drawable primitives, the renderer " +
                                        std::to_string(TREX_RENDER_MAXPRIM));
  if (planes.empty()) planes.assign(4, 0.f);
  if (prims.empty()) prims.resize(1);
  void *pp = nullptr, *pl = nullptr;
  HIP_TRY(hipMalloc(&pp, prims.size() * sizeof(TrexRenderPrim)));
  b->allocs.push_back(pp);
  HIP_TRY(hipMalloc(&pl, planes.size() * sizeof(float)));
  b->allocs.push_back(pl);
  HIP_TRY(hipMemcpy(pp, prims.data(), prims.size() * sizeof(TrexRenderPrim), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(pl, planes.data(), planes.size() * sizeof(float), hipMemcpyHostToDevice));
  b->render_prim = (TrexRenderPrim *)pp; b->render_plane = (float4 *)pl; b->render_nprim = np;
  b->render_ready = true;
  return TREX_OK;
}


int trex_batch_render(TrexBatch *b, const TrexCamera *cam, int width, int height, const int32_t *env_ids, int num_views,
                      uint8_t *rgb_dev, float *depth_dev, int32_t *seg_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!cam) return fail(TREX_E_INVALID, "trex_batch_render: camera is null");
  if (width <= 0 || height <= 0 || width > TREX_RENDER_MAXDIM || height > TREX_RENDER_MAXDIM)
    return fail(TREX_E_INVALID, "trex_batch_render: width and height must lie in [1, " + std::to_string(TREX_RENDER_MAXDIM) + "]");
  if (!rgb_dev && !depth_dev && !seg_dev) return fail(TREX_E_INVALID, "trex_batch_render: all three outputs are null");
  const float cv[] = {cam->distance, cam->yaw_deg, cam->pitch_deg, cam->fov_deg, cam->near_z, cam->far_z,
                      cam->target[0], cam->target[1], cam->target[2]};
  for (float x : cv)
    if (!std::isfinite(x)) return fail(TREX_E_INVALID, "trex_batch_render: camera value is not finite");
  if (!(cam->distance > 0) || !(cam->fov_deg > 0 && cam->fov_deg < 180) || !(cam->near_z > 0 && cam->far_z > cam->near_z))
    return fail(TREX_E_INVALID, "trex_batch_render: camera needs distance > 0, 0 < fov < 180, 0 < near < far");
  if (env_ids) {
    if (num_views <= 0) return fail(TREX_E_INVALID, "trex_batch_render: num_views must be positive");
    for (int v = 0; v < num_views; v++)
      if (env_ids[v] < 0 || env_ids[v] >= b->n)
        return fail(TREX_E_INVALID, "trex_batch_render: env id " + std::to_string(env_ids[v]) + " out of range [0, " +
                                        std::to_string(b->n) + ")");
  } else {
    if (num_views != 0 && num_views != b->n) return fail(TREX_E_INVALID, "trex_batch_render: env_ids NULL needs num_views 0 or N");
    num_views = b->n;
  }
  if (num_views > 65535) return fail(TREX_E_INVALID, "trex_batch_render: at most 65535 views per call");
  DeviceGuard guard(b->device);
  const size_t px = (size_t)num_views * height * width;
  BUF_TRY(rgb_dev, px * 3, "trex_batch_render: rgb");
  BUF_TRY(depth_dev, px * sizeof(float), "trex_batch_render: depth");
  BUF_TRY(seg_dev, px * sizeof(int32_t), "trex_batch_render: seg");
  hipStream_t s = (hipStream_t)stream;
  if (int c = ensure_render_table(b, "trex_batch_render")) return c;
  if (env_ids) {
    if (b->render_ids_cap < (size_t)num_views) {   // (grows rarely: the old buffer may still be read by an earlier call)
      HIP_TRY(hipDeviceSynchronize());
      if (b->render_ids) (void)hipFree(b->render_ids);
      b->render_ids = nullptr; b->render_ids_cap = 0;
      HIP_TRY(hipMalloc((void **)&b->render_ids, (size_t)num_views * sizeof(int32_t)));
      b->render_ids_cap = (size_t)num_views;
    }
    HIP_TRY(hipMemcpyAsync(b->render_ids, env_ids, (size_t)num_views * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  // camera (include/trex_batch.h): eye = target + Rz(yaw) Rx(pitch) (0, -distance, 0), up = Rz(yaw) Rx(pitch) (0, 0, 1)
  const double d2r = 3.14159265358979323846 / 180.0, yw = cam->yaw_deg * d2r, pt = cam->pitch_deg * d2r;
  const double off[3] = {cam->distance * std::cos(pt) * std::sin(yw), -cam->distance * std::cos(pt) * std::cos(yw),
                         -cam->distance * std::sin(pt)};
  const double up0[3] = {std::sin(pt) * std::sin(yw), -std::sin(pt) * std::cos(yw), std::cos(pt)};
  double f[3] = {-off[0] / cam->distance, -off[1] / cam->distance, -off[2] / cam->distance};
  double r[3] = {f[1] * up0[2] - f[2] * up0[1], f[2] * up0[0] - f[0] * up0[2], f[0] * up0[1] - f[1] * up0[0]};
  const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (double &x : r) x /= rl;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  TrexRenderArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q;
  a.env_ids = env_ids ? b->render_ids : nullptr;
  a.prim = b->render_prim; a.plane = b->render_plane;
  a.rgb = rgb_dev; a.depth = depth_dev; a.seg = seg_dev;
  a.num_views = num_views; a.width = width; a.height = height;
  a.nprim = b->render_nprim; a.follow_base = cam->follow_base != 0;
  for (int c = 0; c < 3; c++) {
    a.target[c] = cam->target[c]; a.offset[c] = (float)off[c];
    a.fwd[c] = (float)f[c]; a.right[c] = (float)r[c]; a.up[c] = (float)u[c];
  }
  const double ty = std::tan(0.5 * cam->fov_deg * d2r);
  a.tan_y = (float)ty; a.tan_x = (float)(ty * width / height);
  a.near_z = cam->near_z; a.far_z = cam->far_z;
  a.floor_z = (float)b->floor_z;
  HIP_TRY(trex_launch_render(a, s));
  return TREX_OK;
}

int trex_batch_ray_test(TrexBatch *b, const float *rays_dev, int num_rays, int shared, int link, uint32_t body_mask, int hit_floor,
                        float *fraction_dev, int32_t *body_dev, float *position_dev, float *normal_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!rays_dev || !fraction_dev) return fail(TREX_E_INVALID, "trex_batch_ray_test: rays or fraction is null");
  if (num_rays < 1 || num_rays > TREX_RAY_MAXRAYS)
    return fail(TREX_E_INVALID, "trex_batch_ray_test: num_rays " + std::to_string(num_rays) + " outside [1, " +
                                    std::to_string(TREX_RAY_MAXRAYS) + "]");
  if (link < -1 || link >= (int)b->link_body.size())
    return fail(TREX_E_INVALID, "trex_batch_ray_test: link " + std::to_string(link) + " out of range [-1, " +
                                    std::to_string(b->link_body.size()) + ")");
  DeviceGuard guard(b->device);
  const size_t nr = (size_t)b->n * num_rays;
  BUF_TRY(rays_dev, (shared ? (size_t)num_rays : nr) * 6 * sizeof(float), "trex_batch_ray_test: rays");
  BUF_TRY(fraction_dev, nr * sizeof(float), "trex_batch_ray_test: fraction");
  BUF_TRY(body_dev, nr * sizeof(int32_t), "trex_batch_ray_test: body");
  BUF_TRY(position_dev, nr * 3 * sizeof(float), "trex_batch_ray_test: position");
  BUF_TRY(normal_dev, nr * 3 * sizeof(float), "trex_batch_ray_test: normal");
  if (int c = ensure_render_table(b, "trex_batch_ray_test")) return c;
  TrexRayArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q;
  a.rays = rays_dev; a.fraction = fraction_dev; a.body = body_dev; a.position = position_dev; a.normal = normal_dev;
  a.n_envs = b->n; a.num_rays = num_rays; a.shared = shared != 0;
  a.link_body = -1;
  if (link >= 0) {   // the frame of the link in its body: body <- link of "link_tf"
    const trex::Tf &t = b->link_tf[link];
    a.link_body = b->link_body[link];
    for (int k = 0; k < 9; k++) a.link_tf[k] = (float)t.R.m[k];
    a.link_tf[9] = (float)t.t.x; a.link_tf[10] = (float)t.t.y; a.link_tf[11] = (float)t.t.z;
  }
  a.nprim = b->render_nprim; a.hit_floor = hit_floor != 0;
  a.body_mask = b->nb >= 32 ? body_mask : body_mask & ((1u << b->nb) - 1u);   // (bits beyond the model's bodies mean nothing)
  a.floor_z = (float)b->floor_z;
  HIP_TRY(trex_launch_ray_test(a, b->render_prim, b->render_plane, (hipStream_t)stream));
  return TREX_OK;
}

// ---- link kinematics (link_state.hip)
int trex_batch_set_link_probes(TrexBatch *b, int set, const int32_t *link_host, const double *local_xyz_host, int num_probes) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (set < 0 || set >= TREX_LINK_SETS)
    return fail(TREX_E_INVALID, "trex_batch_set_link_probes: set " + std::to_string(set) + " outside [0, " + std::to_string(TREX_LINK_SETS) + ")");
  if (num_probes < 0 || num_probes > TREX_LINK_MAXPROBES)
    return fail(TREX_E_INVALID, "trex_batch_set_link_probes: num_probes " + std::to_string(num_probes) + " outside [0, " +
                                    std::to_string(TREX_LINK_MAXPROBES) + "]");
  if (num_probes > 0 && (!link_host || !local_xyz_host)) return fail(TREX_E_INVALID, "trex_batch_set_link_probes: null argument");
  std::vector<int32_t> body((size_t)num_probes);
  std::vector<float> tf((size_t)num_probes * 12);
  for (int k = 0; k < num_probes; k++) {
    const int link = link_host[k];
    if (link < 0 || link >= (int)b->link_body.size())
      return fail(TREX_E_INVALID, "trex_batch_set_link_probes: probe " + std::to_string(k) + ": link " + std::to_string(link) +
                                      " out of range [0, " + std::to_string(b->link_body.size()) + ")");
    const double *x = local_xyz_host + 3 * (size_t)k;
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(x[c]))
        return fail(TREX_E_INVALID, "trex_batch_set_link_probes: probe " + std::to_string(k) + ": local_xyz is not finite");
    // body <- link rotation, and the point in the frame of the link's body (as trex_batch_jacobian composes it)
    const trex::Tf &t = b->link_tf[link];
    const double tt[3] = {t.t.x, t.t.y, t.t.z};
    body[k] = b->link_body[link];
    for (int c = 0; c < 9; c++) tf[12 * (size_t)k + c] = (float)t.R.m[c];
    for (int r = 0; r < 3; r++)
      tf[12 * (size_t)k + 9 + r] = (float)(t.R.m[3 * r] * x[0] + t.R.m[3 * r + 1] * x[1] + t.R.m[3 * r + 2] * x[2] + tt[r]);
  }
  DeviceGuard guard(b->device);
  int32_t *body_dev = nullptr;
  float *tf_dev = nullptr;
  if (num_probes > 0) {
    HIP_TRY(hipMalloc((void **)&body_dev, body.size() * sizeof(int32_t)));
    hipError_t e = hipMalloc((void **)&tf_dev, tf.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(body_dev, body.data(), body.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tf_dev, tf.data(), tf.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(body_dev);
      if (tf_dev) (void)hipFree(tf_dev);
      return hip_fail(e, "trex_batch_set_link_probes: table");
    }
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  TrexBatch::ProbeSet &ps = b->probes[set];
  if (ps.body) (void)hipFree(ps.body);
  if (ps.tf) (void)hipFree(ps.tf);
  ps.n = num_probes; ps.body = body_dev; ps.tf = tf_dev; ps.host_body = body;
  return TREX_OK;
}

int trex_batch_link_state(TrexBatch *b, int set, int axes, int proper, const float *accel_dev, float *pose_dev, float *velocity_dev,
                          float *acceleration_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (set < 0 || set >= TREX_LINK_SETS)
    return fail(TREX_E_INVALID, "trex_batch_link_state: set " + std::to_string(set) + " outside [0, " + std::to_string(TREX_LINK_SETS) + ")");
  const TrexBatch::ProbeSet &ps = b->probes[set];
  if (ps.n < 1) return fail(TREX_E_INVALID, "trex_batch_link_state: probe set " + std::to_string(set) + " is empty (trex_batch_set_link_probes)");
  if (axes < TREX_AXES_WORLD || axes > TREX_AXES_BASE)
    return fail(TREX_E_INVALID, "trex_batch_link_state: axes " + std::to_string(axes) + " outside 0..2");
  if (!pose_dev && !velocity_dev && !acceleration_dev) return fail(TREX_E_INVALID, "trex_batch_link_state: all three outputs are null");
  DeviceGuard guard(b->device);
  const size_t nk = (size_t)b->n * ps.n;
  if (acceleration_dev) BUF_TRY(accel_dev, (size_t)b->n * (6 + b->nj) * sizeof(float), "trex_batch_link_state: accel");
  BUF_TRY(pose_dev, nk * 7 * sizeof(float), "trex_batch_link_state: pose");
  BUF_TRY(velocity_dev, nk * 6 * sizeof(float), "trex_batch_link_state: velocity");
  BUF_TRY(acceleration_dev, nk * 6 * sizeof(float), "trex_batch_link_state: acceleration");
  TrexLinkArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q; a.qd = b->arr.qd;
  a.accel = acceleration_dev ? accel_dev : nullptr;
  a.probe_body = ps.body; a.probe_tf = ps.tf;
  a.pose = pose_dev; a.vel = velocity_dev; a.acc = acceleration_dev;
  a.n_envs = b->n; a.num_probes = ps.n; a.D = 6 + b->nj;
  a.axes = axes; a.proper = proper != 0;
  const trex::Tf &t0 = b->link_tf[0];   // URDF link 0's frame in its body
  a.base_body = b->link_body[0];
  for (int k = 0; k < 9; k++) a.base_tf[k] = (float)t0.R.m[k];
  a.base_tf[9] = (float)t0.t.x; a.base_tf[10] = (float)t0.t.y; a.base_tf[11] = (float)t0.t.z;
  HIP_TRY(trex_launch_link_state(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---- inverse kinematics (inverse_kinematics.hip)
int trex_batch_inverse_kinematics(TrexBatch *b, int set, const int32_t *mode_host, int frame, const float *target_dev,
                                  const float *q_init_dev, uint32_t joint_mask, const TrexIkParams *params, float *q_out_dev,
                                  float *info_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_inverse_kinematics: ";
  if (set < 0 || set >= TREX_LINK_SETS)
    return fail(TREX_E_INVALID, me + "set " + std::to_string(set) + " outside [0, " + std::to_string(TREX_LINK_SETS) + ")");
  const TrexBatch::ProbeSet &ps = b->probes[set];
  if (ps.n < 1) return fail(TREX_E_INVALID, me + "probe set " + std::to_string(set) + " is empty (trex_batch_set_link_probes)");
  if (ps.n > TREX_IK_MAXPROBES)
    return fail(TREX_E_INVALID, me + "probe set " + std::to_string(set) + " holds " + std::to_string(ps.n) + " probes, at most " +
                                    std::to_string(TREX_IK_MAXPROBES) + " can be targets");
  if (!mode_host || !target_dev || !q_out_dev) return fail(TREX_E_INVALID, me + "null argument");
  if (frame != TREX_AXES_WORLD && frame != TREX_AXES_BASE)
    return fail(TREX_E_INVALID, me + "frame " + std::to_string(frame) + " is neither TREX_AXES_WORLD nor TREX_AXES_BASE");
  if (frame == TREX_AXES_BASE && b->link_body[0] != 0) return fail(TREX_E_INVALID, me + "URDF link 0 does not belong to the base body");
  TrexIkArgs a{};
  int rows = 0;
  for (int k = 0; k < ps.n; k++) {
    const int m = mode_host[k];
    if (m < 1 || m > 3) return fail(TREX_E_INVALID, me + "mode " + std::to_string(m) + " of target " + std::to_string(k) + " outside 1..3");
    a.body[k] = (uint8_t)ps.host_body[k]; a.mode[k] = (uint8_t)m; a.row0[k] = (uint8_t)rows;
    for (int i = ps.host_body[k]; i > 0; i = b->parent[i]) a.chain[k] |= 1u << i;
    rows += m == 3 ? 6 : 3;
  }
  if (rows > TREX_IK_MAXROWS)
    return fail(TREX_E_INVALID, me + std::to_string(rows) + " task rows, at most " + std::to_string(TREX_IK_MAXROWS));
  for (int k = 0; k < b->nj; k++)
    if ((joint_mask >> k) & 1u) a.move_mask |= 1u << b->obs_order[k];
  if (!a.move_mask) return fail(TREX_E_INVALID, me + "joint_mask lets no joint move");
  const TrexIkParams defaults = TREX_IK_DEFAULTS;
  const TrexIkParams &p = params ? *params : defaults;
  if (p.iterations < 1 || p.iterations > 256)
    return fail(TREX_E_INVALID, me + "iterations " + std::to_string(p.iterations) + " outside 1..256");
  for (float v : {p.damping, p.gain, p.max_step, p.tol_pos, p.tol_ori})
    if (!std::isfinite(v) || v < 0.f) return fail(TREX_E_INVALID, me + "a parameter is negative or not finite");
  DeviceGuard guard(b->device);
  const size_t nj = (size_t)b->n * b->nj * sizeof(float);
  BUF_TRY(target_dev, (size_t)b->n * ps.n * 7 * sizeof(float), "trex_batch_inverse_kinematics: target");
  BUF_TRY(q_init_dev, nj, "trex_batch_inverse_kinematics: q_init");
  BUF_TRY(q_out_dev, nj, "trex_batch_inverse_kinematics: q_out");
  BUF_TRY(info_dev, (size_t)b->n * 4 * sizeof(float), "trex_batch_inverse_kinematics: info");
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q;
  a.probe_tf = ps.tf; a.target = target_dev; a.q_init = q_init_dev; a.q_out = q_out_dev; a.info = info_dev;
  a.n_envs = b->n; a.nb = b->nb; a.K = ps.n; a.M = rows; a.frame = frame;
  const trex::Tf &t0 = b->link_tf[0];   // URDF link 0's frame in the base body
  for (int k = 0; k < 9; k++) a.base_tf[k] = (float)t0.R.m[k];
  a.base_tf[9] = (float)t0.t.x; a.base_tf[10] = (float)t0.t.y; a.base_tf[11] = (float)t0.t.z;
  a.iterations = p.iterations; a.damping2 = p.damping * p.damping; a.gain = p.gain; a.max_step = p.max_step;
  a.tol_pos = p.tol_pos; a.tol_ori = p.tol_ori;
  HIP_TRY(trex_launch_inverse_kinematics(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---- proximity queries (proximity.hip)
int trex_batch_set_proximity_shapes(TrexBatch *b, const int32_t *body_host, const double *capsule_host, int num_capsules,
                                    const int32_t *pair_host, int num_pairs) {
  if (check_batch(b)) return TREX_E_INVALID;
  const char *me = "trex_batch_set_proximity_shapes: ";
  if (num_capsules < 0 || num_capsules > TREX_PROX_MAXCAPS)
    return fail(TREX_E_INVALID, me + ("num_capsules " + std::to_string(num_capsules)) + " outside [0, " + std::to_string(TREX_PROX_MAXCAPS) + "]");
  std::vector<float> cap((size_t)num_capsules * 8, 0.f);
  std::vector<int32_t> cap_body((size_t)num_capsules), pair_first;
  std::vector<uint32_t> test;
  if (num_capsules > 0) {
    if (num_pairs < 1 || num_pairs > TREX_PROX_MAXPAIRS)
      return fail(TREX_E_INVALID, me + ("num_pairs " + std::to_string(num_pairs)) + " outside [1, " + std::to_string(TREX_PROX_MAXPAIRS) + "]");
    if (!body_host || !capsule_host || !pair_host) return fail(TREX_E_INVALID, std::string(me) + "null argument");
    std::vector<std::vector<int>> of_body((size_t)b->nb);   // a body's capsules, table order
    for (int c = 0; c < num_capsules; c++) {
      const int body = body_host[c];
      if (body < 0 || body >= b->nb)
        return fail(TREX_E_INVALID, me + ("capsule " + std::to_string(c)) + ": body " + std::to_string(body) + " out of range [0, " +
                                        std::to_string(b->nb) + ")");
      const double *x = capsule_host + 7 * (size_t)c;
      for (int k = 0; k < 7; k++)
        if (!std::isfinite(x[k])) return fail(TREX_E_INVALID, me + ("capsule " + std::to_string(c)) + ": value is not finite");
      if (x[6] < 0) return fail(TREX_E_INVALID, me + ("capsule " + std::to_string(c)) + ": negative radius");
      const double dx = x[3] - x[0], dy = x[4] - x[1], dz = x[5] - x[2];
      const bool sphere = dx * dx + dy * dy + dz * dz < 1e-12;   // (stored with p1 = p0: the kernel then sees a zero axis exactly)
      float *o = cap.data() + 8 * (size_t)c;
      for (int k = 0; k < 3; k++) { o[k] = (float)x[k]; o[4 + k] = sphere ? o[k] : (float)x[3 + k]; }
      o[3] = (float)x[6];
      cap_body[c] = body;
      of_body[body].push_back(c);
    }
    size_t total = 0;
    for (int p = 0; p < num_pairs; p++) {
      const int A = pair_host[2 * p], B = pair_host[2 * p + 1];
      if (A < 0 || A >= b->nb || B < 0 || B >= b->nb || A == B)
        return fail(TREX_E_INVALID, me + ("pair " + std::to_string(p)) + ": bodies (" + std::to_string(A) + ", " + std::to_string(B) +
                                        ") must be two different bodies of the model");
      if (of_body[A].empty() || of_body[B].empty())
        return fail(TREX_E_INVALID, me + ("pair " + std::to_string(p)) + ": a body of the pair has no capsule");
      total += of_body[A].size() * of_body[B].size();
    }
    if (total > TREX_PROX_MAXTESTS)
      return fail(TREX_E_INVALID, me + (std::to_string(total) + " capsule-pair tests, at most ") + std::to_string(TREX_PROX_MAXTESTS));
    test.reserve(total);
    for (int p = 0; p < num_pairs; p++) {
      pair_first.push_back((int32_t)test.size());
      for (int ca : of_body[pair_host[2 * p]])
        for (int cb : of_body[pair_host[2 * p + 1]]) test.push_back(TREX_PROX_TEST(p, ca, cb));
    }
  }
  DeviceGuard guard(b->device);
  // one allocation, every part at a multiple of 16 bytes
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t o_body = up(cap.size() * sizeof(float)), o_test = o_body + up(cap_body.size() * sizeof(int32_t)),
               o_first = o_test + up(test.size() * sizeof(uint32_t)), bytes = o_first + up(pair_first.size() * sizeof(int32_t));
  char *blob = nullptr;
  if (num_capsules > 0) {
    HIP_TRY(hipMalloc((void **)&blob, bytes));
    hipError_t e = hipMemcpy(blob, cap.data(), cap.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(blob + o_body, cap_body.data(), cap_body.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(blob + o_test, test.data(), test.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(blob + o_first, pair_first.data(), pair_first.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(blob);
      return hip_fail(e, "trex_batch_set_proximity_shapes: table");
    }
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  TrexBatch::ProxTable &pt = b->prox;
  if (pt.blob) (void)hipFree(pt.blob);
  pt = TrexBatch::ProxTable{};
  if (num_capsules > 0) {
    pt.caps = num_capsules; pt.pairs = num_pairs; pt.tests = (int)test.size();
    pt.blob = blob;
    pt.cap = (const float *)blob; pt.cap_body = (const int32_t *)(blob + o_body);
    pt.test = (const uint32_t *)(blob + o_test); pt.pair_first = (const int32_t *)(blob + o_first);
  }
  return TREX_OK;
}

int trex_batch_proximity(TrexBatch *b, float *distance_dev, float *point_a_dev, float *point_b_dev, float *normal_dev,
                         int32_t *capsule_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::ProxTable &pt = b->prox;
  if (pt.caps < 1) return fail(TREX_E_INVALID, "trex_batch_proximity: no table is set (trex_batch_set_proximity_shapes)");
  if (!distance_dev) return fail(TREX_E_INVALID, "trex_batch_proximity: distance is null");
  DeviceGuard guard(b->device);
  const size_t np = (size_t)b->n * pt.pairs;
  BUF_TRY(distance_dev, np * sizeof(float), "trex_batch_proximity: distance");
  BUF_TRY(point_a_dev, np * 3 * sizeof(float), "trex_batch_proximity: point_a");
  BUF_TRY(point_b_dev, np * 3 * sizeof(float), "trex_batch_proximity: point_b");
  BUF_TRY(normal_dev, np * 3 * sizeof(float), "trex_batch_proximity: normal");
  BUF_TRY(capsule_dev, np * 2 * sizeof(int32_t), "trex_batch_proximity: capsule");
  TrexProxArgs a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q;
  a.cap = pt.cap; a.cap_body = pt.cap_body; a.test = pt.test; a.pair_first = pt.pair_first;
  a.distance = distance_dev; a.point_a = point_a_dev; a.point_b = point_b_dev; a.normal = normal_dev; a.capsule = capsule_dev;
  a.n_envs = b->n; a.num_capsules = pt.caps; a.num_pairs = pt.pairs; a.num_tests = pt.tests;
  HIP_TRY(trex_launch_proximity(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---- floor clearance and fall termination (termination.hip)
int trex_batch_body_clearance(TrexBatch *b, float *clearance_dev, float *lowest_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!clearance_dev) return fail(TREX_E_INVALID, "trex_batch_body_clearance: clearance is null");
  DeviceGuard guard(b->device);
  const size_t nb = (size_t)b->n * b->nb;
  BUF_TRY(clearance_dev, nb * sizeof(float), "trex_batch_body_clearance: clearance");
  BUF_TRY(lowest_dev, nb * 3 * sizeof(float), "trex_batch_body_clearance: lowest");
  TrexTermArgs t = term_args(b);
  t.clearance = clearance_dev; t.lowest = lowest_dev;
  HIP_TRY(trex_launch_termination(t, 0, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_set_termination(TrexBatch *b, float head_height_min, float tilt_max_rad, const float *clear_min_host, float penalty) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (std::isinf(head_height_min)) return fail(TREX_E_INVALID, "trex_batch_set_termination: head_height_min is infinite (NaN = off)");
  if (!std::isnan(tilt_max_rad) && !(tilt_max_rad > 0.f && tilt_max_rad <= 3.14159274f))
    return fail(TREX_E_INVALID, "trex_batch_set_termination: tilt_max_rad must lie in (0, pi] (NaN = off)");
  if (!std::isfinite(penalty)) return fail(TREX_E_INVALID, "trex_batch_set_termination: penalty is not finite");
  bool watch = false;
  for (int i = 0; clear_min_host && i < b->nb; i++) watch |= !std::isnan(clear_min_host[i]);
  const bool on = !std::isnan(head_height_min) || !std::isnan(tilt_max_rad) || watch;
  TrexBatch::Termination &tm = b->term;
  if (on && !tm.blob) {   // first enable: a batch that never enables it allocates nothing
    DeviceGuard guard(b->device);
    const size_t n = (size_t)b->n, o_val = n * 3 * b->nj * sizeof(float), o_reason = o_val + n * 3 * sizeof(float),
                 o_mask = o_reason + n * sizeof(int32_t), o_done = o_mask + n, bytes = o_done + n;
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();   // (the zeros are in place before a launch on any stream)
    if (e != hipSuccess) { (void)hipFree(p); return hip_fail(e, "trex_batch_set_termination: buffers"); }
    char *c = (char *)p;
    tm.blob = p; tm.tobs = (float *)c; tm.values = (float *)(c + o_val); tm.reason = (int32_t *)(c + o_reason);
    tm.mask = (uint8_t *)(c + o_mask); tm.done = (uint8_t *)(c + o_done);
  }
  tm.on = on; tm.watch_any = watch;
  tm.head_min = head_height_min; tm.penalty = penalty;
  tm.cos_tilt = std::isnan(tilt_max_rad) ? NAN : (float)std::cos((double)tilt_max_rad);
  for (int i = 0; i < TREX_TL; i++) tm.clear_min[i] = (clear_min_host && i < b->nb) ? clear_min_host[i] : NAN;
  return TREX_OK;
}

int trex_batch_termination_info(TrexBatch *b, int32_t *reason_dev, float *values_dev, float *terminal_obs_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Termination &tm = b->term;
  if (!tm.blob) return fail(TREX_E_INVALID, "trex_batch_termination_info: termination was never enabled (trex_batch_set_termination)");
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(reason_dev, n * sizeof(int32_t), "trex_batch_termination_info: reason");
  BUF_TRY(values_dev, n * 3 * sizeof(float), "trex_batch_termination_info: values");
  BUF_TRY(terminal_obs_dev, n * 3 * b->nj * sizeof(float), "trex_batch_termination_info: terminal_obs");
  hipStream_t s = (hipStream_t)stream;
  if (reason_dev) HIP_TRY(hipMemcpyAsync(reason_dev, tm.reason, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (values_dev) HIP_TRY(hipMemcpyAsync(values_dev, tm.values, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (terminal_obs_dev) HIP_TRY(hipMemcpyAsync(terminal_obs_dev, tm.tobs, n * 3 * b->nj * sizeof(float), hipMemcpyDeviceToDevice, s));
  return TREX_OK;
}

}  // extern "C"
