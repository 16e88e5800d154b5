// C-ABI of include/trex_batch.h: the error plumbing, the model handle, the batch handle and every call that changes what the step
// launches do - the setters, step and reset, state, domain, actuators, the sensor and termination switches. The calls that only read
// the state and write caller buffers are in capi_queries.cpp; the tables either sends to the device are built in host_tables.cpp.
#include <cstring>
#include <memory>

#include "batch.hpp"
#include "step_launch.h"
#include "termination.h"

namespace {

thread_local std::string g_error;

// What every launch of the batch's step kernels is given: the model, the state, the reward weights and the record / buffer of each
// feature that is switched on - a non-null pointer IS the switch (step_launch.h). A reset takes no actions: no wave balance, no
// external wrench, no actuator model. The caller adds the outputs and their strides.
TrexStepArgs step_args(const TrexBatch *b, TrexStepKind kind) {
  TrexStepArgs a{};
  a.model = b->dmodel; a.arr = b->arr; a.n_envs = b->n;
  a.w_distance = b->wd; a.w_energy = b->we; a.w_drift = b->wk;
  a.obs_stride = 3 * b->nj; a.scal_stride = 1; a.n_steps = 1;
  a.warm = b->warm.as<float>(); a.sens = b->sensor();
  if (kind == TREX_KIND_RESET) return a;
  a.bal = b->balance() ? b->arr.balance : nullptr;
  a.ext = b->wrench();
  if (b->act_on()) {
    a.act = b->gains.as<float>(); a.act_vel = b->vel_mask; a.act_tor = b->tor_mask;
    a.act_cols = b->action_cols(); a.act_kp_max = b->kp_max;
  }
  return a;
}
// the outputs as ONE row block: row e = obs | reward | done (| the three penalties) at rows + e * row_stride
int row_cols(const TrexBatch *b) { return 3 * b->nj + (b->pen_in_rows ? 5 : 2); }
// the row_stride refusal of the row-block call `who`, and the bytes its rows buffer must hold for `num_rows` rows
int rows_bytes(const TrexBatch *b, const char *who, int row_stride, size_t num_rows, size_t *bytes) {
  if (row_stride < row_cols(b)) return fail(TREX_E_INVALID, std::string(who) + ": row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  *bytes = ((num_rows - 1) * row_stride + row_cols(b)) * sizeof(float);
  return TREX_OK;
}
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

}  // namespace

// (declared in batch.hpp: capi_randomize.cpp needs it too)
int ensure_gains(TrexBatch *b) {
  if (b->gains) return TREX_OK;
  DeviceGuard guard(b->device);
  DeviceBuf g;
  HIP_TRY(g.alloc((size_t)b->n * TREX_ACT_FLOATS * sizeof(float), false));
  HIP_TRY(trex_launch_copy_gains(b->dmodel, nullptr, nullptr, nullptr, g.as<float>(), b->n, nullptr));
  HIP_TRY(hipDeviceSynchronize());   // (in place before a launch on any stream)
  b->gains = std::move(g);
  return TREX_OK;
}

int trex_fail(int code, const std::string &msg) {
  g_error = msg;
  return code;
}

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
  auto b = std::make_unique<TrexBatch>();   // (an error return below frees, through the DeviceBufs, what was allocated so far)
  b->n = num_envs; b->device = device; b->nb = model->host.nb; b->nj = b->nb - 1;
  b->obs_order = model->host.obs_order; b->parent = model->host.parent;
  b->motion.q_lower = model->host.q_lower; b->motion.q_upper = model->host.q_upper;
  const trex::HostModel &h = model->host;
  hipError_t r = hipSuccess;
  // zeroed device memory owned by the batch, `data` (if any) copied in
  auto A = [&](size_t bytes, const void *data = nullptr) -> void * {
    DeviceBuf buf;
    if (r == hipSuccess) r = buf.alloc(bytes, true);
    if (r == hipSuccess && data) r = hipMemcpy(buf.p, data, bytes, hipMemcpyHostToDevice);
    b->state.push_back(std::move(buf));
    return b->state.back().p;
  };
  const size_t n = (size_t)num_envs, nv = h.hull_xyz.size(), nl = h.link_names.size(), nvis = h.visual_file.size();
  TrexDeviceModel dm;
  trex::fill_device_model(h, dm);
  b->dmodel = (TrexDeviceModel *)A(sizeof dm, &dm);
  b->arr.base = (float *)A(n * 16 * sizeof(float));
  b->arr.q = (float *)A(n * TREX_TL * sizeof(float));
  b->arr.qd = (float *)A(n * TREX_TL * sizeof(float));
  b->arr.mass_scale = (float *)A(n * TREX_TL * sizeof(float));
  b->arr.friction = (float *)A(n * sizeof(float));
  b->arr.balance = (int32_t *)A(TREX_BAL_WORDS(n) * sizeof(int32_t));
  {   // wave balance: before the first step launch every env is filed under contact count 0, in env order
    std::vector<int32_t> bal(TREX_BAL_LISTS + n, 0);
    bal[TREX_BAL_COUNTS + 0] = (int32_t)n;
    for (size_t i = 0; i < n; i++) bal[TREX_BAL_LISTS + i] = (int32_t)i;
    if (r == hipSuccess) r = hipMemcpy(b->arr.balance, bal.data(), bal.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  }
  // the warm-start records exist only for a model with warmstart > 0 (zeroed: every record empty)
  if (h.prm.warmstart > 0 && r == hipSuccess) r = b->warm.alloc(n * TREX_WARM_WORDS * sizeof(float), true);
  b->arr.max_episode_steps = 0;
  b->arr.domain = 0;
  b->floor_z = h.prm.floor_z;
  b->step_seconds = h.prm.dt * h.prm.substeps;
  b->hull_xyz = h.hull_xyz; b->hull_radius = h.hull_radius;
  b->hull_start = h.hull_start; b->hull_group_start = h.hull_group_start;
  b->links.body = h.link_body; b->links.tf = h.link_tf;
  std::vector<float4> hull(nv ? nv : 1);
  for (size_t i = 0; i < nv; i++) hull[i] = make_float4((float)h.hull_xyz[i].x, (float)h.hull_xyz[i].y, (float)h.hull_xyz[i].z, (float)h.hull_radius[i]);
  b->arr.hull = (float4 *)A(hull.size() * sizeof(float4), hull.data());
  std::vector<float> ltf(nl * 12);
  for (size_t l = 0; l < nl; l++) trex::tf12(h.link_tf[l], &ltf[12 * l]);
  b->arr.num_links = (int)nl;
  b->arr.link_body = (const int *)A(nl * sizeof(int), h.link_body.data());
  b->arr.link_tf = (const float *)A(ltf.size() * sizeof(float), ltf.data());
  std::vector<int> vb(nvis ? nvis : 1);
  std::vector<float> vtf(vb.size() * 12);
  for (size_t v = 0; v < nvis; v++) {
    vb[v] = h.link_body[h.visual_link[v]];
    trex::tf12(h.visual_body_tf[v], &vtf[12 * v]);
  }
  b->arr.num_visuals = (int)nvis;
  b->arr.visual_body = (const int *)A(vb.size() * sizeof(int), vb.data());
  b->arr.visual_tf = (const float *)A(vtf.size() * sizeof(float), vtf.data());
  if (r == hipSuccess) r = trex_launch_fill(b->arr.mass_scale, 1.0f, num_envs * TREX_TL, nullptr);
  if (r == hipSuccess) r = trex_launch_fill(b->arr.friction, (float)h.prm.friction, num_envs, nullptr);
  if (r == hipSuccess) r = hipDeviceSynchronize();
  if (r != hipSuccess) return hip_fail(r, "batch initialisation");
  *out = b.release();
  return TREX_OK;
}

void trex_batch_destroy(TrexBatch *b) {
  if (!b) return;
  DeviceGuard guard(b->device);
  (void)hipDeviceSynchronize();
  delete b;   // (every allocation is a DeviceBuf of the batch)
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
  BUF_TRY(b, mask_dev, n, "trex_batch_reset: mask");
  BUF_TRY(b, obs_out_dev, n * 3 * b->nj * sizeof(float), "trex_batch_reset: obs_out");
  TrexStepArgs a = step_args(b, TREX_KIND_RESET);
  a.reset_mask = mask_dev; a.obs = obs_out_dev;
  HIP_TRY(trex_launch_step(&a, TREX_KIND_RESET, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_reset_rows(TrexBatch *b, const uint8_t *mask_dev, float *rows_dev, int row_stride, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!rows_dev) return fail(TREX_E_INVALID, "trex_batch_reset_rows: rows is null");
  size_t rows_need = 0;
  if (int c = rows_bytes(b, "trex_batch_reset_rows", row_stride, (size_t)b->n, &rows_need)) return c;
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(b, mask_dev, n, "trex_batch_reset_rows: mask");
  BUF_TRY(b, rows_dev, rows_need, "trex_batch_reset_rows: rows");
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
  BUF_TRY(b, actions_dev, n * b->action_cols() * sizeof(float), "trex_batch_step: actions");
  BUF_TRY(b, obs_dev, n * 3 * b->nj * sizeof(float), "trex_batch_step: obs");
  BUF_TRY(b, reward_dev, n * sizeof(float), "trex_batch_step: reward");
  BUF_TRY(b, done_dev, n, "trex_batch_step: done");
  BUF_TRY(b, penalties_dev, n * 3 * sizeof(float), "trex_batch_step: penalties");
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
  size_t rows_need = 0;
  if (int c = rows_bytes(b, "trex_batch_step_rows", row_stride, (size_t)b->n, &rows_need)) return c;
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(b, actions_dev, n * b->action_cols() * sizeof(float), "trex_batch_step_rows: actions");
  BUF_TRY(b, rows_dev, rows_need, "trex_batch_step_rows: rows");
  BUF_TRY(b, penalties_dev, n * 3 * sizeof(float), "trex_batch_step_rows: penalties");
  BUF_TRY(b, done_dev, n, "trex_batch_step_rows: done");
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
  size_t rows_need = 0;
  if (int c = rows_bytes(b, "trex_batch_step_many", row_stride, (size_t)num_steps * b->n, &rows_need)) return c;
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n, S = (size_t)num_steps;
  BUF_TRY(b, actions_dev, S * n * b->action_cols() * sizeof(float), "trex_batch_step_many: actions");
  BUF_TRY(b, rows_dev, rows_need, "trex_batch_step_many: rows");
  BUF_TRY(b, penalties_dev, S * n * 3 * sizeof(float), "trex_batch_step_many: penalties");
  BUF_TRY(b, done_dev, S * n, "trex_batch_step_many: done");
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
  BUF_TRY(b, actions_dev, (size_t)b->n * b->nj * sizeof(float), "trex_batch_debug_step: actions");
  BUF_TRY(b, obs_dev, (size_t)b->n * 3 * b->nj * sizeof(float), "trex_batch_debug_step: obs");
  BUF_TRY(b, debug_dev, 4096 * sizeof(float), "trex_batch_debug_step: debug");   // (diagnostic builds: 4096 + 16 N)
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
  BUF_TRY(b, episode_steps_dev, (size_t)b->n * sizeof(int32_t), "trex_batch_set_episode_limit: episode_steps");
  b->arr.max_episode_steps = max_episode_steps;
  HIP_TRY(trex_launch_scalars_set(b->arr, b->n, episode_steps_dev, 1, -1, (hipStream_t)stream));
  return TREX_OK;
}
int trex_batch_get_episode_steps(TrexBatch *b, int32_t *episode_steps_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!episode_steps_dev) return fail(TREX_E_INVALID, "episode_steps is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, episode_steps_dev, (size_t)b->n * sizeof(int32_t), "trex_batch_get_episode_steps: episode_steps");
  HIP_TRY(trex_launch_scalars_get(b->arr, b->n, nullptr, nullptr, episode_steps_dev, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_get_state(TrexBatch *b, float *state_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!state_dev) return fail(TREX_E_INVALID, "state is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, state_dev, (size_t)b->n * (13 + 2 * b->nj) * sizeof(float), "trex_batch_get_state: state");
  HIP_TRY(trex_launch_pack_state(b->dmodel, b->arr, b->n, state_dev, 1, (hipStream_t)stream));
  return TREX_OK;
}
int trex_batch_set_state(TrexBatch *b, const float *state_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!state_dev) return fail(TREX_E_INVALID, "state is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, state_dev, (size_t)b->n * (13 + 2 * b->nj) * sizeof(float), "trex_batch_set_state: state");
  HIP_TRY(trex_launch_pack_state(b->dmodel, b->arr, b->n, const_cast<float *>(state_dev), 0, (hipStream_t)stream));
  if (b->warm)   // the recorded impulses belong to the states just replaced: every record is emptied
    HIP_TRY(hipMemsetAsync(b->warm.p, 0, (size_t)b->n * TREX_WARM_WORDS * sizeof(float), (hipStream_t)stream));
  return TREX_OK;
}
int trex_batch_set_motors_enabled(TrexBatch *b, int enabled, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  HIP_TRY(trex_launch_scalars_set(b->arr, b->n, nullptr, 0, enabled ? 1 : 0, (hipStream_t)stream));
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

int trex_batch_set_domain(TrexBatch *b, const float *mass_scale_dev, const float *friction_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  BUF_TRY(b, mass_scale_dev, (size_t)b->n * b->nb * sizeof(float), "trex_batch_set_domain: mass_scale");
  BUF_TRY(b, friction_dev, (size_t)b->n * sizeof(float), "trex_batch_set_domain: friction");
  if (mass_scale_dev) HIP_TRY(trex_launch_copy_mass_scale(mass_scale_dev, b->arr.mass_scale, b->n, b->nb, (hipStream_t)stream));
  if (friction_dev) HIP_TRY(hipMemcpyAsync(b->arr.friction, friction_dev, b->n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (mass_scale_dev || friction_dev) b->arr.domain = 1;   // from now on the step launches read the per-env arrays
  return TREX_OK;
}

int trex_batch_set_external_wrench(TrexBatch *b, const float *wrench_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Randomization &rd = b->random;
  const int pushes = rd.table.pushes;   // PUSH terms of the episode randomisation: the wrench stays on, this call sets its base
  if (!wrench_dev && pushes == 0) { b->ext_on = false; return TREX_OK; }   // the default kernels again; the buffer stays for the next call
  DeviceGuard guard(b->device);
  BUF_TRY(b, wrench_dev, (size_t)b->n * b->nb * 6 * sizeof(float), "trex_batch_set_external_wrench: wrench");
  if (!b->ext)   // first use: a batch that never sets a wrench allocates nothing
    HIP_TRY(b->ext.alloc((size_t)b->n * 6 * TREX_TL * sizeof(float), false));
  if (wrench_dev) HIP_TRY(trex_launch_copy_wrench(wrench_dev, b->ext.as<float>(), b->n, b->nb, (hipStream_t)stream));
  else HIP_TRY(trex_launch_fill(b->ext.as<float>(), 0.f, b->n * 6 * TREX_TL, (hipStream_t)stream));
  if (pushes > 0)   // the push bodies' columns: the caller's into the batch's copy, base + the force in effect into the buffer
    HIP_TRY(trex_launch_randomize_rebase(rd.blob.as<TrexRandTable>(), rd.st, wrench_dev, b->ext.as<float>(), b->n, b->nb, pushes, 0,
                                         (hipStream_t)stream));
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
  BUF_TRY(b, kp_dev, bytes, "trex_batch_set_motor_gains: kp");
  BUF_TRY(b, kd_dev, bytes, "trex_batch_set_motor_gains: kd");
  BUF_TRY(b, max_force_dev, bytes, "trex_batch_set_motor_gains: max_force");
  const bool any = kp_dev || kd_dev || max_force_dev;
  if (!any && !b->gains) { b->gains_set = false; return TREX_OK; }   // nothing was ever set: nothing to clear, nothing allocated
  if (int c = ensure_gains(b)) return c;
  // (all three NULL: the buffer goes back to the model parameters - control modes and stiffness actions keep reading it)
  HIP_TRY(trex_launch_copy_gains(b->dmodel, kp_dev, kd_dev, max_force_dev, b->gains.as<float>(), b->n, (hipStream_t)stream));
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
    DeviceBuf s;
    HIP_TRY(s.alloc((size_t)b->n * TREX_SENS_FLOATS * sizeof(float), true));
    HIP_TRY(hipDeviceSynchronize());   // (the zeros are in place before a launch on any stream)
    b->sens = std::move(s);
  }
  b->sens_on = true;
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
  BUF_TRY(b, actions_dev, (size_t)b->n * b->action_cols() * sizeof(float), "trex_batch_time_steps: actions");
  BUF_TRY(b, obs_dev, (size_t)b->n * 3 * b->nj * sizeof(float), "trex_batch_time_steps: obs");
  BUF_TRY(b, reward_dev, (size_t)b->n * sizeof(float), "trex_batch_time_steps: reward");
  BUF_TRY(b, done_dev, (size_t)b->n, "trex_batch_time_steps: done");
  struct Event {   // (destroyed on every way out)
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
  } ev0, ev1;
  HIP_TRY(hipEventCreate(&ev0.e));
  HIP_TRY(hipEventCreate(&ev1.e));
  const hipEvent_t e0 = ev0.e, e1 = ev1.e;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipEventRecord(e0, s));
  TrexStepArgs a = step_args(b, TREX_KIND_STEP);
  a.actions = actions_dev; a.obs = obs_dev; a.reward = reward_dev; a.done = done_dev;
  for (int i = 0; i < steps; i++) HIP_TRY(trex_launch_step(&a, TREX_KIND_STEP, s));
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  *avg_ms_out = ms / steps;
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
    DeviceBuf blob;
    HIP_TRY(blob.alloc(bytes, true));
    HIP_TRY(hipDeviceSynchronize());   // (the zeros are in place before a launch on any stream)
    char *c = blob.as<char>();
    tm.blob = std::move(blob); tm.tobs = (float *)c; tm.values = (float *)(c + o_val); tm.reason = (int32_t *)(c + o_reason);
    tm.mask = (uint8_t *)(c + o_mask); tm.done = (uint8_t *)(c + o_done);
  }
  tm.on = on; tm.watch_any = watch;
  tm.head_min = head_height_min; tm.penalty = penalty;
  tm.cos_tilt = std::isnan(tilt_max_rad) ? NAN : (float)std::cos((double)tilt_max_rad);
  for (int i = 0; i < TREX_TL; i++) tm.clear_min[i] = (clear_min_host && i < b->nb) ? clear_min_host[i] : NAN;
  return TREX_OK;
}

}  // extern "C"
