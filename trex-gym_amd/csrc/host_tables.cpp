// The tables the kernels read, built on the host: see host_tables.hpp for the include rule (no HIP in here).
#include "host_tables.hpp"

#include "../../include/trex_policy.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace trex {

size_t row_block_bytes(size_t n, int stride, int width) { return ((n - 1) * (size_t)stride + (size_t)width) * sizeof(float); }

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + nb && q < p + na;
}

void check_env_offset(const std::string &who, uint32_t env_offset, int n_envs) {
  if ((uint64_t)env_offset + (uint64_t)n_envs > (1ull << 32)) throw Refusal(who + "env_offset + N is beyond 2^32");
}

size_t Layout::take(const char *name, size_t member_bytes, size_t align) {
  const size_t at = (bytes + align - 1) / align * align;
  members.push_back({name, at, member_bytes, align});
  bytes = at + member_bytes;
  return at;
}

RewardHistLayout reward_hist_layout(int n_envs, int A_cols, int J_joints, int T_terms) {
  RewardHistLayout l;
  if (T_terms == 0) return l;
  const size_t n = (size_t)n_envs, A = (size_t)A_cols, J = (size_t)J_joints, T = (size_t)T_terms;
  l.prev_act = l.take("prev_act", n * A * 4, 4); l.prev_qd = l.take("prev_qd", n * J * 4, 4);
  l.timer = l.take("timer", n * T * 4, 4); l.held = l.take("held", n * T * 4, 4);
  l.valid = l.take("valid", n * 4, 4);
  return l;
}

MotionClockLayout motion_clock_layout(int n_envs) {
  MotionClockLayout l;
  l.t0 = l.take("t0", (size_t)n_envs * 4, 4); l.k = l.take("k", (size_t)n_envs * 4, 4);
  return l;
}

Layout motion_held_layout(int n_envs, int T_terms) {
  Layout l;
  if (T_terms > 0) l.take("held", (size_t)n_envs * (size_t)T_terms * 4, 4);
  return l;
}

SenseCounterLayout sense_counter_layout(int n_envs, int G_groups) {
  SenseCounterLayout l;
  if (G_groups == 0) return l;
  const size_t n = (size_t)n_envs;
  l.ep = l.take("ep", n * 4, 4); l.k = l.take("k", n * 4, 4); l.started = l.take("started", n * 4, 4);
  l.delay = l.take("delay", n * (size_t)G_groups * 4, 4);
  return l;
}

Layout sense_hist_layout(int n_envs, int cols) {
  Layout l;
  if (cols > 0) l.take("hist", (size_t)TREX_SENSE_SLOTS * (size_t)n_envs * (size_t)cols * 4, 4);
  return l;
}

RandStateLayout rand_state_layout(int n_envs, int T_terms, int P_pushes) {
  RandStateLayout l;
  if (T_terms == 0) return l;
  const size_t n = (size_t)n_envs, T = (size_t)T_terms, P = (size_t)P_pushes;
  l.ep = l.take("ep", n * 4, 4); l.k = l.take("k", n * 4, 4); l.started = l.take("started", n * 4, 4);
  l.off = l.take("off", n * P * 4, 4); l.push_left = l.take("push_left", n * P * 4, 4);
  l.push_force = l.take("push_force", n * P * 3 * 4, 4); l.push_base = l.take("push_base", n * P * 6 * 4, 4);
  l.values = l.take("values", n * T * TREX_TL * 4, 4);
  return l;
}

StartStateLayout start_state_layout(int n_envs, int T_terms) {
  StartStateLayout l;
  if (T_terms == 0) return l;
  const size_t n = (size_t)n_envs, T = (size_t)T_terms;
  l.ep = l.take("ep", n * 4, 4); l.started = l.take("started", n * 4, 4);
  l.shift = l.take("shift", n * 4, 4); l.lowest = l.take("lowest", n * 4, 4);
  l.values = l.take("values", n * T * TREX_TL * 4, 4);
  return l;
}

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
  // the step kernel's packed words (device_model.h), derived from the tables above: what the kernel used to form per lane
  for (int l = 0; l < TREX_TL; l++) {
    const bool body = l < h.nb;
    const int parent = body ? d.parent[l] : 0, depth = body ? d.depth[l] : -1;
    d.tree_pack[l] = (unsigned)(parent < 0 ? 0 : parent) | (unsigned)(depth < 0 ? TREX_NO_DEPTH : depth) << 8;
    unsigned ch4 = 0u;
    for (int k = 0; k < TREX_MAXCH; k++) {
      const int c = body ? d.child[k][l] : -1;
      ch4 |= (unsigned)(c < 0 ? 255 : c) << (8 * k);
    }
    d.child_pack[l] = ch4;
    d.hull_range[l][0] = d.hull_start[body ? l : h.nb]; d.hull_range[l][1] = d.hull_start[body ? l + 1 : h.nb];
    const bool unit = l < d.nchunk;
    const int cb = d.chunk_body[l];
    d.chunk_row[l][0] = unit ? (cb | (d.cm_pack[cb] << 8)) : 0;
    d.chunk_row[l][1] = unit ? d.chunk_v0[l] : 0; d.chunk_row[l][2] = unit ? d.chunk_v1[l] : 0;
    d.chunk_row[l][3] = unit ? d.hull_start[cb] : 0;
    for (int c = 0; c < 3; c++) { d.chunk_box[l][c] = d.chunk_c[c][l]; d.chunk_box[l][4 + c] = d.chunk_h[c][l]; }
    d.chunk_box[l][3] = d.chunk_box[l][7] = 0.f;
  }
}

void tf12(const Tf &t, float out[12]) {
  for (int k = 0; k < 9; k++) out[k] = (float)t.R.m[k];
  out[9] = (float)t.t.x; out[10] = (float)t.t.y; out[11] = (float)t.t.z;
}

LinkPoint link_point(const Links &links, int link, const double x[3]) {
  const Tf &t = links.tf[link];   // body <- link transform of "link_tf"
  const double tt[3] = {t.t.x, t.t.y, t.t.z};
  LinkPoint p;
  p.body = links.body[link];
  for (int r = 0; r < 3; r++)
    p.point[r] = (float)(t.R.m[3 * r] * x[0] + t.R.m[3 * r + 1] * x[1] + t.R.m[3 * r + 2] * x[2] + tt[r]);
  return p;
}

ProbeTable build_probe_table(const Links &links, const int32_t *link_host, const double *local_xyz_host, int num_probes) {
  ProbeTable t;
  t.body.resize((size_t)num_probes);
  t.tf.resize((size_t)num_probes * 12);
  for (int k = 0; k < num_probes; k++) {
    const int link = link_host[k];
    if (link < 0 || link >= (int)links.body.size())
      throw Refusal("trex_batch_set_link_probes: probe " + std::to_string(k) + ": link " + std::to_string(link) +
                    " out of range [0, " + std::to_string(links.body.size()) + ")");
    const double *x = local_xyz_host + 3 * (size_t)k;
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(x[c]))
        throw Refusal("trex_batch_set_link_probes: probe " + std::to_string(k) + ": local_xyz is not finite");
    // body <- link rotation, and the point in the frame of the link's body
    float *o = t.tf.data() + 12 * (size_t)k;
    tf12(links.tf[link], o);
    const LinkPoint p = link_point(links, link, x);
    t.body[k] = p.body;
    std::memcpy(o + 9, p.point, sizeof p.point);
  }
  return t;
}

ProxTable build_prox_table(int nb, const int32_t *body_host, const double *capsule_host, int num_capsules, const int32_t *pair_host,
                           int num_pairs) {
  const std::string me = "trex_batch_set_proximity_shapes: ";
  if (num_capsules < 0 || num_capsules > TREX_PROX_MAXCAPS)
    throw Refusal(me + "num_capsules " + std::to_string(num_capsules) + " outside [0, " + std::to_string(TREX_PROX_MAXCAPS) + "]");
  ProxTable t;
  if (num_capsules == 0) return t;
  if (num_pairs < 1 || num_pairs > TREX_PROX_MAXPAIRS)
    throw Refusal(me + "num_pairs " + std::to_string(num_pairs) + " outside [1, " + std::to_string(TREX_PROX_MAXPAIRS) + "]");
  if (!body_host || !capsule_host || !pair_host) throw Refusal(me + "null argument");
  std::vector<float> cap((size_t)num_capsules * 8, 0.f);
  std::vector<int32_t> cap_body((size_t)num_capsules), pair_first;
  std::vector<uint32_t> test;
  std::vector<std::vector<int>> of_body((size_t)nb);   // a body's capsules, table order
  for (int c = 0; c < num_capsules; c++) {
    const int body = body_host[c];
    if (body < 0 || body >= nb)
      throw Refusal(me + "capsule " + std::to_string(c) + ": body " + std::to_string(body) + " out of range [0, " + std::to_string(nb) + ")");
    const double *x = capsule_host + 7 * (size_t)c;
    for (int k = 0; k < 7; k++)
      if (!std::isfinite(x[k])) throw Refusal(me + "capsule " + std::to_string(c) + ": value is not finite");
    if (x[6] < 0) throw Refusal(me + "capsule " + std::to_string(c) + ": negative radius");
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
    if (A < 0 || A >= nb || B < 0 || B >= nb || A == B)
      throw Refusal(me + "pair " + std::to_string(p) + ": bodies (" + std::to_string(A) + ", " + std::to_string(B) +
                    ") must be two different bodies of the model");
    if (of_body[A].empty() || of_body[B].empty()) throw Refusal(me + "pair " + std::to_string(p) + ": a body of the pair has no capsule");
    total += of_body[A].size() * of_body[B].size();
  }
  if (total > TREX_PROX_MAXTESTS)
    throw Refusal(me + std::to_string(total) + " capsule-pair tests, at most " + std::to_string(TREX_PROX_MAXTESTS));
  test.reserve(total);
  for (int p = 0; p < num_pairs; p++) {
    pair_first.push_back((int32_t)test.size());
    for (int ca : of_body[pair_host[2 * p]])
      for (int cb : of_body[pair_host[2 * p + 1]]) test.push_back(TREX_PROX_TEST(p, ca, cb));
  }
  // one allocation, every part at a multiple of 16 bytes
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  t.caps = num_capsules; t.pairs = num_pairs; t.tests = (int)test.size();
  t.o_body = up(cap.size() * sizeof(float));
  t.o_test = t.o_body + up(cap_body.size() * sizeof(int32_t));
  t.o_first = t.o_test + up(test.size() * sizeof(uint32_t));
  t.blob.assign(t.o_first + up(pair_first.size() * sizeof(int32_t)), 0);
  std::memcpy(t.blob.data(), cap.data(), cap.size() * sizeof(float));
  std::memcpy(t.blob.data() + t.o_body, cap_body.data(), cap_body.size() * sizeof(int32_t));
  std::memcpy(t.blob.data() + t.o_test, test.data(), test.size() * sizeof(uint32_t));
  std::memcpy(t.blob.data() + t.o_first, pair_first.data(), pair_first.size() * sizeof(int32_t));
  return t;
}

IkTask build_ik_task(const std::vector<int32_t> &probe_body, const std::vector<int> &parent, const std::vector<int> &obs_order,
                     const int32_t *mode_host, uint32_t joint_mask, const TrexIkParams *params) {
  const std::string me = "trex_batch_inverse_kinematics: ";
  IkTask a;
  for (size_t k = 0; k < probe_body.size(); k++) {
    const int m = mode_host[k];
    if (m < 1 || m > 3) throw Refusal(me + "mode " + std::to_string(m) + " of target " + std::to_string(k) + " outside 1..3");
    a.body[k] = (uint8_t)probe_body[k]; a.mode[k] = (uint8_t)m; a.row0[k] = (uint8_t)a.rows;
    for (int i = probe_body[k]; i > 0; i = parent[i]) a.chain[k] |= 1u << i;
    a.rows += m == 3 ? 6 : 3;
  }
  if (a.rows > TREX_IK_MAXROWS) throw Refusal(me + std::to_string(a.rows) + " task rows, at most " + std::to_string(TREX_IK_MAXROWS));
  for (size_t k = 0; k < obs_order.size(); k++)
    if ((joint_mask >> k) & 1u) a.move_mask |= 1u << obs_order[k];
  if (!a.move_mask) throw Refusal(me + "joint_mask lets no joint move");
  const TrexIkParams defaults = TREX_IK_DEFAULTS;
  const TrexIkParams &p = params ? *params : defaults;
  if (p.iterations < 1 || p.iterations > 256) throw Refusal(me + "iterations " + std::to_string(p.iterations) + " outside 1..256");
  for (float v : {p.damping, p.gain, p.max_step, p.tol_pos, p.tol_ori})
    if (!std::isfinite(v) || v < 0.f) throw Refusal(me + "a parameter is negative or not finite");
  a.iterations = p.iterations; a.damping2 = p.damping * p.damping; a.gain = p.gain; a.max_step = p.max_step;
  a.tol_pos = p.tol_pos; a.tol_ori = p.tol_ori;
  return a;
}

ObsTable build_obs_table(const Links &links, int nj, int action_cols, const TrexObsChannel *channels, int num_channels) {
  const std::string me = "trex_batch_set_observation: ";
  if (num_channels < 0 || num_channels > TREX_OBS_MAXCHANNELS)
    throw Refusal(me + "num_channels " + std::to_string(num_channels) + " outside [0, " + std::to_string(TREX_OBS_MAXCHANNELS) + "]");
  ObsTable t;
  if (num_channels == 0) return t;
  if (!channels) throw Refusal(me + "null argument");
  std::vector<TrexObsChan> chan((size_t)num_channels);
  std::vector<uint8_t> col_chan;
  const int num_links = (int)links.body.size();
  for (int k = 0; k < num_channels; k++) {
    const TrexObsChannel &c = channels[k];
    const std::string ck = me + "channel " + std::to_string(k) + ": ";
    if (c.kind < 0 || c.kind >= TREX_OBS_KINDS) throw Refusal(ck + "unknown kind " + std::to_string(c.kind));
    for (int i = 0; i < 3; i++)
      if (!std::isfinite(c.local_xyz[i])) throw Refusal(ck + "local_xyz is not finite");
    if (!std::isfinite(c.scale)) throw Refusal(ck + "scale is not finite");
    TrexObsChan &o = chan[k];
    std::memset(&o, 0, sizeof o);
    o.kind = c.kind; o.scale = c.scale;
    o.tf[0] = o.tf[4] = o.tf[8] = 1.0f;
    const bool point = c.kind == TREX_OBS_POINT_POSITION || c.kind == TREX_OBS_POINT_VELOCITY || c.kind == TREX_OBS_POINT_HEIGHT;
    if (point || c.kind == TREX_OBS_CONTACT_FORCE) {
      if (c.link < 0 || c.link >= num_links)
        throw Refusal(ck + "link " + std::to_string(c.link) + " out of range [0, " + std::to_string(num_links) + ")");
      const double x[3] = {c.local_xyz[0], c.local_xyz[1], c.local_xyz[2]};
      const LinkPoint p = link_point(links, c.link, x);
      tf12(links.tf[c.link], o.tf);
      o.body = p.body;
      std::memcpy(o.point, p.point, sizeof p.point);
      if (point) t.body_mask |= 1u << p.body;
    }
    switch (c.kind) {
      case TREX_OBS_BASE_HEIGHT: case TREX_OBS_POINT_HEIGHT: o.width = 1; break;
      case TREX_OBS_CONTACT_FORCE: o.width = 1; t.contact = true; break;
      case TREX_OBS_PREV_ACTION: o.width = action_cols; t.actions = true; break;
      case TREX_OBS_EXTERNAL:
        if (c.link < 1) throw Refusal(ck + "an EXTERNAL channel needs link = k >= 1 columns, got " + std::to_string(c.link));
        o.width = c.link;
        o.body = t.extern_cols;
        break;
      default: o.width = 3;
    }
    const long long total = 3LL * nj + t.extra + o.width;   // (k may be anything up to INT_MAX)
    if (total > TREX_OBS_MAXDIM)
      throw Refusal(me + "3J + E = " + std::to_string(total) + " observation columns with channel " + std::to_string(k) + ", at most " +
                    std::to_string(TREX_OBS_MAXDIM));
    if (c.kind == TREX_OBS_EXTERNAL) t.extern_cols += o.width;
    o.col0 = t.extra;
    t.extra += o.width;
    col_chan.insert(col_chan.end(), (size_t)o.width, (uint8_t)k);
  }
  t.channels = num_channels; t.action_cols = action_cols;
  t.o_col = (chan.size() * sizeof(TrexObsChan) + 15) & ~(size_t)15;
  t.blob.assign(t.o_col + ((col_chan.size() + 15) & ~(size_t)15), 0);
  std::memcpy(t.blob.data(), chan.data(), chan.size() * sizeof(TrexObsChan));
  std::memcpy(t.blob.data() + t.o_col, col_chan.data(), col_chan.size());
  return t;
}

RewTable build_reward_table(const Links &links, const std::vector<int> &obs_order, int nb, int action_cols, const TrexRewardTerm *terms,
                            int num_terms) {
  const std::string me = "trex_batch_set_reward: ";
  if (num_terms < 0 || num_terms > TREX_REW_MAXTERMS)
    throw Refusal(me + "num_terms " + std::to_string(num_terms) + " outside [0, " + std::to_string(TREX_REW_MAXTERMS) + "]");
  RewTable t;
  if (num_terms == 0) return t;
  if (!terms) throw Refusal(me + "null argument");
  const int nj = (int)obs_order.size(), num_links = (int)links.body.size();
  auto low_bits = [](int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); };
  std::vector<TrexRewTerm> out((size_t)num_terms);
  for (int k = 0; k < num_terms; k++) {
    const TrexRewardTerm &c = terms[k];
    const std::string ck = me + "term " + std::to_string(k) + ": ";
    if (c.kind < 0 || c.kind >= TREX_REW_KINDS) throw Refusal(ck + "unknown kind " + std::to_string(c.kind));
    for (int i = 0; i < 3; i++)
      if (!std::isfinite(c.local_xyz[i])) throw Refusal(ck + "local_xyz is not finite");
    if (!std::isfinite(c.weight) || !std::isfinite(c.p0) || !std::isfinite(c.p1)) throw Refusal(ck + "weight, p0 or p1 is not finite");
    TrexRewTerm &o = out[k];
    std::memset(&o, 0, sizeof o);
    o.kind = c.kind; o.weight = c.weight; o.p0 = c.p0; o.p1 = c.p1;
    o.tf[0] = o.tf[4] = o.tf[8] = 1.0f;
    switch (c.kind) {
      case TREX_REW_TRACK_LIN_VEL: case TREX_REW_TRACK_ANG_VEL:
        if (!(c.p0 > 0.f)) throw Refusal(ck + "a tracking term needs p0 > 0");
        t.command = true;
        break;
      case TREX_REW_POINT_HEIGHT: case TREX_REW_FOOT_AIR_TIME: case TREX_REW_FOOT_SLIP: {
        if (c.link < 0 || c.link >= num_links)
          throw Refusal(ck + "link " + std::to_string(c.link) + " out of range [0, " + std::to_string(num_links) + ")");
        const double x[3] = {c.local_xyz[0], c.local_xyz[1], c.local_xyz[2]};
        const LinkPoint p = link_point(links, c.link, x);
        tf12(links.tf[c.link], o.tf);
        o.body = p.body;
        std::memcpy(o.point, p.point, sizeof p.point);
        if (c.kind != TREX_REW_FOOT_AIR_TIME) t.body_mask |= 1u << p.body;
        if (c.kind != TREX_REW_POINT_HEIGHT) t.contact = true;
        break;
      }
      case TREX_REW_JOINT_LIMIT:
        if (!(c.p0 > 0.f && c.p0 <= 1.f)) throw Refusal(ck + "JOINT_LIMIT needs 0 < p0 <= 1");
        [[fallthrough]];
      case TREX_REW_TORQUE: case TREX_REW_JOINT_VEL: case TREX_REW_JOINT_ACC: case TREX_REW_POWER: case TREX_REW_JOINT_POSE:
        if (c.mask & ~low_bits(nj)) throw Refusal(ck + "a mask bit at or beyond J = " + std::to_string(nj));
        o.mask = c.mask ? c.mask : low_bits(nj);
        break;
      case TREX_REW_CONTACT_COUNT:
        if (c.mask & ~low_bits(nb)) throw Refusal(ck + "a mask bit at or beyond the body count " + std::to_string(nb));
        o.mask = c.mask;
        t.contact = true;
        break;
      case TREX_REW_ACTION_RATE: t.actions = true; break;
      default: break;
    }
  }
  int32_t joint_body[TREX_TL] = {};
  for (int j = 0; j < nj && j < TREX_TL; j++) joint_body[j] = obs_order[j];
  t.terms = num_terms; t.action_cols = action_cols;
  t.o_joint = (out.size() * sizeof(TrexRewTerm) + 15) & ~(size_t)15;
  t.blob.assign(t.o_joint + sizeof joint_body, 0);
  std::memcpy(t.blob.data(), out.data(), out.size() * sizeof(TrexRewTerm));
  std::memcpy(t.blob.data() + t.o_joint, joint_body, sizeof joint_body);
  return t;
}

MotionTable build_motion_table(const std::vector<double> &q_lower, const std::vector<double> &q_upper, const std::vector<int> &obs_order,
                               const double *frames, const double *velocities, int num_frames, double frame_dt, int loop) {
  const std::string me = "trex_batch_set_motion: ";
  MotionTable t;
  if (num_frames == 0) return t;
  if (num_frames < 2 || num_frames > TREX_MOT_MAXFRAMES)
    throw Refusal(me + "num_frames " + std::to_string(num_frames) + " outside [2, " + std::to_string(TREX_MOT_MAXFRAMES) + "] (0 clears)");
  if (!frames) throw Refusal(me + "null argument");
  if (!std::isfinite(frame_dt) || !(frame_dt > 0.0) || !((float)frame_dt > 0.f) || !std::isfinite((float)(1.0 / (double)(float)frame_dt)))
    throw Refusal(me + "frame_dt must be positive and finite");
  const int F = num_frames, J = (int)obs_order.size(), wf = 7 + J, wv = 6 + J;
  for (size_t i = 0; i < (size_t)F * wf; i++)
    if (!std::isfinite(frames[i])) throw Refusal(me + "frame " + std::to_string(i / wf) + ": a value is not finite");
  if (velocities)
    for (size_t i = 0; i < (size_t)F * wv; i++)
      if (!std::isfinite(velocities[i])) throw Refusal(me + "frame " + std::to_string(i / wv) + ": a velocity is not finite");
  // the quaternions: unit length, one hemisphere frame after frame
  std::vector<std::array<double, 4>> quat((size_t)F);
  for (int k = 0; k < F; k++) {
    const double *q = frames + (size_t)k * wf + 3;
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(n > 0.0) || !std::isfinite(n)) throw Refusal(me + "frame " + std::to_string(k) + ": a quaternion of norm 0");
    double sign = 1.0;
    if (k > 0) {
      const std::array<double, 4> &p = quat[k - 1];
      if ((q[0] * p[0] + q[1] * p[1] + q[2] * p[2] + q[3] * p[3]) < 0.0) sign = -1.0;
    }
    for (int c = 0; c < 4; c++) quat[k][c] = sign * q[c] / n;
  }
  for (int k = 0; k < F; k++)
    for (int j = 0; j < J; j++) {
      const double q = frames[(size_t)k * wf + 7 + j], lo = q_lower[obs_order[j]], hi = q_upper[obs_order[j]];
      if (q < lo - 1e-6 || q > hi + 1e-6)
        throw Refusal(me + "frame " + std::to_string(k) + ": joint " + std::to_string(j) + " outside its limits");
    }
  t.frames = F; t.nj = J; t.stride = TREX_MOT_STRIDE(J); t.loop = loop != 0;
  t.frame_dt = (float)frame_dt;
  t.inv_dt = (float)(1.0 / (double)t.frame_dt);
  t.duration = (float)((double)(F - 1) * (double)t.frame_dt);
  t.inv_duration = (float)(1.0 / (double)t.duration);
  const double disp[3] = {frames[(size_t)(F - 1) * wf] - frames[0], frames[(size_t)(F - 1) * wf + 1] - frames[1], 0.0};
  t.disp[0] = (float)disp[0]; t.disp[1] = (float)disp[1];
  t.rows.assign((size_t)F * t.stride, 0.f);
  for (int k = 0; k < F; k++) {
    float *row = t.rows.data() + (size_t)k * t.stride;
    const double *f = frames + (size_t)k * wf;
    for (int c = 0; c < 3; c++) row[c] = (float)f[c];
    for (int c = 0; c < 4; c++) row[3 + c] = (float)quat[k][c];
    for (int j = 0; j < J; j++) row[13 + j] = (float)f[7 + j];
    if (velocities) {
      const double *v = velocities + (size_t)k * wv;
      for (int c = 0; c < 6; c++) row[7 + c] = (float)v[c];
      for (int j = 0; j < J; j++) row[13 + J + j] = (float)v[6 + j];
      continue;
    }
    // derived: the frames km and kp around k, kp - km frame intervals apart; on a looping clip frame F-1 is frame 0 of the next
    // cycle, so the neighbour beyond an end is frame F-2 of the cycle before (position less the cycle's displacement) or frame 1
    // of the cycle after (plus it)
    int km = k > 0 ? k - 1 : 0, kp = k < F - 1 ? k + 1 : F - 1;
    double om = 0.0, op = 0.0;   // cycles of displacement on the two neighbours' positions
    if (t.loop && k == 0) { km = F - 2; om = -1.0; }
    if (t.loop && k == F - 1) { kp = 1; op = 1.0; }
    const double span = (t.loop ? 2.0 : (double)(kp - km)) * frame_dt;
    const double *fm = frames + (size_t)km * wf, *fp = frames + (size_t)kp * wf;
    for (int c = 0; c < 3; c++) row[7 + c] = (float)(((fp[c] + op * disp[c]) - (fm[c] + om * disp[c])) / span);
    for (int j = 0; j < J; j++) row[13 + J + j] = (float)((fp[7 + j] - fm[7 + j]) / span);
    // world-frame rotation vector of quat[kp] o quat[km]^-1, the shorter way round
    const std::array<double, 4> &a = quat[kp], &b = quat[km];
    double d[4] = {-a[3] * b[0] + a[0] * b[3] - a[1] * b[2] + a[2] * b[1], -a[3] * b[1] + a[0] * b[2] + a[1] * b[3] - a[2] * b[0],
                   -a[3] * b[2] - a[0] * b[1] + a[1] * b[0] + a[2] * b[3], a[3] * b[3] + a[0] * b[0] + a[1] * b[1] + a[2] * b[2]};
    if (d[3] < 0.0)
      for (double &x : d) x = -x;
    const double s = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double angle = 2.0 * std::atan2(s, d[3]), scale = s > 0.0 ? angle / s / span : 0.0;
    for (int c = 0; c < 3; c++) row[10 + c] = (float)(d[c] * scale);
  }
  return t;
}

std::vector<TrexMotTerm> build_motion_terms(int nj, bool has_probes, const TrexMotionTerm *terms, int num_terms, float step_weight) {
  const std::string me = "trex_batch_set_motion_reward: ";
  if (num_terms < 0 || num_terms > TREX_MOT_MAXTERMS)
    throw Refusal(me + "num_terms " + std::to_string(num_terms) + " outside [0, " + std::to_string(TREX_MOT_MAXTERMS) + "]");
  std::vector<TrexMotTerm> out((size_t)num_terms);
  if (num_terms == 0) return out;
  if (!terms) throw Refusal(me + "null argument");
  if (!std::isfinite(step_weight)) throw Refusal(me + "step_weight is not finite");
  const uint32_t all = nj >= 32 ? 0xffffffffu : ((1u << nj) - 1u);
  for (int k = 0; k < num_terms; k++) {
    const TrexMotionTerm &c = terms[k];
    const std::string ck = me + "term " + std::to_string(k) + ": ";
    if (c.kind < 0 || c.kind >= TREX_MOT_KINDS) throw Refusal(ck + "unknown kind " + std::to_string(c.kind));
    if (!std::isfinite(c.weight) || !std::isfinite(c.scale) || !std::isfinite(c.aux)) throw Refusal(ck + "weight, scale or aux is not finite");
    if (!(c.scale > 0.f)) throw Refusal(ck + "scale must be positive");
    if (c.aux < 0.f) throw Refusal(ck + "aux must not be negative");
    if (c.mask & ~all) throw Refusal(ck + "a mask bit at or beyond J = " + std::to_string(nj));
    if (c.kind == TREX_MOT_END_EFFECTOR && !has_probes) throw Refusal(ck + "END_EFFECTOR needs a clip set with a probe set");
    TrexMotTerm &o = out[k];
    std::memset(&o, 0, sizeof o);
    o.kind = c.kind; o.mask = c.mask ? c.mask : all; o.weight = c.weight; o.scale = c.scale; o.aux = c.aux;
  }
  return out;
}

void check_sense_delay(const std::string &who, int delay_min, int delay_max) {
  if (delay_min < 0 || delay_max > TREX_SENSE_MAXDELAY || delay_min > delay_max)
    throw Refusal(who + "delays [" + std::to_string(delay_min) + ", " + std::to_string(delay_max) + "] outside 0 <= delay_min <= delay_max <= " +
                  std::to_string(TREX_SENSE_MAXDELAY));
}

SenseTable build_sense_table(int obs_dim, const TrexSenseGroup *groups, int num_groups) {
  const std::string me = "trex_batch_set_sensing: ";
  SenseTable t;
  if (num_groups == 0) return t;
  if (num_groups < 0 || num_groups > TREX_SENSE_MAXGROUPS)
    throw Refusal(me + "num_groups " + std::to_string(num_groups) + " outside [0, " + std::to_string(TREX_SENSE_MAXGROUPS) + "]");
  if (!groups) throw Refusal(me + "null argument");
  if (obs_dim < 1 || obs_dim > TREX_SENSE_MAXCOLS) throw Refusal(me + "the observation dimension " + std::to_string(obs_dim) + " is outside [1, " + std::to_string(TREX_SENSE_MAXCOLS) + "]");
  t.groups = num_groups; t.obs_dim = obs_dim;
  t.group.resize((size_t)num_groups);
  t.col_group.assign((size_t)obs_dim, (int16_t)-1);
  t.col_hist.assign((size_t)obs_dim, (int16_t)-1);
  for (int g = 0; g < num_groups; g++) {
    const TrexSenseGroup &c = groups[g];
    const std::string ck = me + "group " + std::to_string(g) + ": ";
    if (c.width < 1 || c.col0 < 0 || c.col0 >= obs_dim || c.width > obs_dim - c.col0)
      throw Refusal(ck + "columns [" + std::to_string(c.col0) + ", " + std::to_string((long long)c.col0 + c.width) + ") outside [0, " + std::to_string(obs_dim) + ")");
    if (c.noise_kind < 0 || c.noise_kind >= TREX_SENSE_KINDS) throw Refusal(ck + "unknown noise_kind " + std::to_string(c.noise_kind));
    if (!std::isfinite(c.noise) || !std::isfinite(c.bias) || !std::isfinite(c.quantum)) throw Refusal(ck + "noise, bias or quantum is not finite");
    if (c.noise < 0.f || c.bias < 0.f || c.quantum < 0.f) throw Refusal(ck + "noise, bias or quantum is negative");
    const float inv = c.quantum > 0.f ? (float)(1.0 / (double)c.quantum) : 0.f;
    if (!std::isfinite(inv)) throw Refusal(ck + "the inverse of quantum is not finite in f32");
    check_sense_delay(ck, c.delay_min, c.delay_max);
    for (int col = c.col0; col < c.col0 + c.width; col++) {
      if (t.col_group[col] >= 0) throw Refusal(ck + "column " + std::to_string(col) + " is in group " + std::to_string(t.col_group[col]) + " already");
      t.col_group[col] = (int16_t)g;
    }
    TrexSenseGrp &o = t.group[g];
    std::memset(&o, 0, sizeof o);
    o.col0 = c.col0; o.width = c.width; o.kind = c.noise_kind;
    o.noise = c.noise; o.bias = c.bias; o.quantum = c.quantum; o.inv_quantum = inv;
    o.delay_min = c.delay_min; o.delay_max = c.delay_max;
  }
  for (int col = 0; col < obs_dim; col++)   // the delayed columns, packed in column order
    if (t.col_group[col] >= 0 && t.group[t.col_group[col]].delay_max > 0) t.col_hist[col] = (int16_t)t.delayed++;
  t.o_col_group = t.group.size() * sizeof(TrexSenseGrp);
  t.o_col_hist = t.o_col_group + (size_t)obs_dim * sizeof(int16_t);
  t.blob.assign(t.o_col_hist + (size_t)obs_dim * sizeof(int16_t), 0);
  std::memcpy(t.blob.data(), t.group.data(), t.o_col_group);
  std::memcpy(t.blob.data() + t.o_col_group, t.col_group.data(), (size_t)obs_dim * sizeof(int16_t));
  std::memcpy(t.blob.data() + t.o_col_hist, t.col_hist.data(), (size_t)obs_dim * sizeof(int16_t));
  return t;
}

RandTable build_random_table(int nb, int nj, bool stiffness, const TrexRandomTerm *terms, int num_terms) {
  const std::string me = "trex_batch_set_randomization: ";
  RandTable t;
  for (int &s : t.push_slot) s = -1;
  if (num_terms == 0) return t;
  if (num_terms < 0 || num_terms > TREX_RAND_MAXTERMS)
    throw Refusal(me + "num_terms " + std::to_string(num_terms) + " outside [0, " + std::to_string(TREX_RAND_MAXTERMS) + "]");
  if (!terms) throw Refusal(me + "null argument");
  uint32_t covered[TREX_RAND_KINDS] = {};   // per kind: the elements (PUSH: the bodies, COMMAND: the components) taken so far
  t.term.assign(terms, terms + num_terms);
  for (int i = 0; i < num_terms; i++) {
    TrexRandomTerm &c = t.term[i];
    const std::string ck = me + "term " + std::to_string(i) + ": ";
    if (c.kind < 0 || c.kind >= TREX_RAND_KINDS) throw Refusal(ck + "unknown kind " + std::to_string(c.kind));
    if (!std::isfinite(c.lo) || !std::isfinite(c.hi)) throw Refusal(ck + "lo or hi is not finite");
    if (c.lo > c.hi) throw Refusal(ck + "lo > hi");
    if (!(c.probability >= 0.f && c.probability <= 1.f)) throw Refusal(ck + "probability outside [0, 1]");
    uint32_t bits = 0u;
    switch (c.kind) {
      case TREX_RAND_MASS: case TREX_RAND_KP: case TREX_RAND_KD: case TREX_RAND_MAX_FORCE: {
        const int count = c.kind == TREX_RAND_MASS ? nb : nj;
        const uint32_t all = count >= 32 ? 0xFFFFFFFFu : (1u << count) - 1u;
        if (c.mask & ~all) throw Refusal(ck + "a mask bit beyond the model's " + std::to_string(count) + (c.kind == TREX_RAND_MASS ? " bodies" : " joints"));
        if ((c.kind == TREX_RAND_KP || c.kind == TREX_RAND_KD) && stiffness)
          throw Refusal(ck + "KP and KD terms are refused while stiffness actions are on (the step launches write those columns)");
        bits = c.mask ? c.mask : all;
        c.mask = bits; c.shared = c.shared != 0;
        if (c.kind == TREX_RAND_MASS) t.mass = true; else t.gains = true;
        break;
      }
      case TREX_RAND_FRICTION:
        bits = 1u; c.mask = 1u; c.shared = 1;
        t.friction = true;
        break;
      case TREX_RAND_PUSH:
        if (c.index < 0 || c.index >= nb) throw Refusal(ck + "body " + std::to_string(c.index) + " outside [0, " + std::to_string(nb) + ")");
        if (c.interval < 1 || c.duration < 1) throw Refusal(ck + "a PUSH term needs interval >= 1 and duration >= 1");
        if (t.pushes >= TREX_RAND_MAXPUSHES) throw Refusal(ck + "more than " + std::to_string(TREX_RAND_MAXPUSHES) + " PUSH terms");
        bits = 1u << c.index; c.mask = 0u;
        break;
      default:   // TREX_RAND_COMMAND
        if (c.index < 0 || c.index > 2) throw Refusal(ck + "command component " + std::to_string(c.index) + " outside [0, 2]");
        if (c.interval < 0) throw Refusal(ck + "a COMMAND term needs interval >= 0");
        bits = 1u << c.index; c.mask = 1u; c.shared = 1;
        t.command = true;
        break;
    }
    if (covered[c.kind] & bits) throw Refusal(ck + "overlaps an earlier term of its kind");
    covered[c.kind] |= bits;
    if (c.kind == TREX_RAND_PUSH) t.push_slot[i] = t.pushes++;
  }
  t.terms = num_terms;
  return t;
}

TrexStartTable build_start_table(int nj, const TrexStartTerm *terms, int num_terms) {
  const std::string me = "trex_batch_set_start_state: ";
  TrexStartTable t;
  std::memset(&t, 0, sizeof t);
  t.clearance_term = -1;
  if (num_terms == 0) return t;
  if (num_terms < 0 || num_terms > TREX_START_MAXTERMS)
    throw Refusal(me + "num_terms " + std::to_string(num_terms) + " outside [0, " + std::to_string(TREX_START_MAXTERMS) + "]");
  if (!terms) throw Refusal(me + "null argument");
  uint32_t covered[TREX_START_KINDS] = {};   // per kind: the joints, or the components, taken so far
  for (int i = 0; i < num_terms; i++) {
    TrexStartTerm c = terms[i];
    const std::string ck = me + "term " + std::to_string(i) + ": ";
    if (c.kind < 0 || c.kind >= TREX_START_KINDS) throw Refusal(ck + "unknown kind " + std::to_string(c.kind));
    if (!std::isfinite(c.lo) || !std::isfinite(c.hi)) throw Refusal(ck + "lo or hi is not finite");
    if (c.lo > c.hi) throw Refusal(ck + "lo > hi");
    uint32_t bits = 0u;
    if (c.kind == TREX_START_JOINT_POSITION || c.kind == TREX_START_JOINT_VELOCITY) {
      const uint32_t all = nj >= 32 ? 0xFFFFFFFFu : (1u << nj) - 1u;
      if (c.mask & ~all) throw Refusal(ck + "a mask bit beyond the model's " + std::to_string(nj) + " joints");
      bits = c.mask ? c.mask : all;
      c.mask = bits; c.shared = c.shared != 0; c.index = 0;
    } else if (c.kind == TREX_START_FLOOR_CLEARANCE) {
      if (t.clearance_term >= 0) throw Refusal(ck + "a second FLOOR_CLEARANCE term");
      t.clearance_term = i;
      bits = 1u; c.mask = 1u; c.shared = 1; c.index = 0;
    } else {
      if (c.index < 0 || c.index > 2) throw Refusal(ck + "index " + std::to_string(c.index) + " outside [0, 2]");
      if (c.kind == TREX_START_BASE_RPY) t.rotate = 1;
      bits = 1u << c.index; c.mask = 1u; c.shared = 1;
    }
    if (covered[c.kind] & bits) throw Refusal(ck + "overlaps an earlier term of its kind");
    covered[c.kind] |= bits;
    t.term[i] = c;
  }
  t.num_terms = num_terms;
  return t;
}

void check_start_apply(int num_terms, bool done, int done_stride, bool rows, int row_stride, int nj, bool pen_in_rows) {
  const std::string me = "trex_batch_apply_start_state: ";
  if (num_terms < 1) throw Refusal(me + "no terms are set (trex_batch_set_start_state)");
  if (!done) throw Refusal(me + "done is null");
  if (done_stride < 1) throw Refusal(me + "done_stride below 1");
  if (rows && row_stride < 3 * nj + (pen_in_rows ? 5 : 2)) throw Refusal(me + "row_stride < 3J + 2 (3J + 5 with penalties in rows)");
}

MonitorLayout monitor_layout(int n_envs, int window, int cols_a, int cols_b, uint32_t env_offset, int block) {
  const std::string me = "trex_batch_set_monitor: ";
  MonitorLayout m;
  if (window == 0) return m;
  if (window < 1 || window > TREX_MON_MAXWINDOW)
    throw Refusal(me + "window " + std::to_string(window) + " outside [0, " + std::to_string(TREX_MON_MAXWINDOW) + "]");
  if (cols_a < 0 || cols_b < 0) throw Refusal(me + "a negative column count");
  if ((long long)cols_a + (long long)cols_b > TREX_MON_MAXCOLS)
    throw Refusal(me + std::to_string((long long)cols_a + (long long)cols_b) + " columns, at most " + std::to_string(TREX_MON_MAXCOLS));
  if (n_envs < 1) throw Refusal(me + "a batch without envs");
  check_env_offset(me, env_offset, n_envs);
  m.window = window; m.cols_a = cols_a; m.cols_b = cols_b; m.cols = cols_a + cols_b;
  while (m.team < m.cols) m.team *= 2;
  const int per = block / m.team;
  m.groups = (n_envs + per - 1) / per;
  const size_t n = (size_t)n_envs, C = (size_t)m.cols, W = (size_t)window;
  m.ret = m.take("ret", n * 8, 8); m.col = m.take("col", n * C * 8, 8);
  m.total = m.take("total", 8, 8); m.by_reason = m.take("by_reason", 4 * 8, 8);
  m.len = m.take("len", n * 4, 4); m.episodes = m.take("episodes", n * 4, 4); m.fin = m.take("fin", n * 4, 4);
  m.last_return = m.take("last_return", n * 4, 4); m.last_length = m.take("last_length", n * 4, 4);
  m.last_reason = m.take("last_reason", n * 4, 4); m.last_t = m.take("last_t", n * 4, 4);
  m.last_cols = m.take("last_cols", n * C * 4, 4);
  m.t = m.take("t", 4, 4);
  m.ring_return = m.take("ring_return", W * 4, 4); m.ring_length = m.take("ring_length", W * 4, 4);
  m.ring_reason = m.take("ring_reason", W * 4, 4); m.ring_env = m.take("ring_env", W * 4, 4); m.ring_t = m.take("ring_t", W * 4, 4);
  m.ring_cols = m.take("ring_cols", W * C * 4, 4);
  m.counts = m.take("counts", (size_t)m.groups * 4, 4);
  return m;
}

void check_monitor_apply(const MonitorLayout &m, bool reward, int reward_stride, bool done, int done_stride, bool block_a, int stride_a,
                         bool block_b, int stride_b) {
  const std::string me = "trex_batch_monitor_apply: ";
  if (m.window < 1) throw Refusal(me + "no monitor is set (trex_batch_set_monitor)");
  if (!reward) throw Refusal(me + "reward is null");
  if (!done) throw Refusal(me + "done is null");
  if (reward_stride < 1) throw Refusal(me + "reward_stride below 1");
  if (done_stride < 1) throw Refusal(me + "done_stride below 1");
  if (m.cols_a > 0 && !block_a) throw Refusal(me + "cols_a is null and its width is " + std::to_string(m.cols_a));
  if (m.cols_b > 0 && !block_b) throw Refusal(me + "cols_b is null and its width is " + std::to_string(m.cols_b));
  if (m.cols_a > 0 && stride_a < m.cols_a) throw Refusal(me + "stride_a " + std::to_string(stride_a) + " below the width " + std::to_string(m.cols_a));
  if (m.cols_b > 0 && stride_b < m.cols_b) throw Refusal(me + "stride_b " + std::to_string(stride_b) + " below the width " + std::to_string(m.cols_b));
}

// ---- the trainer. The message of a refusal is formed when it is thrown: these run on every call of a rollout.
void check_policy_create(int num_envs, int obs_dim, int act_dim, int hidden) {
  using namespace trex_policy;
  if (num_envs <= 0) throw Refusal("num_envs must be positive");
  if (hidden != HID) throw Refusal("the policy kernel is written for hidden = 64 (baselines' MlpPolicy)", TREX_E_UNSUPPORTED);
  if (act_dim < 1 || act_dim > POLICY_MAX_ACT) throw Refusal("act_dim must be in [1, 32]", TREX_E_UNSUPPORTED);
  if (obs_dim < 1 || obs_dim > POLICY_MAX_OBS) throw Refusal("obs_dim must be in [1, 126]", TREX_E_UNSUPPORTED);
}

void check_policy_set_critic(const PolicyShape *p, int critic_dim) {
  if (!p) throw Refusal("trex_policy_set_critic: null policy");
  if (critic_dim < 0 || critic_dim > trex_policy::POLICY_MAX_OBS)
    throw Refusal("trex_policy_set_critic: critic_dim must be in [0, 126] (0 clears)");
}

void check_policy_has_critic(const char *who, const PolicyShape *p, bool arg) {
  if (!p || !arg) throw Refusal(std::string(who) + ": null argument");
  if (!p->Dv) throw Refusal(std::string(who) + ": no critic width is set (trex_policy_set_critic)");
}

void check_policy_observe(const PolicyShape *p, bool rows, int row_stride, bool with_reward) {
  if (!p || !rows) throw Refusal("trex_policy_observe: null argument");
  if (row_stride < p->D + (with_reward ? 2 : 0)) throw Refusal("trex_policy_observe: row_stride too small");
}

void check_policy_critic_observe(const PolicyShape *p, bool rows_v, int stride_v) {
  check_policy_has_critic("trex_policy_critic_observe", p, rows_v);
  if (stride_v < p->Dv) throw Refusal("trex_policy_critic_observe: stride_v < critic_dim");
}

void check_policy_act(const PolicyShape *p, const PolicyActCall &c) {
  if (!p || !c.theta || !c.rows) throw Refusal("trex_policy_act: null argument");
  if (p->Dv) throw Refusal("trex_policy_act: the policy has a critic width set (trex_policy_critic_act takes its row)");
  if (!c.value_only && (!c.noise || !c.actions)) throw Refusal("trex_policy_act: noise / actions are null");
  if (c.value_only && !c.value_out) throw Refusal("trex_policy_act: value_out is null");
  if (c.row_stride < p->D) throw Refusal("trex_policy_act: row_stride < obs_dim");
}

void check_policy_critic_act(const PolicyShape *p, const PolicyActCall &c) {
  check_policy_has_critic("trex_policy_critic_act", p, c.theta);
  if (c.value_only) {
    if (!c.rows_v || !c.value_out) throw Refusal("trex_policy_critic_act: value_only needs rows_v and value_out");
  } else {
    if (!c.rows || !c.noise || !c.actions) throw Refusal("trex_policy_critic_act: rows / noise / actions are null");
    if (!c.rows_v && (c.value_out || c.obs_v_out))
      throw Refusal("trex_policy_critic_act: without rows_v only the policy runs: value_out and obs_v_out must be null");
  }
  if (c.rows && c.row_stride < p->D) throw Refusal("trex_policy_critic_act: row_stride < obs_dim");
  if (c.rows_v && c.stride_v < p->Dv) throw Refusal("trex_policy_critic_act: stride_v < critic_dim");
}

void check_policy_gae(const PolicyShape *p, bool buffers, int T) {
  if (!p || !buffers || T <= 0) throw Refusal("trex_policy_gae: bad argument");
}

void check_policy_minibatch_stats(const PolicyShape *p, bool buffers, int num_minibatches, int mb, int64_t num_samples) {
  if (!p || !buffers || num_minibatches <= 0 || mb <= 0 || num_samples <= 0) throw Refusal("trex_policy_minibatch_stats: bad argument");
}

void check_policy_minibatch(const PolicyShape *p, const PolicyMinibatchCall &c) {
  using namespace trex_policy;
  const auto no = [&](const char *why) { return Refusal(std::string(c.who) + why); };
  if (!p || !c.buffers) throw no(": null argument");
  if (c.mb <= 0 || c.first < 0 || c.num_samples <= 0) throw no(": bad sizes");
  if (c.distill) {
    if (c.kind != TREX_DISTILL_MSE && c.kind != TREX_DISTILL_KL) throw no(": unknown loss kind (TREX_DISTILL_MSE, TREX_DISTILL_KL)");
    if (c.kind == TREX_DISTILL_KL && !c.teacher_logstd) throw no(": the KL loss needs teacher_logstd");
    if (!c.teacher_value && c.vf_coef != 0.f) throw no(": teacher_value may be null only with vf_coef == 0");
    if (p->Dv) throw no(": the policy has a critic width set (a student has no privileged critic)");
  } else {
    // the critic entry points pass obs_v, the plain ones do not; either kind refuses an object of the other kind by name
    if (!c.critic && p->Dv) throw no(": the policy has a critic width set (the trex_policy_critic_minibatch calls take obs_v)");
    if (c.critic && !p->Dv) throw no(": no critic width is set (trex_policy_set_critic)");
    if (p->Dv > LEARN_MAX_OBS) throw no(": the learner stages 96 observation columns (critic_dim <= 96)");
  }
  if (p->D > LEARN_MAX_OBS) throw no(": the learner stages 96 observation columns (obs_dim <= 96)");
  const PolicyLayout &l = p->lay;
  if ((l.vW1 + (l.count - l.logstd)) / 4 > 256 * LEARN_UF || (l.logstd - l.vW1) / 4 > 256 * LEARN_UF)
    throw no(": the learner stages one net's parameters in one trip of 256 x 13 float4s");
}

CameraBasis camera_basis(const TrexCamera &cam, int width, int height) {
  const float cv[] = {cam.distance, cam.yaw_deg, cam.pitch_deg, cam.fov_deg, cam.near_z, cam.far_z, cam.target[0], cam.target[1], cam.target[2]};
  for (float x : cv)
    if (!std::isfinite(x)) throw Refusal("trex_batch_render: camera value is not finite");
  if (!(cam.distance > 0) || !(cam.fov_deg > 0 && cam.fov_deg < 180) || !(cam.near_z > 0 && cam.far_z > cam.near_z))
    throw Refusal("trex_batch_render: camera needs distance > 0, 0 < fov < 180, 0 < near < far");
  // camera (include/trex_batch.h): eye = target + Rz(yaw) Rx(pitch) (0, -distance, 0), up = Rz(yaw) Rx(pitch) (0, 0, 1)
  const double d2r = 3.14159265358979323846 / 180.0, yw = cam.yaw_deg * d2r, pt = cam.pitch_deg * d2r;
  const double off[3] = {cam.distance * std::cos(pt) * std::sin(yw), -cam.distance * std::cos(pt) * std::cos(yw),
                         -cam.distance * std::sin(pt)};
  const double up0[3] = {std::sin(pt) * std::sin(yw), -std::sin(pt) * std::cos(yw), std::cos(pt)};
  double f[3] = {-off[0] / cam.distance, -off[1] / cam.distance, -off[2] / cam.distance};
  double r[3] = {f[1] * up0[2] - f[2] * up0[1], f[2] * up0[0] - f[0] * up0[2], f[0] * up0[1] - f[1] * up0[0]};
  const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (double &x : r) x /= rl;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  CameraBasis b;
  for (int c = 0; c < 3; c++) {
    b.offset[c] = (float)off[c]; b.fwd[c] = (float)f[c]; b.right[c] = (float)r[c]; b.up[c] = (float)u[c];
  }
  const double ty = std::tan(0.5 * cam.fov_deg * d2r);
  b.tan_y = (float)ty; b.tan_x = (float)(ty * width / height);
  return b;
}

// ---- the planner (include/trex_planner.h)

PlannerShape check_planner_create(int groups, int samples, int horizon, int knots, int act_dim, int interpolation) {
  const std::string me = "trex_planner_create: ";
  auto range = [&](const char *what, int v, int lo, int hi) {
    if (v < lo || v > hi) throw Refusal(me + what + " " + std::to_string(v) + " outside [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
  };
  if (groups < 1) throw Refusal(me + "groups " + std::to_string(groups) + " below 1");
  range("samples", samples, 1, TREX_PLAN_MAXSAMPLES);
  range("horizon", horizon, 1, TREX_PLAN_MAXHORIZON);
  range("knots", knots, 1, std::min(horizon, TREX_PLAN_MAXKNOTS));
  range("act_dim", act_dim, 1, TREX_PLAN_MAXACT);
  if (interpolation < 0 || interpolation >= TREX_PLAN_KINDS) throw Refusal(me + "unknown interpolation " + std::to_string(interpolation));
  if ((int64_t)groups * samples * horizon * act_dim >= (int64_t)1 << 31)
    throw Refusal(me + "groups x samples x horizon x act_dim is beyond 2^31: an index would not fit 32 bits");
  PlannerShape p;
  p.G = groups; p.K = samples; p.S = horizon; p.P = knots; p.A = act_dim; p.kind = interpolation; p.N = groups * samples;
  return p;
}

TrexPlanTap plan_tap(int kind, int P, int64_t num, int64_t den) {
  TrexPlanTap tap{};
  double W[4] = {1.0, 0.0, 0.0, 0.0};
  if (P == 1 || den == 0) {
    // the constant
  } else if (kind == TREX_PLAN_HOLD) {
    const int j = (int)std::min<int64_t>(num / den, P - 1);
    for (int &i : tap.i) i = j;
  } else {
    const int j = (int)std::min<int64_t>(num / den, P - 2);
    const double t = (double)(num - (int64_t)j * den) / (double)den;
    if (kind == TREX_PLAN_LINEAR) {
      tap.i[0] = j; tap.i[1] = tap.i[2] = tap.i[3] = j + 1;
      W[0] = 1.0 - t; W[1] = t;
    } else {
      tap.i[0] = std::max(j - 1, 0); tap.i[1] = j; tap.i[2] = j + 1; tap.i[3] = std::min(j + 2, P - 1);
      const double t2 = t * t, t3 = t2 * t;
      W[0] = (-t3 + 2.0 * t2 - t) / 2.0;
      W[1] = (3.0 * t3 - 5.0 * t2 + 2.0) / 2.0;
      W[2] = (-3.0 * t3 + 4.0 * t2 + t) / 2.0;
      W[3] = (t3 - t2) / 2.0;
    }
  }
  int last = 0;
  for (int c = 0; c < 4; c++)
    if (W[c] != 0.0) last = c;
  volatile float sum = 0.f;   // (volatile: every partial sum exists as an f32, whatever the host compiler's excess precision)
  for (int c = 0; c < 4; c++) {
    if (c == last) {
      tap.w[c] = 1.f - sum;
      break;          // (the taps behind it weigh 0)
    }
    tap.w[c] = (float)W[c];
    sum = sum + tap.w[c];
  }
  return tap;
}

std::vector<TrexPlanTap> build_plan_taps(const PlannerShape &p) {
  std::vector<TrexPlanTap> taps((size_t)p.S);
  for (int s = 0; s < p.S; s++) taps[s] = plan_tap(p.kind, p.P, (int64_t)s * (p.P - 1), p.S - 1);
  return taps;
}

int plan_shift_key(const PlannerShape &p, int steps) {
  if (steps < 0) throw Refusal("trex_planner_shift: steps " + std::to_string(steps) + " below 0");
  return std::min(steps, p.S - 1);
}

std::vector<TrexPlanTap> build_plan_shift(const PlannerShape &p, int steps) {
  const int64_t k = plan_shift_key(p, steps), end = (int64_t)(p.P - 1) * (p.S - 1);
  std::vector<TrexPlanTap> taps((size_t)p.P);
  for (int q = 0; q < p.P; q++) taps[q] = plan_tap(p.kind, p.P, std::min((int64_t)q * (p.S - 1) + k * (p.P - 1), end), p.S - 1);
  return taps;
}

std::vector<float> build_plan_discount(int S, float gamma) {
  std::vector<float> g((size_t)S + 1);
  for (int s = 0; s <= S; s++) g[s] = (float)std::pow((double)gamma, s);
  return g;
}

TrexPlanNoise build_plan_noise(const PlannerShape &p, const float *sigma, const float *lo, const float *hi, uint32_t env_offset) {
  const std::string me = "trex_planner_set_noise: ";
  if (!sigma || !lo || !hi) throw Refusal(me + "null argument");
  TrexPlanNoise n;
  for (int a = 0; a < TREX_PLAN_MAXACT; a++) { n.sigma[a] = 0.f; n.lo[a] = -INFINITY; n.hi[a] = INFINITY; }
  for (int a = 0; a < p.A; a++) {
    const std::string ck = me + "action " + std::to_string(a) + ": ";
    if (!std::isfinite(sigma[a]) || sigma[a] < 0.f) throw Refusal(ck + "sigma is negative or not finite");
    if (std::isnan(lo[a]) || std::isnan(hi[a])) throw Refusal(ck + "a limit is NaN");
    if (lo[a] > hi[a]) throw Refusal(ck + "lo > hi");
    n.sigma[a] = sigma[a]; n.lo[a] = lo[a]; n.hi[a] = hi[a];
  }
  check_env_offset(me, env_offset, p.N);
  return n;
}

void check_plan_update(const PlannerShape &p, bool noise_set, bool reward, int64_t step_stride, int64_t env_stride, float gamma,
                       float temperature) {
  const std::string me = "trex_planner_update: ";
  if (!noise_set) throw Refusal(me + "no noise is set (trex_planner_set_noise)");
  if (!reward) throw Refusal(me + "reward is null");
  if (step_stride < 1) throw Refusal(me + "step_stride below 1");
  if (env_stride < 1) throw Refusal(me + "env_stride below 1");
  if (!std::isfinite(gamma) || gamma < 0.f) throw Refusal(me + "gamma is negative or not finite");
  if (!std::isfinite(temperature) || temperature < 0.f) throw Refusal(me + "temperature is negative or not finite");
  // (S - 1) step_stride + (N - 1) env_stride must leave room for the byte count in 63 bits
  if (step_stride > ((int64_t)1 << 40) || env_stride > ((int64_t)1 << 40)) throw Refusal(me + "a stride beyond 2^40");
}

size_t plan_column_bytes(const PlannerShape &p, int64_t step_stride, int64_t env_stride) {
  return ((size_t)(p.S - 1) * (size_t)step_stride + (size_t)(p.N - 1) * (size_t)env_stride + 1) * sizeof(float);
}

// ---- the mirror maps (include/trex_symmetry.h)

MirrorWords build_mirror_words(const int32_t *src, const int8_t *sign, int width) {
  const std::string me = "trex_mirror_table_create: ";
  if (!src || !sign) throw Refusal(me + "null argument");
  if (width < 1 || width > TREX_MIRROR_MAXWIDTH)
    throw Refusal(me + "width " + std::to_string(width) + " outside [1, " + std::to_string(TREX_MIRROR_MAXWIDTH) + "]");
  MirrorWords t;
  t.word.resize(width);
  std::vector<char> taken(width, 0);
  for (int c = 0; c < width; c++) {
    const std::string col = me + "column " + std::to_string(c) + ": ";
    if (src[c] < 0 || src[c] >= width) throw Refusal(col + "src " + std::to_string(src[c]) + " outside [0, width)");
    if (taken[src[c]]) throw Refusal(col + "src " + std::to_string(src[c]) + " is named twice: src is no permutation");
    if (sign[c] != 1 && sign[c] != -1) throw Refusal(col + "sign " + std::to_string((int)sign[c]) + " is neither +1 nor -1");
    taken[src[c]] = 1;
    t.word[c] = (uint32_t)src[c] | (sign[c] < 0 ? TREX_MIRROR_NEG : 0u);
  }
  t.involution = true;
  for (int c = 0; c < width; c++) t.involution = t.involution && src[src[c]] == c && sign[src[c]] == sign[c];
  return t;
}

void check_mirror_rows(int table_width, const void *in, int in_stride, const void *out, int out_stride, int n, int width) {
  const std::string me = "trex_mirror_rows: ";
  if (!in || !out) throw Refusal(me + "null argument");
  if (n < 1) throw Refusal(me + "n " + std::to_string(n) + " below 1");
  if (width != table_width) throw Refusal(me + "width " + std::to_string(width) + " is not the table's " + std::to_string(table_width));
  if (in_stride < width || out_stride < width) throw Refusal(me + "a stride below the width");
  if ((int64_t)n * std::max(in_stride, out_stride) >= (int64_t)1 << 31)
    throw Refusal(me + "n x stride is beyond 2^31: an index would not fit 32 bits");
  if (in == out && in_stride == out_stride) return;      // in place: a row is read completely before any of it is stored
  if (ranges_overlap(in, row_block_bytes((size_t)n, in_stride, width), out, row_block_bytes((size_t)n, out_stride, width)))
    throw Refusal(me + "in and out overlap (only in == out with equal strides may)");
}

void check_mirror_augment(int obs_width, int act_width, int critic_width, bool has_critic_table, bool buffers, bool obs_v,
                          int64_t num_samples, int D, int A, int Dv) {
  const std::string me = "trex_mirror_augment: ";
  if (!buffers) throw Refusal(me + "null argument");
  if (has_critic_table != obs_v || has_critic_table != (Dv != 0))
    throw Refusal(me + "critic_table, obs_v and Dv go together: all given, or NULL, NULL and 0");
  if (num_samples < 1) throw Refusal(me + "num_samples " + std::to_string(num_samples) + " below 1");
  if (D != obs_width) throw Refusal(me + "D " + std::to_string(D) + " is not the obs table's width " + std::to_string(obs_width));
  if (A != act_width) throw Refusal(me + "A " + std::to_string(A) + " is not the act table's width " + std::to_string(act_width));
  if (has_critic_table && Dv != critic_width)
    throw Refusal(me + "Dv " + std::to_string(Dv) + " is not the critic table's width " + std::to_string(critic_width));
  if (num_samples >= ((int64_t)1 << 30) / std::max(D, std::max(A, std::max(Dv, 1))))
    throw Refusal(me + "2 num_samples x the widest width is beyond 2^31: an index would not fit 32 bits");
}

namespace {

struct Frame { double R[9], t[3]; };     // child <- in parent: x_parent = R x_child + t
Frame frame_mul(const Frame &a, const Frame &b) {
  Frame c;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c.R[3 * i + j] = a.R[3 * i] * b.R[j] + a.R[3 * i + 1] * b.R[3 + j] + a.R[3 * i + 2] * b.R[6 + j];
    c.t[i] = a.R[3 * i] * b.t[0] + a.R[3 * i + 1] * b.t[1] + a.R[3 * i + 2] * b.t[2] + a.t[i];
  }
  return c;
}
Frame frame_inverse(const Frame &a) {
  Frame c;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c.R[3 * i + j] = a.R[3 * j + i];
  for (int i = 0; i < 3; i++) c.t[i] = -(c.R[3 * i] * a.t[0] + c.R[3 * i + 1] * a.t[1] + c.R[3 * i + 2] * a.t[2]);
  return c;
}
Frame frame_of(const Mat3 &R, const Vec3 &t) {
  Frame c;
  std::copy(R.m, R.m + 9, c.R);
  c.t[0] = t.x; c.t[1] = t.y; c.t[2] = t.z;
  return c;
}
void rotate(const Frame &f, const Vec3 &v, bool translate, double out[3]) {
  for (int i = 0; i < 3; i++) out[i] = f.R[3 * i] * v.x + f.R[3 * i + 1] * v.y + f.R[3 * i + 2] * v.z + (translate ? f.t[i] : 0.0);
}
double dist3(const double a[3], const double b[3]) {
  return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
}

// every body's frame at q = 0 in URDF link 0's frame
std::vector<Frame> body_frames(const HostModel &h) {
  const Frame link0 = frame_of(h.link_tf[0].R, h.link_tf[0].t);
  std::vector<Frame> T(h.nb);
  for (int i = 0; i < h.nb; i++)
    T[i] = i == 0 ? frame_inverse(link0) : frame_mul(T[h.parent[i]], frame_of(h.joint_rot[i], h.joint_pos[i]));
  return T;
}

// the pairing about one axis; false with `why` where the model has none
bool mirror_about(const HostModel &h, int lat, double tol, ModelMirror &out, std::string &why) {
  const int nb = h.nb, nj = nb - 1;
  // every body's frame at q = 0 in URDF link 0's frame; its joint origin, joint axis and COM there (body 0: link 0's origin, no axis)
  const std::vector<Frame> T = body_frames(h);
  std::vector<std::array<double, 3>> o(nb), a(nb), c(nb);
  for (int i = 0; i < nb; i++) {
    for (int k = 0; k < 3; k++) o[i][k] = i == 0 ? 0.0 : T[i].t[k];
    rotate(T[i], h.joint_axis[i], false, a[i].data());
    rotate(T[i], h.com[i], true, c[i].data());
  }
  auto image = [&](const std::array<double, 3> &v) { std::array<double, 3> r = v; r[lat] = -r[lat]; return r; };
  out.lateral = lat;
  out.body_pair.assign(nb, -1);
  for (int i = 0; i < nb; i++) {
    const std::array<double, 3> want = image(o[i]);
    if (dist3(want.data(), o[i].data()) <= tol) { out.body_pair[i] = i; continue; }
    double best = tol;
    for (int j = 0; j < nb; j++) {
      const double d = dist3(want.data(), o[j].data());
      if (j != i && d <= best && (out.body_pair[i] < 0 || d < best)) { best = d; out.body_pair[i] = j; }
    }
    if (out.body_pair[i] < 0) { why = "body " + std::to_string(i) + " (" + h.body_names[i] + ") has no partner within tol_pos"; return false; }
  }
  for (int i = 0; i < nb; i++) {
    const int j = out.body_pair[i];
    if (out.body_pair[j] != i) { why = "the pairing of body " + std::to_string(i) + " (" + h.body_names[i] + ") is not an involution"; return false; }
    if (i > 0 && out.body_pair[h.parent[i]] != h.parent[j]) {
      why = "the parents of body " + std::to_string(i) + " (" + h.body_names[i] + ") and of its partner are not paired";
      return false;
    }
  }
  std::vector<int> slot(nb, -1);
  for (int k = 0; k < nj; k++) slot[h.obs_order[k]] = k;
  out.pair.assign(nj, 0); out.sign.assign(nj, 1);
  for (double &r : out.residual) r = 0.0;
  for (int i = 0; i < nb; i++) {
    const int j = out.body_pair[i];
    const std::array<double, 3> oj = image(o[j]), cj = image(c[j]);
    out.residual[0] = std::max(out.residual[0], std::fabs(h.mass[i] - h.mass[j]) / std::max(h.mass[i], h.mass[j]));
    out.residual[1] = std::max(out.residual[1], dist3(o[i].data(), oj.data()));
    out.residual[3] = std::max(out.residual[3], dist3(c[i].data(), cj.data()));
    if (i == 0) continue;
    // an axis reflects as an axial vector: the image of a is -S a
    std::array<double, 3> aj = image(a[j]);
    for (double &v : aj) v = -v;
    const double d = a[i][0] * aj[0] + a[i][1] * aj[1] + a[i][2] * aj[2];
    const double cr[3] = {a[i][1] * aj[2] - a[i][2] * aj[1], a[i][2] * aj[0] - a[i][0] * aj[2], a[i][0] * aj[1] - a[i][1] * aj[0]};
    const int8_t s = d < 0.0 ? -1 : 1;
    out.residual[2] = std::max(out.residual[2], std::atan2(std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), std::fabs(d)));
    const double lo = s > 0 ? h.q_lower[j] : -h.q_upper[j], hi = s > 0 ? h.q_upper[j] : -h.q_lower[j];
    if (std::fabs(h.q_lower[i] - lo) > tol || std::fabs(h.q_upper[i] - hi) > tol) {
      why = "the limits of joint " + h.joint_names[i] + " and of its partner's image differ by more than tol_pos";
      return false;
    }
    out.pair[slot[i]] = slot[j]; out.sign[slot[i]] = s;
  }
  out.residual[4] = std::fabs(c[0][lat]);
  return true;
}

}  // namespace

ModelMirror build_model_mirror(const HostModel &h, int lateral, double tol_pos) {
  const std::string me = "trex_model_mirror_table: ";
  if (lateral < -1 || lateral > 2) throw Refusal(me + "lateral " + std::to_string(lateral) + " is none of -1, 0, 1, 2");
  if (!(tol_pos >= 0.0) || !std::isfinite(tol_pos)) throw Refusal(me + "tol_pos is negative or not finite");
  ModelMirror m;
  std::string why;
  if (lateral >= 0) {
    if (!mirror_about(h, lateral, tol_pos, m, why)) throw Refusal(me + why);
    return m;
  }
  // the search: the first axis that pairs some body with ANOTHER one; where none does, the first that pairs at all
  ModelMirror first;
  bool have = false;
  std::string first_why;
  for (int lat = 0; lat < 3; lat++) {
    if (!mirror_about(h, lat, tol_pos, m, why)) { if (first_why.empty()) first_why = "about axis " + std::to_string(lat) + ": " + why; continue; }
    for (int i = 0; i < h.nb; i++)
      if (m.body_pair[i] != i) return m;
    if (!have) { first = m; have = true; }
  }
  if (!have) throw Refusal(me + "no axis of link 0 is normal to a mirror plane of the model (" + first_why + ")");
  return first;
}

RowMirror build_mirror_row_table(const HostModel &h, const ModelMirror &mm, double tol_pos, const TrexObsChannel *channels, int num_channels,
                                 int action_cols, int tail, const int32_t *extern_src, const int8_t *extern_sign) {
  const std::string me = "trex_model_mirror_row_table: ";
  const int nj = h.nb - 1, lat = mm.lateral, links = (int)h.link_body.size();
  if (num_channels < 0 || (num_channels > 0 && !channels)) throw Refusal(me + "null argument");
  if (action_cols != nj && action_cols != 2 * nj) throw Refusal(me + "action_cols " + std::to_string(action_cols) + " is neither J nor 2 J");
  if (tail != 2 && tail != 5) throw Refusal(me + "tail " + std::to_string(tail) + " is neither 2 nor 5");
  // the first column of every channel, its width, and the columns of the EXTERNAL block
  std::vector<int> col0(num_channels), width(num_channels), ext0(num_channels, 0);
  std::vector<int> ext_col;                       // extern index -> column of the row
  int col = 3 * nj;
  for (int k = 0; k < num_channels; k++) {
    const TrexObsChannel &c = channels[k];
    const std::string ck = me + "channel " + std::to_string(k) + ": ";
    if (c.kind < 0 || c.kind >= TREX_OBS_KINDS) throw Refusal(ck + "unknown kind " + std::to_string(c.kind));
    const bool linked = c.kind == TREX_OBS_POINT_POSITION || c.kind == TREX_OBS_POINT_VELOCITY || c.kind == TREX_OBS_POINT_HEIGHT ||
                        c.kind == TREX_OBS_CONTACT_FORCE;
    if (linked && (c.link < 0 || c.link >= links)) throw Refusal(ck + "link " + std::to_string(c.link) + " out of range");
    if (c.kind == TREX_OBS_EXTERNAL && c.link < 1) throw Refusal(ck + "an EXTERNAL channel needs link = k >= 1 columns");
    col0[k] = col;
    width[k] = c.kind == TREX_OBS_PREV_ACTION ? action_cols : c.kind == TREX_OBS_EXTERNAL ? c.link :
               (c.kind == TREX_OBS_BASE_HEIGHT || c.kind == TREX_OBS_POINT_HEIGHT || c.kind == TREX_OBS_CONTACT_FORCE) ? 1 : 3;
    if (c.kind == TREX_OBS_EXTERNAL) {
      ext0[k] = (int)ext_col.size();
      for (int i = 0; i < width[k]; i++) ext_col.push_back(col + i);
      if (!extern_src || !extern_sign) throw Refusal(ck + "an EXTERNAL channel needs extern_src and extern_sign");
    }
    col += width[k];
    if (col + tail > TREX_MIRROR_MAXWIDTH) throw Refusal(me + "the row is wider than " + std::to_string(TREX_MIRROR_MAXWIDTH) + " columns");
  }
  const int X = (int)ext_col.size(), W = col + tail;
  std::vector<char> taken(X, 0);
  for (int e = 0; e < X; e++) {
    if (extern_src[e] < 0 || extern_src[e] >= X || taken[extern_src[e]] || (extern_sign[e] != 1 && extern_sign[e] != -1))
      throw Refusal(me + "extern column " + std::to_string(e) + ": extern_src is no permutation of the EXTERNAL columns or a sign is neither +1 nor -1");
    taken[extern_src[e]] = 1;
  }
  // a channel's point at q = 0 in link 0's frame
  const std::vector<Frame> T = body_frames(h);
  auto point_of = [&](const TrexObsChannel &c, double out[3]) {
    const Frame f = frame_mul(T[h.link_body[c.link]], frame_of(h.link_tf[c.link].R, h.link_tf[c.link].t));
    rotate(f, Vec3{c.local_xyz[0], c.local_xyz[1], c.local_xyz[2]}, true, out);
  };
  auto partner = [&](int k) {
    const TrexObsChannel &c = channels[k];
    if (c.kind <= TREX_OBS_BASE_HEIGHT || c.kind >= TREX_OBS_PREV_ACTION) return k;
    double x[3];
    if (c.kind != TREX_OBS_CONTACT_FORCE) { point_of(c, x); x[lat] = -x[lat]; }
    for (int j = 0; j < num_channels; j++) {
      const TrexObsChannel &d = channels[j];
      if (d.kind != c.kind || d.scale != c.scale || mm.body_pair[h.link_body[c.link]] != h.link_body[d.link]) continue;
      if (c.kind == TREX_OBS_CONTACT_FORCE) return j;
      double y[3];
      point_of(d, y);
      if (dist3(x, y) <= tol_pos) return j;
    }
    throw Refusal(me + "channel " + std::to_string(k) + " has no mirrored channel in the specification (the same kind and scale, the mirrored "
                  "link" + (c.kind == TREX_OBS_CONTACT_FORCE ? ")" : ", the image of local_xyz within tol_pos)"));
  };
  RowMirror r;
  r.src.resize(W); r.sign.assign(W, 1);
  for (int b = 0; b < 3; b++)
    for (int k = 0; k < nj; k++) { r.src[b * nj + k] = b * nj + mm.pair[k]; r.sign[b * nj + k] = mm.sign[k]; }
  for (int k = 0; k < num_channels; k++) {
    const TrexObsChannel &c = channels[k];
    const int p = partner(k);
    for (int i = 0; i < width[k]; i++) {
      const int at = col0[k] + i;
      r.src[at] = col0[p] + i;
      switch (c.kind) {
        case TREX_OBS_PROJECTED_GRAVITY: case TREX_OBS_BASE_LINEAR_VELOCITY: case TREX_OBS_POINT_POSITION: case TREX_OBS_POINT_VELOCITY:
          r.sign[at] = i == lat ? -1 : 1;      // a polar vector in base axes
          break;
        case TREX_OBS_BASE_ANGULAR_VELOCITY:
          r.sign[at] = i == lat ? 1 : -1;      // an axial vector
          break;
        case TREX_OBS_PREV_ACTION:
          r.src[at] = col0[k] + (i < nj ? mm.pair[i] : nj + mm.pair[i - nj]);
          r.sign[at] = i < nj ? mm.sign[i] : 1;
          break;
        case TREX_OBS_EXTERNAL:
          r.src[at] = ext_col[extern_src[ext0[k] + i]];
          r.sign[at] = extern_sign[ext0[k] + i];
          break;
        default: break;                        // a height, a contact force: unchanged
      }
    }
  }
  for (int i = 0; i < tail; i++) r.src[col + i] = col + i;
  return r;
}

void build_mirror_action_table(const int32_t *pair, const int8_t *sign, int nj, bool stiffness, int32_t *src_out, int8_t *sign_out) {
  for (int k = 0; k < nj; k++) {
    src_out[k] = pair[k]; sign_out[k] = sign[k];
    if (stiffness) { src_out[nj + k] = nj + pair[k]; sign_out[nj + k] = 1; }
  }
}

void build_mirror_command_table(int lateral, int32_t src_out[3], int8_t sign_out[3]) {
  for (int k = 0; k < 3; k++) src_out[k] = k;
  sign_out[0] = lateral == 0 ? -1 : 1;
  sign_out[1] = lateral == 1 ? -1 : 1;
  sign_out[2] = lateral == 2 ? 1 : -1;      // wz is the z component of an axial vector
}

}  // namespace trex
