// C-ABI of include/trex_motion.h: the motion clip of a batch, its clocks, its tracking terms and the three launches of motion.hip.
// Apart from trex_batch_motion_reset, which writes the state of the envs it resets, nothing here changes what a step launch does.
#include <cstring>

#include "batch.hpp"
#include "motion.h"

namespace {

// the launch arguments every motion launch shares; `who`: the call, for the refusal of a probe set that changed its size
int motion_args(TrexBatch *b, const std::string &who, TrexMotArgs &a) {
  const TrexBatch::Motion &m = b->motion;
  const trex::MotionTable &t = m.table;
  if (t.frames < 2) return fail(TREX_E_INVALID, who + "no clip is set (trex_batch_set_motion)");
  if (m.probe_set >= 0 && b->probes[m.probe_set].n != m.probes)
    return fail(TREX_E_INVALID, who + "probe set " + std::to_string(m.probe_set) + " holds " + std::to_string(b->probes[m.probe_set].n) +
                                    " probes, the clip was set with " + std::to_string(m.probes) + " (set the clip again)");
  a = TrexMotArgs{};
  a.model = b->dmodel; a.table = m.blob.as<float>();
  a.base = b->arr.base; a.q = b->arr.q; a.qd = b->arr.qd;
  a.t0 = m.st.t0; a.k = m.st.k;
  a.held = m.held.as<float>();
  if (m.probe_set >= 0) {
    a.probe_body = b->probes[m.probe_set].body.as<int32_t>();
    a.probe_tf = b->probes[m.probe_set].tf.as<float>();
  }
  for (size_t k = 0; k < m.terms.size(); k++) a.term[k] = m.terms[k];
  a.n_envs = b->n; a.nj = b->nj; a.frames = t.frames; a.stride = t.stride; a.loop = t.loop ? 1 : 0;
  a.num_terms = (int)m.terms.size(); a.num_probes = m.probes;
  a.frame_dt = t.frame_dt; a.inv_dt = t.inv_dt; a.duration = t.duration; a.inv_duration = t.inv_duration;
  a.disp[0] = t.disp[0]; a.disp[1] = t.disp[1];
  a.Ts = (float)b->step_seconds; a.step_weight = m.step_weight;
  fill_base(b, a);
  return TREX_OK;
}

}  // namespace

extern "C" {

int trex_batch_set_motion(TrexBatch *b, const double *frames_host, const double *velocities_host, int num_frames, double frame_dt,
                          int loop, int probe_set) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_set_motion: ";
  TrexBatch::Motion &m = b->motion;
  trex::MotionTable t;
  trex::MotionClockLayout l;
  if (int c = built([&] {
        t = trex::build_motion_table(m.q_lower, m.q_upper, b->obs_order, frames_host, velocities_host, num_frames, frame_dt, loop);
        l = trex::motion_clock_layout(b->n);
      }))
    return c;
  int probes = 0;
  if (t.frames > 0 && probe_set != -1) {
    if (probe_set < 0 || probe_set >= TREX_LINK_SETS)
      return fail(TREX_E_INVALID, me + "probe set " + std::to_string(probe_set) + " outside [0, " + std::to_string(TREX_LINK_SETS) + ") (-1: none)");
    probes = b->probes[probe_set].n;
    if (probes < 1) return fail(TREX_E_INVALID, me + "probe set " + std::to_string(probe_set) + " is empty (trex_batch_set_link_probes)");
    if (probes > TREX_MOT_MAXPROBES)
      return fail(TREX_E_INVALID, me + "probe set " + std::to_string(probe_set) + " holds " + std::to_string(probes) + " probes, at most " +
                                      std::to_string(TREX_MOT_MAXPROBES));
  }
  DeviceGuard guard(b->device);
  DeviceBuf blob, clock;
  if (t.frames > 0) {
    HIP_TRY(blob.alloc(t.rows.size() * sizeof(float), false));
    HIP_TRY(hipMemcpy(blob.p, t.rows.data(), blob.bytes, hipMemcpyHostToDevice));
    HIP_TRY(clock.alloc(l.bytes, true));
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  t.rows = {};
  m.blob = std::move(blob);   // (frees the old table)
  m.clock = std::move(clock);
  m.st = {};
  if (m.clock) m.st = {member_at<float>(m.clock, l.t0), member_at<int32_t>(m.clock, l.k)};
  m.held.release();
  m.terms.clear();
  m.step_weight = 1.f;
  m.table = std::move(t);
  m.probe_set = m.table.frames > 0 && probes > 0 ? probe_set : -1;
  m.probes = probes;
  return TREX_OK;
}

int trex_batch_motion_info(const TrexBatch *b, int *frames, double *duration, int *num_terms, int *probes) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Motion &m = b->motion;
  if (frames) *frames = m.table.frames;
  if (duration) *duration = (double)m.table.duration;
  if (num_terms) *num_terms = (int)m.terms.size();
  if (probes) *probes = m.probes;
  return TREX_OK;
}

int trex_batch_motion_sample(TrexBatch *b, const float *time_dev, float *state_out, float *points_out, float *phase_out, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_motion_sample: ";
  TrexMotArgs a;
  if (int c = motion_args(b, me, a)) return c;
  if (!state_out && !points_out && !phase_out) return fail(TREX_E_INVALID, me + "state, points and phase are all null");
  if (points_out && a.num_probes < 1) return fail(TREX_E_INVALID, me + "points asked for and the clip has no probe set");
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, time_dev, n * sizeof(float), "trex_batch_motion_sample: time");
  BUF_TRY(b, state_out, n * TREX_MOT_COLS(b->nj) * sizeof(float), "trex_batch_motion_sample: state");
  BUF_TRY(b, points_out, n * a.num_probes * 3 * sizeof(float), "trex_batch_motion_sample: points");
  BUF_TRY(b, phase_out, n * sizeof(float), "trex_batch_motion_sample: phase");
  a.time = time_dev; a.state_out = state_out; a.points_out = points_out; a.phase_out = phase_out;
  HIP_TRY(trex_launch_motion_sample(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_set_motion_reward(TrexBatch *b, const TrexMotionTerm *terms_host, int num_terms, float step_weight) {
  if (check_batch(b)) return TREX_E_INVALID;
  TrexBatch::Motion &m = b->motion;
  if (m.table.frames < 2 && num_terms != 0) return fail(TREX_E_INVALID, "trex_batch_set_motion_reward: no clip is set (trex_batch_set_motion)");
  std::vector<TrexMotTerm> terms;
  trex::Layout l;
  if (int c = built([&] {
        terms = trex::build_motion_terms(b->nj, m.probes > 0, terms_host, num_terms, step_weight);
        l = trex::motion_held_layout(b->n, (int)terms.size());
      }))
    return c;
  DeviceGuard guard(b->device);
  DeviceBuf held;
  if (l.bytes > 0) HIP_TRY(held.alloc(l.bytes, true));
  HIP_TRY(hipDeviceSynchronize());   // (no launch still writes the held values this call replaces)
  m.held = std::move(held);
  m.terms = std::move(terms);
  m.step_weight = m.terms.empty() ? 1.f : step_weight;
  return TREX_OK;
}

int trex_batch_compose_motion_reward(TrexBatch *b, float *rows_dev, int row_stride, float *terms_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_compose_motion_reward: ";
  TrexMotArgs a;
  if (int c = motion_args(b, me, a)) return c;
  if (a.num_terms < 1) return fail(TREX_E_INVALID, me + "no terms are set (trex_batch_set_motion_reward)");
  if (!rows_dev) return fail(TREX_E_INVALID, me + "rows is null");
  const int nobs = 3 * b->nj, tail = b->pen_in_rows ? 5 : 2;
  if (row_stride < nobs + tail) return fail(TREX_E_INVALID, me + "row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, rows_dev, trex::row_block_bytes(n, row_stride, nobs + tail), "trex_batch_compose_motion_reward: rows");
  BUF_TRY(b, terms_dev, n * a.num_terms * sizeof(float), "trex_batch_compose_motion_reward: terms");
  a.rows = rows_dev; a.row_stride = row_stride; a.terms_out = terms_dev;
  HIP_TRY(trex_launch_motion_compose(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_motion_reset(TrexBatch *b, const uint8_t *mask_dev, const float *time_dev, float *rows_dev, int row_stride, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_motion_reset: ";
  TrexMotArgs a;
  if (int c = motion_args(b, me, a)) return c;
  const int nobs = 3 * b->nj, tail = b->pen_in_rows ? 5 : 2;
  if (rows_dev && row_stride < nobs + tail) return fail(TREX_E_INVALID, me + "row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, mask_dev, n, "trex_batch_motion_reset: mask");
  BUF_TRY(b, time_dev, n * sizeof(float), "trex_batch_motion_reset: time");
  BUF_TRY(b, rows_dev, trex::row_block_bytes(n, row_stride, nobs + tail), "trex_batch_motion_reset: rows");
  a.mask = mask_dev; a.time = time_dev; a.rows = rows_dev; a.row_stride = row_stride;
  a.warm = b->warm.as<float>();
  HIP_TRY(trex_launch_motion_reset(a, (hipStream_t)stream));
  return TREX_OK;
}

}  // extern "C"
