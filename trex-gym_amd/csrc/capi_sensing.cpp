// C-ABI of include/trex_sensing.h: the sensor model of a batch - its groups, its counters and history, the action delay - and the
// three launches of sensing.hip. Nothing here changes what a step launch does: the launches rewrite the caller's rows and actions.
#include <cstring>

#include "batch.hpp"
#include "sensing.h"

namespace {

// `bytes` of counters, zeroed, and the pointers into them; an empty layout: no allocation, null pointers
int make_counters(const trex::SenseCounterLayout &l, DeviceBuf &state, TrexBatch::Sensing::Counters &st) {
  st = {};
  if (l.bytes == 0) return TREX_OK;
  HIP_TRY(state.alloc(l.bytes, true));
  st = {member_at<uint32_t>(state, l.ep), member_at<uint32_t>(state, l.k), member_at<uint32_t>(state, l.started),
        member_at<int32_t>(state, l.delay)};
  return TREX_OK;
}

}  // namespace

extern "C" {

int trex_batch_set_sensing(TrexBatch *b, const TrexSenseGroup *groups_host, int num_groups, uint64_t seed, uint32_t env_offset) {
  if (check_batch(b)) return TREX_E_INVALID;
  trex::SenseTable t;
  trex::SenseCounterLayout counters;
  trex::Layout history;
  if (int c = built([&] {
        trex::check_env_offset("trex_batch_set_sensing: ", env_offset, b->n);
        t = trex::build_sense_table(3 * b->nj + b->observation.table.extra, groups_host, num_groups);
        counters = trex::sense_counter_layout(b->n, t.groups);
        history = trex::sense_hist_layout(b->n, t.delayed);
      }))
    return c;
  DeviceGuard guard(b->device);
  DeviceBuf blob, state, hist;
  TrexBatch::Sensing::Counters st;
  if (t.groups > 0) {
    HIP_TRY(blob.alloc(t.blob.size(), false));
    HIP_TRY(hipMemcpy(blob.p, t.blob.data(), blob.bytes, hipMemcpyHostToDevice));
  }
  if (int c = make_counters(counters, state, st)) return c;
  if (history.bytes > 0) HIP_TRY(hist.alloc(history.bytes, true));
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  t.blob = {};
  TrexBatch::Sensing &s = b->sensing;
  s.blob = std::move(blob);   // (frees the old table, counters and history)
  s.state = std::move(state);
  s.hist = std::move(hist);
  s.st = st;
  s.table = std::move(t);
  s.seed = seed; s.env_offset = env_offset;
  return TREX_OK;
}

int trex_batch_apply_sensing(TrexBatch *b, const float *rows_dev, int row_stride, float *out_rows_dev, int out_stride, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_apply_sensing: ";
  const TrexBatch::Sensing &s = b->sensing;
  const trex::SenseTable &t = s.table;
  if (t.groups < 1) return fail(TREX_E_INVALID, me + "no groups are set (trex_batch_set_sensing)");
  const int D = 3 * b->nj + b->observation.table.extra, tail = b->pen_in_rows ? 5 : 2, width = D + tail;
  if (D != t.obs_dim)
    return fail(TREX_E_INVALID, me + "the observation dimension is " + std::to_string(D) + ", the groups were set for " + std::to_string(t.obs_dim) +
                                    " (set the groups again)");
  if (!rows_dev || !out_rows_dev) return fail(TREX_E_INVALID, me + "rows or out_rows is null");
  if (row_stride < width || out_stride < width)
    return fail(TREX_E_INVALID, me + "a stride below " + std::to_string(width) + " = 3J + E + the tail");
  const size_t n = (size_t)b->n;
  const size_t rows_bytes = trex::row_block_bytes(n, row_stride, width), out_bytes = trex::row_block_bytes(n, out_stride, width);
  if (rows_dev == out_rows_dev) {
    if (row_stride != out_stride) return fail(TREX_E_INVALID, me + "in place, and the two strides differ");
  } else if (trex::ranges_overlap(rows_dev, rows_bytes, out_rows_dev, out_bytes)) {
    return fail(TREX_E_INVALID, me + "out_rows overlaps rows in part");
  }
  DeviceGuard guard(b->device);
  BUF_TRY(b, rows_dev, rows_bytes, "trex_batch_apply_sensing: rows");
  BUF_TRY(b, out_rows_dev, out_bytes, "trex_batch_apply_sensing: out_rows");
  TrexSenseArgs a{};
  const char *blob = s.blob.as<char>();
  a.group = (const TrexSenseGrp *)blob; a.col_group = (const int16_t *)(blob + t.o_col_group); a.col_hist = (const int16_t *)(blob + t.o_col_hist);
  a.rows = rows_dev; a.out = out_rows_dev;
  a.ep = s.st.ep; a.k = s.st.k; a.started = s.st.started; a.delay = s.st.delay;
  a.hist = s.hist.as<float>();
  a.n_envs = b->n; a.obs_dim = D; a.tail = tail; a.num_groups = t.groups; a.delayed = t.delayed;
  a.row_stride = row_stride; a.out_stride = out_stride;
  a.lanes = 8;
  while (a.lanes * 4 < width) a.lanes *= 2;   // (width <= 512 + 5: at most 256)
  a.key0 = (uint32_t)s.seed; a.key1 = (uint32_t)(s.seed >> 32); a.env_offset = s.env_offset;
  HIP_TRY(trex_launch_sensing(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_sensing_reset(TrexBatch *b, const uint8_t *mask_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Sensing &s = b->sensing;
  if (!s.state && !s.act_state)
    return fail(TREX_E_INVALID, "trex_batch_sensing_reset: neither groups nor an action delay are set (trex_batch_set_sensing, trex_batch_set_action_delay)");
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, mask_dev, n, "trex_batch_sensing_reset: mask");
  HIP_TRY(trex_launch_sensing_reset(mask_dev, b->n, s.st.started, s.act_st.started, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_set_action_delay(TrexBatch *b, int delay_min, int delay_max) {
  if (check_batch(b)) return TREX_E_INVALID;
  const int cols = b->action_cols();
  trex::SenseCounterLayout counters;
  trex::Layout history;
  if (int c = built([&] {
        trex::check_sense_delay("trex_batch_set_action_delay: ", delay_min, delay_max);
        if (delay_max > 0) {   // the counters of one group, the history of the action's columns
          counters = trex::sense_counter_layout(b->n, 1);
          history = trex::sense_hist_layout(b->n, cols);
        }
      }))
    return c;
  if (cols > 64) return fail(TREX_E_INVALID, "trex_batch_set_action_delay: action rows wider than 64 columns");   // (the launch's 64 lanes per env)
  DeviceGuard guard(b->device);
  DeviceBuf state, hist;
  TrexBatch::Sensing::Counters st;
  if (int c = make_counters(counters, state, st)) return c;
  if (history.bytes > 0) HIP_TRY(hist.alloc(history.bytes, true));
  HIP_TRY(hipDeviceSynchronize());   // (no launch still writes the history this call replaces)
  TrexBatch::Sensing &s = b->sensing;
  s.act_state = std::move(state);
  s.act_hist = std::move(hist);
  s.act_st = st;
  s.act_min = delay_min; s.act_max = delay_max; s.act_cols = delay_max > 0 ? cols : 0;
  return TREX_OK;
}

int trex_batch_delay_actions(TrexBatch *b, const float *actions_dev, const uint8_t *done_prev_dev, float *out_actions_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_delay_actions: ";
  const TrexBatch::Sensing &s = b->sensing;
  if (!s.act_state) return fail(TREX_E_INVALID, me + "no action delay is set (trex_batch_set_action_delay)");
  if (s.act_cols != b->action_cols())
    return fail(TREX_E_INVALID, me + "the action rows are " + std::to_string(b->action_cols()) + " wide, the delay was set with " +
                                    std::to_string(s.act_cols) + " (set the delay again)");
  if (!actions_dev || !out_actions_dev) return fail(TREX_E_INVALID, me + "actions or out_actions is null");
  const size_t n = (size_t)b->n, bytes = n * s.act_cols * sizeof(float);
  if (actions_dev != out_actions_dev && trex::ranges_overlap(actions_dev, bytes, out_actions_dev, bytes))
    return fail(TREX_E_INVALID, me + "out_actions overlaps actions in part");
  DeviceGuard guard(b->device);
  BUF_TRY(b, actions_dev, bytes, "trex_batch_delay_actions: actions");
  BUF_TRY(b, out_actions_dev, bytes, "trex_batch_delay_actions: out_actions");
  BUF_TRY(b, done_prev_dev, n, "trex_batch_delay_actions: done_prev");
  TrexActDelayArgs a{};
  a.actions = actions_dev; a.done_prev = done_prev_dev; a.out = out_actions_dev;
  a.ep = s.act_st.ep; a.k = s.act_st.k; a.started = s.act_st.started; a.delay = s.act_st.delay;
  a.hist = s.act_hist.as<float>();
  a.n_envs = b->n; a.cols = s.act_cols; a.delay_min = s.act_min; a.delay_max = s.act_max;
  a.key0 = (uint32_t)s.seed; a.key1 = (uint32_t)(s.seed >> 32); a.env_offset = s.env_offset;
  HIP_TRY(trex_launch_delay_actions(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_sensing_info(const TrexBatch *b, int *num_groups, int *delayed_columns, int *action_delay_min, int *action_delay_max,
                            int32_t *delays_dev, int32_t *action_delay_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Sensing &s = b->sensing;
  const size_t n = (size_t)b->n;
  const InfoCopy copies[] = {
      {delays_dev, s.st.delay, n * s.table.groups * sizeof(int32_t), "delays", "no groups are set"},
      {action_delay_dev, s.act_st.delay, n * sizeof(int32_t), "action_delay", "no action delay is set", "action delays"},
  };
  if (int c = info_copies(b, "trex_batch_sensing_info: ", copies, stream)) return c;
  if (num_groups) *num_groups = s.table.groups;
  if (delayed_columns) *delayed_columns = s.table.delayed;
  if (action_delay_min) *action_delay_min = s.act_min;
  if (action_delay_max) *action_delay_max = s.act_max;
  return TREX_OK;
}

}  // extern "C"
