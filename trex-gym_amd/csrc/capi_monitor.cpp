// C-ABI of include/trex_monitor.h: the episode monitor of a batch - its state and the launches of monitor.hip. The shape, the layout
// of the state and the strides are checked by host_tables.cpp; here are the batch, the buffers and the HIP calls. The monitor
// writes its own state and nothing else: no switch of the step launches depends on it.
#include "batch.hpp"
#include "monitor.h"

namespace {

TrexMonState point_into(void *base, const trex::MonitorLayout &m) {
  char *p = (char *)base;
  TrexMonState s{};
  s.ret = (double *)(p + m.ret); s.col = (double *)(p + m.col);
  s.total = (unsigned long long *)(p + m.total); s.by_reason = (unsigned long long *)(p + m.by_reason);
  s.len = (int32_t *)(p + m.len); s.episodes = (uint32_t *)(p + m.episodes); s.fin = (uint32_t *)(p + m.fin);
  s.last_return = (float *)(p + m.last_return); s.last_length = (int32_t *)(p + m.last_length);
  s.last_reason = (int32_t *)(p + m.last_reason); s.last_t = (uint32_t *)(p + m.last_t); s.last_cols = (float *)(p + m.last_cols);
  s.t = (uint32_t *)(p + m.t);
  s.ring_return = (float *)(p + m.ring_return); s.ring_length = (int32_t *)(p + m.ring_length);
  s.ring_reason = (int32_t *)(p + m.ring_reason); s.ring_env = (uint32_t *)(p + m.ring_env); s.ring_t = (uint32_t *)(p + m.ring_t);
  s.ring_cols = (float *)(p + m.ring_cols);
  s.counts = (uint32_t *)(p + m.counts);
  return s;
}

}  // namespace

extern "C" {

int trex_batch_set_monitor(TrexBatch *b, int window, int cols_a, int cols_b, uint32_t env_offset) {
  if (check_batch(b)) return TREX_E_INVALID;
  trex::MonitorLayout m;
  if (int c = built([&] { m = trex::monitor_layout(b->n, window, cols_a, cols_b, env_offset, TREX_MON_BLOCK); })) return c;
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the state this call replaces)
  DeviceBuf state;
  if (m.window > 0) {
    HIP_TRY(state.alloc(m.bytes, true));
    HIP_TRY(hipDeviceSynchronize());   // (the zeros are in place on every stream)
  }
  TrexBatch::Monitor &mon = b->monitor;
  mon.state = std::move(state);
  mon.layout = m;
  mon.st = mon.state ? point_into(mon.state.p, m) : TrexMonState{};
  mon.env_offset = m.window > 0 ? env_offset : 0u;
  return TREX_OK;
}

int trex_batch_monitor_apply(TrexBatch *b, const float *reward_dev, int reward_stride, const float *done_dev, int done_stride,
                             const int32_t *reason_dev, const float *cols_a_dev, int stride_a, const float *cols_b_dev, int stride_b,
                             void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Monitor &mon = b->monitor;
  const trex::MonitorLayout &m = mon.layout;
  if (int c = built([&] {
        trex::check_monitor_apply(m, reward_dev != nullptr, reward_stride, done_dev != nullptr, done_stride, cols_a_dev != nullptr, stride_a,
                                  cols_b_dev != nullptr, stride_b);
      }))
    return c;
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, reward_dev, trex::row_block_bytes(n, reward_stride, 1), "trex_batch_monitor_apply: reward");
  BUF_TRY(b, done_dev, trex::row_block_bytes(n, done_stride, 1), "trex_batch_monitor_apply: done");
  BUF_TRY(b, reason_dev, n * sizeof(int32_t), "trex_batch_monitor_apply: reason");
  if (m.cols_a > 0) BUF_TRY(b, cols_a_dev, trex::row_block_bytes(n, stride_a, m.cols_a), "trex_batch_monitor_apply: cols_a");
  if (m.cols_b > 0) BUF_TRY(b, cols_b_dev, trex::row_block_bytes(n, stride_b, m.cols_b), "trex_batch_monitor_apply: cols_b");
  TrexMonArgs a{};
  a.st = mon.st;
  a.reward = reward_dev; a.done = done_dev;
  a.reason = reason_dev ? reason_dev : (b->term.on ? b->term.reason : nullptr);   // (the batch's own buffer, read in place)
  a.cols_a = m.cols_a > 0 ? cols_a_dev : nullptr; a.cols_b = m.cols_b > 0 ? cols_b_dev : nullptr;
  a.reward_stride = reward_stride; a.done_stride = done_stride;
  a.stride_a = m.cols_a > 0 ? stride_a : 0; a.stride_b = m.cols_b > 0 ? stride_b : 0;
  a.n_envs = b->n; a.window = m.window; a.cols_a_n = m.cols_a; a.cols_n = m.cols; a.team = m.team; a.groups = m.groups;
  a.env_offset = mon.env_offset;
  HIP_TRY(trex_launch_monitor(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_monitor_reset(TrexBatch *b, const uint8_t *mask_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Monitor &mon = b->monitor;
  if (mon.layout.window < 1) return fail(TREX_E_INVALID, "trex_batch_monitor_reset: no monitor is set (trex_batch_set_monitor)");
  DeviceGuard guard(b->device);
  BUF_TRY(b, mask_dev, (size_t)b->n, "trex_batch_monitor_reset: mask");
  HIP_TRY(trex_launch_monitor_reset(mon.st, mask_dev, b->n, mon.layout.cols, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_monitor_summary(TrexBatch *b, double *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Monitor &mon = b->monitor;
  if (mon.layout.window < 1) return fail(TREX_E_INVALID, "trex_batch_monitor_summary: no monitor is set (trex_batch_set_monitor)");
  if (!out_dev) return fail(TREX_E_INVALID, "trex_batch_monitor_summary: out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, out_dev, (size_t)(TREX_MON_SUMMARY + mon.layout.cols) * sizeof(double), "trex_batch_monitor_summary: out");
  HIP_TRY(trex_launch_monitor_summary(mon.st, mon.layout.window, mon.layout.cols, out_dev, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_monitor_info(const TrexBatch *b, int *window, int *cols, float *ring_return_dev, int32_t *ring_length_dev,
                            int32_t *ring_reason_dev, uint32_t *ring_env_dev, uint32_t *ring_t_dev, float *ring_cols_dev, double *ret_dev,
                            int32_t *len_dev, uint32_t *episodes_dev, float *last_return_dev, int32_t *last_length_dev,
                            int32_t *last_reason_dev, uint32_t *last_t_dev, float *last_cols_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Monitor &mon = b->monitor;
  const trex::MonitorLayout &m = mon.layout;
  const TrexMonState &s = mon.st;
  const size_t n = (size_t)b->n, W = (size_t)m.window, C = (size_t)m.cols;
  const char *none = "no monitor is set";   // (st holds nulls then)
  const InfoCopy copies[] = {
      {ring_return_dev, s.ring_return, W * 4, "ring_return", none},
      {ring_length_dev, s.ring_length, W * 4, "ring_length", none},
      {ring_reason_dev, s.ring_reason, W * 4, "ring_reason", none},
      {ring_env_dev, s.ring_env, W * 4, "ring_env", none},
      {ring_t_dev, s.ring_t, W * 4, "ring_t", none},
      {ring_cols_dev, s.ring_cols, W * C * 4, "ring_cols", none},
      {ret_dev, s.ret, n * 8, "ret", none},
      {len_dev, s.len, n * 4, "len", none},
      {episodes_dev, s.episodes, n * 4, "episodes", none},
      {last_return_dev, s.last_return, n * 4, "last_return", none},
      {last_length_dev, s.last_length, n * 4, "last_length", none},
      {last_reason_dev, s.last_reason, n * 4, "last_reason", none},
      {last_t_dev, s.last_t, n * 4, "last_t", none},
      {last_cols_dev, s.last_cols, n * C * 4, "last_cols", none},
  };
  if (int c = info_copies(b, "trex_batch_monitor_info: ", copies, stream)) return c;
  if (window) *window = m.window;
  if (cols) *cols = m.cols;
  return TREX_OK;
}

}  // extern "C"
