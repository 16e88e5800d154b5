// C-ABI of include/trex_start_state.h: the start-state randomisation of a batch - its terms and its state - and the launches of
// start_state.hip. The apply launch writes the state the step launches read anyway; no switch of theirs depends on it.
#include <cstring>

#include "batch.hpp"
#include "start_state.h"

extern "C" {

int trex_batch_set_start_state(TrexBatch *b, const TrexStartTerm *terms_host, int num_terms, uint64_t seed, uint32_t env_offset) {
  if (check_batch(b)) return TREX_E_INVALID;
  TrexStartTable t;
  trex::StartStateLayout l;
  if (int c = built([&] {
        trex::check_env_offset("trex_batch_set_start_state: ", env_offset, b->n);
        t = trex::build_start_table(b->nj, terms_host, num_terms);
        l = trex::start_state_layout(b->n, t.num_terms);
      }))
    return c;
  DeviceGuard guard(b->device);
  DeviceBuf blob, state;
  TrexStartState st{};
  if (t.num_terms > 0) {
    HIP_TRY(blob.alloc(sizeof t, false));
    HIP_TRY(hipMemcpy(blob.p, &t, sizeof t, hipMemcpyHostToDevice));
    HIP_TRY(state.alloc(l.bytes, true));
    st = {member_at<uint32_t>(state, l.ep), member_at<uint32_t>(state, l.started), member_at<float>(state, l.shift),
          member_at<int32_t>(state, l.lowest), member_at<float>(state, l.values)};
    HIP_TRY(hipMemset(st.lowest, 0xFF, (size_t)b->n * sizeof(int32_t)));   // -1: no point has decided a placement
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table or the state this call replaces; the new ones are in place on every stream)
  TrexBatch::StartStates &s = b->start;
  s.seed = seed; s.env_offset = env_offset;
  s.blob = std::move(blob);   // (frees the old table and state)
  s.state = std::move(state);
  s.st = st;
  s.table = t;
  return TREX_OK;
}

int trex_batch_apply_start_state(TrexBatch *b, const float *done_dev, int done_stride, float *rows_dev, int row_stride, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::StartStates &s = b->start;
  if (int c = built([&] { trex::check_start_apply(s.table.num_terms, done_dev != nullptr, done_stride, rows_dev != nullptr, row_stride, b->nj, b->pen_in_rows); }))
    return c;
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, done_dev, trex::row_block_bytes(n, done_stride, 1), "trex_batch_apply_start_state: done");
  BUF_TRY(b, rows_dev, trex::row_block_bytes(n, row_stride, 3 * b->nj + (b->pen_in_rows ? 5 : 2)), "trex_batch_apply_start_state: rows");
  TrexStartArgs a{};
  a.table = s.blob.as<TrexStartTable>(); a.model = b->dmodel; a.st = s.st;
  a.done = done_dev; a.done_stride = done_stride; a.rows = rows_dev; a.row_stride = row_stride;
  a.base = b->arr.base; a.q = b->arr.q; a.qd = b->arr.qd; a.hull = b->arr.hull;
  a.warm = b->warm.as<float>();
  a.n_envs = b->n; a.nj = b->nj;
  a.key0 = (uint32_t)s.seed; a.key1 = (uint32_t)(s.seed >> 32); a.env_offset = s.env_offset;
  HIP_TRY(trex_launch_start_state(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_start_state_reset(TrexBatch *b, const uint8_t *mask_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::StartStates &s = b->start;
  if (s.table.num_terms < 1) return fail(TREX_E_INVALID, "trex_batch_start_state_reset: no terms are set (trex_batch_set_start_state)");
  DeviceGuard guard(b->device);
  BUF_TRY(b, mask_dev, (size_t)b->n, "trex_batch_start_state_reset: mask");
  HIP_TRY(trex_launch_start_state_reset(mask_dev, b->n, s.st.started, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_start_state_info(const TrexBatch *b, int *num_terms, float *values_dev, float *shift_dev, int32_t *lowest_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::StartStates &s = b->start;
  const size_t n = (size_t)b->n;
  const InfoCopy copies[] = {
      {values_dev, s.st.values, n * s.table.num_terms * TREX_TL * sizeof(float), "values", "no terms are set"},
      {shift_dev, s.st.shift, n * sizeof(float), "shift", "no terms are set"},
      {lowest_dev, s.st.lowest, n * sizeof(int32_t), "lowest", "no terms are set"},
  };
  if (int c = info_copies(b, "trex_batch_start_state_info: ", copies, stream)) return c;
  if (num_terms) *num_terms = s.table.num_terms;
  return TREX_OK;
}

}  // extern "C"
