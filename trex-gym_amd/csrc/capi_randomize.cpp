// C-ABI of include/trex_randomize.h: the episode randomisation of a batch - its terms, its state and snapshots - and the launches
// of randomize.hip. The apply launch writes the buffers the step launches read anyway (mass scale, friction, gains, wrench); the
// switches those launches depend on are flipped here, in the set and the clear, never by a launch.
#include <cstring>

#include "batch.hpp"
#include "randomize.h"
#include "step_launch.h"

namespace {

// takes back what the terms in force did: gains, wrench, mass scale and friction as they were at the set, the switches as they
// stood then, the state freed. The caller has synchronised the device.
int clear_randomization(TrexBatch *b) {
  TrexBatch::Randomization &r = b->random;
  if (r.table.terms < 1) return TREX_OK;
  const size_t n = (size_t)b->n;
  if (r.nominal) HIP_TRY(hipMemcpy(b->gains.p, r.nominal.p, r.nominal.bytes, hipMemcpyDeviceToDevice));
  if (r.mass0) HIP_TRY(hipMemcpy(b->arr.mass_scale, r.mass0.p, r.mass0.bytes, hipMemcpyDeviceToDevice));
  if (r.friction0) HIP_TRY(hipMemcpy(b->arr.friction, r.friction0.p, n * sizeof(float), hipMemcpyDeviceToDevice));
  if (r.table.pushes > 0)
    HIP_TRY(trex_launch_randomize_rebase(r.blob.as<TrexRandTable>(), r.st, nullptr, b->ext.as<float>(), b->n, b->nb, r.table.pushes, 1, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  if (r.table.mass || r.table.friction) b->arr.domain = r.was_domain ? 1 : 0;
  if (r.table.gains) b->gains_set = r.was_gains_set;
  if (r.table.pushes > 0) b->ext_on = r.was_ext_on;
  r.table = trex::RandTable();
  r.blob.release(); r.state.release(); r.nominal.release(); r.mass0.release(); r.friction0.release();
  r.st = TrexRandState{};
  return TREX_OK;
}

}  // namespace

extern "C" {

int trex_batch_set_randomization(TrexBatch *b, const TrexRandomTerm *terms_host, int num_terms, uint64_t seed, uint32_t env_offset) {
  if (check_batch(b)) return TREX_E_INVALID;
  trex::RandTable t;
  trex::RandStateLayout l;
  if (int c = built([&] {
        trex::check_env_offset("trex_batch_set_randomization: ", env_offset, b->n);
        t = trex::build_random_table(b->nb, b->nj, b->stiff, terms_host, num_terms);
        l = trex::rand_state_layout(b->n, t.terms, t.pushes);
      }))
    return c;
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table or the state this call replaces)
  if (int c = clear_randomization(b)) return c;
  TrexBatch::Randomization &r = b->random;
  r.seed = seed; r.env_offset = env_offset;
  if (t.terms == 0) return TREX_OK;
  const size_t n = (size_t)b->n;
  DeviceBuf blob, state, nominal, mass0, friction0;
  TrexRandTable tab;
  std::memset(&tab, 0, sizeof tab);
  for (int i = 0; i < t.terms; i++) {
    tab.term[i] = t.term[i];
    if (t.push_slot[i] >= 0) tab.push_body[t.push_slot[i]] = t.term[i].index;
  }
  std::memcpy(tab.push_slot, t.push_slot, sizeof tab.push_slot);
  HIP_TRY(blob.alloc(sizeof tab, false));
  HIP_TRY(hipMemcpy(blob.p, &tab, sizeof tab, hipMemcpyHostToDevice));
  HIP_TRY(state.alloc(l.bytes, true));
  const TrexRandState st = {member_at<uint32_t>(state, l.ep),       member_at<uint32_t>(state, l.k),
                            member_at<uint32_t>(state, l.started),  member_at<int32_t>(state, l.off),
                            member_at<int32_t>(state, l.push_left), member_at<float>(state, l.push_force),
                            member_at<float>(state, l.push_base),   member_at<float>(state, l.values)};
  if (t.gains) {
    if (int c = ensure_gains(b)) return c;
    HIP_TRY(nominal.alloc(b->gains.bytes, false));
    HIP_TRY(hipMemcpy(nominal.p, b->gains.p, b->gains.bytes, hipMemcpyDeviceToDevice));
  }
  if (t.mass) {
    HIP_TRY(mass0.alloc(n * TREX_TL * sizeof(float), false));
    HIP_TRY(hipMemcpy(mass0.p, b->arr.mass_scale, mass0.bytes, hipMemcpyDeviceToDevice));
  }
  if (t.friction) {
    HIP_TRY(friction0.alloc(n * sizeof(float), false));
    HIP_TRY(hipMemcpy(friction0.p, b->arr.friction, friction0.bytes, hipMemcpyDeviceToDevice));
  }
  if (t.pushes > 0) {
    if (!b->ext) HIP_TRY(b->ext.alloc(n * 6 * TREX_TL * sizeof(float), false));
    if (!b->ext_on) HIP_TRY(hipMemset(b->ext.p, 0, b->ext.bytes));   // (the caller has set nothing: the base is zeros)
    HIP_TRY(trex_launch_randomize_rebase(blob.as<TrexRandTable>(), st, nullptr, b->ext.as<float>(), b->n, b->nb, t.pushes, 2, nullptr));
  }
  HIP_TRY(hipDeviceSynchronize());   // (table, state and snapshots are in place on every stream)
  r.was_domain = b->arr.domain != 0; r.was_gains_set = b->gains_set; r.was_ext_on = b->ext_on;
  if (t.mass || t.friction) b->arr.domain = 1;
  if (t.gains) b->gains_set = true;
  if (t.pushes > 0) b->ext_on = true;
  r.blob = std::move(blob); r.state = std::move(state); r.nominal = std::move(nominal);
  r.mass0 = std::move(mass0); r.friction0 = std::move(friction0);
  r.st = st;
  r.table = std::move(t);
  return TREX_OK;
}

int trex_batch_apply_randomization(TrexBatch *b, const float *done_dev, int done_stride, float *command_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_apply_randomization: ";
  const TrexBatch::Randomization &r = b->random;
  if (r.table.terms < 1) return fail(TREX_E_INVALID, me + "no terms are set (trex_batch_set_randomization)");
  if (!done_dev) return fail(TREX_E_INVALID, me + "done is null");
  if (done_stride < 1) return fail(TREX_E_INVALID, me + "done_stride below 1");
  if (r.table.command && !command_dev) return fail(TREX_E_INVALID, me + "a COMMAND term is set and command is null");
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, done_dev, trex::row_block_bytes(n, done_stride, 1), "trex_batch_apply_randomization: done");
  BUF_TRY(b, command_dev, n * 3 * sizeof(float), "trex_batch_apply_randomization: command");
  TrexRandArgs a{};
  a.table = r.blob.as<TrexRandTable>(); a.model = b->dmodel; a.st = r.st;
  a.done = done_dev; a.done_stride = done_stride; a.command = command_dev;
  a.mass_scale = b->arr.mass_scale; a.friction = b->arr.friction;
  a.gains = b->gains.as<float>(); a.nominal = r.nominal.as<float>(); a.wrench = b->ext.as<float>();
  a.n_envs = b->n; a.num_terms = r.table.terms; a.num_pushes = r.table.pushes;
  a.key0 = (uint32_t)r.seed; a.key1 = (uint32_t)(r.seed >> 32); a.env_offset = r.env_offset;
  HIP_TRY(trex_launch_randomize(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_randomization_reset(TrexBatch *b, const uint8_t *mask_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Randomization &r = b->random;
  if (r.table.terms < 1) return fail(TREX_E_INVALID, "trex_batch_randomization_reset: no terms are set (trex_batch_set_randomization)");
  DeviceGuard guard(b->device);
  BUF_TRY(b, mask_dev, (size_t)b->n, "trex_batch_randomization_reset: mask");
  HIP_TRY(trex_launch_randomize_reset(mask_dev, b->n, r.st.started, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_randomization_info(const TrexBatch *b, int *num_terms, float *values_dev, float *push_force_dev, int32_t *push_left_dev,
                                  void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Randomization &r = b->random;
  const size_t n = (size_t)b->n, P = (size_t)r.table.pushes;
  const bool pushes = P > 0;   // (without PUSH terms the push members are empty, not absent)
  const InfoCopy copies[] = {
      {values_dev, r.st.values, n * r.table.terms * TREX_TL * sizeof(float), "values", "no terms are set"},
      {push_force_dev, pushes ? r.st.push_force : nullptr, n * P * 3 * sizeof(float), "push_force", "no PUSH terms are set", "push state"},
      {push_left_dev, pushes ? r.st.push_left : nullptr, n * P * sizeof(int32_t), "push_left", "no PUSH terms are set", "push state"},
  };
  if (int c = info_copies(b, "trex_batch_randomization_info: ", copies, stream)) return c;
  if (num_terms) *num_terms = r.table.terms;
  return TREX_OK;
}

}  // extern "C"
