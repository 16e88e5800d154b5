// C-ABI of include/trex_symmetry.h but for trex_policy_symmetrize_stats, which lives with the policy's moments in capi_policy.cpp: the
// mirror table's handle and the two row launches of symmetry.hip. What a call refuses on widths, strides and overlap is a check of
// host_tables.cpp, run before any HIP call; here are the caller's buffers and the HIP calls. The handle knows no batch and no policy.
#include <algorithm>
#include <memory>

#include "../../include/trex_symmetry.h"
#include "batch.hpp"
#include "internal.hpp"
#include "symmetry.h"

struct TrexMirrorTable {
  int device = 0, width = 0;
  bool involution = false;
  DeviceBuf words;                 // [width] words of symmetry_limits.h
  std::vector<TrexSeen> seen;
};

const uint32_t *trex_mirror_table_words(const TrexMirrorTable *t, int *width, int *device) {
  *width = t->width; *device = t->device;
  return t->words.as<uint32_t>();
}

namespace {

TrexMirrorBlock block_of(const TrexMirrorTable *t, const float *in, int in_stride, float *out, int out_stride, int n) {
  const int rows = trex_mirror_tile_rows(t->width);
  return {t->words.as<uint32_t>(), in, out, in_stride, out_stride, n, t->width, (n + rows - 1) / rows};
}

}  // namespace

extern "C" {

int trex_model_mirror_table(const TrexModel *model, int lateral, double tol_pos, int32_t *pair_out, int8_t *sign_out,
                            int32_t *body_pair_out, double *residual_out, int *lateral_out) {
  if (!model) return fail(TREX_E_INVALID, "trex_model_mirror_table: null model");
  trex::ModelMirror m;
  if (int c = built([&] { m = trex::build_model_mirror(model->host, lateral, tol_pos); })) return c;
  if (pair_out) std::copy(m.pair.begin(), m.pair.end(), pair_out);
  if (sign_out) std::copy(m.sign.begin(), m.sign.end(), sign_out);
  if (body_pair_out) std::copy(m.body_pair.begin(), m.body_pair.end(), body_pair_out);
  if (residual_out) std::copy(m.residual, m.residual + 5, residual_out);
  if (lateral_out) *lateral_out = m.lateral;
  return TREX_OK;
}

int trex_model_mirror_row_table(const TrexModel *model, int lateral, double tol_pos, const void *channels_host, int num_channels,
                                int action_cols, int tail, const int32_t *extern_src, const int8_t *extern_sign, int32_t *src_out,
                                int8_t *sign_out, int *width_out) {
  if (!model || !src_out || !sign_out) return fail(TREX_E_INVALID, "trex_model_mirror_row_table: null argument");
  trex::RowMirror r;
  if (int c = built([&] {
        const trex::ModelMirror m = trex::build_model_mirror(model->host, lateral, tol_pos);
        r = trex::build_mirror_row_table(model->host, m, tol_pos, (const TrexObsChannel *)channels_host, num_channels, action_cols, tail,
                                         extern_src, extern_sign);
      }))
    return c;
  std::copy(r.src.begin(), r.src.end(), src_out);
  std::copy(r.sign.begin(), r.sign.end(), sign_out);
  if (width_out) *width_out = (int)r.src.size();
  return TREX_OK;
}

int trex_mirror_action_table(const int32_t *pair, const int8_t *sign, int num_joints, int stiffness, int32_t *src_out, int8_t *sign_out) {
  if (!pair || !sign || !src_out || !sign_out || num_joints < 1) return fail(TREX_E_INVALID, "trex_mirror_action_table: null argument or no joint");
  trex::build_mirror_action_table(pair, sign, num_joints, stiffness != 0, src_out, sign_out);
  return TREX_OK;
}

int trex_mirror_command_table(int lateral, int32_t *src_out, int8_t *sign_out) {
  if (!src_out || !sign_out) return fail(TREX_E_INVALID, "trex_mirror_command_table: null argument");
  if (lateral < 0 || lateral > 2) return fail(TREX_E_INVALID, "trex_mirror_command_table: lateral " + std::to_string(lateral) + " outside [0, 2]");
  trex::build_mirror_command_table(lateral, src_out, sign_out);
  return TREX_OK;
}

int trex_mirror_table_create(const int32_t *src_host, const int8_t *sign_host, int width, int device, TrexMirrorTable **out) {
  if (!out) return fail(TREX_E_INVALID, "trex_mirror_table_create: null argument");
  *out = nullptr;
  trex::MirrorWords words;
  if (int c = built([&] { words = trex::build_mirror_words(src_host, sign_host, width); })) return c;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(TREX_E_HIP, "no HIP device available (the mirror maps have no CPU fallback)");
  if (device < 0 || device >= count) return fail(TREX_E_INVALID, "trex_mirror_table_create: device index out of range");
  TrexDeviceGuard guard(device);
  if (!guard.ok) return fail(TREX_E_HIP, "hipSetDevice failed");
  auto t = std::make_unique<TrexMirrorTable>();      // (an error path frees by returning)
  t->device = device; t->width = width; t->involution = words.involution;
  HIP_TRY(t->words.alloc(words.word.size() * sizeof(uint32_t), false));
  HIP_TRY(hipMemcpy(t->words.p, words.word.data(), words.word.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  *out = t.release();
  return TREX_OK;
}

void trex_mirror_table_destroy(TrexMirrorTable *t) {
  if (!t) return;
  TrexDeviceGuard guard(t->device);
  (void)hipDeviceSynchronize();
  delete t;
}

int trex_mirror_table_info(const TrexMirrorTable *t, int *width, int *involution) {
  if (!t) return fail(TREX_E_INVALID, "trex_mirror_table_info: null table");
  if (width) *width = t->width;
  if (involution) *involution = t->involution ? 1 : 0;
  return TREX_OK;
}

int trex_mirror_rows(TrexMirrorTable *t, const float *in_dev, int in_stride, float *out_dev, int out_stride, int n, int width, void *stream) {
  if (!t) return fail(TREX_E_INVALID, "trex_mirror_rows: null table");
  if (int c = built([&] { trex::check_mirror_rows(t->width, in_dev, in_stride, out_dev, out_stride, n, width); })) return c;
  TrexDeviceGuard guard(t->device);
  BUF_TRY(t, in_dev, trex::row_block_bytes((size_t)n, in_stride, width), "trex_mirror_rows: in");
  BUF_TRY(t, out_dev, trex::row_block_bytes((size_t)n, out_stride, width), "trex_mirror_rows: out");
  HIP_TRY(trex_launch_mirror_rows(block_of(t, in_dev, in_stride, out_dev, out_stride, n), (hipStream_t)stream));
  return TREX_OK;
}

int trex_mirror_augment(TrexMirrorTable *obs_table, TrexMirrorTable *act_table, TrexMirrorTable *critic_table, float *obs_dev,
                        float *act_dev, float *logp_dev, float *val_dev, float *adv_dev, float *ret_dev, float *obs_v_dev,
                        int64_t num_samples, int D, int A, int Dv, void *stream) {
  if (!obs_table || !act_table) return fail(TREX_E_INVALID, "trex_mirror_augment: null table");
  const bool buffers = obs_dev && act_dev && logp_dev && val_dev && adv_dev && ret_dev;
  if (int c = built([&] {
        trex::check_mirror_augment(obs_table->width, act_table->width, critic_table ? critic_table->width : 0, critic_table != nullptr,
                                   buffers, obs_v_dev != nullptr, num_samples, D, A, Dv);
      }))
    return c;
  if (act_table->device != obs_table->device || (critic_table && critic_table->device != obs_table->device))
    return fail(TREX_E_INVALID, "trex_mirror_augment: the tables live on different devices");
  TrexMirrorTable *t = obs_table;     // (its cache of validated buffers serves the call)
  TrexDeviceGuard guard(t->device);
  const size_t rows = 2 * (size_t)num_samples * sizeof(float);
  BUF_TRY(t, obs_dev, rows * D, "trex_mirror_augment: obs");
  BUF_TRY(t, act_dev, rows * A, "trex_mirror_augment: act");
  BUF_TRY(t, logp_dev, rows, "trex_mirror_augment: logp");
  BUF_TRY(t, val_dev, rows, "trex_mirror_augment: val");
  BUF_TRY(t, adv_dev, rows, "trex_mirror_augment: adv");
  BUF_TRY(t, ret_dev, rows, "trex_mirror_augment: ret");
  BUF_TRY(t, obs_v_dev, rows * Dv, "trex_mirror_augment: obs_v");
  const int n = (int)num_samples;
  TrexMirrorAugmentArgs a{};
  a.block[0] = block_of(obs_table, obs_dev, D, obs_dev + (size_t)n * D, D, n);
  a.block[1] = block_of(act_table, act_dev, A, act_dev + (size_t)n * A, A, n);
  if (critic_table) a.block[2] = block_of(critic_table, obs_v_dev, Dv, obs_v_dev + (size_t)n * Dv, Dv, n);
  a.column[0] = logp_dev; a.column[1] = val_dev; a.column[2] = adv_dev; a.column[3] = ret_dev;
  a.n = num_samples;
  a.copy_groups = (n + TREX_MIRROR_COPY_ELEMS - 1) / TREX_MIRROR_COPY_ELEMS;
  HIP_TRY(trex_launch_mirror_augment(a, (hipStream_t)stream));
  return TREX_OK;
}

}  // extern "C"
