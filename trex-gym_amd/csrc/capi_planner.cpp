// C-ABI of include/trex_planner.h: the planner's handle, its device memory and tables, and the launches of planner.hip. What a call
// refuses on sizes, strides and values is a check of host_tables.cpp, run before any HIP call; here are the caller's buffers and
// the HIP calls. The handle knows no batch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>

#include "../../include/trex_planner.h"
#include "internal.hpp"
#include "planner.h"

struct TrexPlanner : trex::PlannerShape {
  int device = 0;
  bool noise_set = false;
  uint64_t seed = 0;
  uint32_t env_offset = 0;
  DeviceBuf nominal, knots, it, taps, noise;          // the state of include/trex_planner.h and the interpolation table
  DeviceBuf returns, weights, best, sums;             // what the update's launches hand one another
  std::map<int, DeviceBuf> shift;                     // the shift tables, by plan_shift_key(steps)
  std::map<uint32_t, DeviceBuf> discount;             // the discount tables, by gamma's bits
  std::vector<TrexSeen> seen;

  TrexPlanState state() const {
    return {nominal.as<float>(), knots.as<float>(), it.as<uint32_t>(), taps.as<TrexPlanTap>(), noise.as<TrexPlanNoise>(), G, K, S, P, A, N};
  }
  size_t knot_bytes(size_t sets) const { return sets * (size_t)P * A * sizeof(float); }
};

namespace {

// a table of host values as a device allocation (a set-up path: it synchronises)
template <class T> hipError_t upload(DeviceBuf &buf, const T *host, size_t count) {
  hipError_t e = buf.alloc(count * sizeof(T), false);
  if (e == hipSuccess) e = hipMemcpy(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

}  // namespace

extern "C" {

int trex_planner_create(int groups, int samples, int horizon, int knots, int act_dim, int interpolation, int device, TrexPlanner **out) {
  if (!out) return fail(TREX_E_INVALID, "trex_planner_create: null argument");
  *out = nullptr;
  trex::PlannerShape shape;
  if (int c = built([&] { shape = trex::check_planner_create(groups, samples, horizon, knots, act_dim, interpolation); })) return c;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(TREX_E_HIP, "no HIP device available (the planner has no CPU fallback)");
  if (device < 0 || device >= count) return fail(TREX_E_INVALID, "trex_planner_create: device index out of range");
  TrexDeviceGuard guard(device);
  if (!guard.ok) return fail(TREX_E_HIP, "hipSetDevice failed");
  auto p = std::make_unique<TrexPlanner>();      // (an error path frees by returning)
  static_cast<trex::PlannerShape &>(*p) = shape;
  p->device = device;
  const std::vector<TrexPlanTap> taps = trex::build_plan_taps(shape);
  TrexPlanNoise none;
  for (int a = 0; a < TREX_PLAN_MAXACT; a++) { none.sigma[a] = 0.f; none.lo[a] = -HUGE_VALF; none.hi[a] = HUGE_VALF; }
  const size_t n = (size_t)p->N, g = (size_t)p->G;
  HIP_TRY(p->nominal.alloc(p->knot_bytes(g), true));
  HIP_TRY(p->knots.alloc(p->knot_bytes(n), true));
  HIP_TRY(p->it.alloc(2 * sizeof(uint32_t), true));
  HIP_TRY(upload(p->taps, taps.data(), taps.size()));
  HIP_TRY(upload(p->noise, &none, 1));
  HIP_TRY(p->returns.alloc(n * sizeof(float), true));
  HIP_TRY(p->weights.alloc(n * sizeof(float), true));
  HIP_TRY(p->best.alloc(g * sizeof(int32_t), true));
  HIP_TRY(p->sums.alloc(g * 4 * sizeof(float), true));
  HIP_TRY(hipDeviceSynchronize());
  *out = p.release();
  return TREX_OK;
}

void trex_planner_destroy(TrexPlanner *p) {
  if (!p) return;
  TrexDeviceGuard guard(p->device);
  (void)hipDeviceSynchronize();
  delete p;
}

int trex_planner_info(const TrexPlanner *p, int *groups, int *samples, int *horizon, int *knots, int *act_dim, int *interpolation,
                      uint32_t *it_host, void *stream) {
  if (!p) return fail(TREX_E_INVALID, "trex_planner_info: null planner");
  if (it_host) {
    TrexDeviceGuard guard(p->device);
    HIP_TRY(hipMemcpyAsync(it_host, p->it.p, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  }
  if (groups) *groups = p->G;
  if (samples) *samples = p->K;
  if (horizon) *horizon = p->S;
  if (knots) *knots = p->P;
  if (act_dim) *act_dim = p->A;
  if (interpolation) *interpolation = p->kind;
  return TREX_OK;
}

int trex_planner_set_nominal(TrexPlanner *p, const float *knots_dev, const uint8_t *mask_dev, void *stream) {
  if (!p || !knots_dev) return fail(TREX_E_INVALID, "trex_planner_set_nominal: null argument");
  TrexDeviceGuard guard(p->device);
  BUF_TRY(p, knots_dev, p->knot_bytes((size_t)p->G), "trex_planner_set_nominal: knots");
  BUF_TRY(p, mask_dev, (size_t)p->G, "trex_planner_set_nominal: mask");
  HIP_TRY(trex_launch_plan_set_nominal(p->state(), knots_dev, mask_dev, (hipStream_t)stream));
  return TREX_OK;
}

int trex_planner_get_nominal(const TrexPlanner *cp, float *knots_dev, void *stream) {
  TrexPlanner *p = const_cast<TrexPlanner *>(cp);      // (the cache of validated buffers is not the planner's state)
  if (!p || !knots_dev) return fail(TREX_E_INVALID, "trex_planner_get_nominal: null argument");
  TrexDeviceGuard guard(p->device);
  BUF_TRY(p, knots_dev, p->knot_bytes((size_t)p->G), "trex_planner_get_nominal: knots");
  HIP_TRY(hipMemcpyAsync(knots_dev, p->nominal.p, p->knot_bytes((size_t)p->G), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TREX_OK;
}

int trex_planner_get_samples(const TrexPlanner *cp, float *knots_dev, void *stream) {
  TrexPlanner *p = const_cast<TrexPlanner *>(cp);
  if (!p || !knots_dev) return fail(TREX_E_INVALID, "trex_planner_get_samples: null argument");
  TrexDeviceGuard guard(p->device);
  BUF_TRY(p, knots_dev, p->knot_bytes((size_t)p->N), "trex_planner_get_samples: knots");
  HIP_TRY(hipMemcpyAsync(knots_dev, p->knots.p, p->knot_bytes((size_t)p->N), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TREX_OK;
}

int trex_planner_set_noise(TrexPlanner *p, const float *sigma_host, const float *lo_host, const float *hi_host, uint64_t seed,
                           uint32_t env_offset) {
  if (!p) return fail(TREX_E_INVALID, "trex_planner_set_noise: null planner");
  TrexPlanNoise noise;
  if (int c = built([&] { noise = trex::build_plan_noise(*p, sigma_host, lo_host, hi_host, env_offset); })) return c;
  TrexDeviceGuard guard(p->device);
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the noise this call replaces)
  HIP_TRY(hipMemcpy(p->noise.p, &noise, sizeof noise, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(p->it.p, 0, 2 * sizeof(uint32_t)));
  HIP_TRY(hipDeviceSynchronize());
  p->seed = seed; p->env_offset = env_offset; p->noise_set = true;
  return TREX_OK;
}

int trex_planner_sample(TrexPlanner *p, float *actions_dev, void *stream) {
  if (!p) return fail(TREX_E_INVALID, "trex_planner_sample: null planner");
  if (!p->noise_set) return fail(TREX_E_INVALID, "trex_planner_sample: no noise is set (trex_planner_set_noise)");
  if (!actions_dev) return fail(TREX_E_INVALID, "trex_planner_sample: actions is null");
  TrexDeviceGuard guard(p->device);
  BUF_TRY(p, actions_dev, (size_t)p->S * p->N * p->A * sizeof(float), "trex_planner_sample: actions");
  TrexPlanSampleArgs a{};
  a.st = p->state();
  a.actions = actions_dev;
  a.tile = std::max(1, std::min(TREX_PLAN_TILE_ENVS, TREX_PLAN_TILE_FLOATS / (p->P * p->A)));
  a.key0 = (uint32_t)p->seed; a.key1 = (uint32_t)(p->seed >> 32); a.env_offset = p->env_offset;
  HIP_TRY(trex_launch_plan_sample(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_planner_update(TrexPlanner *p, const float *reward_dev, int64_t step_stride, int64_t env_stride, const float *done_dev,
                        const float *terminal_dev, float gamma, float temperature, float *returns_out, float *weights_out,
                        int32_t *best_out, float *stats_out, void *stream) {
  if (!p) return fail(TREX_E_INVALID, "trex_planner_update: null planner");
  if (int c = built([&] { trex::check_plan_update(*p, p->noise_set, reward_dev != nullptr, step_stride, env_stride, gamma, temperature); }))
    return c;
  TrexDeviceGuard guard(p->device);
  const size_t column = trex::plan_column_bytes(*p, step_stride, env_stride), n = (size_t)p->N * sizeof(float);
  BUF_TRY(p, reward_dev, column, "trex_planner_update: reward");
  BUF_TRY(p, done_dev, column, "trex_planner_update: done");
  BUF_TRY(p, terminal_dev, n, "trex_planner_update: terminal");
  BUF_TRY(p, returns_out, n, "trex_planner_update: returns_out");
  BUF_TRY(p, weights_out, n, "trex_planner_update: weights_out");
  BUF_TRY(p, best_out, (size_t)p->G * sizeof(int32_t), "trex_planner_update: best_out");
  BUF_TRY(p, stats_out, (size_t)p->G * 4 * sizeof(float), "trex_planner_update: stats_out");
  uint32_t bits;
  std::memcpy(&bits, &gamma, sizeof bits);
  auto found = p->discount.find(bits);
  if (found == p->discount.end()) {          // the first call with this gamma: not inside a capture
    if (p->discount.size() >= 64) p->discount.clear();
    const std::vector<float> g = trex::build_plan_discount(p->S, gamma);
    DeviceBuf table;
    HIP_TRY(upload(table, g.data(), g.size()));
    found = p->discount.emplace(bits, std::move(table)).first;
  }
  TrexPlanUpdateArgs a{};
  a.st = p->state();
  a.reward = reward_dev; a.done = done_dev; a.terminal = terminal_dev;
  a.discount = found->second.as<float>();
  a.step_stride = step_stride; a.env_stride = env_stride;
  a.temperature = temperature;
  a.returns = p->returns.as<float>(); a.weights = p->weights.as<float>(); a.best = p->best.as<int32_t>(); a.sums = p->sums.as<float>();
  a.returns_out = returns_out; a.weights_out = weights_out; a.stats_out = stats_out; a.best_out = best_out;
  HIP_TRY(trex_launch_plan_update(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_planner_shift(TrexPlanner *p, int steps, void *stream) {
  if (!p) return fail(TREX_E_INVALID, "trex_planner_shift: null planner");
  int key = 0;
  if (int c = built([&] { key = trex::plan_shift_key(*p, steps); })) return c;
  TrexDeviceGuard guard(p->device);
  auto found = p->shift.find(key);
  if (found == p->shift.end()) {             // the first call with these steps: not inside a capture
    const std::vector<TrexPlanTap> taps = trex::build_plan_shift(*p, steps);
    DeviceBuf table;
    HIP_TRY(upload(table, taps.data(), taps.size()));
    found = p->shift.emplace(key, std::move(table)).first;
  }
  HIP_TRY(trex_launch_plan_shift(p->state(), found->second.as<TrexPlanTap>(), (hipStream_t)stream));
  return TREX_OK;
}

int trex_planner_action(TrexPlanner *p, int step, float *actions_dev, void *stream) {
  if (!p) return fail(TREX_E_INVALID, "trex_planner_action: null planner");
  if (step < 0 || step >= p->S) return fail(TREX_E_INVALID, "trex_planner_action: step " + std::to_string(step) + " outside [0, S)");
  if (!actions_dev) return fail(TREX_E_INVALID, "trex_planner_action: actions is null");
  TrexDeviceGuard guard(p->device);
  BUF_TRY(p, actions_dev, (size_t)p->G * p->A * sizeof(float), "trex_planner_action: actions");
  HIP_TRY(trex_launch_plan_action(p->state(), step, actions_dev, (hipStream_t)stream));
  return TREX_OK;
}

}  // extern "C"
