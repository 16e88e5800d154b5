// C-ABI of include/trex_policy.h, trex_policy_critic.h and trex_policy_distill.h: the trainer's handle, its device memory and the
// launches of policy_step.hip and ppo_learner.hip (policy_launch.h). What a call refuses on sizes, strides and null pointers is a
// check of host_tables.cpp, run before any HIP call; here are the caller's buffers and the HIP calls.
#include <cstring>
#include <memory>

#include "../../include/trex_policy.h"
#include "../../include/trex_symmetry.h"
#include "internal.hpp"
#include "policy_launch.h"
#include "symmetry.h"

using namespace trex_policy;

// VecNormalize's running moments of a row block `width` columns wide, as observe_kernel keeps them (policy_launch.h, ObserveArgs):
// the f64 statistics [2 width + 5], the per-workgroup partial sums [G][width + 2][2] and the f32 image [2 width + 2].
struct Moments {
  int width = 0;
  DeviceBuf stats, partial, norm;
};

struct TrexPolicy : trex::PolicyShape {      // n, D, A, Dv (0: no critic) and the parameter layout: what the checks read
  int device = 0, G = 0;                     // G: workgroups of the statistics' first launch
  float epsilon = 1e-8f;                     // VecNormalize's
  Moments obs;                               // of the [n, D | reward | done] rows
  // privileged critic (include/trex_policy_critic.h): the moments of its rows, without a reward - the four slots behind the count
  // are never touched. Allocated once, for the widest critic, by the first set; `width` is the one in force
  Moments critic;
  DeviceBuf ret;                             // discounted returns [n]
  DeviceBuf adam_step;                       // int
  // learner workspace, allocated on first use: per-tile gradient partials [grad_tiles][learn_stride], whose row is as long as the
  // parameter vector - trex_policy_set_critic drops it -, and the partial squared norms
  DeviceBuf grad_partial, learn_red;
  int grad_tiles = 0;
  std::vector<TrexSeen> seen;
};

namespace {

// the caller's buffers of one call, each as memory of the policy's device (null: not given), in the order they are refused in
struct Buf { const void *ptr; size_t bytes; const char *what; };
template <size_t N> int check_buffers(TrexPolicy *p, const Buf (&bufs)[N]) {
  for (const Buf &b : bufs) BUF_TRY(p, b.ptr, b.bytes, b.what);
  return TREX_OK;
}

hipError_t alloc_moments(Moments &m, int width, int G) {
  hipError_t e = m.stats.alloc((2 * width + 5) * sizeof(double), true);
  if (e == hipSuccess) e = m.partial.alloc((size_t)G * (width + 2) * 2 * sizeof(double), true);
  if (e == hipSuccess) e = m.norm.alloc((2 * width + 2) * sizeof(float), true);
  return e;
}

// RunningMeanStd(epsilon = 1e-4) of a block `width` wide - mean 0, var 1, count 1e-4, of the rows and of the returns - and its image
int init_moments(const TrexPolicy *p, Moments &m, int width, hipStream_t s) {
  m.width = width;
  std::vector<double> st(2 * width + 5, 0.0);
  for (int k = 0; k < width; k++) st[width + k] = 1.0;
  st[2 * width] = 1e-4; st[2 * width + 2] = 1.0; st[2 * width + 3] = 1e-4;
  HIP_TRY(hipMemcpyAsync(m.stats.p, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(trex_launch_policy_refresh_norm(m.stats.as<double>(), m.norm.as<float>(), width, p->epsilon, s));
  return TREX_OK;
}

// the first `count` statistics: 2 D + 5 of the observation block, 2 Dv + 1 of the critic's (the C-ABI's arrays)
int get_moments(const TrexPolicy *p, const Moments &m, int count, double *host, hipStream_t s) {
  TrexDeviceGuard guard(p->device);
  HIP_TRY(hipMemcpyAsync(host, m.stats.p, count * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return TREX_OK;
}

int set_moments(const TrexPolicy *p, Moments &m, int count, const double *host, hipStream_t s) {
  TrexDeviceGuard guard(p->device);
  HIP_TRY(hipMemcpyAsync(m.stats.p, host, count * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(trex_launch_policy_refresh_norm(m.stats.as<double>(), m.norm.as<float>(), m.width, p->epsilon, s));
  return TREX_OK;
}

// the statistics' two launches on the block `a` names (rows, stride, reward and its outputs), into the moments `m`
int observe(const TrexPolicy *p, Moments &m, ObserveArgs a, hipStream_t s) {
  a.stats = m.stats.as<double>(); a.partial = m.partial.as<double>(); a.norm = m.norm.as<float>();
  a.n = p->n; a.D = m.width; a.epsilon = p->epsilon;
  HIP_TRY(trex_launch_policy_observe(a, s));
  return TREX_OK;
}

// One minibatch call: what the six entry points fill by name. A gradient call (adam false) leaves m, v null and Adam's constants
// at rest - they travel in the reduce launch's block unread. Distillation: `act` is the teacher's mean, `ret` its value (may be
// null), and logp, val, adv, adv_stats stay null.
struct Minibatch {
  const char *who = nullptr;
  bool distill = false, critic = false, adam = false;
  float *theta = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr;
  const float *obs = nullptr, *obs_v = nullptr, *act = nullptr, *logp = nullptr, *val = nullptr, *adv = nullptr, *ret = nullptr;
  const float *adv_stats = nullptr, *teacher_logstd = nullptr;
  int64_t num_samples = 0;
  const int64_t *perm = nullptr;
  int first = 0, mb = 0, kind = 0;
  float cliprange = 0.f, ent_coef = 0.f, vf_coef = 0.f;
  float lr = 0.f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-5f, max_grad_norm = 0.f, grad_scale = 1.f;
  float *loss_sums = nullptr;
  void *stream = nullptr;
};

// workspace of `tiles` partial rows, grown on demand (never inside a graph capture: the first call is eager)
int learn_workspace(TrexPolicy *p, int tiles, int stride) {
  if (tiles <= p->grad_tiles) return TREX_OK;
  p->grad_tiles = 0;
  HIP_TRY(p->grad_partial.alloc((size_t)tiles * stride * sizeof(float), true));     // (pad elements are never written: they stay 0)
  p->grad_tiles = tiles;
  if (!p->learn_red) HIP_TRY(p->learn_red.alloc(LEARN_RED_DOUBLES * sizeof(double), false));
  return TREX_OK;
}

// learn_grad_kernel + learn_reduce_kernel -> grad (UNclipped, times grad_scale), then learn_adam_kernel when the call asks for it
int run_minibatch(TrexPolicy *p, const Minibatch &c) {
  const bool buffers = c.theta && c.grad && c.obs && c.act && c.perm && (!c.adam || (c.m && c.v)) && (!c.critic || c.obs_v) &&
                       (c.distill || (c.logp && c.val && c.adv && c.ret && c.adv_stats));
  const trex::PolicyMinibatchCall call{c.who, c.distill, c.critic, buffers, c.mb, c.first, c.num_samples, c.kind,
                                       c.teacher_logstd != nullptr, c.ret != nullptr, c.vf_coef};
  if (int rc = built([&] { trex::check_policy_minibatch(p, call); })) return rc;
  TrexDeviceGuard guard(p->device);
  const size_t P = (size_t)p->lay.count * sizeof(float), N = (size_t)c.num_samples * sizeof(float);
#define NAMED(ppo_name, distill_name) (c.distill ? "distillation step: " distill_name : "minibatch step: " ppo_name)
  const Buf bufs[] = {
      {c.theta, P, NAMED("theta", "theta")}, {c.grad, P, NAMED("grad", "grad")}, {c.m, P, NAMED("m", "m")}, {c.v, P, NAMED("v", "v")},
      {c.obs, N * p->D, NAMED("obs", "obs")}, {c.obs_v, N * p->Dv, NAMED("obs_v", "obs_v")}, {c.act, N * p->A, NAMED("act", "teacher_mean")},
      {c.logp, N, NAMED("logp", "logp")}, {c.val, N, NAMED("val", "val")}, {c.adv, N, NAMED("adv", "adv")}, {c.ret, N, NAMED("ret", "teacher_value")},
      {c.teacher_logstd, (size_t)p->A * sizeof(float), NAMED("teacher_logstd", "teacher_logstd")},
      {c.perm, ((size_t)c.first + c.mb) * sizeof(int64_t), NAMED("perm", "perm")},
      {c.adv_stats, 2 * sizeof(float), NAMED("adv_stats", "adv_stats")}, {c.loss_sums, 2 * sizeof(float), NAMED("loss_sums", "loss_sums")}};
#undef NAMED
  if (int rc = check_buffers(p, bufs)) return rc;
  const int tiles = (c.mb + TILE - 1) / TILE;
  const int stride = (int)((((size_t)p->lay.count + 3) & ~(size_t)3) + 4);      // a partial row: the parameters, padded to float4, + one float4 of loss sums
  if (int rc = learn_workspace(p, tiles, stride)) return rc;
  const hipStream_t s = (hipStream_t)c.stream;
  const LearnArgs a{c.theta, c.obs, c.act, c.logp, c.val, c.adv, c.ret, reinterpret_cast<const long long *>(c.perm), c.adv_stats,
                    p->grad_partial.as<float>(), c.first, c.mb, stride, c.cliprange, c.vf_coef, p->lay};
  if (c.distill) {
    // The kernel's staging loads are unconditional (no control flow before its first barrier), so an absent buffer gets a stand-in
    // address that is readable and long enough - the teacher's means for its values [N <= N A], the student's own logstd for the
    // teacher's [A] - and a flag / the kind keeps what is read there out of every result.
    LearnArgsD d{};
    static_cast<LearnArgs &>(d) = a;
    d.ret = c.ret ? c.ret : c.act;
    d.teacher_logstd = c.teacher_logstd ? c.teacher_logstd : c.theta + p->lay.logstd;
    d.kind = c.kind;
    d.has_value = c.ret != nullptr;
    HIP_TRY(trex_launch_policy_learn_grad_distill(d, s));
  } else if (c.critic) {
    LearnArgsV av{};
    static_cast<LearnArgs &>(av) = a;
    av.obs_v = c.obs_v; av.Dv = p->Dv;
    HIP_TRY(trex_launch_policy_learn_grad_critic(av, s));
  } else {
    HIP_TRY(trex_launch_policy_learn_grad(a, s));
  }
  const ApplyArgs b{p->grad_partial.as<float>(), c.theta, c.grad, c.m, c.v, c.loss_sums, p->learn_red.as<double>(), nullptr,
                    p->adam_step.as<int>(), tiles, stride, p->lay.count, p->lay.logstd, p->A, c.ent_coef, c.lr, c.beta1, c.beta2, c.eps,
                    c.max_grad_norm, 1.0f / (float)c.mb, c.grad_scale, c.adam ? 1 : 0};
  HIP_TRY(trex_launch_policy_learn_reduce(b, s));
  if (c.adam) HIP_TRY(trex_launch_policy_learn_adam(b, s));
  return TREX_OK;
}

}  // namespace

extern "C" {

int trex_policy_create(int num_envs, int obs_dim, int act_dim, int hidden, int device, TrexPolicy **out) {
  if (!out) return fail(TREX_E_INVALID, "trex_policy_create: null argument");
  *out = nullptr;
  if (int c = built([&] { trex::check_policy_create(num_envs, obs_dim, act_dim, hidden); })) return c;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(TREX_E_HIP, "no HIP device available (the policy step has no CPU fallback)");
  if (device < 0 || device >= count) return fail(TREX_E_INVALID, "device index out of range");
  TrexDeviceGuard guard(device);
  if (!guard.ok) return fail(TREX_E_HIP, "hipSetDevice failed");
  auto p = std::make_unique<TrexPolicy>();      // (an error path frees by returning)
  p->n = num_envs; p->D = obs_dim; p->A = act_dim; p->device = device;
  p->G = (num_envs + OBS_ROWS - 1) / OBS_ROWS;
  p->lay = make_layout(obs_dim, act_dim);
  hipError_t r = alloc_moments(p->obs, obs_dim, p->G);
  if (r == hipSuccess) r = p->ret.alloc((size_t)num_envs * sizeof(float), true);
  if (r == hipSuccess) r = p->adam_step.alloc(sizeof(int), true);
  if (r != hipSuccess) return fail(TREX_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(r));
  if (int c = init_moments(p.get(), p->obs, obs_dim, nullptr)) return c;
  HIP_TRY(hipDeviceSynchronize());
  *out = p.release();
  return TREX_OK;
}

void trex_policy_destroy(TrexPolicy *p) {
  if (!p) return;
  TrexDeviceGuard guard(p->device);
  (void)hipDeviceSynchronize();
  delete p;
}

int trex_policy_param_count(const TrexPolicy *p) { return p ? p->lay.count : fail(TREX_E_INVALID, "null policy"); }

int trex_policy_param_offsets(const TrexPolicy *p, int o[13]) {
  if (!p || !o) return fail(TREX_E_INVALID, "null argument");
  const PolicyLayout &l = p->lay;
  const int v[13] = {l.pW1, l.pb1, l.pW2, l.pb2, l.pW3, l.pb3, l.vW1, l.vb1, l.vW2, l.vb2, l.vW3, l.vb3, l.logstd};
  std::memcpy(o, v, sizeof v);
  return TREX_OK;
}

int trex_policy_get_stats(TrexPolicy *p, double *host, void *stream) {
  if (!p || !host) return fail(TREX_E_INVALID, "null argument");
  return get_moments(p, p->obs, 2 * p->D + 5, host, (hipStream_t)stream);
}

int trex_policy_set_stats(TrexPolicy *p, const double *host, void *stream) {
  if (!p || !host) return fail(TREX_E_INVALID, "null argument");
  return set_moments(p, p->obs, 2 * p->D + 5, host, (hipStream_t)stream);
}

int trex_policy_get_returns(TrexPolicy *p, float *ret_dev, void *stream) {
  if (!p || !ret_dev) return fail(TREX_E_INVALID, "null argument");
  TrexDeviceGuard guard(p->device);
  BUF_TRY(p, ret_dev, (size_t)p->n * sizeof(float), "trex_policy_get_returns: ret");
  HIP_TRY(hipMemcpyAsync(ret_dev, p->ret.p, (size_t)p->n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TREX_OK;
}

int trex_policy_observe(TrexPolicy *p, const float *rows_dev, int row_stride, int with_reward, float gamma, float *raw_rew_out,
                        float *done_out, float *rew_scale_out, void *stream) {
  if (int c = built([&] { trex::check_policy_observe(p, rows_dev != nullptr, row_stride, with_reward != 0); })) return c;
  TrexDeviceGuard guard(p->device);
  const size_t n = (size_t)p->n;
  const Buf bufs[] = {{rows_dev, trex::row_block_bytes(n, row_stride, p->D + (with_reward ? 2 : 0)), "trex_policy_observe: rows"},
                      {raw_rew_out, n * sizeof(float), "trex_policy_observe: raw_rew_out"}, {done_out, n * sizeof(float), "trex_policy_observe: done_out"},
                      {rew_scale_out, sizeof(float), "trex_policy_observe: rew_scale_out"}};
  if (int c = check_buffers(p, bufs)) return c;
  ObserveArgs a{};
  a.rows = rows_dev; a.row_stride = row_stride; a.with_reward = with_reward ? 1 : 0; a.gamma = gamma;
  a.ret = p->ret.as<float>(); a.raw_rew_out = raw_rew_out; a.done_out = done_out; a.rew_scale_out = rew_scale_out;
  return observe(p, p->obs, a, (hipStream_t)stream);
}

int trex_policy_act(TrexPolicy *p, const float *theta_dev, const float *rows_dev, int row_stride, float clip_obs,
                    const float *noise_dev, float *actions_dev, float *obs_out, float *act_out, float *logp_out, float *value_out,
                    int value_only, void *stream) {
  const trex::PolicyActCall call{theta_dev != nullptr, rows_dev != nullptr, false, noise_dev != nullptr, actions_dev != nullptr,
                                 value_out != nullptr, false, row_stride, 0, value_only != 0};
  if (int c = built([&] { trex::check_policy_act(p, call); })) return c;
  TrexDeviceGuard guard(p->device);
  const size_t n = (size_t)p->n * sizeof(float);
  const Buf bufs[] = {{theta_dev, (size_t)p->lay.count * sizeof(float), "trex_policy_act: theta"},
                      {rows_dev, trex::row_block_bytes(p->n, row_stride, p->D), "trex_policy_act: rows"},
                      {noise_dev, n * p->A, "trex_policy_act: noise"}, {actions_dev, n * p->A, "trex_policy_act: actions"},
                      {obs_out, n * p->D, "trex_policy_act: obs_out"}, {act_out, n * p->A, "trex_policy_act: act_out"},
                      {logp_out, n, "trex_policy_act: logp_out"}, {value_out, n, "trex_policy_act: value_out"}};
  if (int c = check_buffers(p, bufs)) return c;
  const ActArgs a{theta_dev, rows_dev, p->obs.norm.as<float>(), noise_dev, actions_dev, obs_out, act_out, logp_out, value_out,
                  p->n, row_stride, value_only ? 1 : 0, clip_obs, p->lay};
  HIP_TRY(trex_launch_policy_act(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---------------------------------------------------------------- privileged critic (include/trex_policy_critic.h)
int trex_policy_set_critic(TrexPolicy *p, int critic_dim, void *stream) {
  if (int c = built([&] { trex::check_policy_set_critic(p, critic_dim); })) return c;
  TrexDeviceGuard guard(p->device);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipDeviceSynchronize());
  if (critic_dim && !p->critic.stats) {      // once, for the widest critic: a later set never allocates
    const hipError_t r = alloc_moments(p->critic, POLICY_MAX_OBS, p->G);
    if (r != hipSuccess) {
      p->critic = Moments{};
      return fail(TREX_E_HIP, std::string("trex_policy_set_critic: hipMalloc: ") + hipGetErrorString(r));
    }
  }
  // the learner workspace's row stride is the parameter count: dropped, the next minibatch call makes its own
  p->grad_partial.release();
  p->grad_tiles = 0;
  p->Dv = critic_dim;
  p->critic.width = critic_dim;
  p->lay = make_layout(p->D, p->A, critic_dim);
  if (critic_dim) {
    if (int c = init_moments(p, p->critic, critic_dim, (hipStream_t)stream)) return c;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  }
  return TREX_OK;
}

int trex_policy_critic_dim(const TrexPolicy *p) { return p ? p->Dv : fail(TREX_E_INVALID, "null policy"); }

int trex_policy_critic_get_stats(TrexPolicy *p, double *host, void *stream) {
  if (int c = built([&] { trex::check_policy_has_critic("trex_policy_critic_get_stats", p, host != nullptr); })) return c;
  return get_moments(p, p->critic, 2 * p->Dv + 1, host, (hipStream_t)stream);
}

int trex_policy_critic_set_stats(TrexPolicy *p, const double *host, void *stream) {
  if (int c = built([&] { trex::check_policy_has_critic("trex_policy_critic_set_stats", p, host != nullptr); })) return c;
  return set_moments(p, p->critic, 2 * p->Dv + 1, host, (hipStream_t)stream);
}

// The observation statistics' two launches on the critic's block, with_reward = 0. Read in observe_kernel: without a reward the
// only loads from the rows are `g.rows[r * row_stride + c]` under `c < D` (the thread c == D is gated by with_reward), the return
// buffer, the reward sum and slots [2 D + 1, 2 D + 5) of the statistics are written under with_reward alone, and the three
// optional outputs are never touched - so pointed at the critic's moments they read columns [0, Dv) and nothing else.
int trex_policy_critic_observe(TrexPolicy *p, const float *rows_v_dev, int stride_v, void *stream) {
  if (int c = built([&] { trex::check_policy_critic_observe(p, rows_v_dev != nullptr, stride_v); })) return c;
  TrexDeviceGuard guard(p->device);
  BUF_TRY(p, rows_v_dev, trex::row_block_bytes((size_t)p->n, stride_v, p->Dv), "trex_policy_critic_observe: rows_v");
  ObserveArgs a{};
  a.rows = rows_v_dev; a.row_stride = stride_v;
  return observe(p, p->critic, a, (hipStream_t)stream);
}

int trex_policy_critic_act(TrexPolicy *p, const float *theta_dev, const float *rows_dev, int row_stride, const float *rows_v_dev,
                           int stride_v, float clip_obs, const float *noise_dev, float *actions_dev, float *obs_out, float *obs_v_out,
                           float *act_out, float *logp_out, float *value_out, int value_only, void *stream) {
  const trex::PolicyActCall call{theta_dev != nullptr, rows_dev != nullptr, rows_v_dev != nullptr, noise_dev != nullptr,
                                 actions_dev != nullptr, value_out != nullptr, obs_v_out != nullptr, row_stride, stride_v, value_only != 0};
  if (int c = built([&] { trex::check_policy_critic_act(p, call); })) return c;
  TrexDeviceGuard guard(p->device);
  const size_t n = (size_t)p->n * sizeof(float);
  const Buf bufs[] = {{theta_dev, (size_t)p->lay.count * sizeof(float), "trex_policy_critic_act: theta"},
                      {rows_dev, trex::row_block_bytes(p->n, row_stride, p->D), "trex_policy_critic_act: rows"},
                      {rows_v_dev, trex::row_block_bytes(p->n, stride_v, p->Dv), "trex_policy_critic_act: rows_v"},
                      {noise_dev, n * p->A, "trex_policy_critic_act: noise"}, {actions_dev, n * p->A, "trex_policy_critic_act: actions"},
                      {obs_out, n * p->D, "trex_policy_critic_act: obs_out"}, {obs_v_out, n * p->Dv, "trex_policy_critic_act: obs_v_out"},
                      {act_out, n * p->A, "trex_policy_critic_act: act_out"}, {logp_out, n, "trex_policy_critic_act: logp_out"},
                      {value_out, n, "trex_policy_critic_act: value_out"}};
  if (int c = check_buffers(p, bufs)) return c;
  // (value_only never reads the policy's row and writes the values alone: the pi workgroups return at once)
  ActArgsV a{};
  static_cast<ActArgs &>(a) = ActArgs{theta_dev, rows_dev, p->obs.norm.as<float>(), noise_dev, actions_dev, value_only ? nullptr : obs_out,
                                     act_out, logp_out, value_out, p->n, row_stride, value_only ? 1 : 0, clip_obs, p->lay};
  a.rows_v = rows_v_dev; a.norm_v = p->critic.norm.as<float>(); a.obs_v_out = value_only ? nullptr : obs_v_out;
  a.stride_v = stride_v; a.Dv = p->Dv;
  HIP_TRY(trex_launch_policy_critic_act(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---------------------------------------------------------------- rollout and optimiser
int trex_policy_gae(TrexPolicy *p, const float *raw_rew_dev, const float *rew_scale_dev, const float *done_dev,
                    const float *values_dev, float *adv_dev, float *ret_dev, int T, float gamma, float lam, float clip_rew,
                    void *stream) {
  const bool buffers = raw_rew_dev && rew_scale_dev && done_dev && values_dev && adv_dev && ret_dev;
  if (int c = built([&] { trex::check_policy_gae(p, buffers, T); })) return c;
  TrexDeviceGuard guard(p->device);
  const size_t n = (size_t)p->n, tn = (size_t)T * n * sizeof(float);
  const Buf bufs[] = {{raw_rew_dev, tn, "trex_policy_gae: raw_rew"}, {rew_scale_dev, (size_t)T * sizeof(float), "trex_policy_gae: rew_scale"},
                      {done_dev, tn, "trex_policy_gae: done"}, {values_dev, tn + n * sizeof(float), "trex_policy_gae: values"},
                      {adv_dev, tn, "trex_policy_gae: adv"}, {ret_dev, tn, "trex_policy_gae: ret"}};
  if (int c = check_buffers(p, bufs)) return c;
  const GaeArgs a{raw_rew_dev, rew_scale_dev, done_dev, values_dev, adv_dev, ret_dev, T, p->n, gamma, lam, clip_rew};
  HIP_TRY(trex_launch_policy_gae(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_policy_adam(TrexPolicy *p, float *theta_dev, float *grad_dev, float *m_dev, float *v_dev, float lr, float beta1,
                     float beta2, float eps, float max_grad_norm, float *grad_norm_out, void *stream) {
  if (!p || !theta_dev || !grad_dev || !m_dev || !v_dev) return fail(TREX_E_INVALID, "trex_policy_adam: null argument");
  TrexDeviceGuard guard(p->device);
  const size_t bytes = (size_t)p->lay.count * sizeof(float);
  const Buf bufs[] = {{theta_dev, bytes, "trex_policy_adam: theta"}, {grad_dev, bytes, "trex_policy_adam: grad"}, {m_dev, bytes, "trex_policy_adam: m"},
                      {v_dev, bytes, "trex_policy_adam: v"}, {grad_norm_out, sizeof(float), "trex_policy_adam: grad_norm_out"}};
  if (int c = check_buffers(p, bufs)) return c;
  const AdamArgs a{theta_dev, grad_dev, m_dev, v_dev, p->lay.count, p->adam_step.as<int>(), lr, beta1, beta2, eps, max_grad_norm, grad_norm_out};
  HIP_TRY(trex_launch_policy_adam(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_policy_adam_reset(TrexPolicy *p, void *stream) {
  if (!p) return fail(TREX_E_INVALID, "null policy");
  TrexDeviceGuard guard(p->device);
  HIP_TRY(hipMemsetAsync(p->adam_step.p, 0, sizeof(int), (hipStream_t)stream));
  return TREX_OK;
}

// ---------------------------------------------------------------- minibatch calls: PPO, with a critic, distillation
int trex_policy_minibatch_stats(TrexPolicy *p, const float *adv_dev, int64_t num_samples, const int64_t *perm_dev, int num_minibatches,
                                int mb, float *stats_out_dev, void *stream) {
  const bool buffers = adv_dev && perm_dev && stats_out_dev;
  if (int c = built([&] { trex::check_policy_minibatch_stats(p, buffers, num_minibatches, mb, num_samples); })) return c;
  TrexDeviceGuard guard(p->device);
  const Buf bufs[] = {{perm_dev, (size_t)num_minibatches * mb * sizeof(int64_t), "trex_policy_minibatch_stats: perm"},
                      {stats_out_dev, (size_t)num_minibatches * 2 * sizeof(float), "trex_policy_minibatch_stats: stats_out"},
                      {adv_dev, (size_t)num_samples * sizeof(float), "trex_policy_minibatch_stats: adv"}};
  if (int c = check_buffers(p, bufs)) return c;
  HIP_TRY(trex_launch_policy_adv_stats(adv_dev, reinterpret_cast<const long long *>(perm_dev), num_minibatches, mb, stats_out_dev,
                                       (hipStream_t)stream));
  return TREX_OK;
}

int trex_policy_minibatch_step(TrexPolicy *p, float *theta_dev, float *grad_dev, float *m_dev, float *v_dev, const float *obs_dev,
                               const float *act_dev, const float *logp_dev, const float *val_dev, const float *adv_dev,
                               const float *ret_dev, int64_t num_samples, const int64_t *perm_dev, int first, int mb,
                               const float *adv_stats_dev, float cliprange, float ent_coef, float vf_coef, float lr, float beta1,
                               float beta2, float eps, float max_grad_norm, float *loss_sums_dev, void *stream) {
  Minibatch c;
  c.who = "trex_policy_minibatch_step"; c.adam = true;
  c.theta = theta_dev; c.grad = grad_dev; c.m = m_dev; c.v = v_dev;
  c.obs = obs_dev; c.act = act_dev; c.logp = logp_dev; c.val = val_dev; c.adv = adv_dev; c.ret = ret_dev; c.adv_stats = adv_stats_dev;
  c.num_samples = num_samples; c.perm = perm_dev; c.first = first; c.mb = mb; c.cliprange = cliprange; c.ent_coef = ent_coef; c.vf_coef = vf_coef;
  c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.max_grad_norm = max_grad_norm; c.loss_sums = loss_sums_dev; c.stream = stream;
  return run_minibatch(p, c);
}

int trex_policy_minibatch_grad(TrexPolicy *p, const float *theta_dev, float *grad_dev, const float *obs_dev, const float *act_dev,
                               const float *logp_dev, const float *val_dev, const float *adv_dev, const float *ret_dev,
                               int64_t num_samples, const int64_t *perm_dev, int first, int mb, const float *adv_stats_dev,
                               float cliprange, float ent_coef, float vf_coef, float grad_scale, float *loss_sums_dev, void *stream) {
  Minibatch c;
  c.who = "trex_policy_minibatch_grad";
  c.theta = const_cast<float *>(theta_dev); c.grad = grad_dev;
  c.obs = obs_dev; c.act = act_dev; c.logp = logp_dev; c.val = val_dev; c.adv = adv_dev; c.ret = ret_dev; c.adv_stats = adv_stats_dev;
  c.num_samples = num_samples; c.perm = perm_dev; c.first = first; c.mb = mb; c.cliprange = cliprange; c.ent_coef = ent_coef; c.vf_coef = vf_coef;
  c.grad_scale = grad_scale; c.loss_sums = loss_sums_dev; c.stream = stream;
  return run_minibatch(p, c);
}

// ---- with a privileged critic (include/trex_policy_critic.h): the same launches, the vf workgroups on obs_v_dev
int trex_policy_critic_minibatch_step(TrexPolicy *p, float *theta_dev, float *grad_dev, float *m_dev, float *v_dev, const float *obs_dev,
                                      const float *obs_v_dev, const float *act_dev, const float *logp_dev, const float *val_dev,
                                      const float *adv_dev, const float *ret_dev, int64_t num_samples, const int64_t *perm_dev, int first,
                                      int mb, const float *adv_stats_dev, float cliprange, float ent_coef, float vf_coef, float lr,
                                      float beta1, float beta2, float eps, float max_grad_norm, float *loss_sums_dev, void *stream) {
  Minibatch c;
  c.who = "trex_policy_critic_minibatch_step"; c.critic = true; c.adam = true;
  c.theta = theta_dev; c.grad = grad_dev; c.m = m_dev; c.v = v_dev;
  c.obs = obs_dev; c.obs_v = obs_v_dev; c.act = act_dev; c.logp = logp_dev; c.val = val_dev; c.adv = adv_dev; c.ret = ret_dev; c.adv_stats = adv_stats_dev;
  c.num_samples = num_samples; c.perm = perm_dev; c.first = first; c.mb = mb; c.cliprange = cliprange; c.ent_coef = ent_coef; c.vf_coef = vf_coef;
  c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.max_grad_norm = max_grad_norm; c.loss_sums = loss_sums_dev; c.stream = stream;
  return run_minibatch(p, c);
}

int trex_policy_critic_minibatch_grad(TrexPolicy *p, const float *theta_dev, float *grad_dev, const float *obs_dev, const float *obs_v_dev,
                                      const float *act_dev, const float *logp_dev, const float *val_dev, const float *adv_dev,
                                      const float *ret_dev, int64_t num_samples, const int64_t *perm_dev, int first, int mb,
                                      const float *adv_stats_dev, float cliprange, float ent_coef, float vf_coef, float grad_scale,
                                      float *loss_sums_dev, void *stream) {
  Minibatch c;
  c.who = "trex_policy_critic_minibatch_grad"; c.critic = true;
  c.theta = const_cast<float *>(theta_dev); c.grad = grad_dev;
  c.obs = obs_dev; c.obs_v = obs_v_dev; c.act = act_dev; c.logp = logp_dev; c.val = val_dev; c.adv = adv_dev; c.ret = ret_dev; c.adv_stats = adv_stats_dev;
  c.num_samples = num_samples; c.perm = perm_dev; c.first = first; c.mb = mb; c.cliprange = cliprange; c.ent_coef = ent_coef; c.vf_coef = vf_coef;
  c.grad_scale = grad_scale; c.loss_sums = loss_sums_dev; c.stream = stream;
  return run_minibatch(p, c);
}

// ---- policy distillation (include/trex_policy_distill.h): the LOSS_DISTILL instantiation of learn_grad_kernel, then the same reduce
int trex_policy_distill_minibatch_step(TrexPolicy *p, float *theta_dev, float *grad_dev, float *m_dev, float *v_dev, const float *obs_dev,
                                       const float *teacher_mean_dev, const float *teacher_value_dev, const float *teacher_logstd_dev,
                                       int64_t num_samples, const int64_t *perm_dev, int first, int mb, int kind, float vf_coef, float lr,
                                       float beta1, float beta2, float eps, float max_grad_norm, float *loss_sums_dev, void *stream) {
  Minibatch c;
  c.who = "trex_policy_distill_minibatch_step"; c.distill = true; c.adam = true;
  c.theta = theta_dev; c.grad = grad_dev; c.m = m_dev; c.v = v_dev;
  c.obs = obs_dev; c.act = teacher_mean_dev; c.ret = teacher_value_dev; c.teacher_logstd = teacher_logstd_dev;
  c.num_samples = num_samples; c.perm = perm_dev; c.first = first; c.mb = mb; c.kind = kind; c.vf_coef = vf_coef;
  c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.max_grad_norm = max_grad_norm; c.loss_sums = loss_sums_dev; c.stream = stream;
  return run_minibatch(p, c);
}

int trex_policy_distill_minibatch_grad(TrexPolicy *p, const float *theta_dev, float *grad_dev, const float *obs_dev,
                                       const float *teacher_mean_dev, const float *teacher_value_dev, const float *teacher_logstd_dev,
                                       int64_t num_samples, const int64_t *perm_dev, int first, int mb, int kind, float vf_coef,
                                       float grad_scale, float *loss_sums_dev, void *stream) {
  Minibatch c;
  c.who = "trex_policy_distill_minibatch_grad"; c.distill = true;
  c.theta = const_cast<float *>(theta_dev); c.grad = grad_dev;
  c.obs = obs_dev; c.act = teacher_mean_dev; c.ret = teacher_value_dev; c.teacher_logstd = teacher_logstd_dev;
  c.num_samples = num_samples; c.perm = perm_dev; c.first = first; c.mb = mb; c.kind = kind; c.vf_coef = vf_coef;
  c.grad_scale = grad_scale; c.loss_sums = loss_sums_dev; c.stream = stream;
  return run_minibatch(p, c);
}

// include/trex_symmetry.h: the moments of a block become those of the stream that holds every row and its mirror image
int trex_policy_symmetrize_stats(TrexPolicy *p, const TrexMirrorTable *obs_table, const TrexMirrorTable *critic_table, void *stream) {
  // (the moments launch is ONE workgroup with a lane per column: a policy's rows, the critic's too, must fit it)
  static_assert(POLICY_MAX_OBS <= TREX_MIRROR_BLOCK, "mirror_moments_kernel takes a column per lane of one workgroup");
  const std::string me = "trex_policy_symmetrize_stats: ";
  if (!p || !obs_table) return fail(TREX_E_INVALID, me + "null argument");
  int width = 0, device = 0, width_v = 0, device_v = p->device;
  const uint32_t *words = trex_mirror_table_words(obs_table, &width, &device);
  const uint32_t *words_v = critic_table ? trex_mirror_table_words(critic_table, &width_v, &device_v) : nullptr;
  if (width != p->D) return fail(TREX_E_INVALID, me + "the obs table is " + std::to_string(width) + " wide, the policy's rows " + std::to_string(p->D));
  if (critic_table && !p->Dv) return fail(TREX_E_INVALID, me + "no critic width is set (trex_policy_set_critic)");
  if (critic_table && width_v != p->Dv)
    return fail(TREX_E_INVALID, me + "the critic table is " + std::to_string(width_v) + " wide, the critic's rows " + std::to_string(p->Dv));
  if (device != p->device || device_v != p->device) return fail(TREX_E_INVALID, me + "a table lives on another device than the policy");
  TrexDeviceGuard guard(p->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(trex_launch_mirror_moments(words, p->obs.stats.as<double>(), p->D, s));
  HIP_TRY(trex_launch_policy_refresh_norm(p->obs.stats.as<double>(), p->obs.norm.as<float>(), p->D, p->epsilon, s));
  if (critic_table) {
    HIP_TRY(trex_launch_mirror_moments(words_v, p->critic.stats.as<double>(), p->Dv, s));
    HIP_TRY(trex_launch_policy_refresh_norm(p->critic.stats.as<double>(), p->critic.norm.as<float>(), p->Dv, p->epsilon, s));
  }
  return TREX_OK;
}

}  // extern "C"
