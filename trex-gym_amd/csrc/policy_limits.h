// Limits of the trainer kernels (include/trex_policy.h) and the layout of the flat parameter vector: what the host checks of the
// trainer's C-ABI (host_tables.cpp) share with policy_step.hip and ppo_learner.hip. No HIP here - policy_launch.h includes this file.
#pragma once

#ifdef __HIPCC__
#define TREX_POLICY_HD __host__ __device__
#else
#define TREX_POLICY_HD
#endif

namespace trex_policy {

constexpr int HID = 64;        // hidden width (two 32-row MFMA tiles)
constexpr int TILE = 32;       // envs per workgroup of act_kernel, samples per workgroup of learn_grad_kernel
constexpr int MAXD = 128;      // LDS row of the observation tile (obs_dim + pad <= MAXD)
constexpr int OBS_ROWS = 64;   // rows per workgroup of observe_kernel
constexpr int LEARN_UF = 13;   // float4s of theta per thread of learn_grad_kernel's staging trip (256 threads)
constexpr int POLICY_MAX_OBS = MAXD - 2;     // 126: the widest row block of act_kernel and observe_kernel (obs_dim, critic_dim)
constexpr int POLICY_MAX_ACT = 32;           // the widest action: one MFMA tile
constexpr int LEARN_MAX_OBS = 96;            // observation columns that learn_grad_kernel stages (3 x 32)
constexpr int LEARN_RED_DOUBLES = 4096;      // the learner's buffer of partial squared norms; its last slot carries the Adam step size

struct PolicyLayout {   // offsets into theta, trex_policy.h order (D: the policy net's input width; a critic's own width Dv only
  int D, A;             // sizes vf.W1 and travels beside the layout: include/trex_policy_critic.h)
  int pW1, pb1, pW2, pb2, pW3, pb3, vW1, vb1, vW2, vb2, vW3, vb3, logstd, count;
};

TREX_POLICY_HD inline PolicyLayout make_layout(int D, int A, int Dv = 0) {      // Dv = 0: the value net reads the policy's row
  // every region starts on a multiple of 4 floats (16-byte loads when the kernels stage the parameters in LDS); the
  // pad elements are ordinary, unused parameters: zero gradient, never read
  PolicyLayout l{};
  l.D = D; l.A = A;
  int o = 0;
  auto take = [&](int n) { const int at = o; o = (o + n + 3) & ~3; return at; };
  l.pW1 = take(D * HID); l.pb1 = take(HID); l.pW2 = take(HID * HID); l.pb2 = take(HID); l.pW3 = take(HID * A); l.pb3 = take(A);
  l.vW1 = take((Dv ? Dv : D) * HID); l.vb1 = take(HID); l.vW2 = take(HID * HID); l.vb2 = take(HID); l.vW3 = take(HID); l.vb3 = take(1);
  l.logstd = take(A);
  l.count = o;
  return l;
}

}  // namespace trex_policy
