// What policy_step.hip and ppo_learner.hip (the trainer-side kernels of include/trex_policy.h) share on the device.
#pragma once
#include <hip/hip_runtime.h>

#include "policy_launch.h"

namespace {

using namespace trex_policy;   // the limits and the parameter layout (policy_limits.h)

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float LOG_2PI = 1.8378770664093453f;

// tanh in ~10 instructions, |error| <= 2e-7 absolute (libm's tanhf expands to ~50 with branches; the policy step
// evaluates 128 per lane): 1 - 2 / (exp(2|x|) + 1) away from 0, the odd series below |x| = 0.1 where that form cancels
__device__ __forceinline__ float tanh_fast(float x) {
  const float ax = fabsf(x), x2 = x * x;
  const float e = __builtin_amdgcn_exp2f(ax * 2.885390081777927f);           // exp(2|x|); inf for large |x| -> t = 1
  const float t = 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
  const float p = x * (1.0f + x2 * (-0.3333333333f + x2 * (0.1333333333f + x2 * (-0.05396825397f))));
  return ax < 0.1f ? p : copysignf(t, x);
}

// tanh_fast of 16 accumulator registers, stage by stage: the two quarter-rate transcendentals of one value
// overlap with those of the others (one value after the other the chain of each costs ~165 cycles: profiles/tools/mfma_chain_bench.hip)
__device__ __forceinline__ void tanh16(f32x16 &v) {
  float e[16];
#pragma unroll
  for (int r = 0; r < 16; r++) e[r] = __builtin_amdgcn_exp2f(fabsf(v[r]) * 2.885390081777927f);
#pragma unroll
  for (int r = 0; r < 16; r++) e[r] = __builtin_amdgcn_rcpf(e[r] + 1.0f);
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const float x = v[r], x2 = x * x;
    const float t = 1.0f - 2.0f * e[r];
    const float p = x * (1.0f + x2 * (-0.3333333333f + x2 * (0.1333333333f + x2 * (-0.05396825397f))));
    v[r] = fabsf(x) < 0.1f ? p : copysignf(t, x);
  }
}

// Every MFMA loop of the policy / learner kernels takes its LDS operands in ONE batch before the first MFMA (LDS_ISSUED is a compiler fence: the reads may
// not sink of the policy / learner kernels it). Left to itself the compiler issued each read right before the MFMA that uses it - read, s_waitcnt
// lgkmcnt(0), MFMA, 170 - 190 cycles per step instead of the MFMA's 64 (scripts/learn_phases.py: layer 1 7.8 k cycles for 40 steps).
#define LDS_ISSUED() asm volatile("" ::: "memory")

// Adam's two moments of one element, the rounding stated: m = fma(b1, m, (1 - b1) g), v = fma(b2, v, ((1 - b2) g) g). Left as
// `b2 * v + (1 - b2) * g * g` the compiler contracted the second one differently in adam_kernel (policy_step.hip) and in
// learn_adam_kernel (ppo_learner.hip: the form above, which both now state), and a minibatch step differed from the same gradient
// followed by trex_policy_adam by one unit in the last place of v (tests/test_gpu_distill.py holds them bitwise equal).
__device__ __forceinline__ void adam_moments(float g, float b1, float b2, float &m, float &v) {
  m = __builtin_fmaf(b1, m, (1.f - b1) * g);
  v = __builtin_fmaf(b2, v, ((1.f - b2) * g) * g);
}

// row of accumulator register `reg` on a lane of half h = lane >> 5 (C/D layout of the 32x32 MFMA forms)
__device__ __forceinline__ constexpr int rowmap(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

}  // namespace
