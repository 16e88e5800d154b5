// Philox4x32-10 and the draws made of its outputs, as include/trex_sensing.h defines them: shared by sensing.hip (K13) and
// randomize.hip (K14), so that both draw from ONE generator. Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC 2011)
__device__ __forceinline__ void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
#pragma unroll
  for (int round = 0; round < 10; round++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ float u_half_open(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }          // [0, 1)
__device__ __forceinline__ float u_open_closed(uint32_t r) { return (float)((r >> 8) + 1u) * 5.9604644775390625e-8f; }  // (0, 1]
__device__ __forceinline__ int draw_int(uint32_t r, int lo, int hi) { return lo + (int)__umulhi(r, (uint32_t)(hi - lo + 1)); }

// The uniform value of include/trex_randomize.h and include/trex_start_state.h (randomize.hip, start_state.hip). The header's
// rounded operations __fsub_rn, __fmul_rn, __fadd_rn are plain operators in this toolchain's headers, and the library is built
// with -ffp-contract=fast, under which the compiler fuses a product that feeds a sum into an fma whatever pragma stands there (seen
// in the ISA). Where a header orders "rounded to f32, no fma", the product passes through rounded(): an empty asm statement that
// the value flows through, so that it exists rounded before the sum reads it.
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ float product(float a, float b) { return rounded(a * b); }
__device__ __forceinline__ float uniform(float lo, float hi, uint32_t r) { return lo + product(hi - lo, u_half_open(r)); }
