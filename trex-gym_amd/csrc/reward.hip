// Reward terms (trex_batch_compose_reward, include/trex_reward.h): the terms of a specification evaluated for every env in one launch at
// the batch's current state, their weighted sum written into the reward column of the caller's rows. A workgroup of 256 lanes serves 8
// whole envs, as observation.hip does.
//
// Phase 1, as observation.hip: lane (slot, body) walks its body's chain once (chain_walk.h) and parks the body's record in LDS - only
// the bodies a term names, and the body of URDF link 0, whose lane also parks that link's frame and velocity in base axes.
// Phase 2: lane j of a slot holds joint j of its env - q, qd, torque from the row, the previous qd, the limits - and its columns of the
// action rows; lane t holds term t's timer and held value. For each term of the table (wave-uniform) the 32 lanes form their summand
// and add it up over a fixed shuffle tree inside their half-wavefront: no atomics, so a value is bitwise repeatable. Every lane carries
// the weighted sum; lane 0 writes it. History goes in and out in one coalesced pass per array.
#include <hip/hip_runtime.h>

#include "../../include/trex_batch.h"
#include "chain_walk.h"
#include "device_math.h"
#include "reward.h"
#include "step_launch.h"

namespace {

constexpr int BLOCK = TREX_REW_BLOCK;
constexpr int MAXENV = TREX_REW_MAXENV;
constexpr int REC = TREX_OBS_REC;
constexpr int SLOT = TREX_OBS_SLOT;
constexpr int FRAME = TREX_OBS_FRAME;
constexpr int TL = TREX_TL;
static_assert(BLOCK == MAXENV * TL, "one lane per (env slot, body)");
static_assert(TREX_REW_MAXTERMS <= TL, "one lane per term");

// the sum of x over the 32 lanes of a slot, in every one of them: a butterfly, the same tree whatever the values
__device__ __forceinline__ float slot_sum(float x) {
#pragma unroll
  for (int o = TL / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, TL);
  return x;
}

}  // namespace

__global__ __launch_bounds__(256) void trex_reward_kernel(TrexRewArgs a) {
  // per env slot and body: R (row-major) | origin, relative to the base origin | w | vo
  __shared__ float sRec[MAXENV * SLOT];
  // per env slot, URDF link 0: A = world <- base axes | origin, relative to the base origin | origin's velocity | angular velocity (base axes)
  __shared__ float sFrame[MAXENV * FRAME];

  const TrexDeviceModel *M = a.model;
  const int t0 = threadIdx.x;
  const int s = t0 >> 5, l = t0 & 31;
  const int env = blockIdx.x * MAXENV + s;
  const bool live = env < a.n_envs;

  // ---- phase 1: lane t0 walks the chain of body l of env slot s
  if (live && l < M->nb && ((a.body_mask >> l) & 1u)) {
    Walk k;
    const float *none = nullptr;
    walk_chain<true, false>(M, a.base, a.q, a.qd, none, env, l, a.D, k);
    float *o = sRec + s * SLOT + l * REC;
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = k.R[c];
#pragma unroll
    for (int c = 0; c < 3; c++) { o[9 + c] = k.r[c]; o[12 + c] = k.w[c]; o[15 + c] = k.vo[c]; }
    if (l == a.base_body) {
      float A[9], d0[3], lin[3];
      matmul3(k.R, a.base_tf, A);
      matvec3(k.R, a.base_tf + 9, d0);
      cross3(k.w, d0, lin);
#pragma unroll
      for (int c = 0; c < 3; c++) lin[c] += k.vo[c];
      float *f = sFrame + s * FRAME;
#pragma unroll
      for (int c = 0; c < 9; c++) f[c] = A[c];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        f[9 + c] = d0[c] + k.r[c];
        f[12 + c] = A[c] * lin[0] + A[3 + c] * lin[1] + A[6 + c] * lin[2];
        f[15 + c] = A[c] * k.w[0] + A[3 + c] * k.w[1] + A[6 + c] * k.w[2];
      }
    }
  }
  __syncthreads();

  // ---- phase 2. (Lanes past the batch's end have met the barrier and write nothing.)
  if (!live) return;
  const int J = a.nj, T = a.num_terms, A = a.act_cols;
  float *row = a.rows + (size_t)env * a.row_stride;
  const bool joint = l < J;
  const float q = joint ? row[l] : 0.f, qd = joint ? row[J + l] : 0.f, tau = joint ? row[2 * J + l] : 0.f;
  const float step_reward = row[3 * J];
  const bool done = row[3 * J + 1] != 0.f;
  const bool valid = a.valid[env] != 0;
  const float qd_prev = joint ? a.prev_qd[(size_t)env * J + l] : 0.f;
  const int jb = joint ? a.joint_body[l] : 0;
  const float lo = M->lower[jb], hi = M->upper[jb], q_start = M->q_start[jb];
  const float timer = l < T ? a.timer[(size_t)env * T + l] : 0.f, held = l < T ? a.held[(size_t)env * T + l] : 0.f;
  // this lane's share of ACTION_RATE; the actions become the previous ones in the same pass
  float da2 = 0.f;
  if (a.actions) {
    for (int c = l; c < A; c += TL) {
      const size_t at = (size_t)env * A + c;
      const float x = a.actions[at], d = x - a.prev_act[at];
      da2 += d * d;
      if (!done) a.prev_act[at] = x;
    }
  }
  const float *F = sFrame + s * FRAME;
  const float *S = a.sens ? a.sens + (size_t)env * TREX_SENS_FLOATS : nullptr;   // (read by the contact kinds only)
  const float floor_z = M->prm[TP_FLOOR_Z], Ts = a.Ts;

  float sum = 0.f, my_product = 0.f, my_value = 0.f, my_timer = 0.f;
  for (int t = 0; t < T; t++) {
    const TrexRewTerm &tm = a.term[t];
    const int kind = tm.kind;
    const bool bit = joint && ((tm.mask >> l) & 1u);
    const float p0 = tm.p0;
    const float timer_t = __shfl(timer, t, TL), held_t = __shfl(held, t, TL);
    float v = 0.f, timer_new = 0.f;
    switch (kind) {
      case TREX_REW_STEP: v = step_reward; break;
      case TREX_REW_ALIVE: v = 1.f; break;
      case TREX_REW_TRACK_LIN_VEL: {
        const float *c = a.command + (size_t)env * 3;
        const float dx = F[12] - c[0], dy = F[13] - c[1];
        v = expf(-(dx * dx + dy * dy) / p0);
        break;
      }
      case TREX_REW_TRACK_ANG_VEL: {
        const float dw = F[17] - a.command[(size_t)env * 3 + 2];
        v = expf(-(dw * dw) / p0);
        break;
      }
      case TREX_REW_LIN_VEL_Z: v = F[14] * F[14]; break;
      case TREX_REW_ANG_VEL_XY: v = F[15] * F[15] + F[16] * F[16]; break;
      case TREX_REW_ORIENTATION: v = F[6] * F[6] + F[7] * F[7]; break;   // g = -(third row of A)
      case TREX_REW_BASE_HEIGHT: {
        const float h = (a.base[(size_t)env * 16 + 2] + F[11]) - floor_z;
        v = (h - p0) * (h - p0);
        break;
      }
      case TREX_REW_POINT_HEIGHT: {
        const float *P = sRec + s * SLOT + tm.body * REC;
        const float pt[3] = {tm.point[0], tm.point[1], tm.point[2]};
        float d[3];
        matvec3(P, pt, d);
        const float h = ((a.base[(size_t)env * 16 + 2] + P[11]) + d[2]) - floor_z;
        v = (h - p0) * (h - p0);
        break;
      }
      case TREX_REW_TORQUE: v = slot_sum(bit ? tau * tau : 0.f); break;
      case TREX_REW_JOINT_VEL: v = slot_sum(bit ? qd * qd : 0.f); break;
      case TREX_REW_JOINT_ACC: {
        const float acc = (qd - qd_prev) / Ts;
        v = slot_sum(bit && valid ? acc * acc : 0.f);
        break;
      }
      case TREX_REW_ACTION_RATE: v = slot_sum(valid ? da2 : 0.f); break;
      case TREX_REW_JOINT_LIMIT: {
        // in f64: the margin is a product of roundings, and the excess what is left of a cancellation against it
        const double m = 0.5 * (1.0 - (double)p0) * ((double)hi - (double)lo);
        const double below = ((double)lo + m) - (double)q, above = (double)q - ((double)hi - m);
        v = slot_sum(bit ? (float)((below > 0.0 ? below : 0.0) + (above > 0.0 ? above : 0.0)) : 0.f);
        break;
      }
      case TREX_REW_POWER: v = slot_sum(bit ? fabsf(tau * qd) : 0.f); break;
      case TREX_REW_JOINT_POSE: v = slot_sum(bit ? (q - q_start) * (q - q_start) : 0.f); break;
      case TREX_REW_CONTACT_COUNT: {
        float hit = 0.f;
        if (l < M->nb && ((tm.mask >> l) & 1u)) {
          const float fx = S[l], fy = S[TL + l], fz = S[2 * TL + l];
          hit = sqrtf(fx * fx + fy * fy + fz * fz) > p0 ? 1.f : 0.f;
        }
        v = slot_sum(hit);
        break;
      }
      case TREX_REW_FOOT_AIR_TIME: {
        const bool contact = S[2 * TL + tm.body] > p0;
        if (!contact) timer_new = timer_t + Ts;
        else if (timer_t > 0.f) v = timer_t - tm.p1;
        break;
      }
      default: {   // FOOT_SLIP: the body's record composed with the point, as the link kinematics query does
        const float *P = sRec + s * SLOT + tm.body * REC;
        const float pt[3] = {tm.point[0], tm.point[1], tm.point[2]};
        float d[3], lin[3];
        matvec3(P, pt, d);
        cross3(P + 12, d, lin);
        const float vx = lin[0] + P[15], vy = lin[1] + P[16];
        v = S[2 * TL + tm.body] > p0 ? vx * vx + vy * vy : 0.f;
      }
    }
    // a done row: the state is the new episode's - every term but STEP repeats the step before
    if (done && kind != TREX_REW_STEP) v = held_t;
    // (the two roundings kept apart: the column is the f32 sum of the f32 products that terms_out shows)
    float product = tm.weight * v;
    asm volatile("" : "+v"(product));   // the rounded product, in a register: the addition below cannot be contracted into an fma
    sum = t == 0 ? product : sum + product;
    if (l == t) { my_product = product; my_value = v; my_timer = timer_new; }
  }

  if (l < T) {
    const size_t at = (size_t)env * T + l;
    if (a.terms_out) a.terms_out[at] = my_product;
    a.timer[at] = done ? 0.f : my_timer;
    if (!done) a.held[at] = my_value;
  }
  if (joint && !done) a.prev_qd[(size_t)env * J + l] = qd;
  if (l == 0) {
    row[3 * J] = sum;
    a.valid[env] = done ? 0 : 1;
  }
}

__global__ void trex_reward_reset_kernel(const uint8_t *mask, int n_envs, int num_terms, float *timer, float *held, int32_t *valid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = i >> 5, l = i & 31;
  if (env >= n_envs || (mask && !mask[env])) return;
  if (l < num_terms) { timer[(size_t)env * num_terms + l] = 0.f; held[(size_t)env * num_terms + l] = 0.f; }
  if (l == 0) valid[env] = 0;
}

extern "C" hipError_t trex_launch_reward(const TrexRewArgs &args, hipStream_t stream) {
  const dim3 grid((unsigned)((args.n_envs + MAXENV - 1) / MAXENV)), block(BLOCK);
  hipLaunchKernelGGL(trex_reward_kernel, grid, block, 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_reward_reset(const uint8_t *mask, int n_envs, int num_terms, float *timer, float *held, int32_t *valid,
                                               hipStream_t stream) {
  const dim3 grid((unsigned)(((size_t)n_envs * TL + 255) / 256)), block(256);
  hipLaunchKernelGGL(trex_reward_reset_kernel, grid, block, 0, stream, mask, n_envs, num_terms, timer, held, valid);
  return hipGetLastError();
}
