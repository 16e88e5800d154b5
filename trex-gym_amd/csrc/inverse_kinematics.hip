// Batched inverse kinematics (trex_batch_inverse_kinematics, include/trex_batch.h): joint angles that bring the probes of a set to
// per-env targets, by Levenberg-Marquardt damped least squares. One env per 64-lane wavefront, resident for all iterations; four
// envs per workgroup. Reads only: the kernel writes nothing but q_out and info.
//
// Every iteration, all of it in the wave's own LDS slots (the iterate, the body records, A, the Gram matrix):
//   1. outward walk, body per lane (chain_walk.h, the iterate read from LDS): origin, axis and rotation of each body parked in LDS
//   2. probe per lane: the point, the link's orientation, the probe's rows of the error e and its two residuals
//   3. Jacobian columns, joint per lane: lanes 0..31 the position rows, lanes 32..63 the orientation rows of each probe; which
//      joints carry a probe is a bit mask in the launch arguments, no chain is walked per entry
//   4. Gram matrix A A^T + lambda2 I: its at most 300 lower-triangle entries spread over the lanes
//   5. Cholesky, row per lane, column by column; the two substitutions in registers (the pivots and the right-hand side travel by
//      lane shuffles); dq = A^T x, the step limit, the clamp
// An env belongs to one wave, so the phases are ordered by wave-level fences only: no workgroup barrier, and a wave that stops
// early - or lies past the batch's end - simply leaves. Nothing an env computes depends on N, on its slot or on its neighbours.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "inverse_kinematics.h"
#include "quat_math.h"

namespace {

constexpr int TL = TREX_TL;
constexpr int WAVES = TREX_IK_WAVES;
constexpr int BLOCK = 64 * WAVES;
constexpr int REC = TREX_IK_REC, AS = TREX_IK_ASTRIDE, GS = TREX_IK_GSTRIDE;
constexpr int MAXROWS = TREX_IK_MAXROWS;
constexpr int PAIRS = (MAXROWS * (MAXROWS + 1) / 2 + 63) / 64;   // lower-triangle entries per lane: 5

// LDS written by some lanes of the wave is read by others: the wave's LDS operations execute in order, the fence keeps the
// compiler from moving them across
#define IK_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// the larger of the two, a NaN winning: a non-finite env must show in its residuals
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ float wave_nan_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = nan_max(v, __shfl_xor(v, off, 64));
  return v;
}
// clamp that keeps a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

__global__ __launch_bounds__(BLOCK) void trex_inverse_kinematics_kernel(TrexIkArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[WAVES * TREX_IK_ENV_FLOATS];

  const TrexDeviceModel *M = a.model;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int env = blockIdx.x * WAVES + wave;
  if (env >= a.n_envs) return;   // (the whole wave: there is no workgroup barrier below)
  float *W = lds + wave * TREX_IK_ENV_FLOATS;
  float *sQ = W + TREX_IK_OFF_Q, *sRec = W + TREX_IK_OFF_REC, *sP = W + TREX_IK_OFF_P, *sX = W + TREX_IK_OFF_X;
  float *sA = W + TREX_IK_OFF_A, *sG = W + TREX_IK_OFF_G;

  const int nb = a.nb, J = nb - 1, K = a.K, Mr = a.M;
  const int bl = lane & 31, half = lane >> 5;
  const bool joint_lane = bl >= 1 && bl < nb;            // this lane's body carries a joint (both halves of the wave)
  const bool is_joint = joint_lane && half == 0;
  const bool moves = is_joint && ((a.move_mask >> bl) & 1u);
  const int slot = is_joint ? M->obs_slot[bl] : 0;
  const float lo = is_joint ? M->lower[bl] : 0.f, hi = is_joint ? M->upper[bl] : 0.f;

  // ---- start: the iterate by body lane, the moving joints clamped to their limits
  float qcur = 0.f;
  if (is_joint) {
    qcur = a.q_init ? a.q_init[(size_t)env * J + slot] : a.q[(size_t)env * TL + bl];
    if (moves) qcur = clamp_keep_nan(qcur, lo, hi);
  }
  if (half == 0) sQ[bl] = qcur;

  // ---- the lower-triangle entries (i, j) this lane owns of the Gram matrix: t = lane + 64 s, packed i << 8 | j, -1 = none
  int pair[PAIRS];
  {
    const int T = Mr * (Mr + 1) / 2;
#pragma unroll
    for (int s = 0; s < PAIRS; s++) {
      const int t = lane + 64 * s;
      int i = 0;
      while ((i + 1) * (i + 2) / 2 <= t) i++;
      pair[s] = t < T ? (i << 8 | (t - i * (i + 1) / 2)) : -1;
    }
  }

  // ---- probe lanes: the probe's body, mode and first row; its target in world axes, relative to the base origin
  const bool is_probe = lane < K;
  const int pk = is_probe ? lane : 0;
  const int pbody = a.body[pk], pmode = is_probe ? a.mode[pk] : 0, prow = a.row0[pk];
  const float *brow = a.base + (size_t)env * 16;
  float pT[3] = {0.f, 0.f, 0.f}, qT[4] = {0.f, 0.f, 0.f, 1.f};
  if (is_probe) {
    const float *t = a.target + ((size_t)env * K + pk) * 7;
    float qn[4] = {t[3], t[4], t[5], t[6]};
    const float inv = 1.0f / sqrtf(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
    for (int c = 0; c < 4; c++) qn[c] *= inv;
    if (a.frame == TREX_AXES_BASE) {   // URDF link 0's frame: a frame of the base body, fixed while the joints move
      const float bq[4] = {brow[3], brow[4], brow[5], brow[6]};
      float Rb[9], R0[9], Rt[9], p0[3], d[3];
      quat_to_mat(bq, Rb);
      matmul3(Rb, a.base_tf, R0);
      matvec3(Rb, a.base_tf + 9, p0);
      const float tp[3] = {t[0], t[1], t[2]};
      matvec3(R0, tp, d);
#pragma unroll
      for (int c = 0; c < 3; c++) pT[c] = p0[c] + d[c];
      quat_to_mat(qn, Rt);
      matmul3(R0, Rt, Rt);
      mat_to_quat(Rt, qT);
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) pT[c] = t[c] - brow[c];
#pragma unroll
      for (int c = 0; c < 4; c++) qT[c] = qn[c];
    }
  }
  IK_WSYNC();

  int it = 0;
  float init_norm = 0.f, res_p = 0.f, res_o = 0.f;
  for (;;) {
    // ---- 1. outward walk at the iterate
    if (lane < nb) {
      Walk k;
      const float *qrow = sQ, *none = nullptr;
      walk_chain<false, false>(M, brow, qrow, none, none, 0, lane, 0, k);
      float *o = sRec + lane * REC;
#pragma unroll
      for (int c = 0; c < 9; c++) o[c] = k.R[c];
#pragma unroll
      for (int c = 0; c < 3; c++) { o[9 + c] = k.r[c]; o[12 + c] = k.a[c]; }
    }
    IK_WSYNC();

    // ---- 2. this lane's probe: point, error rows, residuals
    float rp = 0.f, ro = 0.f;
    if (is_probe) {
      const float *P = sRec + pbody * REC;
      const float *tf = a.probe_tf + 12 * (size_t)pk;
      float d[3], p[3];
      matvec3(P, tf + 9, d);
#pragma unroll
      for (int c = 0; c < 3; c++) { p[c] = P[9 + c] + d[c]; sP[4 * pk + c] = p[c]; }
      int row = prow;
      if (pmode & TREX_IK_POSITION) {
        const float e[3] = {pT[0] - p[0], pT[1] - p[1], pT[2] - p[2]};
#pragma unroll
        for (int c = 0; c < 3; c++) sX[row + c] = e[c];
        rp = sqrtf(dot3(e, e));
        row += 3;
      }
      if (pmode & TREX_IK_ORIENTATION) {
        float Rl[9], ql[4];
        matmul3(P, tf, Rl);
        mat_to_quat(Rl, ql);
        // quat_target o quat_link^-1
        const float ex = -qT[3] * ql[0] + qT[0] * ql[3] - qT[1] * ql[2] + qT[2] * ql[1];
        const float ey = -qT[3] * ql[1] + qT[0] * ql[2] + qT[1] * ql[3] - qT[2] * ql[0];
        const float ez = -qT[3] * ql[2] - qT[0] * ql[1] + qT[1] * ql[0] + qT[2] * ql[3];
        const float ew = qT[3] * ql[3] + qT[0] * ql[0] + qT[1] * ql[1] + qT[2] * ql[2];
        const float sg = ew < 0.f ? -2.f : 2.f;
        sX[row] = sg * ex; sX[row + 1] = sg * ey; sX[row + 2] = sg * ez;
        const float vn = sqrtf(ex * ex + ey * ey + ez * ez);
        ro = 2.f * asinf(vn > 1.f ? 1.f : vn);
      }
    }
    IK_WSYNC();
    float v = lane < Mr ? sX[lane] : 0.f;       // lane i holds e_i from here to the end of the solve
    const float en2 = wave_sum(v * v);
    res_p = wave_nan_max(rp);
    res_o = wave_nan_max(ro);
    if (it == 0) init_norm = sqrtf(en2);
    if (it >= a.iterations) break;
    if ((a.tol_pos > 0.f || a.tol_ori > 0.f) && res_p <= a.tol_pos && res_o <= a.tol_ori) break;

    // ---- 3. Jacobian columns: lanes 0..31 the position rows, lanes 32..63 the orientation rows; joint bl per lane
    {
      const float *Pj = sRec + bl * REC;
      const float ax[3] = {Pj[12], Pj[13], Pj[14]}, rj[3] = {Pj[9], Pj[10], Pj[11]};
      const bool mv = joint_lane && ((a.move_mask >> bl) & 1u);
      for (int k = 0; k < K; k++) {
        const int mode = a.mode[k];
        const bool on = mv && ((a.chain[k] >> bl) & 1u);
        const int r0 = a.row0[k];
        if (half == 0) {
          if (mode & TREX_IK_POSITION) {
            const float lever[3] = {sP[4 * k] - rj[0], sP[4 * k + 1] - rj[1], sP[4 * k + 2] - rj[2]};
            float col[3];
            cross3(ax, lever, col);
#pragma unroll
            for (int c = 0; c < 3; c++) sA[(r0 + c) * AS + bl] = on ? col[c] : 0.f;
          }
        } else if (mode & TREX_IK_ORIENTATION) {
          const int r1 = r0 + ((mode & TREX_IK_POSITION) ? 3 : 0);
#pragma unroll
          for (int c = 0; c < 3; c++) sA[(r1 + c) * AS + bl] = on ? ax[c] : 0.f;
        }
      }
    }
    IK_WSYNC();

    // ---- 4. Gram matrix, lower triangle
    const float lambda2 = a.damping2 + a.gain * en2;
#pragma unroll
    for (int s = 0; s < PAIRS; s++) {
      if (pair[s] < 0) continue;
      const int i = pair[s] >> 8, j = pair[s] & 255;
      const float *Ai = sA + i * AS, *Aj = sA + j * AS;
      float g = 0.f;
      for (int b = 1; b < nb; b++) g = __builtin_fmaf(Ai[b], Aj[b], g);
      sG[i * GS + j] = i == j ? g + lambda2 : g;
    }
    IK_WSYNC();

    // ---- 5. Cholesky G = L L^T in place, lane i row i, column by column; a pivot that is not positive becomes lambda2
    for (int k = 0; k < Mr; k++) {
      float s = 0.f;
      if (lane >= k && lane < Mr) {
        s = sG[lane * GS + k];
        for (int m = 0; m < k; m++) s = __builtin_fmaf(-sG[lane * GS + m], sG[k * GS + m], s);
      }
      float p = __shfl(s, k, 64);
      if (!(p > 0.f)) p = lambda2;
      const float dk = sqrtf(p);
      if (lane == k) sG[k * GS + k] = dk;
      else if (lane > k && lane < Mr) sG[lane * GS + k] = s / dk;
      IK_WSYNC();
    }
    // L y = e, then L^T x = y: lane i ends with x_i
    for (int k = 0; k < Mr; k++) {
      const float yk = __shfl(v, k, 64) / sG[k * GS + k];
      if (lane == k) v = yk;
      else if (lane > k && lane < Mr) v = __builtin_fmaf(-sG[lane * GS + k], yk, v);
    }
    for (int k = Mr - 1; k >= 0; k--) {
      const float xk = __shfl(v, k, 64) / sG[k * GS + k];
      if (lane == k) v = xk;
      else if (lane < k) v = __builtin_fmaf(-sG[k * GS + lane], xk, v);
    }
    if (lane < Mr) sX[lane] = v;
    IK_WSYNC();

    // ---- dq = A^T x, the step limit, the clamp
    float dq = 0.f;
    if (moves) {
      for (int i = 0; i < Mr; i++) dq = __builtin_fmaf(sA[i * AS + bl], sX[i], dq);
    }
    const float big = wave_nan_max(fabsf(dq));
    if (big > a.max_step) dq *= a.max_step / big;
    if (moves) {
      qcur = clamp_keep_nan(qcur + dq, lo, hi);
      sQ[bl] = qcur;
    }
    it++;
    IK_WSYNC();
  }

  if (is_joint) a.q_out[(size_t)env * J + slot] = qcur;
  if (a.info && lane == 0) {
    float *o = a.info + (size_t)env * 4;
    o[0] = res_p; o[1] = res_o; o[2] = (float)it; o[3] = init_norm;
  }
}

extern "C" hipError_t trex_launch_inverse_kinematics(const TrexIkArgs &args, hipStream_t stream) {
  const dim3 grid((unsigned)((args.n_envs + WAVES - 1) / WAVES)), block(BLOCK);
  hipLaunchKernelGGL(trex_inverse_kinematics_kernel, grid, block, 0, stream, args);
  return hipGetLastError();
}
