// Dynamics queries on the batch state: inverse dynamics (RNEA), joint-space mass matrix (CRBA), point Jacobian of a link,
// centroidal quantities, forward dynamics and M^-1 x (ABA). Read-only: nothing here writes the state. gfx950, one env per 64-lane wavefront, one body per lane,
// four envs per workgroup so that the four outputs lie back to back and leave the chip as 16-byte stores.
//
// Conventions (include/trex_batch.h, "dynamics queries"): generalised velocity = base linear v(3), base angular w(3) - world
// axes, v the velocity of the base frame origin - then qd in observation order; accelerations their classical derivatives;
// forces the duals (force on the base, torque about the base origin, joint torques).
//
// Everything is written in world axes with positions RELATIVE TO THE BASE ORIGIN O (a few metres: f32 keeps its digits at any
// world position). Unlike the step kernel's tree block, which refers every spatial quantity to one common point, the passes
// here keep each body's quantities about ITS OWN points - forces at the COM, moments about the body's joint origin, composite
// inertias about the composite's COM - and shift by the short lever between a body and its parent: a distal tail joint's
// diagonal m |c - r|^2 + a.Ic a is then a sum of positive terms and not the difference of two m |r|^2 three metres out.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "dynamics.h"

namespace {

constexpr int TL = TREX_TL;
constexpr int MAXCH = TREX_MAXCH;
constexpr int WAVES = TREX_DYN_WAVES;
constexpr int BLOCK = 64 * WAVES;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// mass, COM offset from the body origin and rotational inertia about the COM (world axes) of body b, the env's mass scale in
struct Inertia { float m, cb[3], Ic[6]; };
__device__ __forceinline__ void body_inertia(const TrexDynArgs &A, const TrexDeviceModel *M, int env, int b, const float *R, Inertia &I) {
  const float sc = A.mass_scale ? A.mass_scale[(size_t)env * TL + b] : 1.0f;
  I.m = M->mass[b] * sc;
  const float comb[3] = {M->com[0][b], M->com[1][b], M->com[2][b]};
  matvec3(R, comb, I.cb);
  float in[6], t[9];
#pragma unroll
  for (int c = 0; c < 6; c++) in[c] = M->inertia[c][b];
  const float Ib[9] = {in[0], in[1], in[2], in[1], in[3], in[4], in[2], in[4], in[5]};
  matmul3(R, Ib, t);
  const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int c = 0; c < 6; c++)
    I.Ic[c] = sc * (t[3 * ia[c]] * R[3 * ib[c]] + t[3 * ia[c] + 1] * R[3 * ib[c] + 1] + t[3 * ia[c] + 2] * R[3 * ib[c] + 2]);
}

// The workgroup's outputs - those of its (up to four) envs, back to back in LDS as in HBM - as 16-byte stores where the
// caller's buffer allows it (four envs are a multiple of 16 bytes whatever D is: only its base address can be odd).
__device__ __forceinline__ void block_store(float *dst, const float *src, int count) {
  const int t = threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const int n4 = count >> 2;
    for (int i = t; i < n4; i += BLOCK) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(src)[i];
    for (int i = (n4 << 2) + t; i < count; i += BLOCK) dst[i] = src[i];
  } else {
    for (int i = t; i < count; i += BLOCK) dst[i] = src[i];
  }
}

template <int Q>
__global__ __launch_bounds__(BLOCK) void trex_dynamics_kernel(TrexDynArgs A) {
  extern __shared__ float4 lds4[];
  float *lds = reinterpret_cast<float *>(lds4);
  const TrexDeviceModel *M = A.model;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int env0 = blockIdx.x * WAVES, env = env0 + wave;
  const int nb = A.nb, D = 6 + nb - 1;
  // (the two ABA queries carry one right-hand side in each half of the wave: body = lane & 31 there)
  constexpr bool ABA = Q == TREX_DYN_FORWARD_DYNAMICS || Q == TREX_DYN_SOLVE_MASS;
  const int per_env = trex_dyn_out_floats(Q, D, Q == TREX_DYN_SOLVE_MASS ? A.num_rhs : 1);
  const bool live = env < A.n_envs;                      // (a wave past the batch's end still meets the barriers)
  const bool is_body = live && (ABA ? lane & 31 : lane) < nb;
  const int b = is_body ? (ABA ? lane & 31 : lane) : 0;
  const int e = live ? env : 0;
  float *rec = lds + wave * trex_dyn_body_floats(Q);     // [32][16] this env's per-body records (ABA: [32][37])
  float *stage = lds + WAVES * trex_dyn_body_floats(Q) + wave * per_env;
  const int depth = is_body ? M->depth[b] : -1;
  const int maxdepth = M->maxdepth;
  const int slot = is_body && b >= 1 ? 6 + M->obs_slot[b] : -1;   // this body's joint among the D velocities

  if constexpr (Q == TREX_DYN_INVERSE_DYNAMICS) {
    // ---- RNEA. Outward (in registers): classical velocity and acceleration of every body frame; the force at the COM
    // and the moment about the body's joint origin that this motion needs.
    Walk k;
    walk_chain<true, true>(M, A.base, A.q, A.qd, A.accel, e, b, D, k);
    Inertia I;
    body_inertia(A, M, e, b, k.R, I);
    float F[3], N[3];
    {
      float t0[3], t1[3], ac[3], Iw[3], Ial[3], wIw[3], cxf[3];
      cross3(k.al, I.cb, t0);
      cross3(k.w, I.cb, t1); cross3(k.w, t1, t1);
#pragma unroll
      for (int c = 0; c < 3; c++) ac[c] = k.ao[c] + t0[c] + t1[c];
#pragma unroll
      for (int c = 0; c < 3; c++) F[c] = I.m * ac[c];
      sym3_mul(I.Ic, k.w, Iw); sym3_mul(I.Ic, k.al, Ial);
      cross3(k.w, Iw, wIw); cross3(I.cb, F, cxf);
#pragma unroll
      for (int c = 0; c < 3; c++) N[c] = Ial[c] + wIw[c] + cxf[c];
    }
    // ---- inward, level by level: a body adds its children's force, and their moment shifted by the lever child -> body
    if (is_body) {
      float *o = rec + 16 * b;
#pragma unroll
      for (int c = 0; c < 3; c++) { o[c] = F[c]; o[3 + c] = N[c]; o[6 + c] = k.r[c]; }
    }
    __syncthreads();
    for (int d = maxdepth - 1; d >= 0; d--) {
      if (depth == d) {
        bool any = false;
        for (int kc = 0; kc < MAXCH; kc++) {
          const int ch = M->child[kc][b];
          if (ch < 0) break;
          const float *o = rec + 16 * ch;
          const float Fc[3] = {o[0], o[1], o[2]}, lever[3] = {o[6] - k.r[0], o[7] - k.r[1], o[8] - k.r[2]};
          float lxf[3];
          cross3(lever, Fc, lxf);
#pragma unroll
          for (int c = 0; c < 3; c++) { F[c] += Fc[c]; N[c] += o[3 + c] + lxf[c]; }
          any = true;
        }
        if (any) {
          float *o = rec + 16 * b;
#pragma unroll
          for (int c = 0; c < 3; c++) { o[c] = F[c]; o[3 + c] = N[c]; }
        }
      }
      __syncthreads();
    }
    if (is_body) {
      if (b == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { stage[c] = F[c]; stage[3 + c] = N[c]; }
      } else {
        stage[slot] = dot3(k.a, N);
      }
    }
  }

  if constexpr (Q == TREX_DYN_MASS_MATRIX) {
    // ---- CRBA. Composite rigid body of every subtree - mass, COM, rotational inertia about that COM - inward level by
    // level (parallel-axis sums of positive terms); then every joint lane walks its ancestor chain: column j of M is the
    // momentum of subtree j turning about joint j, row i its projection on joint i's motion.
    Walk k;
    walk_chain<false, false>(M, A.base, A.q, A.qd, A.accel, e, b, D, k);
    Inertia I;
    body_inertia(A, M, e, b, k.R, I);
    float cm = I.m, cc[3], ci[6];
#pragma unroll
    for (int c = 0; c < 3; c++) cc[c] = k.r[c] + I.cb[c];
#pragma unroll
    for (int c = 0; c < 6; c++) ci[c] = I.Ic[c];
    for (int i = lane; i < per_env; i += 64) stage[i] = 0.f;
    if (is_body) {
      float *o = rec + 16 * b;
      o[0] = cm;
#pragma unroll
      for (int c = 0; c < 3; c++) { o[1 + c] = cc[c]; o[10 + c] = k.a[c]; o[13 + c] = k.r[c]; }
#pragma unroll
      for (int c = 0; c < 6; c++) o[4 + c] = ci[c];
    }
    __syncthreads();
    for (int d = maxdepth - 1; d >= 0; d--) {
      if (depth == d && M->child[0][b] >= 0) {
        // total mass and COM (as an offset from the body's own COM), then every part's inertia shifted to it
        float mt = cm, mo[3] = {0.f, 0.f, 0.f};
        for (int kc = 0; kc < MAXCH; kc++) {
          const int ch = M->child[kc][b];
          if (ch < 0) break;
          const float *o = rec + 16 * ch;
          mt += o[0];
#pragma unroll
          for (int c = 0; c < 3; c++) mo[c] += o[0] * (o[1 + c] - cc[c]);
        }
        float ct[3];
#pragma unroll
        for (int c = 0; c < 3; c++) ct[c] = cc[c] + mo[c] / mt;
        float it[6];
        {
          const float dv[3] = {cc[0] - ct[0], cc[1] - ct[1], cc[2] - ct[2]};
          const float dd = dot3(dv, dv);
          it[0] = ci[0] + cm * (dd - dv[0] * dv[0]); it[1] = ci[1] - cm * dv[0] * dv[1]; it[2] = ci[2] - cm * dv[0] * dv[2];
          it[3] = ci[3] + cm * (dd - dv[1] * dv[1]); it[4] = ci[4] - cm * dv[1] * dv[2]; it[5] = ci[5] + cm * (dd - dv[2] * dv[2]);
        }
        for (int kc = 0; kc < MAXCH; kc++) {
          const int ch = M->child[kc][b];
          if (ch < 0) break;
          const float *o = rec + 16 * ch;
          const float mk = o[0], dv[3] = {o[1] - ct[0], o[2] - ct[1], o[3] - ct[2]};
          const float dd = dot3(dv, dv);
          it[0] += o[4] + mk * (dd - dv[0] * dv[0]); it[1] += o[5] - mk * dv[0] * dv[1]; it[2] += o[6] - mk * dv[0] * dv[2];
          it[3] += o[7] + mk * (dd - dv[1] * dv[1]); it[4] += o[8] - mk * dv[1] * dv[2]; it[5] += o[9] + mk * (dd - dv[2] * dv[2]);
        }
        cm = mt;
#pragma unroll
        for (int c = 0; c < 3; c++) cc[c] = ct[c];
#pragma unroll
        for (int c = 0; c < 6; c++) ci[c] = it[c];
        float *o = rec + 16 * b;
        o[0] = cm;
#pragma unroll
        for (int c = 0; c < 3; c++) o[1 + c] = cc[c];
#pragma unroll
        for (int c = 0; c < 6; c++) o[4 + c] = ci[c];
      }
      __syncthreads();
    }
    // (every entry is written once, and to both triangles from the same register: the output is exactly symmetric)
    if (is_body && b >= 1) {
      // subtree j turning about joint j at unit rate: linear momentum p, angular momentum L about the subtree's COM
      float lev[3] = {cc[0] - k.r[0], cc[1] - k.r[1], cc[2] - k.r[2]}, p[3], L[3], cxp[3];
      cross3(k.a, lev, p);
#pragma unroll
      for (int c = 0; c < 3; c++) p[c] *= cm;
      sym3_mul(ci, k.a, L);
      cross3(cc, p, cxp);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float lin = p[c], ang = L[c] + cxp[c];     // base rows: force, torque about the base origin
        stage[c * D + slot] = lin; stage[slot * D + c] = lin;
        stage[(3 + c) * D + slot] = ang; stage[slot * D + 3 + c] = ang;
      }
      for (int d = depth; d >= 1; d--) {
        const int i = M->anc[d - 1][b];
        const float *o = rec + 16 * i;
        const float ai[3] = {o[10], o[11], o[12]}, li[3] = {cc[0] - o[13], cc[1] - o[14], cc[2] - o[15]};
        float axl[3];
        cross3(ai, li, axl);
        const float v = dot3(ai, L) + dot3(axl, p);
        const int si = 6 + M->obs_slot[i];
        stage[si * D + slot] = v; stage[slot * D + si] = v;
      }
    }
    if (is_body && b == 0) {
      // the base block: the whole robot as one rigid body, its rotational inertia taken to the base origin
      const float dd = dot3(cc, cc);
      const float io[6] = {ci[0] + cm * (dd - cc[0] * cc[0]), ci[1] - cm * cc[0] * cc[1], ci[2] - cm * cc[0] * cc[2],
                           ci[3] + cm * (dd - cc[1] * cc[1]), ci[4] - cm * cc[1] * cc[2], ci[5] + cm * (dd - cc[2] * cc[2])};
      const float io9[9] = {io[0], io[1], io[2], io[1], io[3], io[4], io[2], io[4], io[5]};
      // force of a unit angular velocity e_l: m (e_l x C)
      const float cx[9] = {0.f, cm * cc[2], -cm * cc[1], -cm * cc[2], 0.f, cm * cc[0], cm * cc[1], -cm * cc[0], 0.f};
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
          stage[r * D + c] = r == c ? cm : 0.f;
          stage[(3 + r) * D + 3 + c] = io9[3 * r + c];
          stage[r * D + 3 + c] = cx[3 * r + c]; stage[(3 + c) * D + r] = cx[3 * r + c];
        }
    }
  }

  if constexpr (Q == TREX_DYN_JACOBIAN) {
    Walk k;
    walk_chain<false, false>(M, A.base, A.q, A.qd, A.accel, e, b, D, k);
    const int B = A.jac_body;
    if (is_body && b == B) {
      const float pt[3] = {A.jac_point[0], A.jac_point[1], A.jac_point[2]};
      float o[3];
      matvec3(k.R, pt, o);
#pragma unroll
      for (int c = 0; c < 3; c++) rec[c] = k.r[c] + o[c];
    }
    __syncthreads();
    if (is_body) {
      const float P[3] = {rec[0], rec[1], rec[2]};   // the point, relative to the base origin
      if (b == 0) {
        const float ex[9] = {0.f, P[2], -P[1], -P[2], 0.f, P[0], P[1], -P[0], 0.f};   // row r, column l: (e_l x P)_r
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int c = 0; c < 3; c++) {
            stage[r * D + c] = r == c ? 1.f : 0.f;
            stage[r * D + 3 + c] = ex[3 * r + c];
            stage[(3 + r) * D + c] = 0.f;
            stage[(3 + r) * D + 3 + c] = r == c ? 1.f : 0.f;
          }
      } else {
        // joint b moves the point iff b lies on the chain of the point's body
        const bool on = M->depth[B] >= depth && M->anc[depth - 1][B] == b;
        float lev[3] = {P[0] - k.r[0], P[1] - k.r[1], P[2] - k.r[2]}, lin[3];
        cross3(k.a, lev, lin);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          stage[c * D + slot] = on ? lin[c] : 0.f;
          stage[(3 + c) * D + slot] = on ? k.a[c] : 0.f;
        }
      }
    }
  }

  if constexpr (Q == TREX_DYN_CENTROIDAL) {
    Walk k;
    walk_chain<true, false>(M, A.base, A.q, A.qd, A.accel, e, b, D, k);
    Inertia I;
    body_inertia(A, M, e, b, k.R, I);
    const float m = is_body ? I.m : 0.f;
    float c[3], vc[3], wxc[3], Iw[3];
    cross3(k.w, I.cb, wxc);
    sym3_mul(I.Ic, k.w, Iw);
#pragma unroll
    for (int x = 0; x < 3; x++) { c[x] = k.r[x] + I.cb[x]; vc[x] = k.vo[x] + wxc[x]; }
    const float *base = A.base + (size_t)e * 16;
    const float mt = wave_sum(m);
    float C[3], V[3], p[3], Lb[3], L[3];
#pragma unroll
    for (int x = 0; x < 3; x++) {
      C[x] = wave_sum(m * c[x]) / mt;
      p[x] = wave_sum(m * vc[x]);
      V[x] = p[x] / mt;
    }
    const float ke = wave_sum(is_body ? 0.5f * (m * dot3(vc, vc) + dot3(k.w, Iw)) : 0.f);
    const float pe = wave_sum(m * M->prm[TP_GRAVITY] * (base[2] + c[2]));
    {
      const float dc[3] = {c[0] - C[0], c[1] - C[1], c[2] - C[2]}, dv[3] = {vc[0] - V[0], vc[1] - V[1], vc[2] - V[2]};
      cross3(dc, dv, Lb);
#pragma unroll
      for (int x = 0; x < 3; x++) L[x] = wave_sum(is_body ? Iw[x] + m * Lb[x] : 0.f);
    }
    if (lane == 0) {
#pragma unroll
      for (int x = 0; x < 3; x++) { stage[x] = base[x] + C[x]; stage[3 + x] = V[x]; stage[6 + x] = p[x]; stage[9 + x] = L[x]; }
      stage[12] = ke; stage[13] = pe; stage[14] = mt; stage[15] = 0.f;
    }
  }

  if constexpr (ABA) {
    // ---- ABA in classical accelerations. The acceleration of every body frame is split a = a0 + da: a0 the motion with zero
    // base and joint accelerations (the velocity-product terms, and gravity as the base's upward acceleration - the outward
    // pass of RNEA above), da what the unknown accelerations add. da is LINEAR in them and moves from point to point like a
    // velocity (da_P = da_Q + dal x (P - Q)), so the three passes run on da with the body wrenches of a0 as the bias force
    // (forward dynamics) or none (solve_mass), and the base's da IS its classical acceleration: nothing to convert.
    // Every body's articulated inertia, bias wrench and da are about ITS OWN joint origin; a child's are shifted to the
    // parent's origin by the short lever between the two. A wrench is (moment n, force f), a motion (angular al, linear a):
    // n = IA al + IH a, f = IH^T al + IM a; a rigid body of mass m, COM offset c: IM = m 1, IH = m [c]x, IA = Ic - m [c]x[c]x.
    constexpr bool FD = Q == TREX_DYN_FORWARD_DYNAMICS;
    constexpr int RS = TREX_DYN_ABA_STRIDE, R_ORG = 21, R_SLOT = 24;
    const int half = lane >> 5;
    const int K = FD ? 1 : A.num_rhs;
    const float *none = nullptr;
    Walk k;
    walk_chain<FD, FD>(M, A.base, A.q, A.qd, none, e, b, D, k);
    Inertia I;
    body_inertia(A, M, e, b, k.R, I);
    float F[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 0.f, 0.f};      // forward dynamics: the wrench of a0 on this body (as RNEA's)
    if constexpr (FD) {
      float t0[3], t1[3], ac[3], Iw[3], Ial[3], wIw[3], cxf[3];
      cross3(k.al, I.cb, t0);
      cross3(k.w, I.cb, t1); cross3(k.w, t1, t1);
#pragma unroll
      for (int c = 0; c < 3; c++) ac[c] = k.ao[c] + t0[c] + t1[c];
#pragma unroll
      for (int c = 0; c < 3; c++) F[c] = I.m * ac[c];
      sym3_mul(I.Ic, k.w, Iw); sym3_mul(I.Ic, k.al, Ial);
      cross3(k.w, Iw, wIw); cross3(I.cb, F, cxf);
#pragma unroll
      for (int c = 0; c < 3; c++) N[c] = Ial[c] + wIw[c] + cxf[c];
    }
    // ---- pass 1, inward: articulated inertias, U = I^A S, 1 / d. Both halves compute, half 0 writes.
    float IA[6], IH[9], IM[6] = {I.m, 0.f, 0.f, I.m, 0.f, I.m};
    {
      const float *c = I.cb, m = I.m, cc = dot3(c, c);
      IA[0] = I.Ic[0] + m * (cc - c[0] * c[0]); IA[1] = I.Ic[1] - m * c[0] * c[1]; IA[2] = I.Ic[2] - m * c[0] * c[2];
      IA[3] = I.Ic[3] + m * (cc - c[1] * c[1]); IA[4] = I.Ic[4] - m * c[1] * c[2]; IA[5] = I.Ic[5] + m * (cc - c[2] * c[2]);
      IH[0] = 0.f; IH[1] = -m * c[2]; IH[2] = m * c[1];
      IH[3] = m * c[2]; IH[4] = 0.f; IH[5] = -m * c[0];
      IH[6] = -m * c[1]; IH[7] = m * c[0]; IH[8] = 0.f;
    }
    if (is_body && half == 0) {
#pragma unroll
      for (int c = 0; c < 3; c++) rec[RS * b + R_ORG + c] = k.r[c];
    }
    __syncthreads();
    float lev[3];                                               // parent origin -> this origin
    {
      const float *o = rec + RS * (b >= 1 ? M->parent[b] : 0) + R_ORG;
#pragma unroll
      for (int c = 0; c < 3; c++) lev[c] = k.r[c] - o[c];
    }
    float Un[3] = {0.f, 0.f, 0.f}, Uf[3] = {0.f, 0.f, 0.f}, dinv = 0.f;
    for (int d = maxdepth; d >= 0; d--) {
      if (depth == d) {
        for (int kc = 0; kc < MAXCH; kc++) {
          const int ch = M->child[kc][b];
          if (ch < 0) break;
          const float *o = rec + RS * ch;
          const float l[3] = {o[R_ORG] - k.r[0], o[R_ORG + 1] - k.r[1], o[R_ORG + 2] - k.r[2]};
          float cH[9], Hp[9], x1[9], x2[9];
#pragma unroll
          for (int c = 0; c < 9; c++) cH[c] = o[6 + c];
          const float cM[6] = {o[15], o[16], o[17], o[18], o[19], o[20]};
          const float Mf[9] = {cM[0], cM[1], cM[2], cM[1], cM[3], cM[4], cM[2], cM[4], cM[5]};
          // H' = H + [l]x M;  A' = A + [l]x H^T + H' [l]x^T
#pragma unroll
          for (int j = 0; j < 3; j++) {
            const float col[3] = {Mf[j], Mf[3 + j], Mf[6 + j]};
            float t[3];
            cross3(l, col, t);
#pragma unroll
            for (int i = 0; i < 3; i++) Hp[3 * i + j] = cH[3 * i + j] + t[i];
          }
#pragma unroll
          for (int r = 0; r < 3; r++) { cross3(l, cH + 3 * r, x1 + 3 * r); cross3(l, Hp + 3 * r, x2 + 3 * r); }
          const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
          for (int c = 0; c < 6; c++) {
            IA[c] += o[c] + x1[3 * ib[c] + ia[c]] + x2[3 * ia[c] + ib[c]];
            IM[c] += cM[c];
          }
#pragma unroll
          for (int c = 0; c < 9; c++) IH[c] += Hp[c];
        }
        float *o = rec + RS * b;
        if (b >= 1) {
          // the joint turns about k.a through the body origin: S = (a, 0)
          sym3_mul(IA, k.a, Un);
#pragma unroll
          for (int j = 0; j < 3; j++) Uf[j] = IH[j] * k.a[0] + IH[3 + j] * k.a[1] + IH[6 + j] * k.a[2];
          dinv = 1.0f / dot3(k.a, Un);
          if (half == 0) {
            const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
            for (int c = 0; c < 6; c++) {
              o[c] = IA[c] - Un[ia[c]] * Un[ib[c]] * dinv;
              o[15 + c] = IM[c] - Uf[ia[c]] * Uf[ib[c]] * dinv;
            }
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
              for (int j = 0; j < 3; j++) o[6 + 3 * i + j] = IH[3 * i + j] - Un[i] * Uf[j] * dinv;
          }
        } else if (half == 0) {
          // the floating base: Cholesky factor of its 6 x 6 articulated inertia [[IA, IH], [IH^T, IM]], lower triangle row by
          // row, the diagonal as its reciprocal
          float G[6][6], L[6][6];
          const float Af[9] = {IA[0], IA[1], IA[2], IA[1], IA[3], IA[4], IA[2], IA[4], IA[5]};
          const float Mf[9] = {IM[0], IM[1], IM[2], IM[1], IM[3], IM[4], IM[2], IM[4], IM[5]};
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
              G[i][j] = Af[3 * i + j]; G[3 + i][3 + j] = Mf[3 * i + j];
              G[i][3 + j] = IH[3 * i + j]; G[3 + j][i] = IH[3 * i + j];
            }
#pragma unroll
          for (int j = 0; j < 6; j++) {
            float sd = G[j][j];
#pragma unroll
            for (int x = 0; x < j; x++) sd -= L[j][x] * L[j][x];
            const float inv = 1.0f / sqrtf(sd);
            L[j][j] = inv;
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
              float sv = G[i][j];
#pragma unroll
              for (int x = 0; x < j; x++) sv -= L[i][x] * L[j][x];
              L[i][j] = sv * inv;
            }
          }
#pragma unroll
          for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) o[i * (i + 1) / 2 + j] = L[i][j];
        }
      }
      __syncthreads();
    }
    // ---- passes 2 and 3, once per right-hand side: two at a time, one in each half of the wave
    float *my = rec + RS * b + R_SLOT + 6 * half;
    for (int k0 = 0; k0 < K; k0 += 2) {
      const int col = k0 + half;
      const bool act = is_body && col < K;
      const float *row = nullptr;
      if constexpr (FD) row = A.rhs ? A.rhs + (size_t)e * D : nullptr;
      else row = A.rhs ? A.rhs + ((size_t)e * K + (act ? col : 0)) * D : nullptr;
      float tau = 0.f, bf[3] = {0.f, 0.f, 0.f}, bn[3] = {0.f, 0.f, 0.f};     // this body's share of the right-hand side
      if (act) {
        if (b >= 1) {
          tau = row ? row[slot] : !FD && col == slot ? 1.f : 0.f;
        } else {
#pragma unroll
          for (int c = 0; c < 3; c++) {
            bf[c] = row ? row[c] : !FD && col == c ? 1.f : 0.f;
            bn[c] = row ? row[3 + c] : !FD && col == 3 + c ? 1.f : 0.f;
          }
        }
      }
      // pass 2, inward: bias wrench of the subtree with its joints free, p^a = p^A + U (tau - S . p^A) / d
      float pn[3] = {N[0], N[1], N[2]}, pf[3] = {F[0], F[1], F[2]}, u = 0.f;
      for (int d = maxdepth; d >= 0; d--) {
        if (depth == d && act) {
          for (int kc = 0; kc < MAXCH; kc++) {
            const int ch = M->child[kc][b];
            if (ch < 0) break;
            const float *o = rec + RS * ch;
            const float *w = o + R_SLOT + 6 * half;
            const float l[3] = {o[R_ORG] - k.r[0], o[R_ORG + 1] - k.r[1], o[R_ORG + 2] - k.r[2]}, fc[3] = {w[3], w[4], w[5]};
            float lxf[3];
            cross3(l, fc, lxf);
#pragma unroll
            for (int c = 0; c < 3; c++) { pf[c] += fc[c]; pn[c] += w[c] + lxf[c]; }
          }
          if (b >= 1) {
            u = tau - dot3(k.a, pn);
            const float ud = u * dinv;
#pragma unroll
            for (int c = 0; c < 3; c++) { my[c] = pn[c] + Un[c] * ud; my[3 + c] = pf[c] + Uf[c] * ud; }
          } else {
            // the base: I^A_0 da_0 = (base torque, base force) - p^A_0 by the Cholesky factor
            const float *Lr = rec;
            float y[6] = {bn[0] - pn[0], bn[1] - pn[1], bn[2] - pn[2], bf[0] - pf[0], bf[1] - pf[1], bf[2] - pf[2]};
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
              for (int x = 0; x < i; x++) y[i] -= Lr[i * (i + 1) / 2 + x] * y[x];
              y[i] *= Lr[i * (i + 1) / 2 + i];
            }
#pragma unroll
            for (int i = 5; i >= 0; i--) {
#pragma unroll
              for (int x = i + 1; x < 6; x++) y[i] -= Lr[x * (x + 1) / 2 + i] * y[x];
              y[i] *= Lr[i * (i + 1) / 2 + i];
            }
#pragma unroll
            for (int c = 0; c < 3; c++) { my[c] = y[c]; my[3 + c] = y[3 + c]; stage[col * D + c] = y[3 + c]; stage[col * D + 3 + c] = y[c]; }
          }
        }
        __syncthreads();
      }
      // pass 3, outward: da of the parent moved to this origin, qdd = (u - U . da) / d, da += S qdd
      for (int d = 1; d <= maxdepth; d++) {
        if (depth == d && act) {
          const float *w = rec + RS * M->parent[b] + R_SLOT + 6 * half;
          float al[3] = {w[0], w[1], w[2]}, ap[3];
          cross3(al, lev, ap);
#pragma unroll
          for (int c = 0; c < 3; c++) ap[c] += w[3 + c];
          const float qdd = (u - dot3(Un, al) - dot3(Uf, ap)) * dinv;
#pragma unroll
          for (int c = 0; c < 3; c++) { my[c] = al[c] + k.a[c] * qdd; my[3 + c] = ap[c]; }
          stage[col * D + slot] = qdd;
        }
        __syncthreads();
      }
    }
  }

  __syncthreads();
  const int envs_here = min(WAVES, A.n_envs - env0);
  block_store(A.out + (size_t)env0 * per_env, lds + WAVES * trex_dyn_body_floats(Q), envs_here * per_env);
}

}  // namespace

extern "C" hipError_t trex_launch_dynamics(const TrexDynArgs &args, int query, hipStream_t stream) {
  if (args.n_envs <= 0 || args.nb < 1 || args.nb > TL) return hipErrorInvalidValue;
  const int D = 6 + args.nb - 1;
  const dim3 grid((args.n_envs + WAVES - 1) / WAVES), block(BLOCK);
  if (query == TREX_DYN_SOLVE_MASS && (args.num_rhs < 1 || args.num_rhs > TREX_DYN_MAX_RHS)) return hipErrorInvalidValue;
  const size_t lds = (size_t)trex_dyn_lds_bytes(query, D, args.num_rhs);
  switch (query) {
    case TREX_DYN_INVERSE_DYNAMICS: hipLaunchKernelGGL(trex_dynamics_kernel<TREX_DYN_INVERSE_DYNAMICS>, grid, block, lds, stream, args); break;
    case TREX_DYN_MASS_MATRIX: hipLaunchKernelGGL(trex_dynamics_kernel<TREX_DYN_MASS_MATRIX>, grid, block, lds, stream, args); break;
    case TREX_DYN_JACOBIAN: hipLaunchKernelGGL(trex_dynamics_kernel<TREX_DYN_JACOBIAN>, grid, block, lds, stream, args); break;
    case TREX_DYN_CENTROIDAL: hipLaunchKernelGGL(trex_dynamics_kernel<TREX_DYN_CENTROIDAL>, grid, block, lds, stream, args); break;
    case TREX_DYN_FORWARD_DYNAMICS: hipLaunchKernelGGL(trex_dynamics_kernel<TREX_DYN_FORWARD_DYNAMICS>, grid, block, lds, stream, args); break;
    case TREX_DYN_SOLVE_MASS: hipLaunchKernelGGL(trex_dynamics_kernel<TREX_DYN_SOLVE_MASS>, grid, block, lds, stream, args); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
