// First-order derivatives of the inverse dynamics f = ID(q, v, a) = M(q) a + h(q, v) of dynamics.hip: dfdq [N, D, D] along the
// configuration tangent (base origin, WORLD-axis base rotation vector, joint angles; the numbers of the velocity and of the
// classical accelerations held fixed) and dfdv [N, D, D] along the generalised velocity. Read-only: nothing here writes the state.
// gfx950, the shape of dynamics.hip and joint_wrench.hip: one env per 64-lane wavefront, four envs per workgroup.
//
// A tangent (forward-mode) recursive Newton-Euler algorithm in the own-point formulation: everything in world axes relative to
// the base origin, forces at the COM, moments about the body's own joint origin, shifted to the parent by the short lever between
// the two origins. The nominal outward walk and the nominal inward subtree force and moment run once per env and stay in LDS
// ([component][body] records) and registers. The directions are then taken two at a time, one per lane half (body = lane & 31):
//   outward  every lane walks its chain base -> body over its ancestors' nominal records, carrying the tangents of the rotation
//            (d phi: dR = [d phi]x R), of the angular velocity and acceleration and of the origin's classical acceleration;
//   body     the tangent of the body's force at the COM and of its moment about its origin, [d phi]x Ic - Ic [d phi]x included;
//   inward   level by level through LDS, one wave-level barrier per level:
//            d N_parent += d N_child + d lever x F_child + lever x d F_child;
//   project  d tau_i = d axis_i . N_i + axis_i . d N_i; the base rows are the root's d F and d N.
// A velocity direction turns nothing (d phi = 0), so the same code is instantiated without the terms that d phi feeds. The three
// translation directions of either output are exact zeros (uniform gravity; Galilean invariance of the classical form) and are
// written without a pass. A joint direction k leaves every tangent outside the subtree of k an exact zero, so the entries that
// couple two joints of different branches come out as exact zeros too. A direction's arithmetic depends on nothing but the
// direction: not on its partner in the other lane half, not on its place in the sequence, not on which outputs were asked for.
// The outputs are staged per env in LDS, one row per direction, and leave the chip as whole contiguous blocks in either layout.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "dynamics_derivatives.h"

namespace {

constexpr int TL = TREX_TL;
constexpr int MAXD = TREX_MAXD;
constexpr int MAXCH = TREX_MAXCH;
constexpr int WAVES = TREX_DD_WAVES;
constexpr int BLOCK = 64 * WAVES;

// An env's records are its wavefront's own: LDS written by some lanes of the wave is read by others of the same wave. The wave's
// LDS operations execute in order, the fence keeps the compiler from moving them across; no workgroup barrier couples the four envs.
#define DD_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// components of a body's nominal record, [component][body]
enum { N_AXIS = 0, N_LEVER = 3, N_WP = 6, N_ALP = 9, N_QD = 12, N_QDD = 13, N_F = 14, N_N = 17, N_SLOT = 20 };
static_assert(TREX_DD_NOMINAL == 21, "the nominal record");
// ... of its tangent record in one direction
enum { T_F = 0, T_N = 3, T_LEVER = 6 };
static_assert(TREX_DD_TANGENT == 9, "the tangent record");

__device__ __forceinline__ void load3(const float *rec, int comp, int b, float *o) {
  o[0] = rec[(comp + 0) * TL + b]; o[1] = rec[(comp + 1) * TL + b]; o[2] = rec[(comp + 2) * TL + b];
}
__device__ __forceinline__ void store3(float *rec, int comp, int b, const float *v) {
  rec[(comp + 0) * TL + b] = v[0]; rec[(comp + 1) * TL + b] = v[1]; rec[(comp + 2) * TL + b] = v[2];
}

// what a lane keeps of its body from the nominal passes
struct Nominal {
  float a[3];        // joint axis
  float w[3], al[3]; // angular velocity and acceleration
  float cb[3];       // COM offset from the body origin
  float Ic[6];       // rotational inertia about the COM
  float Iw[3], Ial[3];
  float Fb[3];       // the body's own m a_c
  float Ns[3];       // subtree moment about the body origin
  float m;
  int anc[MAXD], child[MAXCH];
  int depth, slot;
};

// One direction. Q: a configuration direction (else a velocity direction). j: its index, 3 <= j < D: 3 .. 5 the base's world-axis
// rotation vector (its angular velocity), 6 + s the joint of observation slot s. nom: the env's nominal records, tan: this lane
// half's tangent records, row: the direction's staged row [D] or null (an idle half).
template <bool Q>
__device__ __forceinline__ void tangent_pass(const Nominal &k, const float *nom, float *tan, float *row, int j, int b, bool is_body,
                                             int maxdepth) {
  float dphi[3], dw[3], dal[3] = {0.f, 0.f, 0.f}, dao[3] = {0.f, 0.f, 0.f}, dd[3] = {0.f, 0.f, 0.f}, da[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float unit = j - 3 == c ? 1.f : 0.f;
    dphi[c] = Q ? unit : 0.f;
    dw[c] = Q ? 0.f : unit;
  }
  const int js = j - 6;
  // ---- outward, in registers: over the ancestors' nominal records, the parent's tangents in hand
#pragma unroll
  for (int d = 0; d < MAXD; d++) {
    if (d >= maxdepth) break;   // (wave-uniform)
    const int i = k.anc[d];
    if (i < 0) continue;
    float ai[3], lv[3], wp[3], alp[3];
    load3(nom, N_AXIS, i, ai); load3(nom, N_LEVER, i, lv); load3(nom, N_WP, i, wp); load3(nom, N_ALP, i, alp);
    const float qdi = nom[N_QD * TL + i], qddi = nom[N_QDD * TL + i];
    const float s = __float_as_int(nom[N_SLOT * TL + i]) == js ? 1.f : 0.f;
    // the origin: a_o = a_o,parent + al x lever + w x (w x lever), all of the parent
    float t0[3], t1[3], t2[3], wxl[3];
    cross3(wp, lv, wxl);
    if (Q) cross3(dphi, lv, dd);
    cross3(dal, lv, t0);
    cross3(dw, wxl, t1);
    cross3(dw, lv, t2);
    if (Q) {
      float u[3];
      cross3(wp, dd, u);
#pragma unroll
      for (int c = 0; c < 3; c++) t2[c] += u[c];
      cross3(alp, dd, u);
#pragma unroll
      for (int c = 0; c < 3; c++) t0[c] += u[c];
    }
    cross3(wp, t2, t2);
#pragma unroll
    for (int c = 0; c < 3; c++) dao[c] += t0[c] + t1[c] + t2[c];
    // the axis turns with the parent (a x a = 0); the joint's own angle turns the body about it
    if (Q) {
      cross3(dphi, ai, da);
#pragma unroll
      for (int c = 0; c < 3; c++) dphi[c] += ai[c] * s;
    }
    // al = al_parent + a qdd + (w_parent x a) qd
    float dwxa[3], wxa[3];
    cross3(dw, ai, dwxa);
    if (Q) {
      float u[3];
      cross3(wp, da, u);
#pragma unroll
      for (int c = 0; c < 3; c++) dal[c] += da[c] * qddi + (dwxa[c] + u[c]) * qdi;
    } else {
      cross3(wp, ai, wxa);
#pragma unroll
      for (int c = 0; c < 3; c++) dal[c] += dwxa[c] * qdi + wxa[c] * s;
    }
    // w = w_parent + a qd
#pragma unroll
    for (int c = 0; c < 3; c++) dw[c] += Q ? da[c] * qdi : ai[c] * s;
  }
  // ---- the body: F = m a_c at the COM, N = Ic al + w x Ic w + cb x F about its origin
  float dF[3], dN[3];
  {
    float dcb[3] = {0.f, 0.f, 0.f}, t0[3], t1[3], t2[3], u[3];
    if (Q) cross3(dphi, k.cb, dcb);
    cross3(dal, k.cb, t0);
    cross3(k.w, k.cb, u); cross3(dw, u, t1);
    cross3(dw, k.cb, t2);
    if (Q) {
      cross3(k.al, dcb, u);
#pragma unroll
      for (int c = 0; c < 3; c++) t0[c] += u[c];
      cross3(k.w, dcb, u);
#pragma unroll
      for (int c = 0; c < 3; c++) t2[c] += u[c];
    }
    cross3(k.w, t2, t2);
#pragma unroll
    for (int c = 0; c < 3; c++) dF[c] = k.m * (dao[c] + t0[c] + t1[c] + t2[c]);
    float Idal[3], Idw[3], dIw[3] = {0.f, 0.f, 0.f};
    sym3_mul(k.Ic, dal, Idal); sym3_mul(k.Ic, dw, Idw);
    if (Q) {   // d Ic x = d phi x (Ic x) - Ic (d phi x x)
      float v[3];
      cross3(dphi, k.w, u); sym3_mul(k.Ic, u, v); cross3(dphi, k.Iw, dIw);
#pragma unroll
      for (int c = 0; c < 3; c++) dIw[c] -= v[c];
      cross3(dphi, k.al, u); sym3_mul(k.Ic, u, v); cross3(dphi, k.Ial, u);
#pragma unroll
      for (int c = 0; c < 3; c++) Idal[c] += u[c] - v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) dIw[c] += Idw[c];
    cross3(dw, k.Iw, t0); cross3(k.w, dIw, t1); cross3(k.cb, dF, t2);
#pragma unroll
    for (int c = 0; c < 3; c++) dN[c] = Idal[c] + t0[c] + t1[c] + t2[c];
    if (Q) {
      cross3(dcb, k.Fb, u);
#pragma unroll
      for (int c = 0; c < 3; c++) dN[c] += u[c];
    }
  }
  // ---- inward, level by level: a body adds its children's tangents, their moments shifted by the lever child -> body
  if (is_body) { store3(tan, T_F, b, dF); store3(tan, T_N, b, dN); store3(tan, T_LEVER, b, dd); }
  DD_WSYNC();
  for (int d = maxdepth - 1; d >= 0; d--) {
    if (k.depth == d) {
      bool any = false;
#pragma unroll
      for (int kc = 0; kc < MAXCH; kc++) {
        const int ch = k.child[kc];
        if (ch < 0) break;
        float dFc[3], dNc[3], ddc[3], Fc[3], lv[3], t0[3], t1[3];
        load3(tan, T_F, ch, dFc); load3(tan, T_N, ch, dNc); load3(tan, T_LEVER, ch, ddc);
        load3(nom, N_F, ch, Fc); load3(nom, N_LEVER, ch, lv);
        cross3(ddc, Fc, t0); cross3(lv, dFc, t1);
#pragma unroll
        for (int c = 0; c < 3; c++) { dF[c] += dFc[c]; dN[c] += dNc[c] + t0[c] + t1[c]; }
        any = true;
      }
      if (any) { store3(tan, T_F, b, dF); store3(tan, T_N, b, dN); }
    }
    DD_WSYNC();
  }
  // ---- the direction's row of generalised forces
  if (is_body && row) {
    if (b == 0) {
#pragma unroll
      for (int c = 0; c < 3; c++) { row[c] = dF[c]; row[3 + c] = dN[c]; }
    } else {
      row[6 + k.slot] = dot3(da, k.Ns) + dot3(k.a, dN);
    }
  }
}

__global__ __launch_bounds__(BLOCK) void trex_dynamics_derivatives_kernel(TrexDdArgs A) {
  extern __shared__ float4 lds4[];
  float *lds = reinterpret_cast<float *>(lds4);
  const TrexDeviceModel *M = A.model;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int half = lane >> 5, body = lane & (TL - 1);
  const int env0 = blockIdx.x * WAVES, env = env0 + wave;
  const int nb = A.nb, D = 5 + nb, DD = D * D;
  const bool live = env < A.n_envs;                       // (a wave past the batch's end still meets the workgroup's barrier)
  const bool is_body = body < nb;
  const int b = is_body ? body : 0;
  const int e = live ? env : 0;
  float *nom = lds + wave * (TL * (TREX_DD_NOMINAL + 2 * TREX_DD_TANGENT));   // this env's nominal records [21][32]
  float *tan0 = nom + TL * TREX_DD_NOMINAL;                                   // its tangent records [2][9][32]
  float *tan = tan0 + half * TL * TREX_DD_TANGENT;
  float *stage = lds + WAVES * (TL * (TREX_DD_NOMINAL + 2 * TREX_DD_TANGENT));  // [outputs asked for][4][D][D], a row per direction
  float *stage_q = A.dfdq ? stage + wave * DD : nullptr;
  float *stage_v = A.dfdv ? stage + (A.dfdq ? WAVES * DD : 0) + wave * DD : nullptr;
  const int maxdepth = M->maxdepth;
  const bool writer = is_body && half == 0;               // (both halves hold the nominal values; one writes them)

  // ---- nominal outward (in registers): pose, classical velocity and acceleration, mass, COM offset, inertia
  Nominal k;
  float lever[3], wp[3] = {0.f, 0.f, 0.f}, alp[3] = {0.f, 0.f, 0.f}, F[3], N[3];
  {
    Walk kw;
    walk_chain<true, true>(M, A.base, A.q, A.qd, A.accel, e, b, D, kw);
    const float sc = A.mass_scale ? A.mass_scale[(size_t)e * TL + b] : 1.0f;
    k.m = M->mass[b] * sc;
    k.depth = is_body ? M->depth[b] : -1;
    k.slot = M->obs_slot[b];
#pragma unroll
    for (int d = 0; d < MAXD; d++) k.anc[d] = M->anc[d][b];
#pragma unroll
    for (int c = 0; c < MAXCH; c++) k.child[c] = M->child[c][b];
    const float comb[3] = {M->com[0][b], M->com[1][b], M->com[2][b]};
    matvec3(kw.R, comb, k.cb);
    {
      float in[6], t[9];
#pragma unroll
      for (int c = 0; c < 6; c++) in[c] = M->inertia[c][b];
      const float Ib[9] = {in[0], in[1], in[2], in[1], in[3], in[4], in[2], in[4], in[5]};
      matmul3(kw.R, Ib, t);
      const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
      for (int c = 0; c < 6; c++)
        k.Ic[c] = sc * (t[3 * ia[c]] * kw.R[3 * ib[c]] + t[3 * ia[c] + 1] * kw.R[3 * ib[c] + 1] + t[3 * ia[c] + 2] * kw.R[3 * ib[c] + 2]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { k.a[c] = kw.a[c]; k.w[c] = kw.w[c]; k.al[c] = kw.al[c]; }
    // the parent's pose and motion, through the (still unused) tangent records: [R 9, w 3, al 3][32]
    if (writer) {
#pragma unroll
      for (int c = 0; c < 9; c++) tan0[c * TL + b] = kw.R[c];
      store3(tan0, 9, b, kw.w); store3(tan0, 12, b, kw.al);
    }
    DD_WSYNC();
    if (b > 0) {
      const int pa = M->parent[b];
      float Rp[9];
#pragma unroll
      for (int c = 0; c < 9; c++) Rp[c] = tan0[c * TL + pa];
      const float jp[3] = {M->jpos[0][b], M->jpos[1][b], M->jpos[2][b]};
      matvec3(Rp, jp, lever);
      load3(tan0, 9, pa, wp); load3(tan0, 12, pa, alp);
    } else {
      lever[0] = lever[1] = lever[2] = 0.f;
    }
    // the force at the COM and the moment about the body's joint origin that this motion needs
    float t0[3], t1[3], wIw[3], cxf[3];
    cross3(kw.al, k.cb, t0);
    cross3(kw.w, k.cb, t1); cross3(kw.w, t1, t1);
#pragma unroll
    for (int c = 0; c < 3; c++) { k.Fb[c] = k.m * (kw.ao[c] + t0[c] + t1[c]); F[c] = k.Fb[c]; }
    sym3_mul(k.Ic, kw.w, k.Iw); sym3_mul(k.Ic, kw.al, k.Ial);
    cross3(kw.w, k.Iw, wIw); cross3(k.cb, F, cxf);
#pragma unroll
    for (int c = 0; c < 3; c++) N[c] = k.Ial[c] + wIw[c] + cxf[c];
    if (writer) {
      store3(nom, N_AXIS, b, kw.a); store3(nom, N_LEVER, b, lever); store3(nom, N_WP, b, wp); store3(nom, N_ALP, b, alp);
      nom[N_QD * TL + b] = b > 0 ? A.qd[(size_t)e * TL + b] : 0.f;
      nom[N_QDD * TL + b] = b > 0 && A.accel ? A.accel[(size_t)e * D + 6 + k.slot] : 0.f;
      nom[N_SLOT * TL + b] = __int_as_float(k.slot);
      store3(nom, N_F, b, F); store3(nom, N_N, b, N);
    }
  }
  DD_WSYNC();
  // ---- nominal inward: subtree force, and subtree moment about the body's own origin
  for (int d = maxdepth - 1; d >= 0; d--) {
    if (k.depth == d) {
      bool any = false;
#pragma unroll
      for (int kc = 0; kc < MAXCH; kc++) {
        const int ch = k.child[kc];
        if (ch < 0) break;
        float Fc[3], Nc[3], lv[3], lxf[3];
        load3(nom, N_F, ch, Fc); load3(nom, N_N, ch, Nc); load3(nom, N_LEVER, ch, lv);
        cross3(lv, Fc, lxf);
#pragma unroll
        for (int c = 0; c < 3; c++) { F[c] += Fc[c]; N[c] += Nc[c] + lxf[c]; }
        any = true;
      }
      if (any && writer) { store3(nom, N_F, b, F); store3(nom, N_N, b, N); }
    }
    DD_WSYNC();
  }
#pragma unroll
  for (int c = 0; c < 3; c++) k.Ns[c] = N[c];

  // ---- the translation directions: exact zeros, no pass
  for (int i = lane; i < 3 * D; i += 64) {
    if (stage_q) stage_q[i] = 0.f;
    if (stage_v) stage_v[i] = 0.f;
  }
  // ---- the other D - 3 directions of either output, two per pass
  if (stage_q)
    for (int j0 = 3; j0 < D; j0 += 2) {
      const int j = j0 + half;
      tangent_pass<true>(k, nom, tan, j < D ? stage_q + j * D : nullptr, j < D ? j : 3, b, is_body, maxdepth);
    }
  if (stage_v)
    for (int j0 = 3; j0 < D; j0 += 2) {
      const int j = j0 + half;
      tangent_pass<false>(k, nom, tan, j < D ? stage_v + j * D : nullptr, j < D ? j : 3, b, is_body, maxdepth);
    }
  __syncthreads();
  // ---- the workgroup's envs lie back to back in either output: whole blocks, transposed on the way where rows are asked for
  const int count = min(WAVES, A.n_envs - env0) * DD;
  const float *src = stage;
  for (int o = 0; o < 2; o++) {
    float *out = o == 0 ? A.dfdq : A.dfdv;
    if (!out) continue;
    float *dst = out + (size_t)env0 * DD;
    for (int idx = threadIdx.x; idx < count; idx += BLOCK) {
      int at = idx;
      if (!A.by_direction) {
        const int en = idx / DD, r = idx - en * DD, i = r / D, jd = r - i * D;
        at = en * DD + jd * D + i;
      }
      dst[idx] = src[at];
    }
    src += WAVES * DD;
  }
}

}  // namespace

extern "C" hipError_t trex_launch_dynamics_derivatives(const TrexDdArgs &args, hipStream_t stream) {
  if (args.n_envs <= 0 || args.nb < 2 || args.nb > TL || (!args.dfdq && !args.dfdv)) return hipErrorInvalidValue;
  const dim3 grid((args.n_envs + WAVES - 1) / WAVES), block(BLOCK);
  const int outputs = (args.dfdq ? 1 : 0) + (args.dfdv ? 1 : 0);
  const size_t lds = (size_t)trex_dd_lds_bytes(args.nb, outputs);
  hipLaunchKernelGGL(trex_dynamics_derivatives_kernel, grid, block, lds, stream, args);
  return hipGetLastError();
}
