// Motion clip (include/trex_motion.h): the reference state of every env at a time of the clip (sample), the tracking terms against it
// composed into the reward column (compose), and reference state initialisation (reset). A workgroup of 256 lanes serves 8 whole
// envs, 32 lanes each, as observation.hip and reward.hip do.
//
// Phase 0, all three launches: the 32 lanes of a slot map the env's time to a segment of the clip (the same arithmetic in every
// lane: the segment differs from env to env, so the two rows are vector loads, 16-byte aligned and read-only) and interpolate
// columns l, l + 32, l + 64 of the state row into LDS; every lane forms the slerp itself, it is 30 operations.
// Phase 1, sample with points and compose with END_EFFECTOR: lane r < 18 of a slot walks one chain (chain_walk.h) - probe k's body
// at the state (r = k) or at the reference (r = 8 + k), URDF link 0's body at either (16, 17) - and parks R | origin in LDS. The
// reference walk reads its base row and joint angles from LDS in the layout of the batch's arrays.
// Phase 2: lane j holds joint j, lane k probe k, lane t term t's held value; sums over a slot go through a fixed shuffle tree, so
// a value is bitwise repeatable. The interpolation is written with explicit fmaf: the three launches give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/trex_batch.h"
#include "chain_walk.h"
#include "device_math.h"
#include "motion.h"

namespace {

constexpr int BLOCK = TREX_MOT_BLOCK;
constexpr int MAXENV = TREX_MOT_MAXENV;
constexpr int REF = TREX_MOT_REF;
constexpr int REC = TREX_MOT_REC;
constexpr int ROLES = TREX_MOT_ROLES;
constexpr int TL = TREX_TL;
constexpr int MAXK = TREX_MOT_MAXPROBES;
static_assert(BLOCK == MAXENV * TL, "32 lanes per env slot");
static_assert(TREX_MOT_COLS(TL - 1) <= REF && REF <= 3 * TL, "a lane interpolates at most three columns");
static_assert(ROLES == 2 * MAXK + 2 && ROLES <= TL && TREX_MOT_MAXTERMS <= TL, "one lane per chain, per term");

__device__ __forceinline__ float slot_sum(float x) {
#pragma unroll
  for (int o = TL / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, TL);
  return x;
}

// a time of the clip: segment k, u in [0, 1] along it, completed cycles, phase
struct ClipTime { int k; float u, cycles, phase; };

__device__ __forceinline__ ClipTime map_time(const TrexMotArgs &a, float t) {
  const float T = a.duration;
  if (!(t > 0.f)) t = 0.f;
  t = fminf(t, 1.0e30f);
  float cycles = 0.f, tw = t;
  if (a.loop) {
    cycles = floorf(t * a.inv_duration);
    tw = fmaf(-cycles, T, t);
    if (tw < 0.f) { tw += T; cycles -= 1.f; }
    if (tw >= T) { tw -= T; cycles += 1.f; }
  }
  tw = fminf(fmaxf(tw, 0.f), T);   // (also: past the end of a clip that does not loop)
  const float s = tw * a.inv_dt;
  ClipTime c;
  c.k = max(0, min((int)s, a.frames - 2));
  c.u = fminf(fmaxf(s - (float)c.k, 0.f), 1.f);
  c.cycles = cycles;
  c.phase = fminf(tw * a.inv_duration, 1.f);
  return c;
}

// shortest-arc slerp of the quaternions of rows r0, r1 (columns 3..6); normalised lerp where they are closer than acos 0.9995
__device__ __forceinline__ void ref_quat(const float *__restrict__ r0, const float *__restrict__ r1, float u, float *o) {
  const float ax = r0[3], ay = r0[4], az = r0[5], aw = r0[6];
  float bx = r1[3], by = r1[4], bz = r1[5], bw = r1[6];
  float d = fmaf(ax, bx, fmaf(ay, by, fmaf(az, bz, aw * bw)));
  if (d < 0.f) { d = -d; bx = -bx; by = -by; bz = -bz; bw = -bw; }
  float w0 = 1.f - u, w1 = u;
  const bool near = d > 0.9995f;
  if (!near) {
    const float th = acosf(d), sn = sinf(th);
    w0 = sinf(w0 * th) / sn;
    w1 = sinf(u * th) / sn;
  }
  float x = fmaf(w1, bx, w0 * ax), y = fmaf(w1, by, w0 * ay), z = fmaf(w1, bz, w0 * az), w = fmaf(w1, bw, w0 * aw);
  if (near) {
    const float inv = 1.f / sqrtf(fmaf(x, x, fmaf(y, y, fmaf(z, z, w * w))));
    x *= inv; y *= inv; z *= inv; w *= inv;
  }
  o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

// phase 0: the slot's lanes fill ref [13 + 2J] with the clip's state at c (l: the lane of the slot)
__device__ __forceinline__ void fill_reference(const TrexMotArgs &a, const ClipTime &c, int l, float *ref) {
  const float *__restrict__ r0 = a.table + (size_t)c.k * a.stride, *__restrict__ r1 = r0 + a.stride;
  const int cols = TREX_MOT_COLS(a.nj);
  float quat[4];
  ref_quat(r0, r1, c.u, quat);
  const float w0 = 1.f - c.u;
  for (int col = l; col < cols; col += TL) {
    float v = fmaf(c.u, r1[col], w0 * r0[col]);
    if (col < 2) v = fmaf(c.cycles, a.disp[col], v);
    if (col >= 3 && col < 7) v = quat[col - 3];
    ref[col] = v;
  }
}

// the slot's reference joint angles by BODY lane, as walk_chain reads the batch's q array
__device__ __forceinline__ void fill_reference_q(const TrexDeviceModel *M, int l, const float *ref, float *qb) {
  qb[l] = (l >= 1 && l < M->nb) ? ref[13 + M->obs_slot[l]] : 0.f;
}

// phase 1: the chain of role r (motion.h) of env `env`; the reference roles read the slot's LDS rows. rec: the slot's records
__device__ __forceinline__ void walk_role(const TrexMotArgs &a, int env, int r, bool with_state, const float *ref, const float *qb, float *rec) {
  const bool at_ref = r == 2 * MAXK + 1 || (r >= MAXK && r < 2 * MAXK);
  const int probe = r < MAXK ? r : r - MAXK;
  if (r >= ROLES || (r < 2 * MAXK && probe >= a.num_probes) || (!at_ref && !with_state)) return;
  const int body = r < 2 * MAXK ? a.probe_body[probe] : a.base_body;
  const float *none = nullptr;
  const float *base_rows = at_ref ? ref : (const float *)a.base, *q = at_ref ? qb : (const float *)a.q;
  Walk k;
  walk_chain<false, false>(a.model, base_rows, q, none, none, at_ref ? 0 : env, body, 0, k);
  float *o = rec + r * REC;
#pragma unroll
  for (int c = 0; c < 9; c++) o[c] = k.R[c];
#pragma unroll
  for (int c = 0; c < 3; c++) o[9 + c] = k.r[c];
}

// probe `p` relative to URDF link 0's origin in its axes, from the records P of the probe's body and P0 of link 0's body: the
// TREX_AXES_BASE position of link_state.hip
__device__ __forceinline__ void probe_in_base(const TrexMotArgs &a, const float *P, const float *P0, int p, float *out) {
  float A[9], e0[3], d[3], e[3];
  matmul3(P0, a.base_tf, A);
  matvec3(P0, a.base_tf + 9, e0);
  matvec3(P, a.probe_tf + 12 * (size_t)p + 9, d);
#pragma unroll
  for (int c = 0; c < 3; c++) e[c] = (P[9 + c] - (e0[c] + P0[9 + c])) + d[c];
#pragma unroll
  for (int c = 0; c < 3; c++) out[c] = A[c] * e[0] + A[3 + c] * e[1] + A[6 + c] * e[2];
}

}  // namespace

__global__ __launch_bounds__(256) void trex_motion_sample_kernel(TrexMotArgs a) {
  __shared__ __attribute__((aligned(16))) float sRef[MAXENV * REF];
  __shared__ float sQ[MAXENV * TL];
  __shared__ float sRec[MAXENV * ROLES * REC];
  const int s = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int env = blockIdx.x * MAXENV + s;
  const bool live = env < a.n_envs;
  float *ref = sRef + s * REF, *qb = sQ + s * TL, *rec = sRec + s * ROLES * REC;
  ClipTime c{};
  if (live) {
    const float t = a.time ? a.time[env] : fmaf((float)a.k[env], a.Ts, a.t0[env]);
    c = map_time(a, t);
    fill_reference(a, c, l, ref);
  }
  __syncthreads();
  if (live) {
    if (a.state_out) {
      const int cols = TREX_MOT_COLS(a.nj);
      for (int col = l; col < cols; col += TL) a.state_out[(size_t)env * cols + col] = ref[col];
    }
    if (a.phase_out && l == 0) a.phase_out[env] = c.phase;
  }
  if (!a.points_out) return;   // (uniform over the launch)
  if (live) fill_reference_q(a.model, l, ref, qb);
  __syncthreads();
  if (live) walk_role(a, env, l, false, ref, qb, rec);
  __syncthreads();
  if (live && l < a.num_probes) {
    const float *P = rec + (MAXK + l) * REC;
    float d[3];
    matvec3(P, a.probe_tf + 12 * (size_t)l + 9, d);
    float *w = a.points_out + ((size_t)env * a.num_probes + l) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] = (ref[k] + P[9 + k]) + d[k];
  }
}

__global__ __launch_bounds__(256) void trex_motion_compose_kernel(TrexMotArgs a) {
  __shared__ __attribute__((aligned(16))) float sRef[MAXENV * REF];
  __shared__ float sQ[MAXENV * TL];
  __shared__ float sRec[MAXENV * ROLES * REC];
  const int s = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int env = blockIdx.x * MAXENV + s;
  const bool live = env < a.n_envs;
  const int J = a.nj, T = a.num_terms;
  float *ref = sRef + s * REF, *qb = sQ + s * TL, *rec = sRec + s * ROLES * REC;
  float *row = a.rows + (size_t)(live ? env : 0) * a.row_stride;
  bool done = false, effectors = false;
  int k_new = 0;
#pragma unroll
  for (int t = 0; t < TREX_MOT_MAXTERMS; t++) effectors |= t < T && a.term[t].kind == TREX_MOT_END_EFFECTOR;
  if (live) {
    done = row[3 * J + 1] != 0.f;
    k_new = a.k[env] + 1;
    fill_reference(a, map_time(a, fmaf((float)k_new, a.Ts, a.t0[env])), l, ref);
  }
  if (effectors) {   // (uniform over the launch)
    __syncthreads();
    if (live) fill_reference_q(a.model, l, ref, qb);
    __syncthreads();
    if (live && !done) walk_role(a, env, l, true, ref, qb, rec);
  }
  __syncthreads();
  if (!live) return;

  const bool joint = l < J;
  const float q = joint ? row[l] : 0.f, qd = joint ? row[J + l] : 0.f;
  const float qr = joint ? ref[13 + l] : 0.f, qdr = joint ? ref[13 + J + l] : 0.f;
  const float held = l < T ? a.held[(size_t)env * T + l] : 0.f;
  const float *b = a.base + (size_t)env * 16;
  float ee = 0.f;   // this lane's probe: |r_k - r^_k|^2
  if (effectors && !done && l < a.num_probes) {
    float pa[3], pr[3];
    probe_in_base(a, rec + l * REC, rec + 2 * MAXK * REC, l, pa);
    probe_in_base(a, rec + (MAXK + l) * REC, rec + (2 * MAXK + 1) * REC, l, pr);
    const float dx = pa[0] - pr[0], dy = pa[1] - pr[1], dz = pa[2] - pr[2];
    ee = dx * dx + dy * dy + dz * dz;
  }

  float sum = a.step_weight * row[3 * J];
  asm volatile("" : "+v"(sum));   // the rounded product, in a register: no addition below can be contracted into it
  float my_product = 0.f, my_value = 0.f;
  for (int t = 0; t < T; t++) {
    const TrexMotTerm &tm = a.term[t];
    const bool bit = joint && ((tm.mask >> l) & 1u);
    const float held_t = __shfl(held, t, TL);
    float v;
    switch (tm.kind) {
      case TREX_MOT_POSE: v = expf(-tm.scale * slot_sum(bit ? (q - qr) * (q - qr) : 0.f)); break;
      case TREX_MOT_VELOCITY: v = expf(-tm.scale * slot_sum(bit ? (qd - qdr) * (qd - qdr) : 0.f)); break;
      case TREX_MOT_END_EFFECTOR: v = expf(-tm.scale * slot_sum(ee)); break;
      case TREX_MOT_ROOT_POSE: {
        const float dx = b[0] - ref[0], dy = b[1] - ref[1], dz = b[2] - ref[2];
        // base^-1 o reference: w = the dot product, vector part w_a v_b - w_b v_a - v_a x v_b; theta = 2 atan2(|vector|, |w|)
        const float av[3] = {b[3], b[4], b[5]}, bv[3] = {ref[3], ref[4], ref[5]}, aw = b[6], bw = ref[6];
        float cr[3];
        cross3(av, bv, cr);
        const float vx = aw * bv[0] - bw * av[0] - cr[0], vy = aw * bv[1] - bw * av[1] - cr[1], vz = aw * bv[2] - bw * av[2] - cr[2];
        const float w = aw * bw + dot3(av, bv);
        const float theta = 2.f * atan2f(sqrtf(vx * vx + vy * vy + vz * vz), fabsf(w));
        v = expf(-tm.scale * ((dx * dx + dy * dy + dz * dz) + tm.aux * (theta * theta)));
        break;
      }
      default: {   // ROOT_VELOCITY
        const float dx = b[7] - ref[7], dy = b[8] - ref[8], dz = b[9] - ref[9];
        const float wx = b[10] - ref[10], wy = b[11] - ref[11], wz = b[12] - ref[12];
        v = expf(-tm.scale * ((dx * dx + dy * dy + dz * dz) + tm.aux * (wx * wx + wy * wy + wz * wz)));
      }
    }
    if (done) v = held_t;   // the state is the new episode's: the step before, again
    float product = tm.weight * v;
    asm volatile("" : "+v"(product));
    sum += product;
    if (l == t) { my_product = product; my_value = v; }
  }
  if (l < T) {
    const size_t at = (size_t)env * T + l;
    if (a.terms_out) a.terms_out[at] = my_product;
    a.held[at] = done ? 0.f : my_value;
  }
  if (l == 0) {
    row[3 * J] = sum;
    a.k[env] = done ? 0 : k_new;
    if (done) a.t0[env] = 0.f;
  }
}

__global__ __launch_bounds__(256) void trex_motion_reset_kernel(TrexMotArgs a) {
  __shared__ __attribute__((aligned(16))) float sRef[MAXENV * REF];
  const int s = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int env = blockIdx.x * MAXENV + s;
  const bool live = env < a.n_envs && (!a.mask || a.mask[env] != 0);
  float *ref = sRef + s * REF;
  float t = 0.f;
  if (live) {
    t = a.time ? a.time[env] : 0.f;
    if (!(t > 0.f)) t = 0.f;
    fill_reference(a, map_time(a, t), l, ref);
  }
  __syncthreads();
  if (!live) return;
  const TrexDeviceModel *M = a.model;
  const int J = a.nj, T = a.num_terms;
  float *b = a.base + (size_t)env * 16;
  if (l < 13) b[l] = ref[l];
  if (l == TREX_BASE_FLAGS) b[l] = __int_as_float(__float_as_int(b[l]) | TREX_MOTORS_BIT);
  const bool body = l >= 1 && l < M->nb;
  const int slot = body ? M->obs_slot[l] : 0;
  a.q[(size_t)env * TL + l] = body ? ref[13 + slot] : 0.f;
  a.qd[(size_t)env * TL + l] = body ? ref[13 + J + slot] : 0.f;
  if (a.warm) {
    float *w = a.warm + (size_t)env * TREX_WARM_WORDS;
    for (int c = l; c < TREX_WARM_WORDS; c += TL) w[c] = 0.f;
  }
  if (a.held && l < T) a.held[(size_t)env * T + l] = 0.f;
  if (l == 0) { a.t0[env] = t; a.k[env] = 0; }
  if (a.rows && l < J) {
    float *row = a.rows + (size_t)env * a.row_stride;
    row[l] = ref[13 + l]; row[J + l] = ref[13 + J + l]; row[2 * J + l] = 0.f;
  }
}

namespace {
dim3 grid_of(const TrexMotArgs &a) { return dim3((unsigned)((a.n_envs + MAXENV - 1) / MAXENV)); }
}  // namespace

extern "C" hipError_t trex_launch_motion_sample(const TrexMotArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(trex_motion_sample_kernel, grid_of(args), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_motion_compose(const TrexMotArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(trex_motion_compose_kernel, grid_of(args), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_motion_reset(const TrexMotArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(trex_motion_reset_kernel, grid_of(args), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}
