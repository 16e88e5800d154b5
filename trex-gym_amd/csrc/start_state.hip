// Start-state randomisation (trex_batch_apply_start_state / _start_state_reset, include/trex_start_state.h, which states the
// semantics and the random numbers): K20. One launch perturbs the state that an episode start left - joint angles, joint velocities,
// base attitude, base velocity, base position - and places the robot on the floor.
//
// Shape of the apply launch: one env per wavefront, one wavefront per workgroup, as termination.hip, whose chain walk and point
// sweep the floor placement shares (clearance_sweep.h). Every lane reads the env's done flag and its started word in the same
// instructions; a wave whose env is not starting ends there. A starting env: lane b draws the elements of body b's joint and
// writes q, qd and the row's columns of that joint; lane t draws the one value of term t where that is a base kind or the
// clearance, and the wave hands those round with readlanes, so that every lane composes the base row in registers and lane 0
// writes it. With a clearance term the wave then walks the chains from the state it has just written - a workgroup-scope fence and
// a barrier stand between the stores and the loads of the walk -, sweeps all collision points, takes the minimum over the bodies
// and lane 0 writes the shifted base z. LDS: the poses and minima of the sweep; no scratch.
#include "start_state.h"

#include "clearance_sweep.h"
#include "philox.h"

namespace {

constexpr int BLOCK = TREX_START_BLOCK, TL = TREX_TL;
static_assert(BLOCK == TREX_TERM_BLOCK, "the sweep of clearance_sweep.h strides by TREX_TERM_BLOCK lanes");
static_assert(TREX_WARM_WORDS == BLOCK, "one lane empties one word of the warm-start record");
static_assert(TREX_START_MAXTERMS <= BLOCK, "lane t draws the base value of term t");

__global__ __launch_bounds__(BLOCK) void trex_start_state_kernel(TrexStartArgs a) {
  __shared__ __attribute__((aligned(16))) float sPose[TL * CLR_POSE];
  __shared__ int sStart[TL + 1];
  __shared__ unsigned long long sBest[TL];

  const int t = threadIdx.x, env = blockIdx.x;
  const TrexStartState &s = a.st;
  const bool first = a.done[(size_t)env * a.done_stride] != 0.f || s.started[env] == 0u;
  if (!first) return;   // (wave-uniform: the whole workgroup leaves)
  const uint32_t ep = s.ep[env] + 1u;
  if (t == 0) { s.ep[env] = ep; s.started[env] = 1u; }

  const TrexStartTable &tab = *a.table;
  const TrexDeviceModel *M = a.model;
  const int T = tab.num_terms, nb = M->nb, J = a.nj;
  const uint32_t eid = a.env_offset + (uint32_t)env;
  const bool body = t >= 1 && t < nb;   // (nb <= TREX_TL: a body lane indexes the model's per-body arrays)
  const int joint = body ? M->obs_slot[t] : -1;
  float q = 0.f, qd = 0.f;
  if (body) { q = a.q[(size_t)env * TL + t]; qd = a.qd[(size_t)env * TL + t]; }

  // ---- the draws: lane b the element of body b's joint, lane k element 0 of a base or clearance term k
  float mine = 0.f;
  for (int k = 0; k < T; k++) {
    const TrexStartTerm term = tab.term[k];
    const int i = term.kind <= TREX_START_JOINT_VELOCITY ? joint : (t == k ? 0 : -1);
    if (i < 0 || !((term.mask >> i) & 1u)) continue;
    const int src = term.shared ? 0 : i;
    uint32_t r[4];
    philox(eid, 0u, ((uint32_t)TREX_START_STREAM << 16) | (uint32_t)(8 * k + (src >> 2)), ep, a.key0, a.key1, r);
    const uint32_t pick = (src & 2) ? ((src & 1) ? r[3] : r[2]) : ((src & 1) ? r[1] : r[0]);
    const float v = uniform(term.lo, term.hi, pick);
    s.values[((size_t)env * T + k) * TL + i] = v;
    if (term.kind == TREX_START_JOINT_POSITION) q = fminf(fmaxf(q + v, M->lower[t]), M->upper[t]);
    else if (term.kind == TREX_START_JOINT_VELOCITY) qd = qd + v;
    else mine = v;
  }
  if (body) {
    a.q[(size_t)env * TL + t] = q;
    a.qd[(size_t)env * TL + t] = qd;
    if (a.rows) {
      float *row = a.rows + (size_t)env * a.row_stride;
      row[joint] = q; row[J + joint] = qd; row[2 * J + joint] = 0.f;
    }
  }
  if (a.warm) a.warm[(size_t)env * TREX_WARM_WORDS + t] = 0.f;

  // ---- the base row, composed by every lane alike: the values by readlane, the offsets by kind and component
  float rpy[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f}, dw[3] = {0.f, 0.f, 0.f}, dp[3] = {0.f, 0.f, 0.f}, clearance = 0.f;
  uint32_t has_v = 0u, has_w = 0u, has_p = 0u;
  for (int k = 0; k < T; k++) {
    const float v = __shfl(mine, k);
    const int kind = tab.term[k].kind, index = tab.term[k].index;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (index != c) continue;
      if (kind == TREX_START_BASE_RPY) rpy[c] = v;
      if (kind == TREX_START_BASE_LINEAR_VELOCITY) { dv[c] = v; has_v |= 1u << c; }
      if (kind == TREX_START_BASE_ANGULAR_VELOCITY) { dw[c] = v; has_w |= 1u << c; }
      if (kind == TREX_START_BASE_POSITION) { dp[c] = v; has_p |= 1u << c; }
    }
    if (kind == TREX_START_FLOOR_CLEARANCE) clearance = v;
  }
  float *base = a.base + (size_t)env * 16;
  float p[3], quat[4], vl[3], va[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { p[c] = base[c]; vl[c] = base[7 + c]; va[c] = base[10 + c]; }
#pragma unroll
  for (int c = 0; c < 4; c++) quat[c] = base[3 + c];
  if (tab.rotate) {   // R = Rz(yaw) Ry(pitch) Rx(roll) about the base origin: r (x) quat, R v, R w
    const float cr = cosf(0.5f * rpy[0]), sr = sinf(0.5f * rpy[0]), cp = cosf(0.5f * rpy[1]), sp = sinf(0.5f * rpy[1]);
    const float cy = cosf(0.5f * rpy[2]), sy = sinf(0.5f * rpy[2]);
    const float r[4] = {sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy};
    const float x = r[3] * quat[0] + r[0] * quat[3] + r[1] * quat[2] - r[2] * quat[1];
    const float y = r[3] * quat[1] - r[0] * quat[2] + r[1] * quat[3] + r[2] * quat[0];
    const float z = r[3] * quat[2] + r[0] * quat[1] - r[1] * quat[0] + r[2] * quat[3];
    const float w = r[3] * quat[3] - r[0] * quat[0] - r[1] * quat[1] - r[2] * quat[2];
    const float norm = sqrtf(x * x + y * y + z * z + w * w);
    quat[0] = x / norm; quat[1] = y / norm; quat[2] = z / norm; quat[3] = w / norm;
    float R[9];
    quat_to_mat(r, R);
    matvec3(R, vl, vl);
    matvec3(R, va, va);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {   // (an offset is added only where a term names the component: the rest is as found, bit for bit)
    if ((has_v >> c) & 1u) vl[c] = rounded(vl[c]) + dv[c];
    if ((has_w >> c) & 1u) va[c] = rounded(va[c]) + dw[c];
    if ((has_p >> c) & 1u) p[c] = p[c] + dp[c];
  }
  if (t == 0) {
#pragma unroll
    for (int c = 0; c < 3; c++) { base[c] = p[c]; base[7 + c] = vl[c]; base[10 + c] = va[c]; }
#pragma unroll
    for (int c = 0; c < 4; c++) base[3 + c] = quat[c];
  }

  // ---- the floor placement, on the state as written: the lowest collision point to floor_z + clearance
  if (tab.clearance_term < 0) return;
  __threadfence_block();
  __syncthreads();
  TrexTermArgs ta;
  ta.model = M; ta.base = a.base; ta.q = a.q; ta.hull = a.hull;
  uint32_t low;
  float head_z;
  body_clearance<false>(ta, env, t, true, sPose, sStart, sBest, low, head_z);
  unsigned long long best = t < nb ? sBest[t] : ~0ull;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long other = __shfl_xor(best, off);
    best = other < best ? other : best;   // (the index rides in the low word: of two equal heights the earlier point wins)
  }
  if (t == 0) {
    const uint32_t point = (uint32_t)best;
    float shift = 0.f;
    int32_t lowest = -1;
    if (point != CLR_NO_POINT) {
      const float z = (M->prm[TP_FLOOR_Z] + clearance) - clr_ordered_float((uint32_t)(best >> 32));
      shift = z - p[2];
      lowest = (int32_t)point;
      base[2] = z;
    }
    s.shift[env] = shift;
    s.lowest[env] = lowest;
  }
}

__global__ void trex_start_state_reset_kernel(const uint8_t *mask, int n_envs, uint32_t *started) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  started[env] = 0u;
}

}  // namespace

extern "C" hipError_t trex_launch_start_state(const TrexStartArgs &args, hipStream_t stream) {
  hipLaunchKernelGGL(trex_start_state_kernel, dim3((unsigned)args.n_envs), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_start_state_reset(const uint8_t *mask, int n_envs, uint32_t *started, hipStream_t stream) {
  hipLaunchKernelGGL(trex_start_state_reset_kernel, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, stream, mask, n_envs, started);
  return hipGetLastError();
}
