// Episode randomisation (trex_batch_apply_randomization / _randomization_reset, include/trex_randomize.h, which states the
// semantics and the random numbers): K14. One launch redraws what an episode start or an interval redraws - mass scale, friction,
// motor gains, pushes, the velocity command - into the buffers the step launches read.
//
// Shape of the apply launch: an env is a team of TREX_TL = 32 lanes, two envs to a wavefront, eight to a 256-thread workgroup. Lane b
// owns body b - the inner index of the mass scale, the gains and the wrench, so a first row's stores coalesce - and lane t the
// bookkeeping of term t when that is a PUSH or a COMMAND term. Every lane of a team reads the env's done flag and counters in the
// same instructions before its lane 0 writes them (a team never spans wavefronts: no barrier). A row that is no first row leaves
// behind those few words unless a push starts or ends or a command is due: the big buffers are not touched. No LDS, no scratch,
// no atomics.
#include "randomize.h"

#include "philox.h"
#include "step_launch.h"

namespace {

constexpr int BLOCK = TREX_RAND_BLOCK, TL = TREX_TL;
constexpr float TWO_PI = 6.2831855f;

// (rounded(), product(), uniform(): philox.h - the products the header orders rounded before a sum reads them)

__global__ __launch_bounds__(BLOCK) void trex_randomize_kernel(TrexRandArgs a) {
  const int lane = threadIdx.x % TL, env = blockIdx.x * (BLOCK / TL) + threadIdx.x / TL;
  if (env >= a.n_envs) return;   // (the ragged last workgroup: whole teams leave)
  const TrexRandState &s = a.st;
  const bool first = a.done[(size_t)env * a.done_stride] != 0.f || s.started[env] == 0u;
  const uint32_t ep = s.ep[env] + (first ? 1u : 0u), k = first ? 0u : s.k[env] + 1u;
  if (lane == 0) { s.ep[env] = ep; s.k[env] = k; s.started[env] = 1u; }
  const int T = a.num_terms, P = a.num_pushes;
  const uint32_t eid = a.env_offset + (uint32_t)env;
  const TrexRandTable &tab = *a.table;

  if (first) {   // the draws of the episode: lane b body b, or the joint of body b
    const int nb = a.model->nb, joint = (lane >= 1 && lane < nb) ? a.model->obs_slot[lane] : -1;
    for (int t = 0; t < T; t++) {
      const TrexRandomTerm term = tab.term[t];
      if (term.kind >= TREX_RAND_PUSH) continue;
      const int i = term.kind == TREX_RAND_MASS ? (lane < nb ? lane : -1) : term.kind == TREX_RAND_FRICTION ? (lane == 0 ? 0 : -1) : joint;
      if (i < 0 || !((term.mask >> i) & 1u)) continue;
      const int src = term.shared ? 0 : i;
      uint32_t r[4];
      philox(eid, 0u, ((uint32_t)TREX_RAND_STREAM_EPISODE << 16) | (uint32_t)(8 * t + (src >> 2)), ep, a.key0, a.key1, r);
      const uint32_t pick = (src & 2) ? ((src & 1) ? r[3] : r[2]) : ((src & 1) ? r[1] : r[0]);
      const float v = uniform(term.lo, term.hi, pick);
      s.values[((size_t)env * T + t) * TL + i] = v;
      if (term.kind == TREX_RAND_MASS) {
        a.mass_scale[(size_t)env * TL + lane] = v;
      } else if (term.kind == TREX_RAND_FRICTION) {
        a.friction[env] = v;
      } else {   // a negative gain as 0: what trex_batch_set_motor_gains makes of one
        const int row = term.kind == TREX_RAND_KP ? 0 : term.kind == TREX_RAND_KD ? 1 : 3;
        const size_t at = ((size_t)env * TREX_ACT_ROWS + row) * TL + lane;
        float g = product(a.nominal[at], v);
        g = g < 0.f ? 0.f : g;
        a.gains[at] = g;
        if (row == 3) a.gains[at - TL] = product(g, a.model->prm[TP_DT]);   // the largest impulse of a substep
      }
    }
  }

  if (lane >= T) return;
  const TrexRandomTerm term = tab.term[lane];
  if (term.kind == TREX_RAND_PUSH) {
    const size_t at = (size_t)env * P + tab.push_slot[lane];
    int left = 0, off;
    bool changed = first, store = first, on = false;
    float f[3] = {0.f, 0.f, 0.f};
    if (first) {
      uint32_t r[4];
      philox(eid, 0u, ((uint32_t)TREX_RAND_STREAM_EPISODE << 16) | (uint32_t)(8 * lane), ep, a.key0, a.key1, r);
      off = draw_int(r[0], 0, term.interval - 1);
      s.off[at] = off;
    } else {
      off = s.off[at];
      left = s.push_left[at];
      if (left > 0) { left--; store = true; changed = left == 0; }
    }
    if (left == 0 && (k + (uint32_t)off) % (uint32_t)term.interval == 0u) {
      uint32_t r[4];
      philox(eid, k, ((uint32_t)TREX_RAND_STREAM_PUSH << 16) | (uint32_t)lane, ep, a.key0, a.key1, r);
      if (u_half_open(r[0]) < term.probability) {
        const float ang = product(TWO_PI, u_half_open(r[1])), m = uniform(term.lo, term.hi, r[2]);
        f[0] = product(m, cosf(ang)); f[1] = product(m, sinf(ang));
        left = term.duration;
        on = changed = store = true;
      }
    }
    if (store) s.push_left[at] = left;
    if (changed) {   // the push body's columns: base + the force in effect
      const float *base = s.push_base + at * 6;
      float *w = a.wrench + (size_t)env * 6 * TL + term.index;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        s.push_force[at * 3 + c] = f[c];
        w[c * TL] = on ? base[c] + f[c] : base[c];   // (f: a product()'s result, rounded)
        w[(c + 3) * TL] = base[c + 3];
      }
    }
  } else if (term.kind == TREX_RAND_COMMAND) {
    const bool again = !first && term.interval > 0 && k % (uint32_t)term.interval == 0u;
    if (!first && !again) return;
    uint32_t r[4];
    if (first) philox(eid, 0u, ((uint32_t)TREX_RAND_STREAM_EPISODE << 16) | (uint32_t)(8 * lane), ep, a.key0, a.key1, r);
    else philox(eid, k, ((uint32_t)TREX_RAND_STREAM_COMMAND << 16) | (uint32_t)lane, ep, a.key0, a.key1, r);
    const float v = u_half_open(r[0]) < term.probability ? 0.f : uniform(term.lo, term.hi, r[1]);
    a.command[(size_t)env * 3 + term.index] = v;
    s.values[((size_t)env * T + lane) * TL] = v;
  }
}

__global__ void trex_randomize_reset_kernel(const uint8_t *mask, int n_envs, uint32_t *started) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  started[env] = 0u;
}

__global__ void trex_randomize_rebase_kernel(const TrexRandTable *table, TrexRandState s, const float *src, float *wrench, int n_envs, int nb,
                                             int num_pushes, int restore) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_envs * num_pushes) return;
  const int env = i / num_pushes, body = table->push_body[i % num_pushes];
  const bool on = !restore && s.push_left[i] > 0;
  for (int c = 0; c < 6; c++) {
    const float base = restore == 2 ? wrench[((size_t)env * 6 + c) * TL + body] : restore ? s.push_base[(size_t)i * 6 + c]
                       : src ? src[((size_t)env * nb + body) * 6 + c] : 0.f;
    s.push_base[(size_t)i * 6 + c] = base;
    wrench[((size_t)env * 6 + c) * TL + body] = (on && c < 3) ? base + s.push_force[(size_t)i * 3 + c] : base;
  }
}

}  // namespace

extern "C" hipError_t trex_launch_randomize(const TrexRandArgs &args, hipStream_t stream) {
  const int per = BLOCK / TL;
  hipLaunchKernelGGL(trex_randomize_kernel, dim3((unsigned)((args.n_envs + per - 1) / per)), dim3(BLOCK), 0, stream, args);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_randomize_reset(const uint8_t *mask, int n_envs, uint32_t *started, hipStream_t stream) {
  hipLaunchKernelGGL(trex_randomize_reset_kernel, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, stream, mask, n_envs, started);
  return hipGetLastError();
}

extern "C" hipError_t trex_launch_randomize_rebase(const TrexRandTable *table, TrexRandState st, const float *src, float *wrench, int n_envs,
                                                   int nb, int num_pushes, int restore, hipStream_t stream) {
  const int total = n_envs * num_pushes;
  hipLaunchKernelGGL(trex_randomize_rebase_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, table, st, src, wrench, n_envs, nb,
                     num_pushes, restore);
  return hipGetLastError();
}
