// Observation channels (trex_batch_compose_rows, include/trex_batch.h): the extended row obs | channels | tail of every env in one
// launch, the channels evaluated at the batch's current state. A workgroup of 256 lanes serves 8 whole envs. Reads only: the kernel
// writes nothing but the out rows.
//
// Phase 1, as link_state.hip: lane (slot, body) walks its body's chain once (chain_walk.h) and parks the body's record in LDS - only
// the bodies a channel names, and the body of URDF link 0, whose lane also parks that link's frame and velocity: the base axes every
// vector channel is expressed in. Phase 2: the 32 lanes of a slot stride over the columns of their env's out row; a lane finds its
// column's channel in the per-column table, computes that one value and writes it - a row goes out as contiguous 128-byte stores.
#include <hip/hip_runtime.h>

#include "../../include/trex_batch.h"
#include "chain_walk.h"
#include "device_math.h"
#include "observation.h"
#include "step_launch.h"

namespace {

constexpr int BLOCK = TREX_OBS_BLOCK;
constexpr int MAXENV = TREX_OBS_MAXENV;
constexpr int REC = TREX_OBS_REC;
constexpr int SLOT = TREX_OBS_SLOT;
constexpr int FRAME = TREX_OBS_FRAME;
constexpr int TL = TREX_TL;
static_assert(BLOCK == MAXENV * TL, "one lane per (env slot, body)");

// component j of m^T v: a world vector in the axes whose world rotation is m (m in LDS: j may differ between lanes)
__device__ __forceinline__ float tcomp(const float *m, const float *v, int j) { return m[j] * v[0] + m[3 + j] * v[1] + m[6 + j] * v[2]; }

}  // namespace

__global__ __launch_bounds__(256) void trex_observation_kernel(TrexObsArgs a) {
  // per env slot and body: R (row-major) | origin, relative to the base origin | w | vo
  __shared__ float sRec[MAXENV * SLOT];
  // per env slot, URDF link 0: A = world <- base axes | origin, relative to the base origin | origin's velocity | angular velocity (base axes)
  __shared__ float sFrame[MAXENV * FRAME];

  const TrexDeviceModel *M = a.model;
  const int t = threadIdx.x;
  const int s = t >> 5, l = t & 31;
  const int env = blockIdx.x * MAXENV + s;
  const bool live = env < a.n_envs;

  // ---- phase 1: lane t walks the chain of body l of env slot s
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

  // ---- phase 2: the columns l, l + 32, ... of this lane's env. (Lanes past the batch's end have met the barrier and write nothing.)
  if (!live) return;
  const int nobs = a.nobs, E = a.extra, W = nobs + E + a.tail;
  const float *row = a.rows + (size_t)env * a.row_stride;
  float *out = a.out + (size_t)env * a.out_stride;
  const float *F = sFrame + s * FRAME;
  const float floor_z = M->prm[TP_FLOOR_Z];
  for (int c = l; c < W; c += TL) {
    float v;
    if (c < nobs) {
      v = row[c];
    } else if (c >= nobs + E) {
      v = row[c - E];
    } else {
      const TrexObsChan &ch = a.chan[a.col_chan[c - nobs]];
      const int kind = ch.kind, j = c - nobs - ch.col0;
      switch (kind) {
        case TREX_OBS_PROJECTED_GRAVITY: v = -F[6 + j]; break;
        case TREX_OBS_BASE_LINEAR_VELOCITY: v = F[12 + j]; break;
        case TREX_OBS_BASE_ANGULAR_VELOCITY: v = F[15 + j]; break;
        case TREX_OBS_BASE_HEIGHT: v = (a.base[(size_t)env * 16 + 2] + F[11]) - floor_z; break;
        case TREX_OBS_CONTACT_FORCE: v = a.sens[(size_t)env * TREX_SENS_FLOATS + 2 * TL + ch.body]; break;
        case TREX_OBS_PREV_ACTION:
          v = (a.actions && row[nobs + 1] == 0.f) ? a.actions[(size_t)env * a.act_cols + j] : 0.f;
          break;
        case TREX_OBS_EXTERNAL: v = a.ext[(size_t)env * a.ext_stride + ch.body + j]; break;
        default: {   // the point channels: the body's record composed with the point, as the link kinematics query does
          const float *P = sRec + s * SLOT + ch.body * REC;
          const float pt[3] = {ch.point[0], ch.point[1], ch.point[2]};
          float d[3];
          matvec3(P, pt, d);   // body origin -> the point, world axes
          if (kind == TREX_OBS_POINT_HEIGHT) {
            v = ((a.base[(size_t)env * 16 + 2] + P[11]) + d[2]) - floor_z;
          } else if (kind == TREX_OBS_POINT_POSITION) {
            float e[3];
#pragma unroll
            for (int i = 0; i < 3; i++) e[i] = (P[9 + i] - F[9 + i]) + d[i];
            v = tcomp(F, e, j);
          } else {
            float lin[3];
            cross3(P + 12, d, lin);
#pragma unroll
            for (int i = 0; i < 3; i++) lin[i] += P[15 + i];
            v = tcomp(F, lin, j);
          }
        }
      }
      v *= ch.scale;
    }
    out[c] = v;
  }
}

extern "C" hipError_t trex_launch_observation(const TrexObsArgs &args, hipStream_t stream) {
  const dim3 grid((unsigned)((args.n_envs + MAXENV - 1) / MAXENV)), block(BLOCK);
  hipLaunchKernelGGL(trex_observation_kernel, grid, block, 0, stream, args);
  return hipGetLastError();
}
