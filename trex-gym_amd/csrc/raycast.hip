// Batched ray casts (trex_batch_ray_test, include/trex_batch.h): segments from -> to against the collision geometry the
// renderer draws - the convex hulls (or the spheres of primitive collision) of every body, and the floor - at the batch's
// current state. One lane per ray; a workgroup of 256 lanes serves up to 8 whole envs (few rays per env) or one 256-ray chunk
// of one env (many): trex_ray_shape. Reads only: the kernel writes nothing but the outputs.
//
// Unlike render.hip there is no eye and no pixel tile, so nothing is culled per workgroup. Instead each ray is taken into the
// BODY frame once per body (the table lists a body's primitives together); bounding spheres, sphere primitives and hull planes
// are then the table's own body-frame constants - the same for every lane and every env, read through the scalar cache - and
// only the body poses live in LDS, per env.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "raycast.h"
#include "render_pose.h"

namespace {

constexpr int BLOCK = TREX_RAY_BLOCK;
constexpr int MAXENV = TREX_RAY_MAXENV;
constexpr int SLOT = TREX_RAY_SLOT;
constexpr float kInf = __builtin_inff();
constexpr float kEnd = 1.00000011920928955078125f;   // the float after 1: `t < kEnd` is t <= 1

__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ bool finite(float x) { return fabsf(x) < kInf; }

}  // namespace

__global__ __launch_bounds__(256) void trex_ray_kernel(TrexRayArgs a, const TrexRenderPrim *__restrict__ prim,
                                                       const float4 *__restrict__ plane) {
  __shared__ __attribute__((aligned(16))) float sPose[MAXENV * SLOT];   // per env slot: world R (row-major) | p of every body
  __shared__ float sLink[MAXENV][12];                                   // per env slot: world pose of the rays' link frame

  const TrexDeviceModel *M = a.model;
  const int t = threadIdx.x;
  const int R = a.num_rays, epw = a.epw;
  const int group = blockIdx.x / a.cpe, chunk = blockIdx.x - group * a.cpe;
  const int env0 = group * epw;

  // ---- body poses: lane t composes the pose of body t & 31 of env slot t >> 5 - only of the bodies a ray can hit or sit on
  {
    const int s = t >> 5, bd = t & 31, env = env0 + s;
    const uint32_t need = a.body_mask | (a.link_body >= 0 ? 1u << a.link_body : 0u);
    if (s < epw && env < a.n_envs && bd < M->nb && ((need >> bd) & 1u)) {
      const float *b = a.base + (size_t)env * 16;
      TREX_BODY_WORLD_POSE(M, b, a.q, env, bd, Rb, pb)
      float *o = sPose + s * SLOT + bd * 12;
      for (int c = 0; c < 9; c++) o[c] = Rb[c];
      for (int c = 0; c < 3; c++) o[9 + c] = pb[c];
    }
  }
  __syncthreads();
  if (a.link_body >= 0) {   // the link frame of every env slot, once: link = body o link_tf
    if (t < epw && env0 + t < a.n_envs) {
      const float *P = sPose + t * SLOT + a.link_body * 12;
      float Rl[9], pl[3];
      matmul3(P, a.link_tf, Rl);
      matvec3(P, a.link_tf + 9, pl);
      for (int c = 0; c < 9; c++) sLink[t][c] = Rl[c];
      for (int c = 0; c < 3; c++) sLink[t][9 + c] = pl[c] + P[9 + c];
    }
    __syncthreads();
  }

  // ---- this lane's ray
  int s, ray;
  if (epw == 1) {
    s = 0; ray = chunk * BLOCK + t;
  } else {
    s = t / R; ray = t - s * R;
  }
  const bool valid = s < epw && env0 + s < a.n_envs && ray < R;
  if (!__any(valid)) return;   // (a wave without rays: the tail of a workgroup that holds few)
  if (!valid) s = 0;
  const int env = env0 + s;
  const size_t g = (size_t)env * R + ray;
  float from[3] = {0.f, 0.f, 0.f}, to[3] = {0.f, 0.f, 0.f};
  if (valid) {
    const float *rp = a.rays + (a.shared ? (size_t)ray : g) * 6;
    for (int c = 0; c < 3; c++) { from[c] = rp[c]; to[c] = rp[3 + c]; }
    if (a.link_body >= 0) {
      const float *L = sLink[s];
      float f[3], e[3];
      matvec3(L, from, f);
      matvec3(L, to, e);
      for (int c = 0; c < 3; c++) { from[c] = f[c] + L[9 + c]; to[c] = e[c] + L[9 + c]; }
    }
  }
  const float dir[3] = {to[0] - from[0], to[1] - from[1], to[2] - from[2]};
  const float dd = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
  // a zero-length or non-finite ray hits nothing; it takes part in the wave's votes as a lane that is never a candidate
  const bool ok = valid && dd > 0.f && dd < kInf && finite(from[0]) && finite(from[1]) && finite(from[2]);

  // nearest hit so far: `best` the fraction along from -> to; hit -2 nothing, -1 floor, >= 0 primitive; `pl` the entered plane
  float best = ok ? kEnd : -1.f;
  int hit = -2, pl = -1;
  if (a.hit_floor && ok && from[2] >= a.floor_z && dir[2] < 0.f) {   // floor: the half-space z <= floor_z, entered from above
    const float tf = (from[2] - a.floor_z) / (from[2] - to[2]);
    if (tf < best) { best = tf; hit = -1; }
  }

  const float *Ps = sPose + s * SLOT;
  float ob[3] = {0.f, 0.f, 0.f}, db[3] = {0.f, 0.f, 1.f}, idd = 1.f;
  int cur = -1;
  for (int k = 0; k < a.nprim; k++) {
    const TrexRenderPrim P = prim[k];
    if (!((a.body_mask >> P.body) & 1u)) continue;   // (wave-uniform: a masked body costs nothing)
    if (P.body != cur) {   // ray in the body frame: o_b = R^T (from - p), d_b = R^T dir
      cur = P.body;
      const float *Rp = Ps + cur * 12;
      const float e[3] = {from[0] - Rp[9], from[1] - Rp[10], from[2] - Rp[11]};
      for (int c = 0; c < 3; c++) {
        ob[c] = Rp[c] * e[0] + Rp[3 + c] * e[1] + Rp[6 + c] * e[2];
        db[c] = Rp[c] * dir[0] + Rp[3 + c] * dir[1] + Rp[6 + c] * dir[2];
      }
      idd = 1.f / (db[0] * db[0] + db[1] * db[1] + db[2] * db[2]);
    }
    // bounding sphere against the segment. (The closest approach first: r^2 - |oc + tc d|^2 has none of the cancellation of
    // hb^2 - dd (|oc|^2 - r^2).)
    const float oc[3] = {ob[0] - P.c[0], ob[1] - P.c[1], ob[2] - P.c[2]};
    const float tc = -(db[0] * oc[0] + db[1] * oc[1] + db[2] * oc[2]) * idd;
    const float lx = oc[0] + tc * db[0], ly = oc[1] + tc * db[1], lz = oc[2] + tc * db[2];
    const float h2 = P.r * P.r - (lx * lx + ly * ly + lz * lz);
    const float sq = sqrtf(fmaxf(h2, 0.f) * idd);
    const float t0 = tc - sq, t1 = tc + sq;
    if (P.kind == 1) {   // sphere: the interval's start is the hit, unless the origin is inside (t0 < 0)
      if (h2 >= 0.f && t0 >= 0.f && t0 < best) { best = t0; hit = k; }
      continue;
    }
    const bool cand = h2 >= 0.f && t1 >= 0.f && fmaxf(t0, 0.f) < best;
    if (!__any(cand)) continue;
    // Cyrus-Beck: t_enter = max over entering planes, t_exit = min over exiting ones, clipped to best. The planes are the
    // same for every lane; a hull's list is padded to a multiple of 8 with copies of its last plane
    float te = -kInf, tx = cand ? best : -1.f;
    int kp = -1;
    for (int j0 = P.plane0; j0 < P.plane0 + P.nplanes; j0 += 8) {
#pragma unroll
      for (int j = j0; j < j0 + 8; j++) {
        const float4 h = plane[j];
        const float den = h.x * db[0] + h.y * db[1] + h.z * db[2];
        const float num = h.w - (h.x * ob[0] + h.y * ob[1] + h.z * ob[2]);
        const float tj = num * rcp(den);
        const bool enter = den < 0.f, leave = den > 0.f;   // (den == +-0: parallel, outside if num < 0)
        const bool up = enter && tj > te;
        kp = up ? j : kp;
        te = up ? tj : te;
        tx = leave ? fminf(tx, tj) : tx;
        tx = (!enter && !leave && num < 0.f) ? -1.f : tx;
      }
      if (!__any(cand && te <= tx)) break;   // every candidate lane of the wave has left the hull
    }
    // (te < 0: the origin is inside the hull - or the hull lies behind it -, and the ray looks out of it)
    if (te >= 0.f && te <= tx && te < best) { best = te; hit = k; pl = kp; }
  }

  if (!valid) return;
  // ---- write
  float frac = 1.f, pos[3] = {to[0], to[1], to[2]}, nrm[3] = {0.f, 0.f, 0.f};
  int label = -2;
  if (hit != -2) {
    frac = fminf(best, 1.f);
    for (int c = 0; c < 3; c++) pos[c] = from[c] + frac * dir[c];
    if (hit == -1) {
      label = -1;
      nrm[2] = 1.f;
    } else {
      const TrexRenderPrim P = prim[hit];
      const float *Rp = Ps + P.body * 12;
      label = P.body;
      if (P.kind == 1) {   // radial: from the sphere's world centre
        for (int c = 0; c < 3; c++) nrm[c] = pos[c] - (Rp[9 + c] + Rp[3 * c] * P.c[0] + Rp[3 * c + 1] * P.c[1] + Rp[3 * c + 2] * P.c[2]);
      } else {
        const float4 h = plane[pl];
        for (int c = 0; c < 3; c++) nrm[c] = Rp[3 * c] * h.x + Rp[3 * c + 1] * h.y + Rp[3 * c + 2] * h.z;
      }
      const float il = rsqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
      for (int c = 0; c < 3; c++) nrm[c] *= il;
    }
  }
  a.fraction[g] = frac;
  if (a.body) a.body[g] = label;
  if (a.position)
    for (int c = 0; c < 3; c++) a.position[3 * g + c] = pos[c];
  if (a.normal)
    for (int c = 0; c < 3; c++) a.normal[3 * g + c] = nrm[c];
}

extern "C" hipError_t trex_launch_ray_test(const TrexRayArgs &args, const TrexRenderPrim *prim, const float4 *plane, hipStream_t stream) {
  TrexRayArgs a = args;
  trex_ray_shape(a.num_rays, &a.epw, &a.cpe);
  if (!a.body_mask) a.nprim = 0;   // no body may be hit: no primitive loop (the pose pass computes only the link's body)
  const int groups = (a.n_envs + a.epw - 1) / a.epw;
  hipLaunchKernelGGL(trex_ray_kernel, dim3((unsigned)groups * (unsigned)a.cpe), dim3(BLOCK), 0, stream, a, prim, plane);
  return hipGetLastError();
}
