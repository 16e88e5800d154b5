// Batched ray-cast renderer (trex_batch_render, include/trex_batch.h): draws the collision geometry the physics holds -
// the convex hulls (or the spheres of primitive collision) of every body, and the floor - from the batch's state.
// One workgroup per (view, 16 x 16 pixel tile): 4 waves of 8 x 8 pixels, one ray per lane. Reads only: the kernel writes
// nothing but the output images.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "render.h"
#include "render_pose.h"

namespace {

constexpr int TL = TREX_TL;
constexpr int TILE = TREX_RENDER_TILE;
constexpr int MAXPRIM = TREX_RENDER_MAXPRIM;

// shading: a fixed directional light plus ambient, one colour per body (cycled), a 1 m checkerboard floor, a constant sky
__constant__ float kPalette[8][3] = {{0.85f, 0.55f, 0.30f}, {0.35f, 0.65f, 0.35f}, {0.30f, 0.50f, 0.85f}, {0.85f, 0.35f, 0.35f},
                                     {0.75f, 0.75f, 0.30f}, {0.60f, 0.40f, 0.80f}, {0.30f, 0.75f, 0.75f}, {0.80f, 0.80f, 0.80f}};
constexpr float kLight[3] = {0.3713907f, 0.2785430f, 0.8854167f};   // normalize(0.4, 0.3, 0.953...) : toward the light
constexpr float kAmbient = 0.35f;
constexpr float kFloorA[3] = {0.62f, 0.62f, 0.62f}, kFloorB[3] = {0.42f, 0.42f, 0.42f};
constexpr float kSky[3] = {0.60f, 0.75f, 0.92f};

__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ unsigned char to_u8(float c) {
  c = fminf(fmaxf(c, 0.f), 1.f);
  return (unsigned char)(int)floorf(c * 255.f + 0.5f);
}

}  // namespace

__global__ __launch_bounds__(256) void trex_render_kernel(TrexRenderArgs a) {
  __shared__ float sPose[TL][12];          // world R (row-major) | p - base position of every body of the view's env
  __shared__ float4 sSph[MAXPRIM];         // bounding sphere of the culled primitives (as p), list order
  __shared__ int sList[MAXPRIM];           // primitive index, ascending
  __shared__ int sKeep[MAXPRIM];
  __shared__ int sCount;

  const TrexDeviceModel *M = a.model;
  const int view = blockIdx.y;
  const int env = a.env_ids ? a.env_ids[view] : view;
  const int t = threadIdx.x;
  const float *b = a.base + (size_t)env * 16;

  // ---- body poses: lane t < nb composes the base pose with the hinges of its chain (render_pose.h). Everything the rays meet
  // is held RELATIVE TO THE BASE POSITION - poses, bounding spheres, the eye, the floor: in world coordinates an env 64 m from
  // the origin loses 8 bits of every one of them (one ulp there is 4e-6 m), and an oblique facet turns that into 1e-4 of depth
  if (t < M->nb) {
    const float br[7] = {0.f, 0.f, 0.f, b[3], b[4], b[5], b[6]};
    TREX_BODY_WORLD_POSE(M, br, a.q, env, t, R, p)
    for (int c = 0; c < 9; c++) sPose[t][c] = R[c];
    for (int c = 0; c < 3; c++) sPose[t][9 + c] = p[c];
  }

  // ---- camera of this view
  float eye[3];
  for (int c = 0; c < 3; c++) eye[c] = (a.follow_base ? 0.f : a.target[c] - b[c]) + a.offset[c];
  const float floor_z = a.floor_z - b[2];
  const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
  const float invW = 2.f / (float)a.width, invH = 2.f / (float)a.height;
  __syncthreads();

  // ---- cull the primitives against the tile's ray bundle: the four side planes through the eye, near and far
  {
    const float x0 = (float)(tx * TILE) * invW - 1.f, x1 = (float)min(tx * TILE + TILE, a.width) * invW - 1.f;
    const float y1 = 1.f - (float)(ty * TILE) * invH, y0 = 1.f - (float)min(ty * TILE + TILE, a.height) * invH;
    for (int k = t; k < a.nprim; k += blockDim.x) {
      const TrexRenderPrim P = a.prim[k];
      const float *Rp = sPose[P.body];
      float w[3], v[3];
      for (int r = 0; r < 3; r++) w[r] = Rp[9 + r] + Rp[3 * r] * P.c[0] + Rp[3 * r + 1] * P.c[1] + Rp[3 * r + 2] * P.c[2];
      for (int r = 0; r < 3; r++) v[r] = w[r] - eye[r];
      const float cx = v[0] * a.right[0] + v[1] * a.right[1] + v[2] * a.right[2];
      const float cy = v[0] * a.up[0] + v[1] * a.up[1] + v[2] * a.up[2];
      const float cz = v[0] * a.fwd[0] + v[1] * a.fwd[1] + v[2] * a.fwd[2];
      const float r = P.r * 1.001f + 1e-4f;   // (slack for the f32 arithmetic of the test)
      const float ax0 = x0 * a.tan_x, ax1 = x1 * a.tan_x, ay0 = y0 * a.tan_y, ay1 = y1 * a.tan_y;
      bool keep = cz > a.near_z - r && cz < a.far_z + r;
      keep = keep && (cx - ax0 * cz) >= -r * sqrtf(1.f + ax0 * ax0) && (ax1 * cz - cx) >= -r * sqrtf(1.f + ax1 * ax1);
      keep = keep && (cy - ay0 * cz) >= -r * sqrtf(1.f + ay0 * ay0) && (ay1 * cz - cy) >= -r * sqrtf(1.f + ay1 * ay1);
      sKeep[k] = keep ? 1 : 0;
      sSph[k] = make_float4(w[0], w[1], w[2], P.r);
    }
    __syncthreads();
    if (t < 64) {   // wave 0 compacts in primitive order (deterministic list: ties go to the lower index everywhere)
      int n = 0;
      for (int k0 = 0; k0 < a.nprim; k0 += 64) {
        const int k = k0 + t;
        const bool keep = k < a.nprim && sKeep[k];
        const unsigned long long m = __ballot(keep);
        const int pos = n + __popcll(m & ((1ull << t) - 1ull));
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < a.nprim) s = sSph[k];
        __builtin_amdgcn_wave_barrier();
        if (keep) sList[pos] = k;
        n += __popcll(m);
        // (sSph is rewritten in list order: pos <= k, and the entries below k0 + 64 are read above before any write)
        if (keep) sSph[pos] = s;
        __builtin_amdgcn_wave_barrier();
      }
      if (t == 0) sCount = n;
    }
    __syncthreads();
  }

  // ---- this lane's ray
  const int wv = t >> 6, l = t & 63;
  const int px = tx * TILE + (wv & 1) * 8 + (l & 7), py = ty * TILE + (wv >> 1) * 8 + (l >> 3);
  const bool valid = px < a.width && py < a.height;
  const float nx = ((float)px + 0.5f) * invW - 1.f, ny = 1.f - ((float)py + 0.5f) * invH;
  float dir[3];
  for (int c = 0; c < 3; c++) dir[c] = a.fwd[c] + nx * a.tan_x * a.right[c] + ny * a.tan_y * a.up[c];
  const float dd = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];

  // nearest hit so far: t = eye-space depth; kind -2 nothing, -1 floor, >= 0 list entry; `pl` the hull plane that was entered
  float best = valid ? a.far_z : -1.f;   // (an invalid lane never hits anything)
  int hit = -2, pl = -1;
  if (dir[2] < 0.f || eye[2] < floor_z) {   // floor: the half-space z <= floor_z
    const float tf = eye[2] < floor_z ? a.near_z : fmaxf((floor_z - eye[2]) / dir[2], a.near_z);
    if (tf < best) { best = tf; hit = -1; }
  }

  const int n = uni(sCount);
  for (int k = 0; k < n; k++) {
    const float4 S = sSph[k];
    // bounding sphere: skip unless the ray's entry lies before this lane's nearest hit
    const float oc[3] = {eye[0] - S.x, eye[1] - S.y, eye[2] - S.z};
    // (the closest approach first: r^2 - |oc + tc dir|^2 has none of the cancellation of hb^2 - dd (|oc|^2 - r^2))
    const float tc = -(dir[0] * oc[0] + dir[1] * oc[1] + dir[2] * oc[2]) / dd;
    const float lx = oc[0] + tc * dir[0], ly = oc[1] + tc * dir[1], lz = oc[2] + tc * dir[2];
    const float h2 = S.w * S.w - (lx * lx + ly * ly + lz * lz);
    const float sq = sqrtf(fmaxf(h2, 0.f) / dd);
    const float t0 = tc - sq, t1 = tc + sq;
    const float te0 = fmaxf(t0, a.near_z);
    const bool cand = h2 >= 0.f && te0 < best && te0 <= t1;
    if (!__any(cand)) continue;
    const int pi = uni(sList[k]);
    const int kind = uni(a.prim[pi].kind), body = uni(a.prim[pi].body);
    if (kind == 1) {   // sphere: the same interval is the hit
      if (cand) { best = te0; hit = k; }
      continue;
    }
    // ray in the body frame: o_b = R^T (eye - p), d_b = R^T dir
    const float *Rp = sPose[body];
    const float e[3] = {eye[0] - Rp[9], eye[1] - Rp[10], eye[2] - Rp[11]};
    float ob[3], db[3];
    for (int c = 0; c < 3; c++) {
      ob[c] = Rp[c] * e[0] + Rp[3 + c] * e[1] + Rp[6 + c] * e[2];
      db[c] = Rp[c] * dir[0] + Rp[3 + c] * dir[1] + Rp[6 + c] * dir[2];
    }
    // Cyrus-Beck: t_enter = max over entering planes, t_exit = min over exiting ones, clipped to [near, best]. The planes
    // are the same for every lane (one broadcast load per wave); a hull's list is padded to a multiple of 8 with copies of
    // its last plane
    float te = a.near_z, tx_ = cand ? best : -1.f;
    int kp = -1;
    const int p0 = uni(a.prim[pi].plane0), np = uni(a.prim[pi].nplanes);
    for (int j0 = p0; j0 < p0 + np; j0 += 8) {
#pragma unroll
      for (int j = j0; j < j0 + 8; j++) {
        const float4 h = a.plane[j];
        const float den = h.x * db[0] + h.y * db[1] + h.z * db[2];
        const float num = h.w - (h.x * ob[0] + h.y * ob[1] + h.z * ob[2]);
        const float tj = num * rcp(den);
        const bool enter = den < 0.f, leave = den > 0.f;   // (den == +-0: parallel, outside if num < 0)
        const bool up = enter && tj > te;
        kp = up ? j : kp;
        te = up ? tj : te;
        tx_ = leave ? fminf(tx_, tj) : tx_;
        tx_ = (!enter && !leave && num < 0.f) ? -1.f : tx_;
      }
      if (!__any(te <= tx_)) break;   // every lane of the wave has left the hull (or never reached it)
    }
    if (te <= tx_ && te < best) { best = te; hit = k; pl = kp; }
  }

  if (!valid) return;
  // ---- shade and write
  const size_t pix = ((size_t)view * a.height + py) * a.width + px;
  float col[3];
  int seg = -2;
  if (hit == -2) {
    for (int c = 0; c < 3; c++) col[c] = kSky[c];
    best = a.far_z;
  } else {
    float nrm[3] = {0.f, 0.f, 1.f};
    const float hp[3] = {eye[0] + best * dir[0], eye[1] + best * dir[1], eye[2] + best * dir[2]};
    const float *alb;
    if (hit == -1) {
      seg = -1;
      const int parity = ((int)floorf(hp[0] + b[0]) + (int)floorf(hp[1] + b[1])) & 1;   // (the checker is the world's)
      alb = parity ? kFloorB : kFloorA;
    } else {
      const int pi = sList[hit];
      const TrexRenderPrim P = a.prim[pi];
      seg = P.body;
      alb = kPalette[P.body & 7];
      if (P.kind == 1) {
        const float4 S = sSph[hit];
        for (int c = 0; c < 3; c++) nrm[c] = hp[c] - (&S.x)[c];
      } else if (pl >= 0) {
        const float4 h = a.plane[pl];
        const float *Rp = sPose[P.body];
        for (int c = 0; c < 3; c++) nrm[c] = Rp[3 * c] * h.x + Rp[3 * c + 1] * h.y + Rp[3 * c + 2] * h.z;
      } else {   // the near plane cuts the hull: seen from inside
        for (int c = 0; c < 3; c++) nrm[c] = -dir[c];
      }
      const float il = rsqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
      for (int c = 0; c < 3; c++) nrm[c] *= il;
    }
    const float lam = fmaxf(nrm[0] * kLight[0] + nrm[1] * kLight[1] + nrm[2] * kLight[2], 0.f);
    const float sh = kAmbient + (1.f - kAmbient) * lam;
    for (int c = 0; c < 3; c++) col[c] = alb[c] * sh;
  }
  if (a.rgb) {
    uint8_t *o = a.rgb + 3 * pix;
    o[0] = to_u8(col[0]); o[1] = to_u8(col[1]); o[2] = to_u8(col[2]);
  }
  if (a.depth) a.depth[pix] = best;
  if (a.seg) a.seg[pix] = seg;
}

extern "C" hipError_t trex_launch_render(const TrexRenderArgs &args, hipStream_t stream) {
  const int tx = (args.width + TILE - 1) / TILE, ty = (args.height + TILE - 1) / TILE;
  TrexRenderArgs a = args;
  a.tiles_x = tx;
  hipLaunchKernelGGL(trex_render_kernel, dim3(tx * ty, args.num_views), dim3(TILE * TILE), 0, stream, a);
  return hipGetLastError();
}
