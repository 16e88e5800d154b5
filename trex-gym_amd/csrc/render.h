// Ray-cast renderer (trex_batch_render): device-side tables and launch arguments shared by render.cpp, capi.cpp and
// render.hip. The step kernels do not see any of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"

#define TREX_RENDER_TILE 16       /* pixels per side of a workgroup's tile: 256 lanes = 4 waves of 8 x 8 */
#define TREX_RENDER_MAXPRIM 512   /* drawable primitives per model (hulls + spheres): the per-tile cull list lives in LDS */
#define TREX_RENDER_MAXDIM 4096   /* largest width / height of an image */

/* one drawable primitive, body frame: a convex hull (kind 0: planes [plane0, plane0 + nplanes) of the plane table,
 * n.x <= d inside) or a sphere (kind 1: centre c, radius r). c / r of a hull: a sphere that bounds it. */
struct TrexRenderPrim {
  int body, plane0, nplanes, kind;
  float c[3], r;
};

struct TrexRenderArgs {
  const TrexDeviceModel *model;
  const float *base, *q;          /* the batch's state (read only) */
  const int *env_ids;             /* [num_views] device, NULL = view v renders env v */
  const TrexRenderPrim *prim;
  const float4 *plane;            /* (n, d) per plane, body frame */
  uint8_t *rgb;                   /* [V, H, W, 3], nullable */
  float *depth;                   /* [V, H, W], nullable */
  int32_t *seg;                   /* [V, H, W], nullable */
  int num_views, width, height, tiles_x;
  int nprim, follow_base;
  /* camera: eye = target + offset (target = the env's base position when follow_base); ray of NDC (x, y) =
   * fwd + x tan_x right + y tan_y up, so that the ray parameter t of a point IS its eye-space depth */
  float target[3], offset[3], fwd[3], right[3], up[3];
  float tan_x, tan_y, near_z, far_z, floor_z;
};

extern "C" hipError_t trex_launch_render(const TrexRenderArgs &args, hipStream_t stream);   /* render.hip */
