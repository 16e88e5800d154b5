// Batched ray casts (trex_batch_ray_test): launch arguments shared by capi.cpp and raycast.hip. The geometry is the renderer's:
// the primitive / plane table of render.h, built once per batch by whichever of the two calls comes first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_model.h"
#include "render.h"

#define TREX_RAY_BLOCK 256        /* lanes per workgroup = rays per workgroup at most: 4 waves, one ray per lane */
#define TREX_RAY_MAXENV 8         /* envs whose poses one workgroup holds in LDS: 8 x 32 pose lanes = one pass of the 256 lanes */
#define TREX_RAY_MAXRAYS 16384    /* rays per env and call */
/* LDS floats per env slot: TREX_TL poses of 12 floats, + 4 so that the slots of one wave's lanes start 4 banks apart (a
 * 16-byte read of the same body by lanes of different envs then touches disjoint banks) */
#define TREX_RAY_SLOT (TREX_TL * 12 + 4)

struct TrexRayArgs {
  const TrexDeviceModel *model;
  const float *base, *q;          /* the batch's state (read only) */
  const float *rays;              /* [N, R, 6] or, shared, [R, 6]: from xyz, to xyz */
  float *fraction;                /* [N, R] */
  int32_t *body;                  /* [N, R], nullable */
  float *position, *normal;       /* [N, R, 3], nullable */
  int n_envs, num_rays, shared;
  int link_body;                  /* body of the link whose frame the rays are given in, -1 = world frame */
  float link_tf[12];              /* body <- link: R row-major, t ("link_tf") */
  int nprim, hit_floor;
  uint32_t body_mask;
  float floor_z;
  int epw, cpe;                   /* envs per workgroup; workgroups (chunks of 256 rays) per env group: trex_ray_shape */
};

/* How a call of N envs x R rays is cut into workgroups: R >= 256: one env per workgroup, ceil(R / 256) workgroups per env;
 * below: min(8, 256 / R) whole envs per workgroup, lane = slot * R + ray. */
static inline void trex_ray_shape(int num_rays, int *epw, int *cpe) {
  if (num_rays >= TREX_RAY_BLOCK) {
    *epw = 1;
    *cpe = (num_rays + TREX_RAY_BLOCK - 1) / TREX_RAY_BLOCK;
  } else {
    const int e = TREX_RAY_BLOCK / num_rays;
    *epw = e < TREX_RAY_MAXENV ? e : TREX_RAY_MAXENV;
    *cpe = 1;
  }
}

/* raycast.hip; prim / plane: the batch's table (TrexRenderPrim, float4 planes), read through the scalar cache */
extern "C" hipError_t trex_launch_ray_test(const TrexRayArgs &args, const TrexRenderPrim *prim, const float4 *plane, hipStream_t stream);
