// Limits of the planner and the layouts of its device tables: what the host builders of the tables (host_tables.cpp) share with
// planner.hip. No HIP here - planner.h includes this file.
#pragma once
#include <stdint.h>

#include "../../include/trex_planner.h"

#define TREX_PLAN_BLOCK 256          /* lanes of a sample, return or group workgroup */
#define TREX_PLAN_TILE_FLOATS 8192   /* the knots a sample workgroup keeps in LDS: 32 KB */
#define TREX_PLAN_TILE_ENVS 16       /* at most so many envs to a sample workgroup (fewer where their knots exceed the tile) */
#define TREX_PLAN_SUM_BLOCK 64       /* (p, a) elements of a knot-sum workgroup: one per lane of its wave 0, sequential over k */
#define TREX_PLAN_SUM_TILE 112       /* samples of a tile its four waves load together: two tiles of 112 x 64 floats in LDS, 57 KB */

/* The four taps of one time of include/trex_planner.h: value = ((w[0] k[i[0]] + w[1] k[i[1]]) + w[2] k[i[2]]) + w[3] k[i[3]].
 * The interpolation table is S of them, one per step; a shift table is P of them, one per new knot. */
struct TrexPlanTap {
  int32_t i[4];
  float w[4];
};

/* The noise, ONE allocation, as trex_planner_set_noise checked it. */
struct TrexPlanNoise {
  float sigma[TREX_PLAN_MAXACT], lo[TREX_PLAN_MAXACT], hi[TREX_PLAN_MAXACT];
};

/* (The discount table of a gamma is S + 1 floats, g_s = (float)pow((double)gamma, s): a device table of its own per gamma.) */
