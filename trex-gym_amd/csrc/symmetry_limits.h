// Limits of the mirror kernels and the layout of a mirror table on the device: what the host builders and checks (host_tables.cpp)
// share with symmetry.hip. No HIP here - symmetry.h includes this file.
#pragma once
#include <stdint.h>

#include "../../include/trex_symmetry.h"

#define TREX_MIRROR_BLOCK 256          /* lanes of a workgroup of either row launch and of the moments launch */
#define TREX_MIRROR_TILE_FLOATS 4096   /* the rows a workgroup keeps in LDS: 16 KB, so that eight workgroups share a CU */
#define TREX_MIRROR_COPY_ELEMS 2048    /* elements of logp, val, adv or ret that one workgroup of the augment launch copies */
#define TREX_MIRROR_NEG 0x80000000u    /* a table word is src[c] | (sign[c] < 0 ? TREX_MIRROR_NEG : 0): the flag IS the sign bit */

/* rows of `width` floats to a workgroup: as many as fit the tile (7 at the widest row, 4096 at width 1) */
static inline int trex_mirror_tile_rows(int width) { return TREX_MIRROR_TILE_FLOATS / width; }
