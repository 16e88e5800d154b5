// Limits of a motion clip and the layout of its device table: what the host builder of the table (host_tables.cpp) shares with
// motion.hip. No HIP here - motion.h includes this file.
#pragma once
#include <stdint.h>

#define TREX_MOT_MAXFRAMES 4096    /* frames per clip: 4096 rows of at most 76 floats, about 1.2 MB */
#define TREX_MOT_MAXTERMS 8        /* terms per specification: they travel in the launch arguments, no table */
#define TREX_MOT_MAXPROBES 8       /* end effectors per clip: one lane of an env's 32 each */
/* The clip table: F rows of the state layout of trex_batch_get_state, [pos 3 | quat xyzw 4 | v 3 | w 3 | q J | qd J] as f32, each
 * row padded to a multiple of 4 floats, so that every row starts on a 16-byte boundary of the ONE allocation. */
#define TREX_MOT_COLS(nj) (13 + 2 * (nj))
#define TREX_MOT_STRIDE(nj) ((TREX_MOT_COLS(nj) + 3) & ~3)

/* One term as the kernel reads it: 8 words. */
struct TrexMotTerm {
  int32_t kind;        /* TREX_MOT_* of include/trex_motion.h */
  uint32_t mask;       /* POSE, VELOCITY: bit j = joint j, observation order (a mask of 0 arrives here as all J bits) */
  float weight, scale, aux;
  int32_t pad[3];
};
