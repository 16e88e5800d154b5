// Limits of an observation specification and the entry of its channel table: what the host builder of the table (host_tables.cpp)
// shares with observation.hip. No HIP here - observation.h includes this file.
#pragma once
#include <stdint.h>

#define TREX_OBS_MAXCHANNELS 64    /* channels per specification */
#define TREX_OBS_MAXDIM 512        /* observation columns of a composed row: 3J + the channels' widths */

/* One channel as the kernel reads it, host-built: 20 words, so that an array of them keeps every entry 16-byte aligned. */
struct TrexObsChan {
  int32_t kind;        /* TREX_OBS_* of include/trex_batch.h */
  int32_t body;        /* POINT_*, CONTACT_FORCE: the body of the channel's link; EXTERNAL: the channel's first column in a row of
                          extern_dev; else 0 */
  int32_t col0;        /* the channel's first column, counted from column 3J of the composed row */
  int32_t width;       /* its columns */
  float tf[12];        /* body <- link transform of the link: rotation row-major (9) | translation (3); identity without a link */
  float point[3];      /* the channel's point in the BODY frame: rotation x local_xyz + translation */
  float scale;
};
