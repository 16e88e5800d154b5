// Limits of the sensor model and the layout of its device table: what the host builder of the table (host_tables.cpp) shares with
// sensing.hip. No HIP here - sensing.h includes this file.
#pragma once
#include <stdint.h>

#define TREX_SENSE_SLOTS 9         /* TREX_SENSE_MAXDELAY + 1 rows of history per env: row k lives in slot k % 9 */
#define TREX_SENSE_MAXCOLS 512     /* observation columns of a row: TREX_OBS_MAXDIM */

/* One group as the kernel reads it: 10 words. */
struct TrexSenseGrp {
  int32_t col0, width, kind;       /* TREX_SENSE_* of include/trex_sensing.h */
  float noise, bias, quantum, inv_quantum;
  int32_t delay_min, delay_max;
  int32_t pad;
};
/* The table, ONE allocation: TrexSenseGrp [G] | int16 col_group [D] (-1: in no group) | int16 col_hist [D] (the column's place
 * among the delayed columns, -1: its group has delay_max == 0). */
