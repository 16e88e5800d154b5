// Limits of the start-state randomisation and the layout of its device table: what the host builder of the table
// (host_tables.cpp) shares with start_state.hip. No HIP here - start_state.h includes this file.
#pragma once
#include <stdint.h>

#include "../../include/trex_start_state.h"

#define TREX_START_BLOCK 64        /* lanes per workgroup: one env per wavefront, one wavefront per workgroup (TREX_TERM_BLOCK) */

/* The table, ONE allocation: the terms as host_tables.cpp checked them - a joint mask of 0 expanded to all the model's joints, a
 * base kind and FLOOR_CLEARANCE as element 0 alone -, and what the launch decides on before it reads a term: is there a BASE_RPY
 * term (else quaternion and velocities stay as found), and the FLOOR_CLEARANCE term (-1: none). */
struct TrexStartTable {
  TrexStartTerm term[TREX_START_MAXTERMS];
  int32_t num_terms, rotate, clearance_term, pad;
};
