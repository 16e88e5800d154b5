// Limits of a reward specification and the entry of its term table: what the host builder of the table (host_tables.cpp) shares with
// reward.hip. No HIP here - reward.h includes this file.
#pragma once
#include <stdint.h>

#define TREX_REW_MAXTERMS 32       /* terms per specification: one lane of an env's 32 holds a term's value, timer and held value */

/* One term as the kernel reads it, host-built: 24 words, so that an array of them keeps every entry 16-byte aligned. */
struct TrexRewTerm {
  int32_t kind;        /* TREX_REW_* of include/trex_reward.h */
  int32_t body;        /* POINT_HEIGHT, FOOT_AIR_TIME, FOOT_SLIP: the body of the term's link; else 0 */
  uint32_t mask;       /* joint-sum kinds: bit j = joint j, observation order (a mask of 0 arrives here as all J bits);
                          CONTACT_COUNT: bit b = body b */
  float tf[12];        /* body <- link transform of the link: rotation row-major (9) | translation (3); identity without a link */
  float point[3];      /* the term's point in the BODY frame: rotation x local_xyz + translation */
  float weight, p0, p1;
  int32_t pad[3];      /* (term t's timer and held value are entry t of the env's rows of the history: no index is stored) */
};
