// Limits of a proximity table and the packing of its test words: what the host builder of the table (host_tables.cpp) shares with
// proximity.hip. No HIP here - proximity.h includes this file.
#pragma once
#include <stdint.h>

#define TREX_PROX_MAXCAPS 256      /* capsules per table */
#define TREX_PROX_MAXPAIRS 1024    /* body pairs per table */
#define TREX_PROX_MAXTESTS 65536   /* capsule-pair tests per table: the sum over pairs of capsules(A) x capsules(B) */

/* One capsule-pair test, host-built, sorted by (pair, capsule of A, capsule of B): pair << 16 | capsule of A << 8 | capsule of B
 * (capsule = index into the table). The index of a test in the list is its rank in the tie rule. */
#define TREX_PROX_TEST(pair, ca, cb) (((uint32_t)(pair) << 16) | ((uint32_t)(ca) << 8) | (uint32_t)(cb))
