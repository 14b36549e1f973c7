/*
 * jmhip_spiral.h — a unit seam of the search kernels' spiral decode.  The fast full search names a
 * full-pel winner by its index in JM's spiral order (Init_Motion_Search_Module); k_mb_analyse and
 * k_mb_flow turn that index into a position in registers (csrc/jmh_spiral.h, jms_decode_dev: a ring
 * candidate from the device's square root instruction, repaired in integers).  This entry runs that
 * device function over every index of a search range and returns the positions, so that a test can
 * hold the device's own instruction against the table.  Part of the C ABI of jmhip.h (which
 * includes this file after jmhip_rgb.h).  Additive only: JMH_ABI_VERSION stays 14.
 */
#ifndef JMHIP_SPIRAL_H
#define JMHIP_SPIRAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out_xy[2 n], out_xy[2 n + 1] = the position (x, y) of spiral index n, for n = 0 .. (2 sr + 1)^2 - 1,
 * decoded on the context's device.  search_range 1..32 (the LDS-resident window of the fast full
 * search; it need not be the context's own), else JMH_E_INVALID_ARG.  Synchronous. */
int  jmh_spiral_positions(jmh_ctx *c, int search_range, int32_t *out_xy);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_SPIRAL_H */
