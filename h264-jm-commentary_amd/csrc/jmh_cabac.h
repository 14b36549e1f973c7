// jmh_cabac.h — host entry of the device CABAC writer (jmh_cabac.hip), called by the C ABI
// (jmhip_abi.hip: jmh_cabac_write_slices / jmh_cabac_write_results).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/jmhip.h"

struct jmh_cabac_state;   // the writer's stream and buffers, created on first use
// slice_data() + rbsp_trailing_bits of every slice, from results on the device (d_res; the launches
// wait for `after`, may be null) or from the caller's host results (h_res: uploaded).  Returns a
// JMH_* status; where[n] is filled once the slices were coded.
int jmh_cabac_run(jmh_cabac_state **state, const jmh_mb_result *d_res, const jmh_mb_result *h_res, hipEvent_t after, int mbw, int mbh,
                  int t8mode, int cip, int n, const jmh_cabac_slice_desc *slices, uint8_t *out, size_t cap, jmh_cabac_slice_bytes *where);
void jmh_cabac_free(jmh_cabac_state *s);
