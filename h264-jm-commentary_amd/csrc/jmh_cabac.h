// jmh_cabac.h — host entry of the device CABAC writer (jmh_cabac.hip), called by the C ABI
// (jmhip_abi.hip: jmh_cabac_write_slices / jmh_cabac_write_results, and the coded pictures).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/jmhip.h"
#include "jmh_coded.h"

struct jmh_cabac_state;   // the writer's stream and buffers, created on first use
// slice_data() + rbsp_trailing_bits of every slice, from results on the device (d_res; the launches
// wait for `after`, may be null) or from the caller's host results (h_res: uploaded).  Returns a
// JMH_* status; where[n] is filled once the slices were coded.
int jmh_cabac_run(jmh_cabac_state **state, const jmh_mb_result *d_res, const jmh_mb_result *h_res, hipEvent_t after, int mbw, int mbh,
                  int t8mode, int cip, int n, const jmh_cabac_slice_desc *slices, uint8_t *out, size_t cap, jmh_cabac_slice_bytes *where);
// JMH_OK when the n descriptors are raster runs that tile nmb macroblocks (what jmh_cabac_run checks)
int jmh_cabac_check(int nmb, int n, const jmh_cabac_slice_desc *slices);
// The same six launches queued behind `after` with no host wait between them: counts, offsets and
// the overflow word stay on the device (job->d_meta, job->d_where); the record and scratch buffers
// are sized from job->out_cap before anything is queued.  *stream: the writer's stream.
int jmh_cabac_enqueue(jmh_cabac_state **state, const jmh_mb_result *d_res, hipEvent_t after, int mbw, int mbh, int t8mode, int cip, int n,
                      const jmh_writer_job *job, hipStream_t *stream);
void jmh_cabac_free(jmh_cabac_state *s);
