// jmh_cavlc.h — host entry of the device CAVLC writer (jmh_cavlc.hip), called by the C ABI
// (jmhip_abi.hip: jmh_cavlc_write_slices / jmh_cavlc_write_results, and the coded pictures).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/jmhip.h"
#include "jmh_coded.h"

struct jmh_cavlc_state;   // the writer's stream and buffers, created on first use
// slice_data() + rbsp_trailing_bits of every slice, from results on the device (d_res; the launches
// wait for `after`, may be null) or from the caller's host results (h_res: uploaded).  Returns a
// JMH_* status; where[n] is filled once the count pass ran.
int jmh_cavlc_run(jmh_cavlc_state **state, const jmh_mb_result *d_res, const jmh_mb_result *h_res, hipEvent_t after, int mbw, int mbh,
                  int t8mode, int cip, int n, const jmh_slice_desc *slices, uint8_t *out, size_t cap, jmh_slice_bytes *where);
// JMH_OK when the n descriptors are raster runs that tile nmb macroblocks (what jmh_cavlc_run checks)
int jmh_cavlc_check(int nmb, int n, const jmh_slice_desc *slices);
// The same three passes queued behind `after` with no host wait between them: sizes, offsets and
// the overflow word stay on the device (job->d_meta, job->d_where).  *stream: the writer's stream,
// for what the caller queues behind the passes.
int jmh_cavlc_enqueue(jmh_cavlc_state **state, const jmh_mb_result *d_res, hipEvent_t after, int mbw, int mbh, int t8mode, int cip, int n,
                      const jmh_writer_job *job, hipStream_t *stream);
void jmh_cavlc_free(jmh_cavlc_state *s);
