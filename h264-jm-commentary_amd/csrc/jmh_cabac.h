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
                  int t8mode, int cip, int n, const jmh_cabac_slice_desc *slices, uint8_t *out, size_t cap, jmh_cabac_slice_bytes *where,
                  int chunk_bins);
// JMH_OK when the n descriptors are raster runs that tile nmb macroblocks (what jmh_cabac_run checks)
int jmh_cabac_check(int nmb, int n, const jmh_cabac_slice_desc *slices);
// The same six launches queued behind `after` with no host wait between them: counts, offsets and
// the overflow word stay on the device (job->d_meta, job->d_where); the record and scratch buffers
// are sized from job->out_cap before anything is queued.  *stream: the writer's stream.
int jmh_cabac_enqueue(jmh_cabac_state **state, const jmh_mb_result *d_res, hipEvent_t after, int mbw, int mbh, int t8mode, int cip, int n,
                      const jmh_writer_job *job, hipStream_t *stream, int chunk_bins);
void jmh_cabac_free(jmh_cabac_state *s);
// chunk_bins of the two calls above: 0 codes a slice on one wave (k_cabac_code); 16..65536 cuts every
// slice into chunks of that many bins and codes all of them at once (jmh_cabac_split.hip)
void jmh_cabac_split_last(const jmh_cabac_state *s, jmh_cabac_split_info *out);   // the last jmh_cabac_run

// jmh_cabac_split.hip: the launches that stand in k_cabac_code's place, on the writer's stream and buffers
struct jmh_split_state;
int jmh_split_enqueue(jmh_split_state **state, hipStream_t st, const jmh_cabac_slice_desc *d_sl, int nslices, const uint64_t *d_off,
                      const uint64_t *d_soff, uint16_t *d_rec, uint64_t rec_cap, uint8_t *d_scratch, int64_t *d_slbytes, const uint32_t *d_ovf,
                      int chunk_bins, bool totals);
uint64_t jmh_split_bytes(const jmh_split_state *s);
const uint64_t *jmh_split_totals(const jmh_split_state *s);
void jmh_split_free(jmh_split_state *s);
