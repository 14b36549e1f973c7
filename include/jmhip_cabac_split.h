/*
 * jmhip_cabac_split.h — one CABAC slice coded on many waves: the device CABAC
 * writer of jmhip_cabac.h cuts every slice's bins into chunks of chunk_bins and codes all chunks of
 * all slices of a picture at once, instead of one wave per slice.  Part of the C ABI of jmhip.h
 * (which includes this file after jmhip_coded.h).  Additive only: JMH_ABI_VERSION stays 14, no
 * struct or entry point of the other four headers changes, jmh_config is not touched.
 *
 * The setting is off after jmh_create.  It serves jmh_cabac_write_slices, jmh_cabac_write_results
 * and the CABAC coded pictures of jmhip_coded.h alike; their signatures and contracts do not change,
 * and the bytes, nbytes and nbins they return are the same with and without it.
 */
#ifndef JMHIP_CABAC_SPLIT_H
#define JMHIP_CABAC_SPLIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jmh_cabac_split_info {
    int32_t chunk_bins;              /* the setting the call ran with; 0: the unsplit coder         */
    int32_t reserved;
    int64_t chunks;                  /* chunks coded, over every slice of the picture                */
    int64_t longest_slice_chunks;    /* the chunks of the slice that has the most                    */
    int64_t scratch_bytes;           /* device memory the split passes hold beyond the unsplit coder's */
} jmh_cabac_split_info;

/* chunk_bins 0: off.  16..65536: on, that many bins per chunk.  Anything else: JMH_E_INVALID_ARG.
 * JMH_E_UNSUPPORTED_CFG: the context's symbol_mode is 0.  JMH_E_INVALID_ARG: ctx is NULL.  Nothing
 * changes when the call fails.  It takes effect for the next writer call and for pictures pushed
 * after it; pictures already queued keep what they were queued with. */
int  jmh_cabac_set_split(jmh_ctx *ctx, int chunk_bins);
/* the setting; JMH_E_INVALID_ARG for a NULL context */
int  jmh_cabac_get_split(const jmh_ctx *ctx);
/* what the last synchronous writer call (jmh_cabac_write_slices / _results) did; all zero before
 * the first one and after one that ran unsplit.  A coded picture that fell back (jmh_coded_stats
 * .fallback) is coded at its pop by the same synchronous writer: with the setting of that moment,
 * not the one it was pushed with (the bytes are the same), and it counts as the last call here. */
int  jmh_cabac_split_stats(const jmh_ctx *ctx, jmh_cabac_split_info *out);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_CABAC_SPLIT_H */
