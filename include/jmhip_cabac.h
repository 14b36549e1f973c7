/*
 * jmhip_cabac.h — CABAC slice data written on the device: replaces the
 * write_one_macroblock loop of JM 8.6 slice.c › encode_one_slice [J] for SymbolMode 1.  Part of the
 * C ABI of jmhip.h (which includes this file after jmhip_cavlc.h).  Additive only: JMH_ABI_VERSION
 * stays 14, no struct or entry point of jmhip.h or jmhip_cavlc.h changes, jmh_config is not touched.
 *
 * The caller writes each slice header and the cabac_alignment_one_bits on the host, so the device
 * output starts on a byte boundary (no lead bits).  Contract: for every slice, out[offset .. offset +
 * nbytes) equals, byte for byte, what host/cabac.c › jm_cabac_slice_start .. jm_cabac_slice_end append
 * behind that point: slice_data() of 7.3.4 coded by 9.3 with the fixed model (cabac_init_idc 0),
 * mb_qp_delta 0, end_of_slice_flag, EncodeFlush; the last byte holds the rbsp_stop_one_bit.  nbins
 * is the slice's bin count (what jm_cabac_slice_end returns): the caller needs the picture's sum
 * for cabac_zero_words (7.4.2.10).  Offsets are contiguous and ascending.  NAL wrapping stays with
 * the caller.  transform_8x8_mode and constrained_intra_pred come from the context's configuration.
 */
#ifndef JMHIP_CABAC_H
#define JMHIP_CABAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jmh_cabac_slice_desc {   /* in: one per slice, raster runs covering the picture    */
    int32_t first_mb, n_mb;
    int32_t slice_type;                 /* JMH_P_SLICE / JMH_I_SLICE                               */
    int32_t slice_qp;                   /* SliceQPY of the header, 0..51: the context initialisation */
} jmh_cabac_slice_desc;
typedef struct jmh_cabac_slice_bytes {  /* out: where slice i lies in out                          */
    int64_t offset, nbytes;
    int64_t nbins;
} jmh_cabac_slice_bytes;

/* slice_data() + rbsp_trailing_bits of every slice of the picture last popped / waited for.
 * JMH_E_STATE: no picture has been popped.  JMH_E_INVALID_ARG: descriptors that do not tile the
 * picture in raster order, a slice type other than I / P, slice_qp outside 0..51, or cap below the
 * size the device found; out is then untouched, and where[n] is filled whenever the device ran,
 * so that the caller can grow out and call again. */
int  jmh_cabac_write_slices(jmh_ctx *ctx, int n, const jmh_cabac_slice_desc *slices, uint8_t *out, size_t cap,
                            jmh_cabac_slice_bytes *where);
/* unit seam: the same for caller-supplied results (mbw * mbh entries), no picture needed          */
int  jmh_cabac_write_results(jmh_ctx *ctx, const jmh_mb_result *res, int n, const jmh_cabac_slice_desc *slices,
                             uint8_t *out, size_t cap, jmh_cabac_slice_bytes *where);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_CABAC_H */
