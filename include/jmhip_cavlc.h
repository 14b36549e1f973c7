/*
 * jmhip_cavlc.h — CAVLC slice data written on the device: replaces the
 * write_one_macroblock loop of JM 8.6 slice.c › encode_one_slice [J] for SymbolMode 0.  Part of the
 * C ABI of jmhip.h (which includes this file).  Additive only: JMH_ABI_VERSION stays 14, no struct
 * or entry point of jmhip.h changes, jmh_config is not touched.
 *
 * The caller writes each slice header on the host and hands over the bits of the header's last,
 * partial byte; the device writes slice_data() and rbsp_trailing_bits behind them.  Contract: for
 * every slice, (the header's whole bytes) || out[offset .. offset + nbytes) equals, byte for byte,
 * the RBSP that host/bitstream.c › jm_write_slice / jm_slice_restart produce; the first device byte
 * carries lead_bits in its top lead_nbits bits.  NAL wrapping (start code, emulation prevention)
 * stays with the caller.  transform_8x8_mode and constrained_intra_pred come from the context's
 * configuration.
 */
#ifndef JMHIP_CAVLC_H
#define JMHIP_CAVLC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jmh_slice_desc {      /* in: one per slice, raster runs covering the picture       */
    int32_t first_mb, n_mb;
    int32_t slice_type;              /* JMH_P_SLICE / JMH_I_SLICE                                  */
    int32_t lead_nbits;              /* 0..7: bits of the slice header's last, partial byte        */
    uint32_t lead_bits;              /* their value (low lead_nbits bits, first bit most significant) */
} jmh_slice_desc;
typedef struct jmh_slice_bytes {     /* out: where slice i lies in out                             */
    int64_t offset, nbytes;          /* nbytes = nbits / 8 + 1: rbsp_trailing_bits included        */
    int64_t nbits;                   /* lead_nbits + the bits of slice_data()                      */
} jmh_slice_bytes;

/* slice_data() + rbsp_trailing_bits of every slice of the picture last popped / waited for.
 * JMH_E_STATE: no picture has been popped.  JMH_E_INVALID_ARG: descriptors that do not tile the
 * picture in raster order, or cap below the counted size; out is then untouched (the size is
 * counted on the device before anything is written).  where[n] is filled whenever the count ran. */
int  jmh_cavlc_write_slices(jmh_ctx *ctx, int n, const jmh_slice_desc *slices, uint8_t *out, size_t cap,
                            jmh_slice_bytes *where);
/* unit seam: the same for caller-supplied results (mbw * mbh entries), no picture needed          */
int  jmh_cavlc_write_results(jmh_ctx *ctx, const jmh_mb_result *res, int n, const jmh_slice_desc *slices,
                             uint8_t *out, size_t cap, jmh_slice_bytes *where);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_CAVLC_H */
