/*
 * jmhip_coded.h — coded pictures: a pipelined picture whose slice data is written
 * on the device behind its last macroblock, under the pictures still in flight, and whose pop
 * returns the slice bytes and the distortion only.  Part of the C ABI of jmhip.h (which includes
 * this file after jmhip_cavlc.h and jmhip_cabac.h).  Additive only: JMH_ABI_VERSION stays 14, no
 * struct or entry point of the other three headers changes, jmh_config is not touched.
 *
 * The entropy coder follows jmh_config.symbol_mode of the context (0: CAVLC, 1: CABAC).  Contract:
 * for every slice, out[offset .. offset + nbytes) is byte for byte what jmh_cavlc_write_slices /
 * jmh_cabac_write_slices produce for the same picture and descriptors, and nbytes, nbits (CAVLC)
 * and nbins (CABAC) are equal too; their meaning is that of jmhip_cavlc.h and jmhip_cabac.h (the
 * field of the other coder is 0).  Slice headers, NAL wrapping and cabac_zero_words stay with the
 * caller.
 *
 * A coded picture is not read back: no macroblock results, reconstruction or deblocked picture
 * cross to the host at its pop, and jmh_get_mb_result returns NULL for it.  jmh_read_recon /
 * jmh_read_deblocked after its pop copy the picture from the device on demand.  Coded and ordinary
 * pictures may be mixed in one context: they share the ring and the reference chain
 * (jmh_set_reference_slot with -1 / -2 as before), and are popped in push order, each by its own pop.
 */
#ifndef JMHIP_CODED_H
#define JMHIP_CODED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jmh_coded_slice {     /* in: one per slice, raster runs tiling the picture          */
    int32_t first_mb, n_mb;
    int32_t slice_type;              /* JMH_P_SLICE / JMH_I_SLICE                                  */
    int32_t slice_qp;                /* CABAC (symbol_mode 1): SliceQPY of the header, 0..51       */
    int32_t lead_nbits;              /* CAVLC (symbol_mode 0): as jmh_slice_desc                   */
    uint32_t lead_bits;
} jmh_coded_slice;
typedef struct jmh_coded_bytes {     /* out: where slice i lies in out                             */
    int64_t offset, nbytes;
    int64_t nbits;                   /* CAVLC: as jmh_slice_bytes.nbits; CABAC: 0                  */
    int64_t nbins;                   /* CABAC: as jmh_cabac_slice_bytes.nbins; CAVLC: 0            */
} jmh_coded_bytes;
typedef struct jmh_coded_stats {
    uint64_t ssd[3];                 /* Y, U, V: sum over crop_w x crop_h (chroma: both halved) of
                                        (source as pushed - the picture's output)^2; the output is
                                        the deblocked picture when fp->deblock is set, else the
                                        reconstruction.  Exact, for 8-bit and 9 / 10-bit samples  */
    int32_t fallback;                /* 1: a counted size exceeded the capacity queued with the
                                        picture, which was then coded by the synchronous path at
                                        its pop; the capacities of later pictures have grown      */
    int32_t reserved;
} jmh_coded_stats;

/* jmh_frame_push with the picture's n slices: its slice data is queued behind its last macroblock.
 * JMH_E_INVALID_ARG, with nothing queued: descriptors that do not tile the picture in raster
 * order (or a lead / QP field out of range for the context's coder), a crop outside 1..width x
 * 1..height.  Otherwise as jmh_frame_push. */
int  jmh_frame_push_coded(jmh_ctx *ctx, const uint8_t *y, const uint8_t *u, const uint8_t *v, int stride_y, int stride_c,
                          const jmh_frame_params *fp, int n, const jmh_coded_slice *slices, int crop_w, int crop_h);
int  jmh_frame_push_coded_u16(jmh_ctx *ctx, const uint16_t *y, const uint16_t *u, const uint16_t *v, int stride_y, int stride_c,
                              const jmh_frame_params *fp, int n, const jmh_coded_slice *slices, int crop_w, int crop_h);
/* The oldest pushed picture, which must be a coded one: where[n], stats, and the bytes into out.
 * JMH_E_STATE, nothing consumed: no picture is waiting, or the oldest one is an ordinary picture
 * (jmh_frame_pop on a coded picture answers the same).  JMH_E_INVALID_ARG with where[] filled and
 * the picture still waiting: cap is below the picture's bytes (where[n - 1].offset + nbytes); grow
 * out and pop again. */
int  jmh_frame_pop_coded(jmh_ctx *ctx, uint8_t *out, size_t cap, jmh_coded_bytes *where, jmh_coded_stats *stats);
/* The ring entries of the context (each holds one picture's buffers, the writer's among them):
 * after this many pushes every entry has had a second occupant.  At least jmh_pipeline_depth + 2. */
int  jmh_coded_ring_entries(const jmh_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_CODED_H */
