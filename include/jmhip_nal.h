/*
 * jmhip_nal.h — NAL units finished on the device: start code, NAL header byte,
 * emulation prevention and cabac_zero_words, so that what a coded picture's pop returns is the
 * picture's Annex B access unit.  Part of the C ABI of jmhip.h (which includes this file after
 * jmhip_input.h).  Additive only: JMH_ABI_VERSION stays 14, no struct or entry point of the other
 * headers changes, jmh_config is not touched.
 *
 * A NAL unit's RBSP is two parts read as one string: its head (host bytes, a slice header for one)
 * and its payload (a byte range of a buffer: of a coded picture, the slice writer's bytes on the
 * device).  Unit i of the output is 00 00 00 01, the byte (nal_ref_idc << 5) | nal_unit_type, then
 * the string with a 03 before every byte <= 3 that follows two zero bytes (7.4.1).  With a positive
 * bin count the cabac_zero_words of 7.4.2.10 / 9.3.4.6 follow the last unit, each as 00 00 03,
 * and count towards it.
 */
#ifndef JMHIP_NAL_H
#define JMHIP_NAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JMH_NAL_HEAD_MAX 64
typedef struct jmh_nal_head {        /* in: one per NAL unit                                        */
    int32_t nal_ref_idc, nal_unit_type;
    int32_t nbytes;                  /* 0..JMH_NAL_HEAD_MAX bytes of the RBSP ahead of the payload */
    uint8_t bytes[JMH_NAL_HEAD_MAX];
} jmh_nal_head;
typedef struct jmh_nal_range {       /* a unit's payload in, its place in the access unit out      */
    int64_t offset, nbytes;
} jmh_nal_range;

/* The constants of the kernels: the input bytes of one wave step and of one wave.  Needs no context
 * and no device. */
int  jmh_nal_geometry(int *tile_bytes, int *chunk_bytes);
/* The synchronous seam: n units of host bytes in, the access unit out, on the context's device.
 * where_in[i] places unit i's payload in payload; nbins_total <= 0: no zero words, else the
 * picture's bins, counted against the context's picture size and bit depth.  where_out[i] places
 * unit i, start code included, in out; *total: the access unit's bytes.  JMH_E_INVALID_ARG with
 * where_out and *total filled, nothing written: cap is below *total. */
int  jmh_nal_wrap(jmh_ctx *ctx, int n, const jmh_nal_head *heads, const uint8_t *payload, const jmh_nal_range *where_in,
                  int64_t nbins_total, uint8_t *out, size_t cap, jmh_nal_range *where_out, int64_t *total);
/* Arms the next coded push of the context (host, 16-bit or device picture) with the heads of its n
 * slices: that picture's writer is followed by the NAL kernels, and its jmh_frame_pop_coded returns
 * the access unit in out, where[i].offset / nbytes placing NAL unit i with its start code (the zero
 * words count towards the last one); nbits / nbins and stats are those of the slice data as ever.
 * The bins of a CABAC picture are the sum of its slices' nbins.  A push whose n differs answers
 * JMH_E_INVALID_ARG with nothing queued; that push, like any other push in between, drops the
 * arming.  A picture whose finished bytes exceed the region queued with it is finished by the
 * synchronous calls at its pop (stats.fallback = 1), with the same bytes. */
int  jmh_coded_nal_heads(jmh_ctx *ctx, int n, const jmh_nal_head *heads);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_NAL_H */
