/*
 * jmhip_input.h — pictures that are already on the device: a decoder's, a
 * renderer's or a tensor pipeline's frame is pushed from device memory, in the layout it was born
 * in, and the library packs and pads it with one kernel where a host picture is packed on the CPU
 * and uploaded.  Part of the C ABI of jmhip.h (which includes this file last).  Additive only:
 * JMH_ABI_VERSION stays 14, no struct or entry point of the other headers changes, jmh_config is
 * not touched.
 *
 * Padding.  The picture has width x height luma samples, the context's coded size or less.  It is
 * extended to the coded size as host/yuv.c jm_pad_picture does: the last column is replicated to
 * the right and the last row downwards, chroma likewise at half size.
 *
 * Formats.  I420 and NV12 need an 8-bit context, I010 a 9- or 10-bit one, P010 a 10-bit one (its
 * sample is word >> 6); anything else answers JMH_E_UNSUPPORTED_CFG.  An I010 sample above
 * (1 << bit depth) - 1 cannot reject the picture synchronously as jmh_frame_push_u16 does: the
 * kernel stores min(sample, maxv) (what lencod's reader of 16-bit files does) and counts such
 * samples of the width x height source; jmh_device_input_clamped returns the count.  The RGB layouts
 * (format 16 to 19 with their flag bits, converted to 4:2:0 by the library) are jmhip_rgb.h's.
 *
 * JMH_E_INVALID_ARG, with nothing claimed or queued: a null picture or plane (plane[2] of NV12 and
 * P010 is not read), a format outside the enum, a width or height that is odd, below 2 or above
 * the coded size, a stride below the row's bytes, and for the 16-bit formats an odd plane address
 * or an odd stride.  These checks come before every other one.
 *
 * Ordering.  The packing kernel runs on the context's stream where a host picture's upload runs,
 * so everything that reads the source afterwards is ordered as before.  With a non-NULL stream the
 * kernel waits for the work queued on that stream so far, and the stream is made to wait for the
 * kernel: work queued on it after the push returns may overwrite the planes.  With stream NULL the
 * planes must be complete when the push is called; before they are rewritten from the host or from
 * any other stream, call jmh_device_input_wait.  The kernel reads, of every row, only the aligned
 * 16-byte blocks that hold one of the row's bytes.
 *
 * No host staging buffer is allocated or written for a device picture.  Host-pushed and
 * device-pushed pictures, coded or ordinary, may alternate in one context; pops are unchanged.
 */
#ifndef JMHIP_INPUT_H
#define JMHIP_INPUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { JMH_PIX_I420 = 0,   /* 8-bit planar Y, U, V                                   */
       JMH_PIX_NV12 = 1,   /* 8-bit Y plane + interleaved UV plane (plane[2] unused)  */
       JMH_PIX_I010 = 2,   /* 16-bit planar, sample in the low bits (bit depth 9/10)  */
       JMH_PIX_P010 = 3 }; /* 16-bit Y + interleaved UV, sample in the HIGH 10 bits   */

typedef struct jmh_device_picture {
    int32_t format, width, height;  /* source size in luma samples: even, 2..coded size  */
    const void *plane[3];           /* device addresses                                  */
    int64_t stride[3];              /* bytes per row; >= the row's bytes                 */
    void *stream;                   /* hipStream_t on which the planes are complete; NULL: complete now */
} jmh_device_picture;

/* jmh_frame_push / jmh_frame_push_coded of a device picture; everything but the source as there */
int  jmh_frame_push_device(jmh_ctx *ctx, const jmh_device_picture *pic, const jmh_frame_params *fp);
int  jmh_frame_push_coded_device(jmh_ctx *ctx, const jmh_device_picture *pic, const jmh_frame_params *fp, int n,
                                 const jmh_coded_slice *slices, int crop_w, int crop_h);
/* Unit seam: the same kernel into a scratch picture, returned as planes of the coded size (strides
 * in samples, as jmh_read_recon; 16-bit samples in a 9 / 10-bit context).  No picture is pushed;
 * jmh_device_input_clamped afterwards answers for this call. */
int  jmh_ingest_picture(jmh_ctx *ctx, const jmh_device_picture *pic, void *y, void *u, void *v, int stride_y, int stride_c);
/* The host blocks until the last pushed device picture has been packed (its planes are free). */
int  jmh_device_input_wait(jmh_ctx *ctx);
/* Samples above maxv of the picture last popped (0 unless it was an I010 device picture). */
int  jmh_device_input_clamped(const jmh_ctx *ctx, uint64_t *n);

/* For callers without a HIP runtime of their own (lencod, the tests): memory and streams of the
 * context's device.  jmh_device_upload copies n host bytes; src may be reused when it returns.
 * With a stream the copy is queued on it (through a pinned buffer of the context), with NULL it
 * has completed on return. */
int  jmh_device_malloc(jmh_ctx *ctx, size_t n, void **p);
int  jmh_device_free(jmh_ctx *ctx, void *p);
int  jmh_device_upload(jmh_ctx *ctx, void *dst, const void *src, size_t n, void *stream);
int  jmh_device_stream_create(jmh_ctx *ctx, void **stream);
int  jmh_device_stream_destroy(jmh_ctx *ctx, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_INPUT_H */
