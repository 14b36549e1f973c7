/*
 * jmhip_output.h — decoded pictures pulled on the device: the picture a decoder
 * of the stream will show (the deblocked one) or the reconstruction before the loop filter, written
 * by one kernel into device memory of the caller as YUV planes, as packed RGB or as an RGB tensor.
 * The mirror of jmhip_input.h, jmhip_rgb.h and jmhip_tensor.h.  Part of the C ABI of jmhip.h (which
 * includes this file last).  Additive only: JMH_ABI_VERSION stays 14, every struct, enum value and
 * entry point of the other headers keeps its meaning.
 *
 * Which picture.  A pull reads the current picture: the one the last jmh_frame_pop,
 * jmh_frame_pop_coded or jmh_frame_wait returned, the picture jmh_read_deblocked reads, coded or
 * ordinary alike, from the device buffers of its ring entry.  JMH_E_STATE: there is no current
 * picture, or JMH_OUT_DEBLOCKED is asked of a picture that was not deblocked on the device.
 *
 * Size.  width x height is the top-left crop of the coded picture, the display size: even, at
 * least 2, at most the coded size.
 *
 * Formats of jmh_pull_picture (format of jmhip_input.h / jmhip_rgb.h):
 *   JMH_PIX_I420, JMH_PIX_NV12           8-bit context        a cropped copy
 *   JMH_PIX_I010                         9- or 10-bit context a cropped copy, sample in the low bits
 *   JMH_PIX_P010                         10-bit context       word = sample << 6
 *   JMH_PIX_BGRA8, JMH_PIX_RGBA8         8-bit context        converted, alpha 0xFF
 *   JMH_PIX_RGB10A2, JMH_PIX_BGR10A2     10-bit context       converted, alpha 3
 * The four RGB formats are OR-ed with JMH_PIX_BT709 and JMH_PIX_FULL_RANGE as in jmhip_rgb.h.
 * Element types of jmh_pull_tensor (dtype of jmhip_tensor.h): JMH_T_U8 needs an 8-bit context,
 * JMH_T_U16 a 10-bit one, the three float types an 8- or 10-bit one.  A 9-bit context gives neither
 * RGB nor tensors.  A valid destination in a context of the wrong depth: JMH_E_UNSUPPORTED_CFG.
 *
 * Conversion, in 32-bit integers, exact.  Chroma is upsampled by replication: every pixel of a 2x2
 * block takes the block's U and V.  That is the transpose of the box filter of jmhip_rgb.h, so no
 * chroma siting is invented; a filtered upsampler is not offered.  With d = Y - Yo, e = U - Co,
 * f = V - Co and M = (1 << bit depth) - 1 (>> is an arithmetic shift):
 *   R = clamp((iy d         + irv f + 2^13) >> 14, 0, M)
 *   G = clamp((iy d + igu e + igv f + 2^13) >> 14, 0, M)
 *   B = clamp((iy d + ibu e         + 2^13) >> 14, 0, M)
 * jmh_yuv_coefficients returns iy, irv, igu, igv, ibu, Yo, Co, M: the exact rationals M/Ys,
 * 2(1-Kr) M/Cs, -2 Kb(1-Kb)/Kg M/Cs, -2 Kr(1-Kr)/Kg M/Cs, 2(1-Kb) M/Cs times 2^14, rounded half away
 * from zero, with Kr, Kb, Ys, Cs, Yo, Co of jmhip_rgb.h.  The stream does not signal the matrix or the
 * range (no VUI): the flags say how the caller wants the samples read, as they do on the input side.
 *
 * Dequantisation.  JMH_T_U8 and JMH_T_U16 store the component q.  A float stores
 * float32(q) / float32(M), an IEEE round-to-nearest division (no reciprocal approximation), converted
 * to F16 or BF16 with round-to-nearest-even.  jmh_tensor_quantise of the stored element gives q back
 * for every q and every (dtype, bit depth) pair but BF16 at 10 bits: eight significand bits cannot
 * hold 1024 levels, and 511 of the 1024 come back changed.
 *
 * What is written.  Only bytes of destination elements inside width x height: a tensor with
 * stride_x of four elements keeps its fourth channel, row padding and every byte before the first
 * and after the last element stay as they were.
 *
 * JMH_E_INVALID_ARG, checked before anything else, with nothing queued and nothing written: a null
 * descriptor, a null plane or channel (plane[2] of NV12 and P010 and plane[1], plane[2] of RGB are
 * not looked at), a format or dtype outside the enums, a flag on a YUV format or any other bit, a
 * width or height that is odd, below 2 or above the coded size, a stride below the row's bytes,
 * stride_x < es, negative strides, an address or stride that is no multiple of the element size
 * (4 for RGB, 2 for 16-bit planes, es for a tensor), which outside 0..1.
 *
 * Ordering and lifetime.  A pull is one kernel launch, with no allocation in steady state.  With a
 * non-NULL stream the kernel is queued on that stream: it runs behind everything queued there so
 * far (the last consumer of the destination), what is queued there afterwards sees the picture,
 * and the host does not wait.  With stream NULL the picture is complete on return.  The ring entry
 * a pull reads is not rewritten under it: the push that next claims the entry makes the context's
 * stream wait, on the device, for the entry's last pull.  jmh_device_output_wait is the host-side
 * form; draining the context and jmh_destroy include it.
 */
#ifndef JMHIP_OUTPUT_H
#define JMHIP_OUTPUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { JMH_OUT_DEBLOCKED = 0,   /* what a decoder shows                  */
       JMH_OUT_RECON = 1 };     /* the reconstruction before the filter  */

typedef struct jmh_device_picture_out {   /* jmh_device_picture with writable planes */
    int32_t format, width, height;
    void *plane[3];
    int64_t stride[3];
    void *stream;
} jmh_device_picture_out;

typedef struct jmh_device_tensor_out {    /* jmh_device_tensor with writable channels */
    int32_t dtype, flags, width, height;
    void *chan[3];
    int64_t stride_x, stride_y;
    void *stream;
} jmh_device_tensor_out;

int  jmh_pull_picture(jmh_ctx *ctx, int which, const jmh_device_picture_out *dst);
int  jmh_pull_tensor(jmh_ctx *ctx, int which, const jmh_device_tensor_out *dst);
/* Unit seams: host planes of the coded size (strides in samples, as jmh_read_recon; 16-bit samples
 * in a 9 / 10-bit context) uploaded to a scratch picture, the same kernel, complete on return. */
int  jmh_convert_picture(jmh_ctx *ctx, const void *y, const void *u, const void *v, int stride_y, int stride_c,
                         const jmh_device_picture_out *dst);
int  jmh_convert_tensor(jmh_ctx *ctx, const void *y, const void *u, const void *v, int stride_y, int stride_c,
                        const jmh_device_tensor_out *dst);
/* The host blocks until every pull queued so far has completed. */
int  jmh_device_output_wait(jmh_ctx *ctx);
/* The mirror of jmh_device_upload: n bytes of device memory to the host, behind the work queued on
 * stream so far (NULL: behind nothing); dst is complete on return. */
int  jmh_device_download(jmh_ctx *ctx, void *dst, const void *src, size_t n, void *stream);
/* The conversion of the flags (JMH_PIX_BT709 | JMH_PIX_FULL_RANGE) at a bit depth of 8 or 10.  Needs
 * no context and no device.  JMH_E_INVALID_ARG: any other bit, any other depth, a null out. */
int  jmh_yuv_coefficients(int flags, int bit_depth, int32_t out[8]);
/* The dequantiser on the host: n components q (clamped to [0, M]) to n elements of dtype at elems
 * (any alignment).  JMH_E_INVALID_ARG / JMH_E_UNSUPPORTED_CFG by the rules above.  Needs no context
 * and no device. */
int  jmh_tensor_dequantise(int dtype, int bit_depth, const int32_t *q, size_t n, void *elems);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_OUTPUT_H */
