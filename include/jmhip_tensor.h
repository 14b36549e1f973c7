/*
 * jmhip_tensor.h — RGB tensors pushed from the device: a tensor pipeline's frame is
 * a (3, H, W) or (H, W, 3 or 4) array of uint8, uint16, float16, bfloat16 or float32, the floats in
 * [0, 1].  It is pushed as it is: one kernel quantises it, converts it to 4:2:0, packs and pads it
 * where an RGB device picture (jmhip_rgb.h) is converted.  Part of the C ABI of jmhip.h (which
 * includes this file after jmhip_rgb.h).  Additive only: JMH_ABI_VERSION stays 14, every struct,
 * format value and entry point of the other headers keeps its meaning.
 *
 * The descriptor.  Three channel addresses (R, G, B, at pixel (0, 0)) that share one element type
 * of es bytes, one byte stride between pixels and one between rows; the element of channel c at
 * pixel (x, y) lies at chan[c] + y * stride_y + x * stride_x.  No copy is made by the caller:
 *   CHW planar        chan[i] = base + i * H * W * es, stride_x = es
 *   HWC, C = 3 or 4   chan[i] = base + i * es,         stride_x = C * es
 *   BGR, GBR planar   the same with the addresses permuted
 *   a cropped view    the same, offset to the view's origin
 * flags: JMH_PIX_BT709 and JMH_PIX_FULL_RANGE of jmhip_rgb.h, nothing else.
 *
 * Quantisation.  One element becomes an integer component q in [0, M], M = (1 << bit depth) - 1:
 *   JMH_T_U8    q is the byte                                             (8-bit context)
 *   JMH_T_U16   q = min(v, M)                                            (10-bit context)
 *   the floats  q = floor(x * M + 1/2) in exact arithmetic after x is clamped to [0, 1]: NaN and
 *               everything <= 0 (-0 and -inf too) give 0, everything >= 1 (+inf too) gives M; F16
 *               and BF16 are widened exactly first                  (8- or 10-bit context)
 * A 9-bit context takes no tensor.  Conversion and padding are those of jmhip_rgb.h, applied to the
 * quantised components: Y per pixel, box chroma from the sums of a 2x2 block, both clamped, the
 * picture extended to the coded size as jm_pad_picture of host/yuv.c extends the converted one.
 *
 * JMH_E_INVALID_ARG, checked before anything else, with nothing claimed or queued: a null tensor or
 * channel, a dtype outside the enum, any flag bit but the two, a width or height that is odd,
 * below 2 or above the coded size, stride_x < es, stride_y < (width - 1) * stride_x + es (negative
 * strides are invalid), any address or stride that is no multiple of es.
 * JMH_E_UNSUPPORTED_CFG: a valid tensor in a context of the wrong bit depth.
 *
 * Ordering, streams, the armed NAL heads of jmhip_nal.h and the wait are those of jmhip_input.h's
 * device pictures; tensor pushes alternate freely with host, device-picture and RGB pushes.  The
 * count of clamped input samples of jmhip_input.h answers 0 after a tensor.  The kernel reads only
 * bytes of source elements.  The stream does not signal the matrix or the range (no VUI).
 */
#ifndef JMHIP_TENSOR_H
#define JMHIP_TENSOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { JMH_T_U8 = 0, JMH_T_U16 = 1, JMH_T_F16 = 2, JMH_T_BF16 = 3, JMH_T_F32 = 4 };

typedef struct jmh_device_tensor {
    int32_t dtype, flags, width, height;   /* flags: JMH_PIX_BT709 | JMH_PIX_FULL_RANGE only */
    const void *chan[3];                   /* device addresses of R, G, B at pixel (0, 0)   */
    int64_t stride_x, stride_y;            /* bytes between pixels / rows, shared by the three */
    void *stream;                          /* as jmh_device_picture.stream */
} jmh_device_tensor;

/* jmh_frame_push_device / jmh_frame_push_coded_device of a tensor */
int  jmh_frame_push_tensor(jmh_ctx *ctx, const jmh_device_tensor *tensor, const jmh_frame_params *fp);
int  jmh_frame_push_coded_tensor(jmh_ctx *ctx, const jmh_device_tensor *tensor, const jmh_frame_params *fp, int n,
                                 const jmh_coded_slice *slices, int crop_w, int crop_h);
/* The unit seam of the kernel: the tensor converted into a scratch picture, the packed planes of the
 * coded size copied to the host (samples of 1 byte in an 8-bit context, else 2; strides in samples). */
int  jmh_ingest_tensor(jmh_ctx *ctx, const jmh_device_tensor *tensor, void *y, void *u, void *v, int stride_y, int stride_c);
/* The quantiser on the host: n elements of dtype at elems (any alignment) to q.  JMH_E_INVALID_ARG /
 * JMH_E_UNSUPPORTED_CFG by the rules above.  Needs no context and no device. */
int  jmh_tensor_quantise(int dtype, int bit_depth, const void *elems, size_t n, int32_t *q);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_TENSOR_H */
