/*
 * jmhip_rgb.h — RGB pictures pushed from the device: a renderer's or a tensor
 * pipeline's frame is BGRA or RGBA at 8 bits, or packed 10-bit RGB; it is pushed as it is and one
 * kernel converts it to 4:2:0, packs and pads it where a YUV device picture (jmhip_input.h) is only
 * packed and padded.  Part of the C ABI of jmhip.h (which includes this file after jmhip_nal.h).
 * Additive only: JMH_ABI_VERSION stays 14, jmh_device_picture keeps its layout, the entry points of
 * jmhip_input.h take the new formats and need no new argument, formats 0 to 3 are as they were.
 *
 * Formats.  New values of jmh_device_picture.format; 4 to 15 stay invalid.  One source plane:
 * plane[0] with stride[0], one little-endian dword per pixel; plane[1], plane[2] and their strides
 * are not read.  Alpha is ignored.  JMH_PIX_BT709 and JMH_PIX_FULL_RANGE are OR-ed into the format:
 * without the first the matrix is BT.601, without the second the range is limited.  The 8-bit
 * layouts need an 8-bit context, the 10-bit ones a 10-bit context; anything else (a 9-bit context,
 * for one) answers JMH_E_UNSUPPORTED_CFG.
 *
 * JMH_E_INVALID_ARG, checked before anything else, with nothing claimed or queued: a null picture
 * or plane[0], a width or height that is odd, below 2 or above the coded size, stride[0] below
 * 4 * width, a plane[0] address or a stride that is no multiple of 4, either flag on a YUV format,
 * any other bit set in the format.
 *
 * Conversion.  In 32-bit integers, Q14 coefficients c (the table of csrc/jmh_rgb.h; what
 * jmh_rgb_coefficients returns), M = (1 << bit depth) - 1:
 *   Y = min(M, Yo + ((cyr R + cyg G + cyb B + 2^13) >> 14))                    for every pixel,
 *   U = clamp(Co + ((cur Rs + cug Gs + cub Bs + 2^15) >> 16), 0, M), V alike   for every 2x2 block,
 * Rs, Gs, Bs the sums of the block's four pixels (box chroma) and >> an arithmetic shift.  The
 * picture is extended to the coded size as jm_pad_picture of host/yuv.c extends the converted one.
 * jmh_device_input_clamped answers 0 for these formats (it counts I010 source samples).
 *
 * The stream does not signal the matrix or the range (no VUI): a decoder's display stage has to be
 * told them.  Ordering, streams and jmh_device_input_wait are those of jmhip_input.h; the kernel
 * reads only dwords of source pixels.
 */
#ifndef JMHIP_RGB_H
#define JMHIP_RGB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { JMH_PIX_BGRA8 = 16,     /* bytes B, G, R, A                              ( 8-bit context) */
       JMH_PIX_RGBA8 = 17,     /* bytes R, G, B, A                              ( 8-bit context) */
       JMH_PIX_RGB10A2 = 18,   /* R bits 0-9, G 10-19, B 20-29, A 30-31         (10-bit context) */
       JMH_PIX_BGR10A2 = 19,   /* B bits 0-9, G 10-19, R 20-29, A 30-31         (10-bit context) */
       JMH_PIX_BT709 = 1 << 8,        /* flag: BT.709 matrix (else BT.601)  */
       JMH_PIX_FULL_RANGE = 1 << 9 }; /* flag: full range (else limited)    */

/* The conversion of a format with its flags at a bit depth: cyr cyg cyb, cur cug cub, cvr cvg cvb,
 * then Yo, Co and M.  JMH_E_INVALID_ARG / JMH_E_UNSUPPORTED_CFG by the rules above (a YUV format is
 * an invalid argument here).  Needs no context and no device. */
int  jmh_rgb_coefficients(int format, int bit_depth, int32_t out[12]);

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_RGB_H */
