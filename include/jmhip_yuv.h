/*
 * jmhip_yuv.h — 4:2:2 and 4:4:4 pictures pushed from the device: a capture
 * card's frame is UYVY, YUY2 or Y210, a JPEG, ProRes or DNx decoder hands over 4:2:2 or 4:4:4 planes,
 * a renderer that works in YUV has AYUV or Y410.  The picture is pushed as it is and one kernel
 * reduces its chroma to 4:2:0, packs and pads it where a 4:2:0 device picture (jmhip_input.h) is only
 * packed and padded.  Part of the C ABI of jmhip.h (which includes this file after jmhip_rgb.h).
 * Additive only: JMH_ABI_VERSION stays 14, jmh_device_picture keeps its layout, the entry points of
 * jmhip_input.h (jmh_frame_push_device, jmh_frame_push_coded_device, jmh_ingest_picture) take the new
 * formats and need no new argument, formats 0 to 3 and 16 to 19 are as they were.  This header
 * declares no function.
 *
 * Formats.  New values of jmh_device_picture.format; 4 to 15, 20 to 31, 38, 39 and everything from
 * 45 on stay invalid.  width and height are the luma size: even, 2..coded size (under
 * jmh_input_scale: 2..JMH_SCALE_SRC_MAX; the picture is reduced at its own size and then scaled as
 * a 4:2:0 one is, jmhip_scale.h).  Planes a format does not use and their strides are not read.
 *   4:2:2  I422  planar Y, U, V; the chroma planes have width / 2 samples x height rows
 *          NV16  Y plane, and plane[1] of U,V byte pairs: width bytes x height rows
 *          YUYV  plane[0] alone, bytes Y0 U Y1 V per pixel pair (YUY2); stride >= 2 * width
 *          UYVY  plane[0] alone, bytes U Y0 V Y1
 *          I210  I422 in 16-bit words, the sample in the low bits
 *          P210  NV16 in 16-bit words, sample = word >> 6
 *          Y210  YUYV in 16-bit words, sample = word >> 6; stride >= 4 * width
 *   4:4:4  I444  planar, three planes of width x height
 *          VUYA8 plane[0] alone, a dword per pixel: bytes V, U, Y, A (AYUV); alpha is ignored
 *          I410  I444 in 16-bit words, the sample in the low bits
 *          Y410  plane[0] alone, a dword per pixel: U bits 0-9, Y 10-19, V 20-29, A 30-31
 * The 8-bit formats need an 8-bit context, I210 and I410 a 9- or 10-bit one, P210, Y210 and Y410 a
 * 10-bit one; anything else answers JMH_E_UNSUPPORTED_CFG.
 *
 * JMH_PIX_CHROMA_LEFT is OR-ed into the format.  It says where the 4:2:0 chroma samples are to lie
 * horizontally (with the left luma column; without it: centred between the two, as the box filter
 * of jmhip_rgb.h puts them) and has a meaning for the 4:4:4 formats only.  On the 4:2:2 formats it is
 * accepted and has no effect: their chroma is sited already and only rows are merged.  On formats
 * 0 to 3 and 16 to 19 it is an invalid argument, as every unknown bit is.
 *
 * JMH_E_INVALID_ARG, checked before anything else, with nothing claimed or queued: a null picture
 * or a null plane that the format reads, a width or height that is odd, below 2 or above the bound,
 * a stride below the row's bytes, for the formats of 16-bit words an odd plane address or stride,
 * for the two formats of dwords (VUYA8, Y410) a plane address or stride that is no multiple of 4
 * (as jmhip_rgb.h asks of its dwords), JMH_PIX_BT709 or JMH_PIX_FULL_RANGE or any other bit but
 * JMH_PIX_CHROMA_LEFT.
 *
 * Arithmetic, in exact integers.  M = (1 << bit depth) - 1.  A sample of I210 or I410 above M is
 * taken as M before anything else and counted once (luma and both chroma planes of the
 * width x height source, not the padding): jmh_device_input_clamped returns the count, as for I010.
 * Luma is copied.  Output chroma sample (i, j) of a source chroma plane C (rows C[r], r < height):
 *   4:2:2                              (C[2j][i] + C[2j+1][i] + 1) >> 1
 *   4:4:4 centred (default)            (C[2j][2i] + C[2j][2i+1] + C[2j+1][2i] + C[2j+1][2i+1] + 2) >> 2
 *   4:4:4 with JMH_PIX_CHROMA_LEFT     h(r) = C[r][max(2i-1, 0)] + 2 C[r][2i] + C[r][2i+1],
 *                                      (h(2j) + h(2j+1) + 4) >> 3
 * Vertically the result lies between the two rows in all three.  The reduced picture (width x height
 * luma, half of each in chroma) is extended to the coded size as jm_pad_picture of host/yuv.c
 * extends a picture: its last column and row replicated.  So a 4:2:2 or centred 4:4:4 source whose
 * chroma is the replication of a 4:2:0 picture's chroma gives that picture back, byte for byte.
 *
 * Ordering, streams and jmh_device_input_wait are those of jmhip_input.h; the kernel reads, of every
 * source row, only the aligned 16-byte blocks that hold one of the row's bytes.
 */
#ifndef JMHIP_YUV_H
#define JMHIP_YUV_H

#ifdef __cplusplus
extern "C" {
#endif

enum { JMH_PIX_I422 = 32,    /* 8-bit planar 4:2:2                                      ( 8-bit context) */
       JMH_PIX_NV16 = 33,    /* 8-bit Y plane + interleaved UV plane, 4:2:2             ( 8-bit context) */
       JMH_PIX_YUYV = 34,    /* bytes Y0 U Y1 V (YUY2)                                  ( 8-bit context) */
       JMH_PIX_UYVY = 35,    /* bytes U Y0 V Y1                                         ( 8-bit context) */
       JMH_PIX_I444 = 36,    /* 8-bit planar 4:4:4                                      ( 8-bit context) */
       JMH_PIX_VUYA8 = 37,   /* bytes V, U, Y, A (AYUV)                                 ( 8-bit context) */
       JMH_PIX_I210 = 40,    /* 16-bit planar 4:2:2, sample in the low bits        (9- / 10-bit context) */
       JMH_PIX_P210 = 41,    /* 16-bit Y + interleaved UV, sample in the HIGH 10 bits   (10-bit context) */
       JMH_PIX_Y210 = 42,    /* words Y0 U Y1 V, sample in the HIGH 10 bits             (10-bit context) */
       JMH_PIX_I410 = 43,    /* 16-bit planar 4:4:4, sample in the low bits        (9- / 10-bit context) */
       JMH_PIX_Y410 = 44,    /* U bits 0-9, Y 10-19, V 20-29, A 30-31                   (10-bit context) */
       JMH_PIX_CHROMA_LEFT = 1 << 10 };   /* flag: 4:4:4 is reduced to left-sited chroma (else centred) */

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_YUV_H */
