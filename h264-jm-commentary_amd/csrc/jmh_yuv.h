/*
 * jmh_yuv.h — what a sample of the coded picture is when the device picture is 4:2:2 or 4:4:4
 * (include/jmhip_yuv.h).  The single statement of
 *   - the eleven layouts: where the samples of Y, U and V lie in a source row (jmy_comp: the plane,
 *     the bits between consecutive samples, the first sample's bit, the sample's bits and its shift),
 *     so a sample is one bit field of the row for planar, semi-planar and packed layouts alike,
 *   - the value: field >> shift (P210, Y210: the high 10 bits of a word), min(field, maxv) for the
 *     low-bit 16-bit layouts (I210, I410) and which samples count as clamped (those of the source,
 *     each once),
 *   - the three reductions of chroma to 4:2:0 (jmy_hsum over a source row, jmy_round over two rows),
 *   - the padding: coded sample (x, y) is the reduced picture's (min(x, n - 1), min(y, m - 1)): the
 *     reduction at the source size and then host/yuv.c jm_pad_picture,
 *   - the argument rules (jmy_check).
 *
 * k_ingest_yuv (jmh_yuv.hip) takes every offset and value from here; the runs it loads whole are
 * runs of samples whose fields are consecutive.  jmy_reduce below is the same walk sample by sample:
 * the reference of the kernel's tests and what tests/harness/yuv_check.c runs on exact-size planes
 * under ASan.
 *
 * All arithmetic is in unsigned 32-bit integers; the largest sum is 8 * 1023 + 4.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_YUV_H
#define JMH_YUV_H

#include <stdint.h>
#include <string.h>
#include "jmh_ingest.h"   /* JMI_FN, jmi_clamp, jmi_dst_off: the padding and the packed layout are the same */

/* jmh_device_picture.format: a layout, OR-ed with the flag */
#define JMY_I422 32    /* planar Y, U, V; chroma w/2 x h                                  8-bit context */
#define JMY_NV16 33    /* Y plane + plane of U,V byte pairs, w bytes x h                  8-bit context */
#define JMY_YUYV 34    /* one plane, bytes Y0 U Y1 V                                      8-bit context */
#define JMY_UYVY 35    /* one plane, bytes U Y0 V Y1                                      8-bit context */
#define JMY_I444 36    /* planar, three full-size planes                                  8-bit context */
#define JMY_VUYA8 37   /* one plane of dwords, bytes V, U, Y, A                           8-bit context */
#define JMY_I210 40    /* 16-bit planar 4:2:2, sample in the low bits               9- or 10-bit context */
#define JMY_P210 41    /* 16-bit Y + interleaved UV, sample = word >> 6                  10-bit context */
#define JMY_Y210 42    /* one plane, words Y0 U Y1 V, sample = word >> 6                 10-bit context */
#define JMY_I410 43    /* 16-bit planar 4:4:4, sample in the low bits               9- or 10-bit context */
#define JMY_Y410 44    /* one plane of dwords: U bits 0-9, Y 10-19, V 20-29, A 30-31     10-bit context */
#define JMY_CHROMA_LEFT (1 << 10)   /* 4:4:4: the 4:2:0 chroma is left-sited (else centred); 4:2:2: no effect */

JMI_PRED int jmy_layout(int format) { return format & ~JMY_CHROMA_LEFT; }
/* one of the eleven layouts with no bit but the flag */
JMI_PRED int jmy_is_yuv(int format) {
    return format >= 0 && ((jmy_layout(format) >= JMY_I422 && jmy_layout(format) <= JMY_VUYA8) || (jmy_layout(format) >= JMY_I210 && jmy_layout(format) <= JMY_Y410));
}
JMI_PRED int jmy_wide(int layout) { return layout >= JMY_I210; }                                   /* 16-bit output samples */
JMI_PRED int jmy_444(int layout) { return layout == JMY_I444 || layout == JMY_VUYA8 || layout == JMY_I410 || layout == JMY_Y410; }
JMI_PRED int jmy_clamps(int layout) { return layout == JMY_I210 || layout == JMY_I410; }           /* min(sample, maxv), counted */
JMI_PRED int jmy_dwords(int layout) { return layout == JMY_VUYA8 || layout == JMY_Y410; }          /* a pixel is a dword */
JMI_PRED int jmy_planes(int layout) {                                                              /* source planes read */
    return layout == JMY_NV16 || layout == JMY_P210 ? 2 : layout == JMY_I422 || layout == JMY_I444 || layout == JMY_I210 || layout == JMY_I410 ? 3 : 1;
}
/* the left-sited reduction is asked for and means something */
JMI_PRED int jmy_left(int format) { return (format & JMY_CHROMA_LEFT) && jmy_444(jmy_layout(format)); }
/* the bit depths of a context that takes the format */
JMI_FN int jmy_depth_ok(int format, int bd) {
    const int l = jmy_layout(format);
    return !jmy_wide(l) ? bd == 8 : jmy_clamps(l) ? bd == 9 || bd == 10 : bd == 10;
}

/* Component c (0 Y, 1 U, 2 V) of a layout: its sample k of a row is the bit field of `bits` bits at
 * bit k * pitch + first of the row of plane sp (little-endian), shifted right by `shift`. */
typedef struct jmy_field { int sp, pitch, first, bits, shift; } jmy_field;
#if defined(__cplusplus)
#define JMY_F(...) jmy_field{__VA_ARGS__}
#else
#define JMY_F(...) (jmy_field){__VA_ARGS__}
#endif
JMI_PRED jmy_field jmy_comp(int layout, int c) {
    return layout == JMY_I422 || layout == JMY_I444 ? JMY_F(c, 8, 0, 8, 0)
         : layout == JMY_NV16 ? (c == 0 ? JMY_F(0, 8, 0, 8, 0) : JMY_F(1, 16, 8 * (c - 1), 8, 0))
         : layout == JMY_YUYV ? (c == 0 ? JMY_F(0, 16, 0, 8, 0) : JMY_F(0, 32, 16 * c - 8, 8, 0))
         : layout == JMY_UYVY ? (c == 0 ? JMY_F(0, 16, 8, 8, 0) : JMY_F(0, 32, 16 * (c - 1), 8, 0))
         : layout == JMY_VUYA8 ? JMY_F(0, 32, 16 - 8 * c, 8, 0)
         : layout == JMY_I210 || layout == JMY_I410 ? JMY_F(c, 16, 0, 16, 0)
         : layout == JMY_P210 ? (c == 0 ? JMY_F(0, 16, 0, 16, 6) : JMY_F(1, 32, 16 * (c - 1), 16, 6))
         : layout == JMY_Y210 ? (c == 0 ? JMY_F(0, 32, 0, 16, 6) : JMY_F(0, 64, 32 * c - 16, 16, 6))
         : /* JMY_Y410 */       JMY_F(0, 32, c == 0 ? 10 : c == 1 ? 0 : 20, 10, 0);
}
/* samples of component c in a source row of w luma samples */
JMI_PRED int jmy_comp_width(int layout, int c, int w) { return c == 0 || jmy_444(layout) ? w : w / 2; }
/* bytes of a row of source plane sp that hold samples */
JMI_FN int64_t jmy_row_bytes(int layout, int sp, int w) {
    int64_t n = 0;
    for (int c = 0; c < 3; c++) {
        const jmy_field f = jmy_comp(layout, c);
        const int64_t b = (int64_t)jmy_comp_width(layout, c, w) * f.pitch / 8;
        if (f.sp == sp && b > n) n = b;
    }
    return n;
}

/* the raw field of sample k of a row (row: the row's first byte in the field's plane) */
JMI_FN uint32_t jmy_raw(jmy_field f, const uint8_t *row, int k) {
    const int64_t bit = (int64_t)k * f.pitch + f.first;
    const uint8_t *p = row + bit / 8;
    if (f.bits == 8) return p[0];
#if defined(__HIP_DEVICE_COMPILE__)
    if (f.bits == 16) return *(const uint16_t *)p;                              /* word aligned by the argument rule  */
    return *(const uint32_t *)(row + (int64_t)4 * k) >> f.first & 1023u;        /* dword aligned by the argument rule */
#else
    if (f.bits == 16) return (uint32_t)p[0] | (uint32_t)p[1] << 8;
    p = row + (int64_t)4 * k;
    return ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24) >> f.first & 1023u;
#endif
}
/* the stored value of a raw field; *over is raised by one when it was clamped */
JMI_FN uint32_t jmy_value(int layout, jmy_field f, uint32_t raw, uint32_t maxv, uint32_t *over) {
    if (jmy_clamps(layout) && raw > maxv) { *over += 1; return maxv; }
    return raw >> f.shift;
}
/* sample k of a row: jmy_raw and jmy_value */
JMI_FN uint32_t jmy_sample(int layout, jmy_field f, const uint8_t *row, int k, uint32_t maxv, uint32_t *over) {
    return jmy_value(layout, f, jmy_raw(f, row, k), maxv, over);
}

/* The reductions.  A source chroma row gives one sum per output column i from its samples
 * l = C[max(2i - 1, 0)] (left-sited only), a = C[2i], b = C[2i + 1] (4:2:2: a = C[i] alone); the
 * output sample is the rounded mean of the sums of source rows 2j and 2j + 1. */
JMI_FN uint32_t jmy_hsum(int is444, int left, uint32_t l, uint32_t a, uint32_t b) { return !is444 ? a : left ? l + 2 * a + b : a + b; }
JMI_FN uint32_t jmy_round(int is444, int left, uint32_t h0, uint32_t h1) {
    return !is444 ? (h0 + h1 + 1) >> 1 : left ? (h0 + h1 + 4) >> 3 : (h0 + h1 + 2) >> 2;
}

/* Sample (x, y) of plane pl (0 Y, 1 U, 2 V) of the coded picture from a w x h source.  *over is
 * raised by the clamped samples of the source this sample is the first to read: its own when it
 * lies inside the reduced picture (not a replica of the padding); the left neighbour belongs to the
 * column before. */
JMI_FN uint32_t jmy_coded_sample(int format, const uint8_t *const *plane, const int64_t *stride, int pl, int x, int y, int w, int h, uint32_t maxv,
                                 uint32_t *over) {
    const int layout = jmy_layout(format), is444 = jmy_444(layout), left = jmy_left(format);
    const jmy_field f = jmy_comp(layout, pl);
    const int cx = jmi_clamp(x, pl ? w / 2 : w), cy = jmi_clamp(y, pl ? h / 2 : h);
    const int mine = x == cx && y == cy;
    uint32_t o = 0, none = 0, v;
    if (pl == 0) {
        v = jmy_sample(layout, f, plane[f.sp] + (int64_t)cy * stride[f.sp], cx, maxv, &o);
    } else {
        uint32_t hs[2];
        for (int r = 0; r < 2; r++) {
            const uint8_t *row = plane[f.sp] + (int64_t)(2 * cy + r) * stride[f.sp];
            const int k = is444 ? 2 * cx : cx;
            const uint32_t a = jmy_sample(layout, f, row, k, maxv, &o);
            const uint32_t b = is444 ? jmy_sample(layout, f, row, k + 1, maxv, &o) : 0;
            const uint32_t l = left ? jmy_sample(layout, f, row, k ? k - 1 : 0, maxv, &none) : 0;
            hs[r] = jmy_hsum(is444, left, l, a, b);
        }
        v = jmy_round(is444, left, hs[0], hs[1]);
    }
    if (mine) *over += o;
    return v;
}

/* JMH_OK's 0, or -1: the argument rules of jmhip_yuv.h (everything but the context's bit depth).
 * Planes the layout does not read and their strides are not looked at. */
JMI_FN int jmy_check(int format, int w, int h, int W, int H, const void *const *plane, const int64_t *stride) {
    if (!jmy_is_yuv(format)) return -1;
    const int layout = jmy_layout(format);
    if (w < 2 || h < 2 || (w & 1) || (h & 1) || w > W || h > H) return -1;
    const unsigned align = jmy_dwords(layout) ? 3 : jmy_wide(layout) ? 1 : 0;
    for (int sp = 0; sp < jmy_planes(layout); sp++) {
        if (!plane[sp] || stride[sp] < jmy_row_bytes(layout, sp, w)) return -1;
        if (((uintptr_t)plane[sp] | (uint64_t)stride[sp]) & align) return -1;
    }
    return 0;
}

/* The whole picture sample by sample into dst (packed W x H, 4:2:0, samples of 1 byte in an 8-bit
 * context, else 2); returns the clamped samples of the source. */
JMI_FN uint64_t jmy_reduce(int format, const uint8_t *const *plane, const int64_t *stride, int w, int h, int W, int H, uint32_t maxv, uint8_t *dst) {
    const int es = jmy_wide(jmy_layout(format)) ? 2 : 1;
    uint64_t clamped = 0;
    for (int pl = 0; pl < 3; pl++) {
        const int PW = pl ? W / 2 : W, PH = pl ? H / 2 : H;
        uint8_t *d = dst + jmi_dst_off(pl, W, H) * es;
        for (int y = 0; y < PH; y++)
            for (int x = 0; x < PW; x++) {
                uint32_t over = 0;
                const uint32_t v = jmy_coded_sample(format, plane, stride, pl, x, y, w, h, maxv, &over);
                clamped += over;
                if (es == 2) { const uint16_t t = (uint16_t)v; memcpy(d + ((size_t)y * PW + x) * 2, &t, 2); }
                else d[(size_t)y * PW + x] = (uint8_t)v;
            }
    }
    return clamped;
}

#endif /* JMH_YUV_H */
