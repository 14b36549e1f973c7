/*
 * jmh_output.h — what an element of the caller's destination is when a decoded picture is pulled on
 * the device (include/jmhip_output.h).  The single statement of
 *   - the inverse conversion: Q14 coefficients (the table below, literals), R, G and B of a pixel
 *     from its Y and the U and V of its 2x2 block (chroma by replication), clamped (jmout_rgb),
 *   - the dequantiser: how a component q in [0, M] becomes an element of a tensor (jmout_dequant):
 *     q itself for U8 and U16, float32(q) / float32(M) under IEEE division for the floats, rounded
 *     to nearest even into F16 and BF16,
 *   - the packers: the dword of an RGB pixel (jmout_pack), the stored word of a YUV sample
 *     (jmout_yuv_value), where an element lies (jmi_src's and jmt_src_off's arithmetic, reused),
 *   - the argument rules (jmout_check_picture, jmout_check_tensor and the two depth rules), which are
 *     those of the input side and are taken from there, not restated.
 *
 * k_pull_picture and k_pull_tensor (jmh_output.hip) take every value from here; jmout_picture and
 * jmout_tensor below are the same walk sample by sample, writing nothing but destination elements:
 * the reference of the kernels' tests and what tests/harness/output_check.c runs into exact-size
 * destinations under ASan.
 *
 * All arithmetic is in 32-bit integers; >> of a negative value is an arithmetic shift (it floors).
 * Every operand fits 24 bits (coefficients: 34711 at most; differences within +-1023) and the sums
 * stay below 2^26, so a 24-bit multiply-add (JMR_MAD) is exact.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_OUTPUT_H
#define JMH_OUTPUT_H

#include <stdint.h>
#include <string.h>
#include "jmh_tensor.h"   /* jmh_rgb.h and jmh_ingest.h with it: formats, dtypes, flags, the argument rules */

#define JMOUT_DEBLOCKED 0
#define JMOUT_RECON 1

/* the conversion of one picture: the 8 words of jmh_yuv_coefficients */
typedef struct jmout_coef { int32_t iy, irv, igu, igv, ibu, yo, co, maxv; } jmout_coef;

/* c = the exact rational times 2^14, rounded half away from zero, of iy = M/Ys, irv = 2(1-Kr) M/Cs,
 * igu = -2 Kb(1-Kb)/Kg M/Cs, igv = -2 Kr(1-Kr)/Kg M/Cs, ibu = 2(1-Kb) M/Cs; Kr, Kb, Ys, Cs as in
 * jmh_rgb.h, Kg = 1 - Kr - Kb.  Rows as jmr_table_row: matrix * 3 + (full range: 2, else 10-bit: 1,
 * else 0). */
JMI_FN void jmout_table_row(int row, int32_t *c) {
    static const int32_t T[6][5] = {
        {19077, 26149, -6419, -13320, 33050},    /* 601  8 limited */
        {19133, 26226, -6438, -13359, 33148},    /* 601 10 limited */
        {16384, 22970, -5638, -11700, 29032},    /* 601 full       */
        {19077, 29372, -3494, -8731, 34610},     /* 709  8 limited */
        {19133, 29459, -3504, -8757, 34711},     /* 709 10 limited */
        {16384, 25802, -3069, -7670, 30402}};    /* 709 full       */
    for (int i = 0; i < 5; i++) c[i] = T[row][i];
}
/* the conversion of the flags (JMR_BT709 | JMR_FULL_RANGE; other bits are not looked at) at bd 8 or 10 */
JMI_FN void jmout_coefficients(int flags, int bd, jmout_coef *k) {
    const int full = (flags & JMR_FULL_RANGE) != 0;
    int32_t c[5];
    jmout_table_row(((flags & JMR_BT709) ? 3 : 0) + (full ? 2 : bd == 10 ? 1 : 0), c);
    k->iy = c[0]; k->irv = c[1]; k->igu = c[2]; k->igv = c[3]; k->ibu = c[4];
    k->yo = full ? 0 : 16 << (bd - 8);
    k->co = 1 << (bd - 1);
    k->maxv = (1 << bd) - 1;
}

/* what the U and V of a 2x2 block add to R, G and B of its four pixels, rounding term included */
JMI_FN void jmout_chroma_terms(const jmout_coef *k, int32_t u, int32_t v, int32_t *t) {
    const int32_t e = u - k->co, f = v - k->co, half = 1 << (JMR_Q - 1);
    t[0] = JMR_MAD(k->irv, f, half);
    t[1] = JMR_MAD(k->igu, e, JMR_MAD(k->igv, f, half));
    t[2] = JMR_MAD(k->ibu, e, half);
}
/* R, G, B of the pixel with luma y in a block with these terms */
JMI_FN void jmout_rgb_terms(const jmout_coef *k, int32_t y, const int32_t *t, int32_t *rgb) {
    const int32_t d = y - k->yo;
    for (int c = 0; c < 3; c++) rgb[c] = jmr_clip(JMR_MAD(k->iy, d, t[c]) >> JMR_Q, k->maxv);
}
JMI_FN void jmout_rgb(const jmout_coef *k, int32_t y, int32_t u, int32_t v, int32_t *rgb) {
    int32_t t[3];
    jmout_chroma_terms(k, u, v, t);
    jmout_rgb_terms(k, y, t, rgb);
}

/* float32 bits of a value in {0} or [2^-14, 1] to binary16 bits, round to nearest even (every
 * q / M with M <= 1023 lies there: no denormal, no overflow) */
JMI_FN uint32_t jmout_f16_bits(uint32_t bits) {
    if (!(bits & 0x7fffffffu)) return 0;
    uint32_t h = ((bits >> 23) - 112) << 10 | (bits >> 13 & 0x3ffu);    /* bias 127 -> 15; truncated */
    const uint32_t rem = bits & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) h++;              /* a carry runs into the exponent: the next binade */
    return h;
}
/* float32 bits of a finite value to bfloat16 bits, round to nearest even */
JMI_FN uint32_t jmout_bf16_bits(uint32_t bits) { return (bits + 0x7fffu + (bits >> 16 & 1)) >> 16; }

/* the raw bits of the element that holds component q in [0, M] */
JMI_FN uint32_t jmout_dequant(int dtype, int32_t q, int32_t M) {
    if (!jmt_is_float(dtype)) return (uint32_t)q;
    const float x = (float)q / (float)M;            /* IEEE division, round to nearest */
#if defined(__HIP_DEVICE_COMPILE__)
    if (dtype == JMT_F16) {                         /* v_cvt_f16_f32: round to nearest even */
        const _Float16 hf = (_Float16)x;
        uint16_t t;
        memcpy(&t, &hf, 2);
        return t;
    }
#endif
    uint32_t bits;
    memcpy(&bits, &x, 4);
    return dtype == JMT_F32 ? bits : dtype == JMT_F16 ? jmout_f16_bits(bits) : jmout_bf16_bits(bits);
}

/* the dword of an RGB pixel: alpha all ones */
JMI_FN uint32_t jmout_pack(int layout, const int32_t *rgb) {
    const int sh = jmr_ten(layout) ? 10 : 8;
    const int r_low = layout == JMR_RGBA8 || layout == JMR_RGB10A2;    /* as jmr_unpack reads it */
    const uint32_t lo = (uint32_t)rgb[r_low ? 0 : 2], hi = (uint32_t)rgb[r_low ? 2 : 0];
    return lo | (uint32_t)rgb[1] << sh | hi << 2 * sh | (jmr_ten(layout) ? 3u << 30 : 0xffu << 24);
}
/* the stored word of a sample in a YUV format */
JMI_FN uint32_t jmout_yuv_value(int format, uint32_t s) { return format == JMI_P010 ? s << 6 : s; }

/* sample (x, y) of plane pl (0 Y, 1 U, 2 V) of the packed W x H picture at src, es bytes a sample */
JMI_FN uint32_t jmout_sample(const uint8_t *src, int es, int pl, int x, int y, int W, int H) {
    const size_t i = jmi_dst_off(pl, W, H) + (size_t)y * (pl ? W / 2 : W) + x;
    if (es == 2) { uint16_t t; memcpy(&t, src + 2 * i, 2); return t; }
    return src[i];
}
/* an element of es bytes stored byte by byte (the host walk: any alignment) */
JMI_FN void jmout_put(uint8_t *p, int es, uint32_t v) {
    for (int i = 0; i < es; i++) p[i] = (uint8_t)(v >> 8 * i);
}

/* JMH_OK's 0, or -1: the argument rules of jmhip_output.h (everything but the context's bit depth
 * and which), those of jmhip_input.h / jmhip_rgb.h and of jmhip_tensor.h */
JMI_FN int jmout_check_picture(int format, int w, int h, int W, int H, const void *const *plane, const int64_t *stride) {
    return jmr_is_rgb(format) ? jmr_check(format, w, h, W, H, plane, stride) : jmi_check(format, w, h, W, H, plane, stride);
}
JMI_FN int jmout_check_tensor(int dtype, int flags, int w, int h, int W, int H, const void *const *chan, int64_t sx, int64_t sy) {
    return jmt_check(dtype, flags, w, h, W, H, chan, sx, sy);
}
JMI_FN int jmout_picture_depth_ok(int format, int bd) { return jmr_is_rgb(format) ? jmr_depth_ok(format, bd) : jmi_depth_ok(format, bd); }
JMI_FN int jmout_tensor_depth_ok(int dtype, int bd) { return jmt_depth_ok(dtype, bd); }

/* The w x h crop of the packed W x H picture at src (samples of 1 byte in an 8-bit context, else 2)
 * into the planes of a picture format, element by element. */
JMI_FN void jmout_picture(int format, int bd, const uint8_t *src, int W, int H, int w, int h, uint8_t *const *plane, const int64_t *stride) {
    const int ses = bd > 8 ? 2 : 1;
    if (jmr_is_rgb(format)) {
        jmout_coef k;
        jmout_coefficients(format, bd, &k);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int32_t rgb[3];
                jmout_rgb(&k, (int32_t)jmout_sample(src, ses, 0, x, y, W, H), (int32_t)jmout_sample(src, ses, 1, x / 2, y / 2, W, H),
                          (int32_t)jmout_sample(src, ses, 2, x / 2, y / 2, W, H), rgb);
                jmout_put(plane[0] + jmr_src_off(x, y, stride[0]), 4, jmout_pack(jmr_layout(format), rgb));
            }
        return;
    }
    const int es = jmi_wide(format) ? 2 : 1;
    for (int pl = 0; pl < 3; pl++)
        for (int y = 0; y < (pl ? h / 2 : h); y++)
            for (int x = 0; x < (pl ? w / 2 : w); x++) {
                int sp;
                int64_t off;
                jmi_src(format, pl, x, y, w, h, stride, &sp, &off);   /* inside the crop nothing is clamped */
                jmout_put(plane[sp] + off, es, jmout_yuv_value(format, jmout_sample(src, ses, pl, x, y, W, H)));
            }
}
/* The same into the channels of a tensor.  chan: R, G, B. */
JMI_FN void jmout_tensor(int dtype, int flags, int bd, const uint8_t *src, int W, int H, int w, int h, uint8_t *const *chan, int64_t sx,
                         int64_t sy) {
    const int ses = bd > 8 ? 2 : 1;
    jmout_coef k;
    jmout_coefficients(flags, bd, &k);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int32_t rgb[3];
            jmout_rgb(&k, (int32_t)jmout_sample(src, ses, 0, x, y, W, H), (int32_t)jmout_sample(src, ses, 1, x / 2, y / 2, W, H),
                      (int32_t)jmout_sample(src, ses, 2, x / 2, y / 2, W, H), rgb);
            for (int c = 0; c < 3; c++) jmout_put(chan[c] + jmt_src_off(x, y, sx, sy), jmt_es(dtype), jmout_dequant(dtype, rgb[c], k.maxv));
        }
}

#endif /* JMH_OUTPUT_H */
