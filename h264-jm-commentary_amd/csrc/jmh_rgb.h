/*
 * jmh_rgb.h — what a sample of the coded picture is when the device picture is RGB
 * (include/jmhip_rgb.h).  The single statement of
 *   - the four pixel layouts (jmr_unpack: a little-endian dword to R, G, B; alpha is ignored) and the
 *     two flag bits of jmh_device_picture.format,
 *   - the integer conversion: Q14 coefficients (the table below, literals), one luma sample per
 *     pixel, box chroma from the sums of a 2x2 block (as libyuv's ARGBToI420), both clamped,
 *   - the padding: coded luma (x, y) is the Y of pixel (min(x, w - 1), min(y, h - 1)), coded chroma
 *     (x, y) that of block (min(x, w/2 - 1), min(y, h/2 - 1)): converting at the source size and
 *     then host/yuv.c jm_pad_picture,
 *   - the argument rules (jmr_check).
 *
 * k_ingest_rgb (jmh_rgb.hip) takes every value from here; jmr_convert below is the same walk sample
 * by sample: the reference of the kernel's tests, what tests/harness/rgb_check.c runs on exact-size
 * planes under ASan, and what a host consumer of the source planes would be filled with.
 *
 * All arithmetic is in 32-bit integers; >> of a negative value is an arithmetic shift (it floors).
 * Operands stay below 2^24 (sums of four 10-bit samples: 4092; coefficients: 11718 at most), so a
 * 24-bit multiply-add is exact.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_RGB_H
#define JMH_RGB_H

#include <stdint.h>
#include <string.h>
#include "jmh_ingest.h"   /* jmi_clamp, jmi_dst_off: the padding and the packed layout are the same */

#if defined(__HIP_DEVICE_COMPILE__)
#define JMR_MAD(a, b, c) (__mul24((a), (b)) + (c))   /* v_mad_i32_i24 */
#else
#define JMR_MAD(a, b, c) ((a) * (b) + (c))
#endif

/* jmh_device_picture.format: a layout, OR-ed with the flags */
#define JMR_BGRA8 16     /* bytes B, G, R, A                                               8-bit context */
#define JMR_RGBA8 17     /* bytes R, G, B, A                                               8-bit context */
#define JMR_RGB10A2 18   /* dword: R bits 0-9, G 10-19, B 20-29, A 30-31                  10-bit context */
#define JMR_BGR10A2 19   /* dword: B bits 0-9, G 10-19, R 20-29, A 30-31                  10-bit context */
#define JMR_BT709 (1 << 8)        /* else BT.601       */
#define JMR_FULL_RANGE (1 << 9)   /* else limited range */
#define JMR_FLAGS (JMR_BT709 | JMR_FULL_RANGE)
#define JMR_Q 14

JMI_PRED int jmr_layout(int format) { return format & ~JMR_FLAGS; }
/* one of the four layouts with none but the two flag bits */
JMI_PRED int jmr_is_rgb(int format) { return jmr_layout(format) >= JMR_BGRA8 && jmr_layout(format) <= JMR_BGR10A2; }
JMI_PRED int jmr_ten(int layout) { return layout >= JMR_RGB10A2; }   /* 10-bit components, 16-bit output samples */
/* the bit depth of a context that takes the format */
JMI_FN int jmr_depth_ok(int format, int bd) { return jmr_ten(jmr_layout(format)) ? bd == 10 : bd == 8; }

/* The conversion of one picture: cyr cyg cyb | cur cug cub | cvr cvg cvb, then Yo, Co, maxv (the 12
 * words of jmh_rgb_coefficients) */
typedef struct jmr_coef { int32_t c[9], yo, co, maxv; } jmr_coef;

/* c = rint(k 2^14) of kyr = Kr Ys/M, kyb = Kb Ys/M, kub = kvr = Cs/2M, kur = -Kr/(2(1 - Kb)) Cs/M,
 * kvb = -Kb/(2(1 - Kr)) Cs/M; the green terms close the sums: cyg = rint(Ys/M 2^14) - cyr - cyb,
 * cug = -cur - cub, cvg = -cvr - cvb.  (Kr, Kb) = (0.299, 0.114) BT.601, (0.2126, 0.0722) BT.709;
 * limited range Ys = 219 2^(b-8), Cs = 224 2^(b-8), Yo = 16 2^(b-8); full range Ys = Cs = M, Yo = 0.
 * Rows: matrix * 3 + (full range: 2, else 10-bit: 1, else 0). */
JMI_FN void jmr_table_row(int row, int32_t *c) {
    static const int16_t T[6][9] = {
        {4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170},    /* 601  8 limited */
        {4195, 8236, 1599, -2421, -4754, 7175, 7175, -6008, -1167},    /* 601 10 limited */
        {4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332},    /* 601 full       */
        {2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660},    /* 709  8 limited */
        {2983, 10034, 1013, -1644, -5531, 7175, 7175, -6517, -658},    /* 709 10 limited */
        {3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751}};   /* 709 full       */
    for (int i = 0; i < 9; i++) c[i] = T[row][i];
}
/* the conversion of a format (one that jmr_is_rgb and jmr_depth_ok accept) */
JMI_FN void jmr_coefficients(int format, int bd, jmr_coef *k) {
    const int full = (format & JMR_FULL_RANGE) != 0;
    jmr_table_row(((format & JMR_BT709) ? 3 : 0) + (full ? 2 : bd == 10 ? 1 : 0), k->c);
    k->yo = full ? 0 : 16 << (bd - 8);
    k->co = 1 << (bd - 1);
    k->maxv = (1 << bd) - 1;
}

/* a raw dword (little-endian) to its components */
JMI_FN void jmr_unpack(int layout, uint32_t raw, int32_t *r, int32_t *g, int32_t *b) {
    const int sh = jmr_ten(layout) ? 10 : 8;
    const uint32_t m = (1u << sh) - 1;
    const int32_t lo = (int32_t)(raw & m), hi = (int32_t)(raw >> 2 * sh & m);
    *g = (int32_t)(raw >> sh & m);
    if (layout == JMR_RGBA8 || layout == JMR_RGB10A2) { *r = lo; *b = hi; }
    else { *r = hi; *b = lo; }
}
JMI_FN int32_t jmr_clip(int32_t v, int32_t maxv) { return v < 0 ? 0 : v > maxv ? maxv : v; }
/* Y of one pixel (it cannot leave its range; clamped anyway) */
JMI_FN int32_t jmr_luma(const jmr_coef *k, int32_t r, int32_t g, int32_t b) {
    const int32_t s = JMR_MAD(k->c[0], r, JMR_MAD(k->c[1], g, JMR_MAD(k->c[2], b, 1 << (JMR_Q - 1))));
    return jmr_clip(k->yo + (s >> JMR_Q), k->maxv);
}
/* U (which 0) or V (which 1) of a 2x2 block from the sums of its four pixels (a live clamp: full-range
 * pure blue gives U = maxv + 1 before it) */
JMI_FN int32_t jmr_chroma(const jmr_coef *k, int which, int32_t rs, int32_t gs, int32_t bs) {
    const int32_t *c = k->c + 3 + 3 * which;
    const int32_t s = JMR_MAD(c[0], rs, JMR_MAD(c[1], gs, JMR_MAD(c[2], bs, 1 << (JMR_Q + 1))));
    return jmr_clip(k->co + (s >> (JMR_Q + 2)), k->maxv);
}
/* the same before the clamp (the CPU check counts the samples the clamp changes) */
JMI_FN int32_t jmr_chroma_raw(const jmr_coef *k, int which, int32_t rs, int32_t gs, int32_t bs) {
    const int32_t *c = k->c + 3 + 3 * which;
    return k->co + ((c[0] * rs + c[1] * gs + c[2] * bs + (1 << (JMR_Q + 1))) >> (JMR_Q + 2));
}

/* the dword of source pixel (x, y): byte offset from plane[0] */
JMI_FN int64_t jmr_src_off(int x, int y, int64_t stride) { return (int64_t)y * stride + (int64_t)4 * x; }
JMI_FN uint32_t jmr_load(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const uint32_t *)p;   /* dword aligned by the argument rule */
#else
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
#endif
}

/* JMH_OK's 0, or -1: the argument rules of jmhip_rgb.h (everything but the context's bit depth).
 * plane[1], plane[2] and their strides are not looked at. */
JMI_FN int jmr_check(int format, int w, int h, int W, int H, const void *const *plane, const int64_t *stride) {
    if (format < 0 || !jmr_is_rgb(format)) return -1;
    if (w < 2 || h < 2 || (w & 1) || (h & 1) || w > W || h > H) return -1;
    if (!plane[0] || stride[0] < (int64_t)4 * w) return -1;
    if (((uintptr_t)plane[0] | (uint64_t)stride[0]) & 3) return -1;
    return 0;
}

/* The whole picture sample by sample into dst (packed W x H, 4:2:0, samples of 1 byte in an 8-bit
 * context, 2 bytes in a 10-bit one); returns the chroma samples of the source the clamp changed. */
JMI_FN uint64_t jmr_convert(int format, int bd, const uint8_t *plane, int64_t stride, int w, int h, int W, int H, uint8_t *dst) {
    const int layout = jmr_layout(format), es = bd > 8 ? 2 : 1;
    uint64_t clamped = 0;
    jmr_coef k;
    jmr_coefficients(format, bd, &k);
    for (int pl = 0; pl < 3; pl++) {
        const int PW = pl ? W / 2 : W, PH = pl ? H / 2 : H;
        uint8_t *d = dst + jmi_dst_off(pl, W, H) * es;
        for (int y = 0; y < PH; y++)
            for (int x = 0; x < PW; x++) {
                const int cx = jmi_clamp(x, pl ? w / 2 : w), cy = jmi_clamp(y, pl ? h / 2 : h);
                int32_t r, g, b, v;
                if (pl == 0) {
                    jmr_unpack(layout, jmr_load(plane + jmr_src_off(cx, cy, stride)), &r, &g, &b);
                    v = jmr_luma(&k, r, g, b);
                } else {
                    int32_t rs = 0, gs = 0, bs = 0;
                    for (int i = 0; i < 4; i++) {
                        jmr_unpack(layout, jmr_load(plane + jmr_src_off(2 * cx + (i & 1), 2 * cy + (i >> 1), stride)), &r, &g, &b);
                        rs += r; gs += g; bs += b;
                    }
                    v = jmr_chroma(&k, pl - 1, rs, gs, bs);
                    if (x == cx && y == cy && v != jmr_chroma_raw(&k, pl - 1, rs, gs, bs)) clamped++;
                }
                if (es == 2) { const uint16_t t = (uint16_t)v; memcpy(d + ((size_t)y * PW + x) * 2, &t, 2); }
                else d[(size_t)y * PW + x] = (uint8_t)v;
            }
    }
    return clamped;
}

#endif /* JMH_RGB_H */
