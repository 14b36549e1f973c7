/*
 * jmh_tensor.h — what a sample of the coded picture is when the source is a device tensor
 * (include/jmhip_tensor.h).  The single statement of
 *   - the element types and how one element becomes an integer component q in [0, M],
 *     M = 2^b - 1 (jmt_quant): the byte of U8; min(v, M) of U16; for the floats
 *     floor(x M + 1/2) in exact arithmetic after x is clamped to [0, 1], F16 and BF16 widened
 *     exactly first (jmt_widen),
 *   - where the element of channel c at pixel (x, y) lies (jmt_src_off): chan[c] + y stride_y +
 *     x stride_x, which covers CHW, HWC with 3 or 4 channels, any channel order and cropped views,
 *   - the argument rules (jmt_check, jmt_depth_ok).
 * The conversion of the quantised components to 4:2:0 and the padding are jmh_rgb.h's, reused and not
 * restated: jmr_coefficients with the flags, jmr_luma per pixel, jmr_chroma on the 2x2 sums, the
 * clamped pixel / block, jmi_dst_off.
 *
 * Why the float quantiser is exact.  x is a float32 in (0, 1), 24 significant bits, and M < 2^10 an
 * integer, so the product x M has at most 34 significant bits: a float64 multiply does not round it.
 * Where x M >= 2^-10 its lowest set bit is 2^-43 or higher and x M + 1/2 is below 2^10: the sum lies
 * within 53 bits, the add does not round, and neither does a fused multiply-add, which rounds once
 * what needs no rounding.  Where x M < 2^-10 the sum may round, but it lies in [1/2, 1/2 + 2^-10]
 * before and after, so its floor is 0 whatever the rounding did.  Hence (double)x * M + 0.5, floored,
 * is floor(x M + 1/2) of the reals for every float32 x, fused or not, on the host and on the device;
 * the truncating conversion to an integer is that floor, the sum being positive.  NaN and everything
 * <= 0 (-0, -inf) give 0 and everything >= 1 (+inf) gives M by the comparisons, before any arithmetic.
 *
 * k_ingest_tensor (jmh_tensor.hip) takes every value from here; jmt_convert below is the same walk
 * sample by sample: the reference of the kernel's tests and what tests/harness/tensor_check.c runs on
 * exact-size channels under ASan.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_TENSOR_H
#define JMH_TENSOR_H

#include <stdint.h>
#include <string.h>
#include "jmh_rgb.h"

/* jmh_device_tensor.dtype */
#define JMT_U8 0
#define JMT_U16 1
#define JMT_F16 2     /* IEEE binary16 */
#define JMT_BF16 3    /* the high half of a binary32 */
#define JMT_F32 4
#define JMT_NDTYPES 5

JMI_PRED int jmt_es(int dtype) { return dtype == JMT_U8 ? 1 : dtype == JMT_F32 ? 4 : 2; }   /* bytes of an element */
JMI_PRED int jmt_is_float(int dtype) { return dtype >= JMT_F16; }
/* the bit depths of a context that takes the dtype: a 9-bit context takes none */
JMI_FN int jmt_depth_ok(int dtype, int bd) { return dtype == JMT_U8 ? bd == 8 : dtype == JMT_U16 ? bd == 10 : bd == 8 || bd == 10; }

/* the float32 that a 2-byte float element is, exactly, as its bit pattern */
JMI_FN uint32_t jmt_widen(int dtype, uint32_t raw) {
    if (dtype == JMT_BF16) return raw << 16;
#if defined(__HIP_DEVICE_COMPILE__)
    /* v_cvt_f32_f16: the same value (were a denormal flushed, it would quantise to 0 as the denormal does) */
    const uint16_t t = (uint16_t)raw;
    _Float16 hf;
    memcpy(&hf, &t, 2);
    const float f = (float)hf;
    uint32_t bits;
    memcpy(&bits, &f, 4);
    return bits;
#else
    /* binary16: 1 sign, 5 exponent (bias 15), 10 mantissa bits */
    const uint32_t s = (raw & 0x8000u) << 16, e = raw >> 10 & 31u, m = raw & 0x3ffu;
    if (e == 31) return s | 0x7f800000u | m << 13;                  /* inf, NaN */
    if (e) return s | (e + 112) << 23 | m << 13;                    /* normal: bias 15 -> 127 */
    if (!m) return s;                                               /* +-0 */
    int sh = 0;                                                     /* denormal m 2^-24: normalise */
    uint32_t n = m;
    while (!(n & 0x400u)) { n <<= 1; sh++; }
    return s | (uint32_t)(113 - sh) << 23 | (n & 0x3ffu) << 13;
#endif
}
/* a float32 in the nominal range [0, 1] to q in [0, M] */
JMI_FN int32_t jmt_quant_f32(float x, int32_t M) {
    if (!(x > 0.0f)) return 0;          /* NaN, -0, +0, negatives, -inf */
    if (x >= 1.0f) return M;            /* 1, above, +inf */
    return (int32_t)((double)x * (double)M + 0.5);
}
/* the raw bits of one element (zero-extended) to q */
JMI_FN int32_t jmt_quant(int dtype, uint32_t raw, int32_t M) {
    if (dtype == JMT_U8) return (int32_t)raw;
    if (dtype == JMT_U16) return (int32_t)raw < M ? (int32_t)raw : M;
    const uint32_t bits = dtype == JMT_F32 ? raw : jmt_widen(dtype, raw);
    float x;
    memcpy(&x, &bits, 4);
    return jmt_quant_f32(x, M);
}

/* the element of a channel at pixel (x, y): byte offset from the channel's address */
JMI_FN int64_t jmt_src_off(int x, int y, int64_t sx, int64_t sy) { return (int64_t)y * sy + (int64_t)x * sx; }
/* the raw bits of the element at p (aligned to its size by the argument rule) */
JMI_FN uint32_t jmt_load(int dtype, const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return jmt_es(dtype) == 1 ? (uint32_t)*p : jmt_es(dtype) == 2 ? (uint32_t)*(const uint16_t *)p : *(const uint32_t *)p;
#else
    uint32_t v = 0;
    for (int i = 0; i < jmt_es(dtype); i++) v |= (uint32_t)p[i] << 8 * i;
    return v;
#endif
}

/* JMH_OK's 0, or -1: the argument rules of jmhip_tensor.h (everything but the context's bit depth) */
JMI_FN int jmt_check(int dtype, int flags, int w, int h, int W, int H, const void *const *chan, int64_t sx, int64_t sy) {
    if (dtype < 0 || dtype >= JMT_NDTYPES) return -1;
    if (flags & ~JMR_FLAGS) return -1;
    if (w < 2 || h < 2 || (w & 1) || (h & 1) || w > W || h > H) return -1;
    const int64_t es = jmt_es(dtype);
    if (sx < es || sy < (int64_t)(w - 1) * sx + es) return -1;      /* negative strides included */
    uint64_t low = (uint64_t)sx | (uint64_t)sy;
    for (int c = 0; c < 3; c++) {
        if (!chan[c]) return -1;
        low |= (uint64_t)(uintptr_t)chan[c];
    }
    return (low & (uint64_t)(es - 1)) ? -1 : 0;
}

/* The whole picture sample by sample into dst (packed W x H, 4:2:0, samples of 1 byte in an 8-bit
 * context, 2 bytes in a 10-bit one).  chan: R, G, B. */
JMI_FN void jmt_convert(int dtype, int flags, int bd, const uint8_t *const *chan, int64_t sx, int64_t sy, int w, int h, int W, int H,
                        uint8_t *dst) {
    const int es = bd > 8 ? 2 : 1;
    jmr_coef k;
    jmr_coefficients(flags, bd, &k);
    for (int pl = 0; pl < 3; pl++) {
        const int PW = pl ? W / 2 : W, PH = pl ? H / 2 : H;
        uint8_t *d = dst + jmi_dst_off(pl, W, H) * es;
        for (int y = 0; y < PH; y++)
            for (int x = 0; x < PW; x++) {
                const int cx = jmi_clamp(x, pl ? w / 2 : w), cy = jmi_clamp(y, pl ? h / 2 : h);
                int32_t q[3], v;
                if (pl == 0) {
                    for (int c = 0; c < 3; c++) q[c] = jmt_quant(dtype, jmt_load(dtype, chan[c] + jmt_src_off(cx, cy, sx, sy)), k.maxv);
                    v = jmr_luma(&k, q[0], q[1], q[2]);
                } else {
                    q[0] = q[1] = q[2] = 0;
                    for (int i = 0; i < 4; i++)
                        for (int c = 0; c < 3; c++)
                            q[c] += jmt_quant(dtype, jmt_load(dtype, chan[c] + jmt_src_off(2 * cx + (i & 1), 2 * cy + (i >> 1), sx, sy)), k.maxv);
                    v = jmr_chroma(&k, pl - 1, q[0], q[1], q[2]);
                }
                if (es == 2) { const uint16_t t = (uint16_t)v; memcpy(d + ((size_t)y * PW + x) * 2, &t, 2); }
                else d[(size_t)y * PW + x] = (uint8_t)v;
            }
    }
}

#endif /* JMH_TENSOR_H */
