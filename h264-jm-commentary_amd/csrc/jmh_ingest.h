/*
 * jmh_ingest.h — where a sample of the coded picture comes from in a device picture
 * (include/jmhip_input.h).  The single statement of
 *   - the clamped coordinates min(x, w - 1), min(y, h - 1) that pad the source to the coded size
 *     (host/yuv.c jm_pad_picture: last column to the right, last row downwards, chroma at half size),
 *   - the UV de-interleave of NV12 / P010, for one sample (jmi_src) and for a pair of dwords
 *     (jmi_deint),
 *   - the value transform: word >> 6 of P010, min(sample, maxv) of I010 and which samples count
 *     as clamped (those of the source, not their replicas in the padding).
 *
 * k_ingest (jmh_ingest.hip) takes row addresses, vector validity and every value from here; the
 * vectors it moves untouched are runs of samples whose jmi_src offsets are consecutive.
 * jmi_ingest below is the same walk sample by sample: the reference of the kernel's tests and what
 * tests/harness/ingest_check.c runs on exact-size planes under ASan.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_INGEST_H
#define JMH_INGEST_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define JMI_FN __host__ __device__ static inline
#define JMI_PRED __host__ __device__ static constexpr inline   /* a property of the format: a constant in k_ingest<format> */
#else
#define JMI_FN static inline
#define JMI_PRED static inline
#endif

/* the formats of jmhip_input.h */
#define JMI_I420 0
#define JMI_NV12 1
#define JMI_I010 2
#define JMI_P010 3
#define JMI_NFORMATS 4

JMI_PRED int jmi_wide(int format) { return format >= JMI_I010; }                       /* 16-bit samples        */
JMI_PRED int jmi_semi(int format) { return format == JMI_NV12 || format == JMI_P010; } /* interleaved UV plane  */
JMI_PRED int jmi_planes(int format) { return jmi_semi(format) ? 2 : 3; }               /* source planes read    */
/* the bit depths of a context that takes the format */
JMI_FN int jmi_depth_ok(int format, int bd) {
    return format == JMI_P010 ? bd == 10 : format == JMI_I010 ? bd == 9 || bd == 10 : bd == 8;
}
/* bytes of a row of source plane sp (0..jmi_planes - 1) that hold samples, w luma samples wide */
JMI_FN int64_t jmi_row_bytes(int format, int sp, int w) {
    const int64_t es = jmi_wide(format) ? 2 : 1;
    return (sp == 0 || jmi_semi(format) ? (int64_t)w : (int64_t)(w / 2)) * es;
}
JMI_FN int jmi_rows(int sp, int h) { return sp ? h / 2 : h; }

/* the padding: coordinate x of an n-sample axis, replicated beyond its end */
JMI_FN int jmi_clamp(int x, int n) { return x < n - 1 ? x : n - 1; }

/* Sample (x, y) of plane pl (0 Y, 1 U, 2 V) of the coded picture, from a w x h source: the source
 * plane it is read from and its byte offset there. */
JMI_FN void jmi_src(int format, int pl, int x, int y, int w, int h, const int64_t *stride, int *sp, int64_t *off) {
    const int es = jmi_wide(format) ? 2 : 1;
    const int cx = jmi_clamp(x, pl ? w / 2 : w), cy = jmi_clamp(y, pl ? h / 2 : h);
    if (pl && jmi_semi(format)) {
        *sp = 1;
        *off = (int64_t)cy * stride[1] + ((int64_t)2 * cx + (pl - 1)) * es;   /* U0 V0 U1 V1 ... */
    } else {
        *sp = pl;
        *off = (int64_t)cy * stride[pl] + (int64_t)cx * es;
    }
}
/* whether sample (x, y) of plane pl is one of the source (counted when it is clamped) or a replica */
JMI_FN int jmi_in_source(int pl, int x, int y, int w, int h) { return x < (pl ? w / 2 : w) && y < (pl ? h / 2 : h); }

/* the stored value of a raw sample; *over is raised by one when it was clamped */
JMI_FN uint32_t jmi_value(int format, uint32_t raw, uint32_t maxv, uint32_t *over) {
    if (format == JMI_P010) return raw >> 6;
    if (format == JMI_I010 && raw > maxv) { *over += 1; return maxv; }
    return raw;
}
/* two 16-bit samples in a dword */
JMI_FN uint32_t jmi_value_x2(int format, uint32_t d, uint32_t maxv, uint32_t *over) {
    return jmi_value(format, d & 0xffffu, maxv, over) | jmi_value(format, d >> 16, maxv, over) << 16;
}

/* Two consecutive dwords lo, hi of an interleaved UV row: the dword of their U samples (which 0)
 * or V samples (which 1), in order.  wide: 16-bit samples (two pairs), else 8-bit (four pairs). */
JMI_FN uint32_t jmi_deint(uint32_t lo, uint32_t hi, int which, int wide) {
#if defined(__HIP_DEVICE_COMPILE__)
    /* v_perm_b32: selector bytes 0..3 pick from lo, 4..7 from hi */
    return wide ? __builtin_amdgcn_perm(hi, lo, which ? 0x07060302u : 0x05040100u)
                : __builtin_amdgcn_perm(hi, lo, which ? 0x07050301u : 0x06040200u);
#else
    if (wide) return which ? (lo >> 16) | (hi & 0xffff0000u) : (lo & 0xffffu) | hi << 16;
    if (which) { lo >>= 8; hi >>= 8; }
    return (lo & 0xffu) | (lo >> 8 & 0xff00u) | (hi & 0xffu) << 16 | (hi >> 8 & 0xff00u) << 16;
#endif
}

/* offset, in samples, of plane pl in the packed W x H picture (Y, then U, then V) */
JMI_FN size_t jmi_dst_off(int pl, int W, int H) {
    return pl == 0 ? 0 : (size_t)W * H + (pl == 2 ? (size_t)(W / 2) * (H / 2) : 0);
}

/* JMH_OK's 0, or -1: the argument rules of jmhip_input.h (everything but the context's bit depth) */
JMI_FN int jmi_check(int format, int w, int h, int W, int H, const void *const *plane, const int64_t *stride) {
    if (format < 0 || format >= JMI_NFORMATS) return -1;
    if (w < 2 || h < 2 || (w & 1) || (h & 1) || w > W || h > H) return -1;
    for (int sp = 0; sp < jmi_planes(format); sp++) {
        if (!plane[sp] || stride[sp] < jmi_row_bytes(format, sp, w)) return -1;
        if (jmi_wide(format) && (((uintptr_t)plane[sp] | (uint64_t)stride[sp]) & 1)) return -1;
    }
    return 0;
}

/* The whole picture sample by sample into dst (packed W x H, 4:2:0, samples of 1 or 2 bytes);
 * returns the clamped samples. */
JMI_FN uint64_t jmi_ingest(int format, const uint8_t *const *plane, const int64_t *stride, int w, int h, int W, int H, uint32_t maxv,
                           uint8_t *dst) {
    const int es = jmi_wide(format) ? 2 : 1;
    uint64_t clamped = 0;
    for (int pl = 0; pl < 3; pl++) {
        const int PW = pl ? W / 2 : W, PH = pl ? H / 2 : H;
        uint8_t *d = dst + jmi_dst_off(pl, W, H) * es;
        for (int y = 0; y < PH; y++)
            for (int x = 0; x < PW; x++) {
                int sp;
                int64_t off;
                uint32_t over = 0, raw;
                jmi_src(format, pl, x, y, w, h, stride, &sp, &off);
                if (es == 2) { uint16_t t; memcpy(&t, plane[sp] + off, 2); raw = t; }
                else raw = plane[sp][off];
                const uint32_t v = jmi_value(format, raw, maxv, &over);
                if (jmi_in_source(pl, x, y, w, h)) clamped += over;
                if (es == 2) { const uint16_t t = (uint16_t)v; memcpy(d + ((size_t)y * PW + x) * 2, &t, 2); }
                else d[(size_t)y * PW + x] = (uint8_t)v;
            }
    }
    return clamped;
}

#endif /* JMH_INGEST_H */
