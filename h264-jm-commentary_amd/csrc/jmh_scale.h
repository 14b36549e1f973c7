/*
 * jmh_scale.h — the scaler of device pushes (include/jmhip_scale.h).  The single
 * statement of
 *   - the tap tables of an axis (jms_taps: host only, IEEE double, in the order the header writes),
 *   - the two pass formulas for one sample (jms_hpass, jms_vpass),
 *   - the argument rules (jms_check_setting, jms_check),
 *   - the layout of the tables k_scale reads (jms_pack_axis, jms_span).
 * jms_scale below is the whole picture sample by sample: the reference of the kernel's tests and
 * what tests/harness/scale_check.c runs on exact-size buffers under ASan.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_SCALE_H
#define JMH_SCALE_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "jmh_ingest.h"

#define JMS_OFF 0
#define JMS_BILINEAR 1
#define JMS_BICUBIC 2
#define JMS_LANCZOS3 3
#define JMS_CHROMA_LEFT 1
#define JMS_FLAGS 1
#define JMS_TAPS_MAX 24
#define JMS_SRC_MAX 8192
#define JMS_ONE 16384

/* the statuses of the functions below: JMH_OK, JMH_E_INVALID_ARG and JMH_E_UNSUPPORTED_CFG by their values */
#define JMS_OK 0
#define JMS_INVALID (-1)
#define JMS_UNSUPPORTED (-4)

/* k_scale's tile of one plane and the intermediate rows it keeps (jms_span checks the span) */
#define JMS_TILE_W 64
#define JMS_TILE_H 16
#define JMS_SPAN_MAX 208
#define JMS_HPAIRS (JMS_TAPS_MAX / 2)        /* dwords of a column's packed taps     */
#define JMS_VPAIRS (JMS_TAPS_MAX / 2 + 1)    /* dwords of a row's taps, parity-aligned */

/* the support S of a filter's kernel, 0: no such filter */
JMI_FN int jms_support(int filter) { return filter >= JMS_BILINEAR && filter <= JMS_LANCZOS3 ? filter : 0; }

/* T = 2 ceil(S s), s = max(1, n_src / n_dst): the ceiling of the exact rational */
JMI_FN int jms_ntaps(int n_src, int n_dst, int filter) {
    const int64_t S = jms_support(filter);
    return n_src > n_dst ? (int)(2 * ((S * n_src + n_dst - 1) / n_dst)) : (int)(2 * S);
}

/* the horizontal pass of one sample: sum = sum(q_j src_j), P = 14 - bit depth */
JMI_FN int32_t jms_hpass(int32_t sum, int P) { return (sum + (1 << (13 - P))) >> (14 - P); }
/* the vertical pass: sum = sum(q_k h_k) */
JMI_FN int32_t jms_vpass(int32_t sum, int P, int32_t maxv) {
    const int32_t v = (sum + (1 << (13 + P))) >> (14 + P);
    return v < 0 ? 0 : v > maxv ? maxv : v;
}
/* tap j of an n-sample axis: edge replication */
JMI_FN int jms_tap_at(int j, int n) { return j < 0 ? 0 : j > n - 1 ? n - 1 : j; }

/* the rules of jmh_input_scale: an active setting in a W x H context */
JMI_FN int jms_check_setting(int filter, int flags, int ow, int oh, int W, int H) {
    if (!jms_support(filter) || (flags & ~JMS_FLAGS)) return JMS_INVALID;
    if (ow < 2 || oh < 2 || (ow & 1) || (oh & 1) || ow > W || oh > H) return JMS_INVALID;
    return JMS_OK;
}
/* the rules of a w x h source under a valid setting: the size, then the taps of the four axes */
JMI_FN int jms_check(int w, int h, int ow, int oh, int filter) {
    if (w < 2 || h < 2 || (w & 1) || (h & 1) || w > JMS_SRC_MAX || h > JMS_SRC_MAX) return JMS_INVALID;
    if (jms_ntaps(w, ow, filter) > JMS_TAPS_MAX || jms_ntaps(h, oh, filter) > JMS_TAPS_MAX) return JMS_UNSUPPORTED;
    if (jms_ntaps(w / 2, ow / 2, filter) > JMS_TAPS_MAX || jms_ntaps(h / 2, oh / 2, filter) > JMS_TAPS_MAX) return JMS_UNSUPPORTED;
    return JMS_OK;
}

/* host only from here on (plain functions: IEEE double, malloc) */

static inline double jms_kernel(int filter, double t) {
    const double a = fabs(t);
    if (filter == JMS_BILINEAR) return a < 1.0 ? 1.0 - a : 0.0;
    if (filter == JMS_BICUBIC) {
        if (a <= 1.0) return (1.5 * a - 2.5) * a * a + 1.0;
        if (a < 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
        return 0.0;
    }
    if (a >= 3.0) return 0.0;
    if (a == 0.0) return 1.0;
    {
        const double pi = 3.14159265358979323846, x = pi * a, y = x / 3.0;
        return sin(x) / x * (sin(y) / y);
    }
}

/* The tables of jmh_scale_taps.  first / taps NULL: only *ntaps.  JMS_INVALID: sizes outside
 * 1..JMS_SRC_MAX or no such filter; JMS_UNSUPPORTED: T > JMS_TAPS_MAX (*ntaps is still T). */
static inline int jms_taps(int n_src, int n_dst, int filter, int chroma_left, int32_t *first, int16_t *taps, int *ntaps) {
    if (!jms_support(filter) || n_src < 1 || n_dst < 1 || n_src > JMS_SRC_MAX || n_dst > JMS_SRC_MAX || !ntaps) return JMS_INVALID;
    const int T = jms_ntaps(n_src, n_dst, filter);
    *ntaps = T;
    if (T > JMS_TAPS_MAX) return JMS_UNSUPPORTED;
    if (!first && !taps) return JMS_OK;
    if (!first || !taps) return JMS_INVALID;
    const double r = (double)n_src / (double)n_dst, s = r > 1.0 ? r : 1.0, phi = chroma_left ? 0.25 : 0.5;
    for (int i = 0; i < n_dst; i++) {
        volatile double pos = ((double)i + phi) * r;   /* rounded before the subtraction: no fused multiply-add */
        const double c = pos - phi;
        const int f = (int)floor(c - (double)(T / 2)) + 1;
        double w[JMS_TAPS_MAX], sum = 0.0;
        int32_t q[JMS_TAPS_MAX], total = 0, best = 0, mag = 0;
        for (int j = 0; j < T; j++) { w[j] = jms_kernel(filter, ((double)(f + j) - c) / s); sum += w[j]; }
        for (int j = 0; j < T; j++) {
            q[j] = (int32_t)floor(w[j] / sum * (double)JMS_ONE + 0.5);
            total += q[j];
            if (q[j] > q[best]) best = j;
        }
        q[best] += JMS_ONE - total;
        for (int j = 0; j < T; j++) mag += q[j] < 0 ? -q[j] : q[j];
        if (mag > 32767) return JMS_UNSUPPORTED;        /* h would not fit an int16_t: no filter here comes near */
        first[i] = f;
        for (int j = 0; j < T; j++) taps[(size_t)i * T + j] = (int16_t)q[j];
    }
    return JMS_OK;
}

/* The tables of one axis as k_scale reads them.  Horizontal: a column's taps as JMS_HPAIRS dwords
 * (q[2p] low, q[2p + 1] high, zeros behind T).  Vertical: a row's taps as JMS_VPAIRS dwords that pair
 * the intermediate rows 2m, 2m + 1 (they share a dword in LDS): a row whose first is odd starts with
 * the pair (0, q[0]).  The pairs in use: T / 2, and one more for the vertical axis. */
static inline void jms_pack_axis(const int32_t *first, const int16_t *taps, int n, int T, int vertical, uint32_t *out) {
    const int np = vertical ? JMS_VPAIRS : JMS_HPAIRS;
    for (int i = 0; i < n; i++) {
        int16_t t[2 * JMS_VPAIRS + 2];
        memset(t, 0, sizeof t);
        const int lead = vertical ? (first[i] & 1) : 0;
        for (int j = 0; j < T; j++) t[lead + j] = taps[(size_t)i * T + j];
        for (int p = 0; p < np; p++) out[(size_t)i * np + p] = (uint32_t)(uint16_t)t[2 * p] | (uint32_t)(uint16_t)t[2 * p + 1] << 16;
    }
}
/* the intermediate rows the tallest tile of a vertical axis needs, from the even row at or below its
 * first one through the row the last (possibly zero) tap pair reads; PH: the padded plane's rows */
static inline int jms_span(const int32_t *first, int n_dst, int T, int PH) {
    int worst = 0;
    for (int y0 = 0; y0 < PH; y0 += JMS_TILE_H) {
        const int y1 = y0 + JMS_TILE_H - 1 < PH - 1 ? y0 + JMS_TILE_H - 1 : PH - 1;
        const int lo = first[jmi_clamp(y0, n_dst)] & ~1, hi = (first[jmi_clamp(y1, n_dst)] & ~1) + T + 1;
        if (hi - lo + 1 > worst) worst = hi - lo + 1;
    }
    return worst;
}

/* The whole picture sample by sample: src a packed 4:2:0 picture of pw x ph samples (pw >= w,
 * ph >= h, both even) of which the top-left w x h is the source, dst the packed W x H picture; bd the
 * bit depth (samples of 1 byte at 8 bits, else 2).  The arguments must have passed
 * jms_check_setting and jms_check.  Returns JMS_OK, or JMS_INVALID when memory for the tables or
 * the intermediate plane is not to be had. */
static inline int jms_scale(const uint8_t *src, int w, int h, int pw, int ph, uint8_t *dst, int W, int H, int ow, int oh, int filter, int flags,
                            int bd) {
    const int es = bd > 8 ? 2 : 1, P = 14 - bd;
    const int32_t maxv = (1 << bd) - 1;
    int st = JMS_OK;
    for (int pl = 0; pl < 3 && st == JMS_OK; pl++) {
        const int sw = pl ? w / 2 : w, sh = pl ? h / 2 : h, dw = pl ? ow / 2 : ow, dh = pl ? oh / 2 : oh;
        const int SPW = pl ? pw / 2 : pw, PW = pl ? W / 2 : W, PH = pl ? H / 2 : H;
        const uint8_t *s = src + jmi_dst_off(pl, pw, ph) * es;
        uint8_t *d = dst + jmi_dst_off(pl, W, H) * es;
        int Th = 0, Tv = 0;
        int32_t *fh = (int32_t *)malloc(sizeof(int32_t) * dw), *fv = (int32_t *)malloc(sizeof(int32_t) * dh);
        int16_t *th = (int16_t *)malloc(sizeof(int16_t) * dw * JMS_TAPS_MAX), *tv = (int16_t *)malloc(sizeof(int16_t) * dh * JMS_TAPS_MAX);
        int16_t *mid = (int16_t *)malloc(sizeof(int16_t) * (size_t)sh * dw);
        if (!fh || !fv || !th || !tv || !mid) st = JMS_INVALID;
        if (st == JMS_OK) st = jms_taps(sw, dw, filter, pl && (flags & JMS_CHROMA_LEFT), fh, th, &Th);
        if (st == JMS_OK) st = jms_taps(sh, dh, filter, 0, fv, tv, &Tv);
        if (st == JMS_OK) {
            for (int y = 0; y < sh; y++)
                for (int x = 0; x < dw; x++) {
                    int32_t sum = 0;
                    for (int j = 0; j < Th; j++) {
                        const size_t at = (size_t)y * SPW + jms_tap_at(fh[x] + j, sw);
                        uint32_t v;
                        if (es == 2) { uint16_t t; memcpy(&t, s + at * 2, 2); v = t; }
                        else v = s[at];
                        sum += th[(size_t)x * Th + j] * (int32_t)v;
                    }
                    mid[(size_t)y * dw + x] = (int16_t)jms_hpass(sum, P);
                }
            for (int y = 0; y < PH; y++)
                for (int x = 0; x < PW; x++) {
                    const int cx = jmi_clamp(x, dw), cy = jmi_clamp(y, dh);   /* the padding: the last column and row again */
                    int32_t sum = 0;
                    for (int k = 0; k < Tv; k++) sum += tv[(size_t)cy * Tv + k] * (int32_t)mid[(size_t)jms_tap_at(fv[cy] + k, sh) * dw + cx];
                    const int32_t v = jms_vpass(sum, P, maxv);
                    if (es == 2) { const uint16_t t = (uint16_t)v; memcpy(d + ((size_t)y * PW + x) * 2, &t, 2); }
                    else d[(size_t)y * PW + x] = (uint8_t)v;
                }
        }
        free(fh); free(fv); free(th); free(tv); free(mid);
    }
    return st;
}
#endif /* JMH_SCALE_H */
