/*
 * yuv_check.c — the 4:2:2 / 4:4:4 device-picture core (csrc/jmh_yuv.h, the text k_ingest_yuv of
 * csrc/jmh_yuv.hip compiles) on the CPU (TEST INFRASTRUCTURE).  For every format, and for both
 * sitings of the 4:4:4 ones, the source planes are built in malloc blocks of exactly their bytes
 * ((rows - 1) * stride + the row's bytes), so an offset outside a plane is an ASan error.  The
 * picture is reduced through the core (jmy_reduce) and compared with a plain restatement that shares
 * no line with it: the samples kept planar, clamped, reduced with the formulas of
 * include/jmhip_yuv.h written out, then jm_pad_picture (host/yuv.c).  The planes are packed here
 * format by format, not through jmy_comp.
 *
 * Coded 32x32 with sources 32x32, 18x18, 30x2, 2x30, 2x2 (chroma 1x1); coded 48x32 with 34x18.
 * Strides: tight, +1 (the formats of single bytes), +4, +28 bytes.  I210 and I410 (bit depths 10
 * and 9) sources hold 0, maxv, maxv + 1 and 65535 among random samples of which about one in eight
 * exceeds maxv; the clamp count must equal the number of such source samples.  Also the argument
 * rules of jmy_check.
 *
 * Exit 0: everything equal.  Built with -fsanitize=address,undefined (tests/harness/yuv.mk).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../h264-jm-commentary_amd/csrc/jmh_yuv.h"
#include "jmhost.h"

static uint64_t rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(void) {
    rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
    return (uint32_t)((rng * 0x2545F4914F6CDD1DULL) >> 32);
}

static long s_pics, s_bad, s_clamped;

static void put16(uint8_t *p, uint32_t v) { const uint16_t t = (uint16_t)v; memcpy(p, &t, 2); }
static void or32(uint8_t *p, uint32_t v) { uint32_t t; memcpy(&t, p, 4); t |= v; memcpy(p, &t, 4); }

/* where sample k of component c lies in its row, format by format: the plane, and the byte in the row */
static void place(int layout, int c, int k, int *sp, int64_t *byte) {
    switch (layout) {
    case JMY_I422: case JMY_I444: *sp = c; *byte = k; break;
    case JMY_I210: case JMY_I410: *sp = c; *byte = 2 * (int64_t)k; break;
    case JMY_NV16: *sp = c ? 1 : 0; *byte = c ? 2 * (int64_t)k + (c - 1) : k; break;
    case JMY_P210: *sp = c ? 1 : 0; *byte = c ? 4 * (int64_t)k + 2 * (c - 1) : 2 * (int64_t)k; break;
    case JMY_YUYV: *sp = 0; *byte = c == 0 ? 2 * (int64_t)k : c == 1 ? 4 * (int64_t)k + 1 : 4 * (int64_t)k + 3; break;
    case JMY_UYVY: *sp = 0; *byte = c == 0 ? 2 * (int64_t)k + 1 : c == 1 ? 4 * (int64_t)k : 4 * (int64_t)k + 2; break;
    case JMY_Y210: *sp = 0; *byte = c == 0 ? 4 * (int64_t)k : c == 1 ? 8 * (int64_t)k + 2 : 8 * (int64_t)k + 6; break;
    case JMY_VUYA8: *sp = 0; *byte = 4 * (int64_t)k + (c == 0 ? 2 : c == 1 ? 1 : 0); break;
    default /* JMY_Y410 */: *sp = 0; *byte = 4 * (int64_t)k; break;
    }
}
/* bytes of a row of plane sp, format by format */
static int64_t row_bytes(int layout, int sp, int w) {
    switch (layout) {
    case JMY_I422: return sp ? w / 2 : w;
    case JMY_I210: return sp ? w : 2 * w;
    case JMY_NV16: return sp < 2 ? w : 0;
    case JMY_P210: return sp < 2 ? 2 * w : 0;
    case JMY_YUYV: case JMY_UYVY: return sp ? 0 : 2 * w;
    case JMY_I444: return w;
    case JMY_I410: return 2 * w;
    default /* Y210, VUYA8, Y410 */: return sp ? 0 : 4 * w;
    }
}

/* one picture: format (with its flag), coded W x H, source w x h, pad bytes per row, bit depth */
static void one(int format, int W, int H, int w, int h, int pad, int bd) {
    const int layout = format & ~JMY_CHROMA_LEFT, left = (format & JMY_CHROMA_LEFT) != 0;
    const int wide = layout >= JMY_I210, es = wide ? 2 : 1;
    const int is444 = layout == JMY_I444 || layout == JMY_VUYA8 || layout == JMY_I410 || layout == JMY_Y410;
    const int low = layout == JMY_I210 || layout == JMY_I410, high = layout == JMY_P210 || layout == JMY_Y210;
    const uint32_t maxv = (1u << bd) - 1;
    const int cw[3] = {w, is444 ? w : w / 2, is444 ? w : w / 2};
    uint16_t *smp[3];
    uint64_t expect_clamped = 0;
    /* the planar samples as the source holds them (P210, Y210: before the shift) */
    for (int c = 0; c < 3; c++) {
        const int n = cw[c] * h;
        smp[c] = malloc((size_t)n * sizeof(uint16_t));
        for (int i = 0; i < n; i++) {
            uint32_t v = rnd();
            if (low) v = (v & 7) == 0 ? maxv + 1 + (v >> 8) % (65535 - maxv) : (v >> 8) & maxv;
            else v = (v >> 8) & (wide ? 1023 : 255);
            smp[c][i] = (uint16_t)v;
        }
        if (low) {
            const uint16_t special[4] = {0, (uint16_t)maxv, (uint16_t)(maxv + 1), 65535};
            for (int i = 0; i < 4; i++) smp[c][(n - 1) * i / 3] = special[i];   /* the first and the last sample among them */
            for (int i = 0; i < n; i++) expect_clamped += smp[c][i] > maxv;
        }
    }
    /* the source planes, exact size */
    uint8_t *plane[3] = {NULL, NULL, NULL};
    int64_t stride[3] = {0, 0, 0};
    for (int sp = 0; sp < 3; sp++) {
        const int64_t rb = row_bytes(layout, sp, w);
        if (!rb) continue;
        stride[sp] = rb + pad;
        const size_t bytes = (size_t)((h - 1) * stride[sp] + rb);
        plane[sp] = malloc(bytes);
        memset(plane[sp], layout == JMY_Y410 ? 0 : 0xA5, bytes);
    }
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < h; y++)
            for (int k = 0; k < cw[c]; k++) {
                int sp;
                int64_t byte;
                place(layout, c, k, &sp, &byte);
                uint8_t *d = plane[sp] + (size_t)y * stride[sp] + byte;
                uint32_t v = smp[c][y * cw[c] + k];
                if (high) v = v << 6 | (rnd() & 63);
                if (layout == JMY_Y410) or32(d, v << (c == 0 ? 10 : c == 1 ? 0 : 20) | (c == 0 ? rnd() << 30 : 0));
                else if (wide) put16(d, v);
                else *d = (uint8_t)v;
                if (layout == JMY_VUYA8 && c == 0) d[1] = (uint8_t)rnd();       /* alpha */
            }
    int bad = 0;
    if (jmy_check(format, w, h, W, H, (const void *const *)plane, stride) || !jmy_depth_ok(format, bd)) bad = 1;
    /* through the core */
    uint8_t *got = malloc((size_t)W * H * 3 / 2 * es);
    const uint64_t clamped = jmy_reduce(format, (const uint8_t *const *)plane, stride, w, h, W, H, maxv, got);
    /* the restatement */
    jm_pic ref;
    if (jm_pic_alloc_bd(&ref, W, H, bd)) { fprintf(stderr, "out of memory\n"); exit(2); }
#define S(c, x, y) ((uint32_t)(smp[c][(y) * cw[c] + (x)] > maxv ? maxv : smp[c][(y) * cw[c] + (x)]))
    for (int pl = 0; pl < 3; pl++) {
        const int PW = pl ? W / 2 : W, rw = pl ? w / 2 : w, rh = pl ? h / 2 : h;
        for (int y = 0; y < rh; y++)
            for (int x = 0; x < rw; x++) {
                uint32_t v;
                if (pl == 0) v = S(0, x, y);
                else if (!is444) v = (S(pl, x, 2 * y) + S(pl, x, 2 * y + 1) + 1) >> 1;
                else if (!left) v = (S(pl, 2 * x, 2 * y) + S(pl, 2 * x + 1, 2 * y) + S(pl, 2 * x, 2 * y + 1) + S(pl, 2 * x + 1, 2 * y + 1) + 2) >> 2;
                else {
                    const int xl = 2 * x - 1 > 0 ? 2 * x - 1 : 0;
                    const uint32_t h0 = S(pl, xl, 2 * y) + 2 * S(pl, 2 * x, 2 * y) + S(pl, 2 * x + 1, 2 * y);
                    const uint32_t h1 = S(pl, xl, 2 * y + 1) + 2 * S(pl, 2 * x, 2 * y + 1) + S(pl, 2 * x + 1, 2 * y + 1);
                    v = (h0 + h1 + 4) >> 3;
                }
                if (wide) (pl == 0 ? ref.Y : pl == 1 ? ref.U : ref.V)[(size_t)y * PW + x] = (uint16_t)v;
                else (pl == 0 ? ref.y : pl == 1 ? ref.u : ref.v)[(size_t)y * PW + x] = (uint8_t)v;
            }
    }
#undef S
    jm_pad_picture(&ref, w, h);
    if (memcmp(got, wide ? (const void *)ref.Y : (const void *)ref.y, (size_t)W * H * 3 / 2 * es)) bad = 1;
    if (clamped != expect_clamped) bad = 1;
    if (bad) {
        fprintf(stderr, "format %d%s coded %dx%d source %dx%d pad %d depth %d: differs (clamped %llu, expected %llu)\n", layout, left ? " left" : "", W, H,
                w, h, pad, bd, (unsigned long long)clamped, (unsigned long long)expect_clamped);
        s_bad++;
    }
    s_pics++;
    s_clamped += (long)clamped;
    jm_pic_free(&ref);
    free(got);
    for (int i = 0; i < 3; i++) { free(smp[i]); free(plane[i]); }
}

static void check_rules(void) {
    _Alignas(16) static uint8_t mem[64];
    const void *pl[3] = {mem, mem + 16, mem + 32};
    const void *odd[3] = {mem + 1, mem + 16, mem + 32};
    const void *by2[3] = {mem + 2, NULL, NULL};
    const void *one_[3] = {mem, NULL, NULL};
    const void *two[3] = {mem, mem + 16, NULL};
    const int64_t s8[3] = {8, 4, 4}, s444[3] = {8, 8, 8},s16[3] = {16, 8, 8}, s32[3] = {32, 32, 32}, sh[3] = {8, 3, 4}, s30[3] = {30, 0, 0}, s31[3] = {31, 0, 0};
    int bad = 0;
    bad |= jmy_check(JMY_I422, 8, 2, 8, 2, pl, s8) != 0;
    bad |= jmy_check(JMY_I422, 8, 2, 8, 2, two, s8) == 0;                /* a null plane that is read */
    bad |= jmy_check(JMY_I422, 8, 2, 8, 2, pl, sh) == 0;                 /* a short chroma stride */
    bad |= jmy_check(JMY_I422 | JMY_CHROMA_LEFT, 8, 2, 8, 2, pl, s8) != 0;   /* accepted, no effect */
    bad |= jmy_left(JMY_I422 | JMY_CHROMA_LEFT) || !jmy_left(JMY_I444 | JMY_CHROMA_LEFT) || jmy_left(JMY_I444);
    bad |= jmy_check(JMY_NV16, 8, 2, 8, 2, two, s444) != 0;              /* plane[2] is not read */
    bad |= jmy_check(JMY_NV16, 8, 2, 8, 2, two, s8) == 0;                /* the UV row needs 8 bytes */
    bad |= jmy_check(JMY_YUYV, 8, 2, 8, 2, one_, s16) != 0 || jmy_check(JMY_UYVY, 8, 2, 8, 2, odd, s16) != 0;   /* bytes: any address */
    bad |= jmy_check(JMY_YUYV, 8, 2, 8, 2, one_, s8) == 0;               /* 2 * width */
    bad |= jmy_check(JMY_I444, 8, 2, 8, 2, pl, s444) != 0 || jmy_check(JMY_I444, 8, 2, 8, 2, pl, s8) == 0;        /* full-size chroma rows */
    bad |= jmy_check(JMY_VUYA8, 8, 2, 8, 2, one_, s32) != 0 || jmy_check(JMY_VUYA8, 8, 2, 8, 2, by2, s32) == 0;   /* dwords */
    bad |= jmy_check(JMY_VUYA8, 7, 2, 8, 2, one_, s30) == 0 || jmy_check(JMY_VUYA8, 6, 2, 8, 2, one_, s30) == 0;  /* odd; a stride that is no multiple of 4 */
    bad |= jmy_check(JMY_I210, 8, 2, 8, 2, pl, s16) != 0 || jmy_check(JMY_I210, 8, 2, 8, 2, odd, s16) == 0;       /* an odd 16-bit address */
    bad |= jmy_check(JMY_Y210, 6, 2, 8, 2, by2, s30) != 0 || jmy_check(JMY_Y210, 6, 2, 8, 2, one_, s31) == 0;     /* words: even is enough; an odd stride */
    bad |= jmy_check(JMY_Y410, 6, 2, 8, 2, by2, s32) == 0 || jmy_check(JMY_Y410, 8, 2, 8, 2, one_, s32) != 0;
    bad |= jmy_check(JMY_I444, 8, 4, 8, 2, pl, s444) == 0 || jmy_check(JMY_I444, 0, 2, 8, 2, pl, s444) == 0;         /* beyond the coded size; below 2 */
    for (int f = -1; f < 64; f++) {
        const int known = (f >= 32 && f <= 37) || (f >= 40 && f <= 44);
        bad |= jmy_is_yuv(f) != known || jmy_is_yuv(f | JMY_CHROMA_LEFT) != (known && f >= 0) || (f >= 0 && (jmy_is_yuv(f | 1 << 8) || jmy_is_yuv(f | 1 << 9) || jmy_is_yuv(f | 1 << 11)));
    }
    bad |= !jmy_depth_ok(JMY_UYVY, 8) || jmy_depth_ok(JMY_UYVY, 10) || !jmy_depth_ok(JMY_I210, 9) || !jmy_depth_ok(JMY_I410 | JMY_CHROMA_LEFT, 10) ||
           jmy_depth_ok(JMY_I210, 8) || jmy_depth_ok(JMY_P210, 9) || jmy_depth_ok(JMY_Y210, 8) || !jmy_depth_ok(JMY_Y410, 10) || jmy_depth_ok(JMY_Y410, 9);
    if (bad) { fprintf(stderr, "jmy_check / jmy_is_yuv / jmy_depth_ok: a rule differs\n"); s_bad++; }
}

int main(void) {
    static const int sizes[6][4] = {{32, 32, 32, 32}, {32, 32, 18, 18}, {32, 32, 30, 2}, {32, 32, 2, 30}, {32, 32, 2, 2}, {48, 32, 34, 18}};
    static const int pads[4] = {0, 1, 4, 28};
    static const int formats[15] = {JMY_I422, JMY_NV16, JMY_YUYV, JMY_UYVY, JMY_I444, JMY_I444 | JMY_CHROMA_LEFT, JMY_VUYA8, JMY_VUYA8 | JMY_CHROMA_LEFT,
                                    JMY_I210, JMY_P210, JMY_Y210, JMY_I410, JMY_I410 | JMY_CHROMA_LEFT, JMY_Y410, JMY_Y410 | JMY_CHROMA_LEFT};
    for (int s = 0; s < 6; s++)
        for (int f = 0; f < 15; f++)
            for (int p = 0; p < 4; p++) {
                const int layout = formats[f] & ~JMY_CHROMA_LEFT;
                const int bytes = layout <= JMY_I444;                    /* formats of single bytes */
                if (!bytes && (pads[p] & 1)) continue;
                one(formats[f], sizes[s][0], sizes[s][1], sizes[s][2], sizes[s][3], pads[p], layout >= JMY_I210 ? 10 : 8);
                if (layout == JMY_I210 || layout == JMY_I410) one(formats[f], sizes[s][0], sizes[s][1], sizes[s][2], sizes[s][3], pads[p], 9);
            }
    check_rules();
    printf("yuv check: %ld pictures, %ld clamped samples, %ld differ\n", s_pics, s_clamped, s_bad);
    return s_bad ? 1 : 0;
}
