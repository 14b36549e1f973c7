/*
 * ingest_check.c — the device-picture core (csrc/jmh_ingest.h, the text k_ingest of
 * csrc/jmh_ingest.hip compiles) on the CPU (TEST INFRASTRUCTURE).  For every format the source
 * planes are built in malloc blocks of exactly their bytes ((rows - 1) * stride + the row's bytes),
 * so an offset outside a plane is an ASan error.  The picture is ingested through the core
 * (jmi_ingest) and compared with a plain restatement: the samples unpacked to planar, clamped as
 * host/yuv.c read_hbd clamps them, then jm_pad_picture (host/yuv.c).
 *
 * Coded 32x32 with sources 32x32, 18x18, 30x2, 2x30, 2x2 (chroma 1x1); coded 48x32 with 34x18.
 * Strides: tight, +1 (8-bit), +2, +26 bytes.  I010 (bit depths 9 and 10) sources hold 0, maxv,
 * maxv + 1 and 65535 among random samples of which about one in eight exceeds maxv; the clamp
 * count must equal the number of such source samples.  Also: jmi_deint and jmi_value_x2 against
 * their per-sample meaning, and the argument rules of jmi_check.
 *
 * Exit 0: everything equal.  Built with -fsanitize=address,undefined (tests/harness/ingest.mk).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../h264-jm-commentary_amd/csrc/jmh_ingest.h"
#include "jmhost.h"

static uint64_t rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(void) {
    rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
    return (uint32_t)((rng * 0x2545F4914F6CDD1DULL) >> 32);
}

static long s_pics, s_bad, s_clamped;

/* one picture: format, coded W x H, source w x h, pad bytes per row, bit depth */
static void one(int format, int W, int H, int w, int h, int pad, int bd) {
    const int wide = jmi_wide(format), semi = jmi_semi(format), es = wide ? 2 : 1;
    const uint32_t maxv = (1u << bd) - 1;
    const int pw[3] = {w, w / 2, w / 2}, ph[3] = {h, h / 2, h / 2};
    uint16_t *smp[3];
    uint64_t expect_clamped = 0;
    /* the planar samples as the source holds them (P010: before the shift) */
    for (int pl = 0; pl < 3; pl++) {
        const int n = pw[pl] * ph[pl];
        smp[pl] = malloc((size_t)n * sizeof(uint16_t));
        for (int i = 0; i < n; i++) {
            uint32_t v = rnd();
            if (format == JMI_I010) v = (v & 7) == 0 ? maxv + 1 + (v >> 8) % (65535 - maxv) : (v >> 8) & maxv;
            else v = (v >> 8) & (wide ? 1023 : 255);
            smp[pl][i] = (uint16_t)v;
        }
        if (format == JMI_I010) {
            const uint16_t special[4] = {0, (uint16_t)maxv, (uint16_t)(maxv + 1), 65535};
            for (int i = 0; i < 4; i++) smp[pl][(n - 1) * i / 3] = special[i];   /* the first and the last sample among them */
            for (int i = 0; i < n; i++) expect_clamped += smp[pl][i] > maxv;
        }
    }
    /* the source planes, exact size */
    uint8_t *plane[3] = {NULL, NULL, NULL};
    int64_t stride[3] = {0, 0, 0};
    for (int sp = 0; sp < jmi_planes(format); sp++) {
        const int64_t rb = jmi_row_bytes(format, sp, w);
        const int rows = jmi_rows(sp, h);
        stride[sp] = rb + pad;
        const size_t bytes = (size_t)((rows - 1) * stride[sp] + rb);
        plane[sp] = malloc(bytes);
        memset(plane[sp], 0xA5, bytes);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < (int)(rb / es); x++) {
                int pl = sp, sx = x;
                if (sp && semi) { pl = 1 + (x & 1); sx = x >> 1; }
                uint32_t v = smp[pl][y * pw[pl] + sx];
                if (format == JMI_P010) v = v << 6 | (rnd() & 63);
                uint8_t *d = plane[sp] + (size_t)y * stride[sp] + (size_t)x * es;
                if (wide) { const uint16_t t = (uint16_t)v; memcpy(d, &t, 2); }
                else *d = (uint8_t)v;
            }
    }
    int bad = 0;
    if (jmi_check(format, w, h, W, H, (const void *const *)plane, stride) || !jmi_depth_ok(format, bd)) bad = 1;
    /* through the core */
    uint8_t *got = malloc((size_t)W * H * 3 / 2 * es);
    const uint64_t clamped = jmi_ingest(format, (const uint8_t *const *)plane, stride, w, h, W, H, maxv, got);
    /* the restatement */
    jm_pic ref;
    if (jm_pic_alloc_bd(&ref, W, H, bd)) { fprintf(stderr, "out of memory\n"); exit(2); }
    for (int pl = 0; pl < 3; pl++) {
        const int PW = pl ? W / 2 : W;
        for (int y = 0; y < ph[pl]; y++)
            for (int x = 0; x < pw[pl]; x++) {
                const uint32_t s = smp[pl][y * pw[pl] + x], v = s > maxv ? maxv : s;
                if (wide) (pl == 0 ? ref.Y : pl == 1 ? ref.U : ref.V)[(size_t)y * PW + x] = (uint16_t)v;
                else (pl == 0 ? ref.y : pl == 1 ? ref.u : ref.v)[(size_t)y * PW + x] = (uint8_t)v;
            }
    }
    jm_pad_picture(&ref, w, h);
    if (memcmp(got, wide ? (const void *)ref.Y : (const void *)ref.y, (size_t)W * H * 3 / 2 * es)) bad = 1;
    if (clamped != expect_clamped) bad = 1;
    if (bad) {
        fprintf(stderr, "format %d coded %dx%d source %dx%d pad %d depth %d: differs (clamped %llu, expected %llu)\n", format, W, H, w, h, pad,
                bd, (unsigned long long)clamped, (unsigned long long)expect_clamped);
        s_bad++;
    }
    s_pics++;
    s_clamped += (long)clamped;
    jm_pic_free(&ref);
    free(got);
    for (int i = 0; i < 3; i++) { free(smp[i]); free(plane[i]); }
}

static void check_words(void) {
    for (int i = 0; i < 4096; i++) {
        const uint32_t lo = rnd(), hi = rnd();
        const uint8_t b[8] = {(uint8_t)lo, (uint8_t)(lo >> 8), (uint8_t)(lo >> 16), (uint8_t)(lo >> 24),
                              (uint8_t)hi, (uint8_t)(hi >> 8), (uint8_t)(hi >> 16), (uint8_t)(hi >> 24)};
        for (int which = 0; which < 2; which++) {
            const uint32_t e8 = (uint32_t)b[which] | (uint32_t)b[2 + which] << 8 | (uint32_t)b[4 + which] << 16 | (uint32_t)b[6 + which] << 24;
            const uint32_t e16 = (uint32_t)b[2 * which] | (uint32_t)b[2 * which + 1] << 8 | (uint32_t)b[4 + 2 * which] << 16 |
                                 (uint32_t)b[5 + 2 * which] << 24;
            if (jmi_deint(lo, hi, which, 0) != e8 || jmi_deint(lo, hi, which, 1) != e16) { fprintf(stderr, "jmi_deint differs\n"); s_bad++; return; }
        }
        uint32_t over = 0, o2 = 0;
        const uint32_t a = jmi_value(JMI_I010, lo & 0xffff, 511, &o2), c = jmi_value(JMI_I010, lo >> 16, 511, &o2);
        if (jmi_value_x2(JMI_I010, lo, 511, &over) != (a | c << 16) || over != o2 || a > 511 || c > 511 ||
            jmi_value_x2(JMI_P010, lo, 1023, &over) != ((lo & 0xffff) >> 6 | (lo >> 22) << 16)) { fprintf(stderr, "jmi_value_x2 differs\n"); s_bad++; return; }
    }
}

static void check_rules(void) {
    _Alignas(16) static uint8_t mem[64];
    const void *pl[3] = {mem, mem + 16, mem + 32};
    const void *odd[3] = {mem, mem + 17, mem + 32};
    const void *two[3] = {mem, mem + 16, NULL};
    const int64_t st8[3] = {32, 16, 16}, st16[3] = {64, 32, 32}, sh[3] = {32, 15, 16}, so[3] = {64, 33, 32}, semi16[3] = {64, 64, 0};
    int bad = 0;
    bad |= jmi_check(JMI_I420, 32, 32, 32, 32, pl, st8) != 0;
    bad |= jmi_check(JMI_NV12, 32, 32, 32, 32, two, st8) == 0;          /* the UV row needs 32 bytes */
    bad |= jmi_check(JMI_P010, 32, 32, 32, 32, two, semi16) != 0;       /* plane[2] is not read */
    bad |= jmi_check(JMI_I420, 32, 32, 32, 32, two, st8) == 0;          /* a null plane */
    bad |= jmi_check(JMI_I420, 31, 32, 32, 32, pl, st8) == 0;           /* odd */
    bad |= jmi_check(JMI_I420, 32, 34, 32, 32, pl, st8) == 0;           /* beyond the coded size */
    bad |= jmi_check(JMI_I420, 0, 32, 32, 32, pl, st8) == 0;
    bad |= jmi_check(JMI_I420, 32, 32, 32, 32, pl, sh) == 0;            /* a short stride */
    bad |= jmi_check(JMI_I010, 32, 32, 32, 32, pl, st16) != 0;
    bad |= jmi_check(JMI_I010, 32, 32, 32, 32, odd, st16) == 0;         /* an odd 16-bit address */
    bad |= jmi_check(JMI_I010, 32, 32, 32, 32, pl, so) == 0;            /* an odd 16-bit stride */
    bad |= jmi_check(JMI_I420, 32, 32, 32, 32, odd, st8) != 0;          /* 8 bits: any address */
    bad |= jmi_check(4, 32, 32, 32, 32, pl, st8) == 0 || jmi_check(-1, 32, 32, 32, 32, pl, st8) == 0;
    bad |= jmi_depth_ok(JMI_I420, 10) || jmi_depth_ok(JMI_NV12, 9) || jmi_depth_ok(JMI_I010, 8) || jmi_depth_ok(JMI_P010, 9) ||
           !jmi_depth_ok(JMI_I010, 9) || !jmi_depth_ok(JMI_P010, 10);
    if (bad) { fprintf(stderr, "jmi_check / jmi_depth_ok: a rule differs\n"); s_bad++; }
}

int main(void) {
    static const int sizes[6][4] = {{32, 32, 32, 32}, {32, 32, 18, 18}, {32, 32, 30, 2}, {32, 32, 2, 30}, {32, 32, 2, 2}, {48, 32, 34, 18}};
    static const int pads[4] = {0, 1, 2, 26};
    for (int s = 0; s < 6; s++)
        for (int format = 0; format < JMI_NFORMATS; format++)
            for (int p = 0; p < 4; p++) {
                if (jmi_wide(format) && (pads[p] & 1)) continue;
                one(format, sizes[s][0], sizes[s][1], sizes[s][2], sizes[s][3], pads[p], format == JMI_I420 || format == JMI_NV12 ? 8 : 10);
                if (format == JMI_I010) one(format, sizes[s][0], sizes[s][1], sizes[s][2], sizes[s][3], pads[p], 9);
            }
    check_words();
    check_rules();
    printf("ingest check: %ld pictures, %ld clamped samples, %ld differ\n", s_pics, s_clamped, s_bad);
    return s_bad ? 1 : 0;
}
