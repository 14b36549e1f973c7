/*
 * rgb_check.c — the RGB device-picture core (csrc/jmh_rgb.h, the text k_ingest_rgb of csrc/jmh_rgb.hip
 * compiles) on the CPU (TEST INFRASTRUCTURE).  The source plane is built in a malloc block of exactly
 * its bytes ((h - 1) * stride + 4 * w), so an offset outside it is an ASan error.  Every combination
 * of the four layouts, the two matrices and the two ranges is converted through the core
 * (jmr_convert) and compared with a plain restatement: the words unpacked, converted at the source
 * size with the formulas of include/jmhip_rgb.h, then jm_pad_picture (host/yuv.c).
 *
 * Coded 32x32 with sources 32x32, 18x18, 30x2, 2x30, 2x2 (one chroma sample); coded 48x32 with 34x18.
 * Strides: tight, +4, +52 bytes.  The sources are random words (alpha noise included) and hold the
 * eight RGB corners as 2x2 blocks (2x2: the one block of the pure high component), so every full-range
 * picture has chroma the clamp changes; the count of such samples must equal the core's.
 * Also: (b) every row of the coefficient table against its float64 derivation from (Kr, Kb);
 * (c) every sample before its clamp within 0.5 + 3 M 2^-15 of the real-valued formula (0.5 for the
 * final rounding, 2^-15 M for each of the three rounded coefficients: derived, not measured);
 * (e) jmr_check and jmr_depth_ok against the argument rules.
 *
 * Exit 0: everything equal.  Built with -fsanitize=address,undefined (tests/harness/rgb.mk).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../h264-jm-commentary_amd/csrc/jmh_rgb.h"
#include "jmhost.h"

static uint64_t rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(void) {
    rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
    return (uint32_t)((rng * 0x2545F4914F6CDD1DULL) >> 32);
}

static long s_pics, s_bad, s_clamped, s_unclamped_full;
static double s_worst;   /* largest distance from the real-valued formula, in units of the bound */

/* the real-valued gains of a format at a bit depth: kyr kyg kyb | kur kug kub | kvr kvg kvb */
static void gains(int format, int bd, double *k, double *ys_out) {
    const double kr = (format & JMR_BT709) ? 0.2126 : 0.299, kb = (format & JMR_BT709) ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
    const double M = (double)((1 << bd) - 1), sc = (double)(1 << (bd - 8));
    const double ys = (format & JMR_FULL_RANGE) ? M : 219.0 * sc, cs = (format & JMR_FULL_RANGE) ? M : 224.0 * sc;
    k[0] = kr * ys / M; k[1] = kg * ys / M; k[2] = kb * ys / M;
    k[3] = -kr / (2 * (1 - kb)) * cs / M; k[4] = -kg / (2 * (1 - kb)) * cs / M; k[5] = 0.5 * cs / M;
    k[6] = 0.5 * cs / M; k[7] = -kg / (2 * (1 - kr)) * cs / M; k[8] = -kb / (2 * (1 - kr)) * cs / M;
    *ys_out = ys;
}

/* (b) the table row of a format against the derivation */
static void check_row(int format, int bd) {
    double k[9], ys;
    jmr_coef c;
    gains(format, bd, k, &ys);
    jmr_coefficients(format, bd, &c);
    const double M = (double)((1 << bd) - 1), q = 16384.0;
    int32_t e[9];
    e[0] = (int32_t)rint(k[0] * q); e[2] = (int32_t)rint(k[2] * q); e[1] = (int32_t)rint(ys / M * q) - e[0] - e[2];
    e[3] = (int32_t)rint(k[3] * q); e[5] = (int32_t)rint(k[5] * q); e[4] = -e[3] - e[5];
    e[6] = (int32_t)rint(k[6] * q); e[8] = (int32_t)rint(k[8] * q); e[7] = -e[6] - e[8];
    int bad = memcmp(e, c.c, sizeof(e)) != 0;
    bad |= c.yo != ((format & JMR_FULL_RANGE) ? 0 : 16 << (bd - 8)) || c.co != 1 << (bd - 1) || c.maxv != (1 << bd) - 1;
    /* black, white and grey: Yo, Yo + Ys, Co */
    const int32_t m = c.maxv;
    bad |= jmr_luma(&c, 0, 0, 0) != c.yo || jmr_luma(&c, m, m, m) != c.yo + (int32_t)ys;
    for (int g = 0; g <= m; g += m / 5) bad |= jmr_chroma(&c, 0, 4 * g, 4 * g, 4 * g) != c.co || jmr_chroma(&c, 1, 4 * g, 4 * g, 4 * g) != c.co;
    if (bad) { fprintf(stderr, "format %#x depth %d: the coefficient row differs from its derivation\n", format, bd); s_bad++; }
}

/* the words of a corner: component bits 0..2 of i in the low, middle, high field, alpha set */
static uint32_t corner(int layout, int i) {
    const int sh = jmr_ten(layout) ? 10 : 8;
    const uint32_t top = (1u << sh) - 1;
    return ((i & 1) ? top : 0) | ((i & 2) ? top << sh : 0) | ((i & 4) ? top << 2 * sh : 0) | (jmr_ten(layout) ? 3u << 30 : 0xffu << 24);
}

/* one picture: format with flags, coded W x H, source w x h, pad bytes per row */
static void one(int format, int W, int H, int w, int h, int pad) {
    const int layout = jmr_layout(format), bd = jmr_ten(layout) ? 10 : 8, es = bd > 8 ? 2 : 1;
    uint32_t *px = malloc((size_t)w * h * sizeof(uint32_t));
    for (int i = 0; i < w * h; i++) px[i] = rnd();
    for (int i = 0; i < 8; i++)                      /* (d) the eight corners as 2x2 blocks */
        for (int j = 0; j < 4; j++) {
            if (w >= 16) px[(j >> 1) * w + 2 * i + (j & 1)] = corner(layout, i);
            else if (h >= 16) px[(2 * i + (j >> 1)) * w + (j & 1)] = corner(layout, i);
            else px[(j >> 1) * w + (j & 1)] = corner(layout, 4);
        }
    /* the source plane, exact size */
    const int64_t stride = (int64_t)4 * w + pad;
    const size_t bytes = (size_t)((h - 1) * stride + 4 * w);
    uint8_t *plane = malloc(bytes);
    memset(plane, 0xA5, bytes);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t v = px[y * w + x];
            uint8_t *d = plane + (size_t)y * stride + (size_t)4 * x;
            d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24);
        }
    int bad = 0;
    const void *pl[3] = {plane, NULL, NULL};
    const int64_t st[3] = {stride, 0, 0};
    if (jmr_check(format, w, h, W, H, pl, st) || !jmr_depth_ok(format, bd)) bad = 1;
    /* through the core */
    uint8_t *got = malloc((size_t)W * H * 3 / 2 * es);
    const uint64_t clamped = jmr_convert(format, bd, plane, stride, w, h, W, H, got);
    /* the restatement, with (c) on the way */
    double k[9], ys;
    gains(format, bd, k, &ys);
    jmr_coef c;
    jmr_coefficients(format, bd, &c);
    const double bound = 0.5 + 3.0 * c.maxv / 32768.0;
    uint64_t expect_clamped = 0;
    jm_pic ref;
    if (jm_pic_alloc_bd(&ref, W, H, bd)) { fprintf(stderr, "out of memory\n"); exit(2); }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int32_t r, g, b;
            jmr_unpack(layout, px[y * w + x], &r, &g, &b);
            const int32_t v = c.yo + ((c.c[0] * r + c.c[1] * g + c.c[2] * b + 8192) >> 14);
            const double d = fabs(v - (c.yo + k[0] * r + k[1] * g + k[2] * b)) / bound;
            if (d > s_worst) s_worst = d;
            if (v < 0 || v > c.maxv) bad = 1;       /* Y cannot leave its range */
            if (bd > 8) ref.Y[(size_t)y * W + x] = (uint16_t)v; else ref.y[(size_t)y * W + x] = (uint8_t)v;
        }
    for (int y = 0; y < h / 2; y++)
        for (int x = 0; x < w / 2; x++) {
            int32_t rs = 0, gs = 0, bs = 0;
            for (int i = 0; i < 4; i++) {
                int32_t r, g, b;
                jmr_unpack(layout, px[(2 * y + (i >> 1)) * w + 2 * x + (i & 1)], &r, &g, &b);
                rs += r; gs += g; bs += b;
            }
            for (int which = 0; which < 2; which++) {
                const int32_t *q = c.c + 3 + 3 * which;
                const int32_t raw = c.co + ((q[0] * rs + q[1] * gs + q[2] * bs + 32768) >> 16);
                const int32_t v = raw < 0 ? 0 : raw > c.maxv ? c.maxv : raw;
                const double d = fabs(raw - (c.co + (k[3 + 3 * which] * rs + k[4 + 3 * which] * gs + k[5 + 3 * which] * bs) / 4.0)) / bound;
                if (d > s_worst) s_worst = d;
                expect_clamped += v != raw;
                if (bd > 8) (which ? ref.V : ref.U)[(size_t)y * (W / 2) + x] = (uint16_t)v;
                else (which ? ref.v : ref.u)[(size_t)y * (W / 2) + x] = (uint8_t)v;
            }
        }
    jm_pad_picture(&ref, w, h);
    if (memcmp(got, bd > 8 ? (const void *)ref.Y : (const void *)ref.y, (size_t)W * H * 3 / 2 * es)) bad = 1;
    if (clamped != expect_clamped) bad = 1;
    if (!(format & JMR_FULL_RANGE) && clamped) bad = 1;              /* limited range stays inside 16..240 */
    if ((format & JMR_FULL_RANGE) && !clamped) s_unclamped_full++;   /* (d) */
    if (bad) {
        fprintf(stderr, "format %#x coded %dx%d source %dx%d pad %d: differs (clamped %llu, expected %llu)\n", format, W, H, w, h, pad,
                (unsigned long long)clamped, (unsigned long long)expect_clamped);
        s_bad++;
    }
    s_pics++;
    s_clamped += (long)clamped;
    jm_pic_free(&ref);
    free(got); free(plane); free(px);
}

static void check_words(void) {
    int bad = 0;
    int32_t r, g, b;
    jmr_unpack(JMR_BGRA8, 0xAA332211u, &r, &g, &b);   bad |= r != 0x33 || g != 0x22 || b != 0x11;
    jmr_unpack(JMR_RGBA8, 0xAA332211u, &r, &g, &b);   bad |= r != 0x11 || g != 0x22 || b != 0x33;
    jmr_unpack(JMR_RGB10A2, 3u << 30 | 0x3A1u << 20 | 0x155u << 10 | 0x2C3u, &r, &g, &b); bad |= r != 0x2C3 || g != 0x155 || b != 0x3A1;
    jmr_unpack(JMR_BGR10A2, 1u << 30 | 0x3A1u << 20 | 0x155u << 10 | 0x2C3u, &r, &g, &b); bad |= r != 0x3A1 || g != 0x155 || b != 0x2C3;
    jmr_coef c;
    jmr_coefficients(JMR_RGBA8 | JMR_FULL_RANGE, 8, &c);
    bad |= jmr_chroma_raw(&c, 0, 0, 0, 4 * 255) != 256 || jmr_chroma(&c, 0, 0, 0, 4 * 255) != 255;   /* pure blue: the live clamp */
    bad |= jmr_chroma_raw(&c, 1, 4 * 255, 0, 0) != 256 || jmr_chroma(&c, 1, 4 * 255, 0, 0) != 255;
    if (bad) { fprintf(stderr, "jmr_unpack / jmr_chroma: a word differs\n"); s_bad++; }
}

/* (e) */
static void check_rules(void) {
    _Alignas(16) static uint8_t mem[64];
    const void *pl[3] = {mem, NULL, NULL}, *two[3] = {mem + 2, NULL, NULL}, *four[3] = {mem + 4, NULL, NULL}, *none[3] = {NULL, mem, mem};
    const int64_t st[3] = {128, 0, 0}, sh[3] = {124, 0, 0}, so[3] = {130, 0, 0}, s4[3] = {132, 0, 0}, big[3] = {256, 0, 0};
    int bad = 0;
    for (int f = JMR_BGRA8; f <= JMR_BGR10A2; f++)
        for (int fl = 0; fl < 4; fl++) bad |= jmr_check(f | fl << 8, 32, 32, 32, 32, pl, st) != 0;
    bad |= jmr_check(JMR_BGRA8, 32, 32, 32, 32, four, s4) != 0;               /* any multiple of 4 */
    bad |= jmr_check(JMR_BGRA8, 32, 32, 32, 32, none, st) == 0;               /* a null plane[0] */
    bad |= jmr_check(JMR_BGRA8, 32, 32, 32, 32, pl, sh) == 0;                 /* stride 4w - 4 */
    bad |= jmr_check(JMR_BGRA8, 32, 32, 32, 32, two, st) == 0;                /* address + 2 */
    bad |= jmr_check(JMR_BGRA8, 32, 32, 32, 32, pl, so) == 0;                 /* stride + 2 */
    bad |= jmr_check(JMR_BGRA8, 31, 32, 32, 32, pl, st) == 0 || jmr_check(JMR_BGRA8, 32, 31, 32, 32, pl, st) == 0;   /* odd */
    bad |= jmr_check(JMR_BGRA8, 0, 32, 32, 32, pl, st) == 0 || jmr_check(JMR_BGRA8, 32, 0, 32, 32, pl, st) == 0;
    bad |= jmr_check(JMR_BGRA8, 32, 34, 32, 32, pl, st) == 0 || jmr_check(JMR_BGRA8, 34, 32, 32, 32, pl, big) == 0;   /* beyond the coded size */
    bad |= jmr_check(JMR_BGRA8 | 1 << 10, 32, 32, 32, 32, pl, st) == 0 || jmr_check(JMR_BGRA8 | 1 << 7, 32, 32, 32, 32, pl, st) == 0;   /* another bit */
    bad |= jmr_check(-1, 32, 32, 32, 32, pl, st) == 0 || jmr_check((-2147483647 - 1) | JMR_BGRA8, 32, 32, 32, 32, pl, st) == 0;
    for (int f = 0; f < 16; f++) bad |= jmr_is_rgb(f) || jmr_is_rgb(f | JMR_BT709) || jmr_check(f, 32, 32, 32, 32, pl, st) == 0;
    bad |= jmr_is_rgb(20) || jmr_is_rgb(20 | JMR_FULL_RANGE);
    /* the YUV rules see the flags as a format outside their enum */
    {
        const void *yuv[3] = {mem, mem + 16, mem + 32};
        const int64_t sy[3] = {16, 8, 8};
        bad |= jmi_check(JMI_I420, 16, 2, 16, 16, yuv, sy) != 0 || jmi_check(JMI_I420 | JMR_BT709, 16, 2, 16, 16, yuv, sy) == 0 ||
               jmi_check(JMI_NV12 | JMR_FULL_RANGE, 16, 2, 16, 16, yuv, sy) == 0;
    }
    for (int fl = 0; fl < 4; fl++)
        bad |= !jmr_depth_ok(JMR_BGRA8 | fl << 8, 8) || !jmr_depth_ok(JMR_RGBA8 | fl << 8, 8) || !jmr_depth_ok(JMR_RGB10A2 | fl << 8, 10) ||
               !jmr_depth_ok(JMR_BGR10A2 | fl << 8, 10) || jmr_depth_ok(JMR_BGRA8 | fl << 8, 10) || jmr_depth_ok(JMR_RGB10A2 | fl << 8, 8) ||
               jmr_depth_ok(JMR_BGRA8 | fl << 8, 9) || jmr_depth_ok(JMR_RGBA8 | fl << 8, 9) || jmr_depth_ok(JMR_RGB10A2 | fl << 8, 9) ||
               jmr_depth_ok(JMR_BGR10A2 | fl << 8, 9);
    if (bad) { fprintf(stderr, "jmr_check / jmr_depth_ok: a rule differs\n"); s_bad++; }
}

int main(void) {
    static const int sizes[6][4] = {{32, 32, 32, 32}, {32, 32, 18, 18}, {32, 32, 30, 2}, {32, 32, 2, 30}, {32, 32, 2, 2}, {48, 32, 34, 18}};
    static const int pads[3] = {0, 4, 52};
    for (int layout = JMR_BGRA8; layout <= JMR_BGR10A2; layout++)
        for (int fl = 0; fl < 4; fl++) {
            const int format = layout | fl << 8;
            check_row(format, jmr_ten(layout) ? 10 : 8);
            for (int s = 0; s < 6; s++)
                for (int p = 0; p < 3; p++) one(format, sizes[s][0], sizes[s][1], sizes[s][2], sizes[s][3], pads[p]);
        }
    check_words();
    check_rules();
    if (s_worst > 1.0) { fprintf(stderr, "a sample is %.4f bounds from the real-valued formula\n", s_worst); s_bad++; }
    if (s_unclamped_full) { fprintf(stderr, "%ld full-range pictures without a clamped chroma sample\n", s_unclamped_full); s_bad++; }
    printf("rgb check: %ld pictures, %ld clamped samples, worst %.4f of the bound, %ld differ\n", s_pics, s_clamped, s_worst, s_bad);
    return s_bad ? 1 : 0;
}
