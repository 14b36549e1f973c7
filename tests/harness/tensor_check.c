/*
 * tensor_check.c — the device-tensor core (csrc/jmh_tensor.h, the text k_ingest_tensor of
 * csrc/jmh_tensor.hip compiles) on the CPU (TEST INFRASTRUCTURE).  Every channel sits in a malloc
 * block of exactly its bytes (CHW: (h - 1) * stride_y + w * es per channel; interleaved: one block
 * that ends with the last pixel's third channel; GBR-planar: one block of the three planes that ends
 * with R's last element), so an offset outside it is an ASan error.
 *
 * (a) Pictures.  Every valid (dtype, context bit depth) pair, as CHW, HWC with 3 and with 4 channels
 * and GBR-planar, with both matrices and both ranges, is converted through the core (jmt_convert) and
 * compared with a plain restatement: every element quantised by integer arithmetic on its decoded
 * mantissa and exponent (no floating point), the formulas of include/jmhip_rgb.h at the source size,
 * then jm_pad_picture (host/yuv.c).  Coded 32x32 with sources 32x32, 18x18, 30x2, 2x30, 2x2; coded 48x32
 * with 34x18.  Row strides: tight, +es, +52 es.  Every float picture holds a NaN, a negative value, a
 * value above 1 and the exact tie 1/2.
 * (b) The quantiser, jmt_quant against the same integer restatement: all 65,536 patterns of F16 and
 * of BF16 at both depths; for F32 at both depths, for every k in [0, M] the floats nearest k / M and
 * (k + 1/2) / M with two neighbours on each side, +-0, denormals, +-inf, NaNs, values just outside
 * [0, 1], and 2^20 random bit patterns.  Hand-worked values.
 * (c) jmt_check and jmt_depth_ok against the argument rules of include/jmhip_tensor.h.
 *
 * Exit 0: everything equal.  Built with -fsanitize=address,undefined (tests/harness/tensor.mk).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../h264-jm-commentary_amd/csrc/jmh_tensor.h"
#include "jmhost.h"

static uint64_t rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(void) {
    rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
    return (uint32_t)((rng * 0x2545F4914F6CDD1DULL) >> 32);
}

static long s_pics, s_quant, s_bad;

/* floor(mant 2^exp M + 1/2) clamped, in integers: the restatement of the float quantiser.  special: 0 a
 * finite value, 1 +inf, 2 -inf or NaN */
static int32_t quant_int(int neg, uint64_t mant, int exp, int special, int32_t M) {
    if (special == 1) return M;
    if (special == 2 || neg || mant == 0) return 0;
    if (exp >= 0 || (exp > -64 && (mant >> -exp) >= 1)) return M;        /* x >= 1 */
    const int s = -exp;
    if (s > 44) return 0;                                                 /* x M < 2^24 2^10 2^-45: below 1/2 */
    return (int32_t)((2 * mant * (uint64_t)M + ((uint64_t)1 << s)) >> (s + 1));
}
/* the raw bits of an element of a float dtype, decoded by the format's own rules (not through float32) */
static int32_t quant_ref(int dtype, uint32_t raw, int32_t M) {
    if (dtype == JMT_U8) return (int32_t)raw;
    if (dtype == JMT_U16) return raw > (uint32_t)M ? M : (int32_t)raw;
    if (dtype == JMT_F16) {
        const int neg = raw >> 15 & 1, e = raw >> 10 & 31;
        const uint64_t m = raw & 0x3ff;
        if (e == 31) return quant_int(neg, 0, 0, m ? 2 : neg ? 2 : 1, M);
        return e ? quant_int(neg, m | 0x400, e - 25, 0, M) : quant_int(neg, m, -24, 0, M);
    }
    if (dtype == JMT_BF16) raw <<= 16;
    const int neg = raw >> 31, e = raw >> 23 & 255;
    const uint64_t m = raw & 0x7fffff;
    if (e == 255) return quant_int(neg, 0, 0, m ? 2 : neg ? 2 : 1, M);
    return e ? quant_int(neg, m | 0x800000, e - 150, 0, M) : quant_int(neg, m, -149, 0, M);
}

static uint32_t f32_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
/* a float32 as an element of a float dtype, by truncation (content only: any bits will do) */
static uint32_t elem_of(int dtype, float f) {
    const uint32_t b = f32_bits(f);
    if (dtype == JMT_F32) return b;
    if (dtype == JMT_BF16) return b >> 16;
    const uint32_t e = b >> 23 & 255;
    if (e == 255) return (b >> 16 & 0x8000) | 0x7c00 | ((b & 0x7fffff) ? 0x200 : 0);
    if (e < 113) return b >> 16 & 0x8000;                   /* below 2^-14: a zero */
    if (e > 142) return (b >> 16 & 0x8000) | 0x7bff;
    return (b >> 16 & 0x8000) | (e - 112) << 10 | (b >> 13 & 0x3ff);
}
static uint32_t random_elem(int dtype) {
    if (dtype == JMT_U8) return rnd() & 255;
    if (dtype == JMT_U16) return (rnd() & 7) ? rnd() & 1023 : rnd() & 65535;   /* some above M */
    return elem_of(dtype, (float)(rnd() % 5121) / 4096.0f - 0.125f);            /* [-0.125, 1.125] */
}
static void put(uint8_t *p, int es, uint32_t v) { for (int i = 0; i < es; i++) p[i] = (uint8_t)(v >> 8 * i); }

enum { L_CHW, L_HWC3, L_HWC4, L_GBR, L_COUNT };

/* one picture: dtype in a bd-bit context, layout, flags, coded W x H, source w x h, pad elements per row */
static void one(int dtype, int bd, int layout, int flags, int W, int H, int w, int h, int pad) {
    const int es = jmt_es(dtype), oes = bd > 8 ? 2 : 1;
    const int32_t M = (1 << bd) - 1;
    uint32_t *px[3];   /* the raw elements of R, G, B */
    for (int c = 0; c < 3; c++) {
        px[c] = malloc((size_t)w * h * sizeof(uint32_t));
        for (int i = 0; i < w * h; i++) px[c][i] = random_elem(dtype);
    }
    int bad = 0;
    if (jmt_is_float(dtype)) {   /* the condition: NaN, negative, above 1, the tie 1/2, in the one block a 2x2 source has */
        px[0][0] = elem_of(dtype, NAN); px[1][0] = elem_of(dtype, -0.25f); px[2][0] = elem_of(dtype, 1.5f); px[0][1] = elem_of(dtype, 0.5f);
        px[1][1] = elem_of(dtype, -0.0f); px[2][1] = elem_of(dtype, INFINITY); px[0][w] = elem_of(dtype, -INFINITY);
        bad |= quant_ref(dtype, px[0][0], M) != 0 || quant_ref(dtype, px[1][0], M) != 0 || quant_ref(dtype, px[2][0], M) != M ||
               quant_ref(dtype, px[0][1], M) != (M + 1) / 2 || quant_ref(dtype, px[2][1], M) != M || quant_ref(dtype, px[0][w], M) != 0;
    }
    /* the channels, exact size */
    const int planar = layout == L_CHW || layout == L_GBR, C = layout == L_HWC4 ? 4 : 3;
    const int64_t sx = planar ? es : (int64_t)C * es, sy = (int64_t)w * sx + (int64_t)pad * es;
    uint8_t *block[3] = {NULL, NULL, NULL};
    const uint8_t *chan[3];
    if (layout == L_CHW) {
        const size_t bytes = (size_t)((h - 1) * sy + (int64_t)w * es);
        for (int c = 0; c < 3; c++) { block[c] = malloc(bytes); memset(block[c], 0xA5, bytes); chan[c] = block[c]; }
    } else if (layout == L_GBR) {   /* one block of the planes G, B, R (a gbrp file's frame): the addresses permuted */
        const size_t plane = (size_t)(h * sy), bytes = 2 * plane + (size_t)((h - 1) * sy + (int64_t)w * es);
        block[0] = malloc(bytes);
        memset(block[0], 0xA5, bytes);
        chan[0] = block[0] + 2 * plane; chan[1] = block[0]; chan[2] = block[0] + plane;
    } else {
        const size_t bytes = (size_t)((h - 1) * sy + ((int64_t)(w - 1) * C + 3) * es);
        block[0] = malloc(bytes);
        memset(block[0], 0xA5, bytes);
        for (int c = 0; c < 3; c++) chan[c] = block[0] + c * es;
    }
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) put((uint8_t *)chan[c] + jmt_src_off(x, y, sx, sy), es, px[c][y * w + x]);
    const void *cv[3] = {chan[0], chan[1], chan[2]};
    if (jmt_check(dtype, flags, w, h, W, H, cv, sx, sy) || !jmt_depth_ok(dtype, bd)) bad = 1;
    /* through the core */
    uint8_t *got = malloc((size_t)W * H * 3 / 2 * oes);
    jmt_convert(dtype, flags, bd, chan, sx, sy, w, h, W, H, got);
    /* the restatement */
    jmr_coef k;
    jmr_coefficients(flags, bd, &k);
    jm_pic ref;
    if (jm_pic_alloc_bd(&ref, W, H, bd)) { fprintf(stderr, "out of memory\n"); exit(2); }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int32_t r = quant_ref(dtype, px[0][y * w + x], M), g = quant_ref(dtype, px[1][y * w + x], M), b = quant_ref(dtype, px[2][y * w + x], M);
            int32_t v = k.yo + ((k.c[0] * r + k.c[1] * g + k.c[2] * b + 8192) >> 14);
            if (v < 0 || v > k.maxv) bad = 1;       /* Y cannot leave its range */
            if (bd > 8) ref.Y[(size_t)y * W + x] = (uint16_t)v; else ref.y[(size_t)y * W + x] = (uint8_t)v;
        }
    for (int y = 0; y < h / 2; y++)
        for (int x = 0; x < w / 2; x++) {
            int32_t s[3] = {0, 0, 0};
            for (int i = 0; i < 4; i++)
                for (int c = 0; c < 3; c++) s[c] += quant_ref(dtype, px[c][(2 * y + (i >> 1)) * w + 2 * x + (i & 1)], M);
            for (int which = 0; which < 2; which++) {
                const int32_t *q = k.c + 3 + 3 * which;
                const int32_t raw = k.co + ((q[0] * s[0] + q[1] * s[1] + q[2] * s[2] + 32768) >> 16);
                const int32_t v = raw < 0 ? 0 : raw > k.maxv ? k.maxv : raw;
                if (bd > 8) (which ? ref.V : ref.U)[(size_t)y * (W / 2) + x] = (uint16_t)v;
                else (which ? ref.v : ref.u)[(size_t)y * (W / 2) + x] = (uint8_t)v;
            }
        }
    jm_pad_picture(&ref, w, h);
    if (memcmp(got, bd > 8 ? (const void *)ref.Y : (const void *)ref.y, (size_t)W * H * 3 / 2 * oes)) bad = 1;
    if (bad) {
        fprintf(stderr, "dtype %d depth %d layout %d flags %#x coded %dx%d source %dx%d pad %d: differs\n", dtype, bd, layout, flags, W, H, w, h, pad);
        s_bad++;
    }
    s_pics++;
    jm_pic_free(&ref);
    free(got);
    for (int c = 0; c < 3; c++) { free(block[c]); free(px[c]); }
}

/* (b) */
static void quant_one(int dtype, uint32_t raw, int32_t M) {
    const int32_t a = jmt_quant(dtype, raw, M), b = quant_ref(dtype, raw, M);
    if (a != b || a < 0 || a > M) {
        if (s_bad < 20) fprintf(stderr, "dtype %d M %d bits %#x: jmt_quant %d, integer arithmetic %d\n", dtype, M, raw, a, b);
        s_bad++;
    }
    s_quant++;
}
static void check_quantiser(void) {
    static const uint32_t special[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x80000001u, 0x807fffffu, 0x7f800000u,
                                       0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x7fffffffu, 0x3f800000u, 0x3f800001u,
                                       0x3f7fffffu, 0x3f7ffffeu, 0xbf800000u, 0x3f000000u, 0x3effffffu, 0x3f000001u, 0x40000000u, 0x7f7fffffu,
                                       0xff7fffffu, 0x33800000u, 0x34000000u};
    for (int bd = 8; bd <= 10; bd += 2) {
        const int32_t M = (1 << bd) - 1;
        for (uint32_t v = 0; v < 65536; v++) { quant_one(JMT_F16, v, M); quant_one(JMT_BF16, v, M); }
        for (int k = 0; k <= M; k++)
            for (int half = 0; half < 2; half++) {
                const uint32_t c = f32_bits((float)((k + 0.5 * half) / M));
                for (int d = -2; d <= 2; d++)
                    if ((int64_t)c + d >= 0) quant_one(JMT_F32, (uint32_t)((int64_t)c + d), M);
            }
        for (size_t i = 0; i < sizeof(special) / sizeof(special[0]); i++) quant_one(JMT_F32, special[i], M);
        for (int i = 0; i < 1 << 20; i++) quant_one(JMT_F32, rnd(), M);
        for (uint32_t v = 0; v < 65536; v += 13) quant_one(JMT_U16, v, 1023);
    }
    for (uint32_t v = 0; v < 256; v++) quant_one(JMT_U8, v, 255);
    /* by hand: 0.5f at 8 bits is 127.5, a tie, and rounds up; at 10 bits 511.5 */
    int bad = jmt_quant(JMT_F32, f32_bits(0.5f), 255) != 128 || jmt_quant(JMT_F32, f32_bits(0.5f), 1023) != 512;
    bad |= jmt_quant(JMT_F16, 0x3800, 255) != 128 || jmt_quant(JMT_BF16, 0x3f00, 255) != 128;                    /* 0.5 */
    bad |= jmt_quant(JMT_F16, 0x3c00, 1023) != 1023 || jmt_quant(JMT_F16, 0x7c00, 255) != 255 || jmt_quant(JMT_F16, 0xfc00, 255) != 0 ||
           jmt_quant(JMT_F16, 0x7e00, 255) != 0 || jmt_quant(JMT_F16, 0x8000, 255) != 0 || jmt_quant(JMT_F16, 0x0001, 1023) != 0;
    bad |= jmt_widen(JMT_F16, 0x0001) != 0x33800000u || jmt_widen(JMT_F16, 0x03ff) != 0x387fc000u || jmt_widen(JMT_F16, 0x0400) != 0x38800000u ||
           jmt_widen(JMT_F16, 0xbc00) != 0xbf800000u || jmt_widen(JMT_BF16, 0x3f80) != 0x3f800000u;
    bad |= jmt_quant(JMT_U16, 1024, 1023) != 1023 || jmt_quant(JMT_U16, 1022, 1023) != 1022 || jmt_quant(JMT_U8, 255, 255) != 255;
    /* pure blue, full range, BT.601, 8 bits: Y 29, U clamped to 255, V 107; white and black, limited, 10 bits, BT.709: 940 and 64 */
    jmr_coef k;
    jmr_coefficients(JMR_FULL_RANGE, 8, &k);
    const int32_t one = jmt_quant(JMT_F32, f32_bits(1.0f), 255);
    bad |= jmr_luma(&k, 0, 0, one) != 29 || jmr_chroma(&k, 0, 0, 0, 4 * one) != 255 || jmr_chroma(&k, 1, 0, 0, 4 * one) != 107;
    jmr_coefficients(JMR_BT709, 10, &k);
    const int32_t top = jmt_quant(JMT_F32, f32_bits(1.0f), 1023);
    bad |= jmr_luma(&k, top, top, top) != 940 || jmr_luma(&k, 0, 0, 0) != 64 || jmr_chroma(&k, 0, 4 * top, 4 * top, 4 * top) != 512;
    if (bad) { fprintf(stderr, "jmt_quant / jmt_widen: a hand-worked value differs\n"); s_bad++; }
}

/* (c) */
static void check_rules(void) {
    _Alignas(16) static uint8_t mem[256];
    const void *ok[3] = {mem, mem + 64, mem + 128}, *same[3] = {mem, mem, mem}, *odd1[3] = {mem, mem + 65, mem + 128},
               *odd2[3] = {mem + 2, mem + 64, mem + 128}, *nul[3] = {mem, NULL, mem + 128};
    int bad = 0;
    for (int dt = 0; dt < JMT_NDTYPES; dt++) {
        const int es = jmt_es(dt);
        for (int fl = 0; fl < 4; fl++) bad |= jmt_check(dt, fl << 8, 32, 32, 32, 32, ok, es, 32 * es) != 0;          /* tight planar */
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, same, es, 32 * es) != 0;                                             /* one address three times */
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, ok, 3 * es, 96 * es) != 0 || jmt_check(dt, 0, 32, 32, 32, 32, ok, 4 * es, 128 * es + es) != 0;
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, ok, 4 * es, 31 * 4 * es + es) != 0;                                  /* the least row stride */
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, ok, 4 * es, 31 * 4 * es) == 0;                                       /* one element less */
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, ok, es, 31 * es) == 0;
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, ok, 0, 32 * es) == 0 || jmt_check(dt, 0, 32, 32, 32, 32, ok, -es, 32 * es) == 0;   /* stride_x < es */
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, ok, es, -32 * es) == 0;                                              /* a negative row stride */
        bad |= jmt_check(dt, 0, 32, 32, 32, 32, nul, es, 32 * es) == 0;                                              /* a null channel */
        bad |= jmt_check(dt, 1, 32, 32, 32, 32, ok, es, 32 * es) == 0 || jmt_check(dt, 1 << 10, 32, 32, 32, 32, ok, es, 32 * es) == 0 ||
               jmt_check(dt, JMR_BGRA8, 32, 32, 32, 32, ok, es, 32 * es) == 0 || jmt_check(dt, -1, 32, 32, 32, 32, ok, es, 32 * es) == 0;   /* another flag bit */
        bad |= jmt_check(dt, 0, 31, 32, 32, 32, ok, es, 32 * es) == 0 || jmt_check(dt, 0, 32, 31, 32, 32, ok, es, 32 * es) == 0;   /* odd */
        bad |= jmt_check(dt, 0, 0, 32, 32, 32, ok, es, 32 * es) == 0 || jmt_check(dt, 0, 32, 0, 32, 32, ok, es, 32 * es) == 0;
        bad |= jmt_check(dt, 0, 34, 32, 32, 32, ok, es, 64 * es) == 0 || jmt_check(dt, 0, 32, 34, 32, 32, ok, es, 32 * es) == 0;   /* beyond the coded size */
        if (es > 1) {
            bad |= jmt_check(dt, 0, 32, 32, 32, 32, odd1, es, 32 * es) == 0;                                         /* an address + 1 */
            bad |= jmt_check(dt, 0, 32, 32, 32, 32, ok, es + 1, 64 * es) == 0 || jmt_check(dt, 0, 32, 32, 32, 32, ok, es, 32 * es + 1) == 0;
        } else bad |= jmt_check(dt, 0, 32, 32, 32, 32, odd1, es, 32 * es) != 0;
        if (es > 2) bad |= jmt_check(dt, 0, 32, 32, 32, 32, odd2, es, 32 * es) == 0;                                 /* an address + 2 */
        else bad |= jmt_check(dt, 0, 32, 32, 32, 32, odd2, es, 32 * es) != 0;
        bad |= jmt_depth_ok(dt, 9) || jmt_depth_ok(dt, 12);                                                          /* a 9-bit context takes none */
    }
    bad |= jmt_check(-1, 0, 32, 32, 32, 32, ok, 1, 32) == 0 || jmt_check(JMT_NDTYPES, 0, 32, 32, 32, 32, ok, 1, 32) == 0;
    bad |= !jmt_depth_ok(JMT_U8, 8) || jmt_depth_ok(JMT_U8, 10) || jmt_depth_ok(JMT_U16, 8) || !jmt_depth_ok(JMT_U16, 10);
    for (int dt = JMT_F16; dt <= JMT_F32; dt++) bad |= !jmt_depth_ok(dt, 8) || !jmt_depth_ok(dt, 10);
    bad |= jmt_es(JMT_U8) != 1 || jmt_es(JMT_U16) != 2 || jmt_es(JMT_F16) != 2 || jmt_es(JMT_BF16) != 2 || jmt_es(JMT_F32) != 4;
    if (bad) { fprintf(stderr, "jmt_check / jmt_depth_ok: a rule differs\n"); s_bad++; }
}

int main(void) {
    static const int sizes[6][4] = {{32, 32, 32, 32}, {32, 32, 18, 18}, {32, 32, 30, 2}, {32, 32, 2, 30}, {32, 32, 2, 2}, {48, 32, 34, 18}};
    static const int pads[3] = {0, 1, 52};
    static const int pairs[8][2] = {{JMT_U8, 8}, {JMT_F16, 8}, {JMT_BF16, 8}, {JMT_F32, 8}, {JMT_U16, 10}, {JMT_F16, 10}, {JMT_BF16, 10}, {JMT_F32, 10}};
    for (int p = 0; p < 8; p++)
        for (int layout = 0; layout < L_COUNT; layout++)
            for (int fl = 0; fl < 4; fl++)
                for (int s = 0; s < 6; s++)
                    for (int q = 0; q < 3; q++) one(pairs[p][0], pairs[p][1], layout, fl << 8, sizes[s][0], sizes[s][1], sizes[s][2], sizes[s][3], pads[q]);
    check_quantiser();
    check_rules();
    printf("tensor check: %ld pictures, %ld quantiser values, %ld differ\n", s_pics, s_quant, s_bad);
    return s_bad ? 1 : 0;
}
