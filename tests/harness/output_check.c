/*
 * output_check.c — the pulled-picture core (csrc/jmh_output.h, the text k_pull_picture and
 * k_pull_tensor of csrc/jmh_output.hip compile) on the CPU (TEST INFRASTRUCTURE).
 *
 *   output_check rules
 *       jmout_check_picture, jmout_check_tensor and the two depth rules against the argument rules of
 *       include/jmhip_output.h, one call per rule; hand-worked values of the conversion, the packers
 *       and the dequantiser.  Prints "output rules: N checks, B differ".
 *   output_check walk <cases> <out>
 *       <cases> holds records written by tests/test_output_core.py: 24 little-endian int64 words
 *         kind (0 picture, 1 tensor), format or dtype, flags, bit depth, W, H, w, h,
 *         offset[3], stride[3] (a tensor: stride_x, stride_y, 0), nbytes, 9 spare words
 *       followed by the packed W x H 4:2:0 source (samples of 1 byte at 8 bits, else 2).  For each
 *       record the destination is a malloc block of exactly nbytes bytes filled with 0xA5, the
 *       planes or channels lie at the offsets in it, the reference walk (jmout_picture /
 *       jmout_tensor) runs after the argument rules accepted the descriptor, and the block is
 *       appended to <out>.  The source sits in a malloc block of exactly its bytes too.  A byte read
 *       or written outside either block is an ASan error.  Prints "output walk: N cases".
 *
 * Exit 0: nothing differs.  Built with -fsanitize=address,undefined (tests/harness/output.mk).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../h264-jm-commentary_amd/csrc/jmh_output.h"

static long s_checks, s_bad;
#define EXPECT(cond)                                                           \
    do {                                                                       \
        s_checks++;                                                            \
        if (!(cond)) { s_bad++; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static int pic(int format, int w, int h, void *p0, void *p1, void *p2, int64_t s0, int64_t s1, int64_t s2) {
    const void *plane[3] = {p0, p1, p2};
    const int64_t stride[3] = {s0, s1, s2};
    return jmout_check_picture(format, w, h, 32, 32, plane, stride);
}
static int ten(int dtype, int flags, int w, int h, void *c0, void *c1, void *c2, int64_t sx, int64_t sy) {
    const void *chan[3] = {c0, c1, c2};
    return jmout_check_tensor(dtype, flags, w, h, 32, 32, chan, sx, sy);
}

static int rules(void) {
    static uint32_t mem[4096];
    uint8_t *b = (uint8_t *)mem;
    /* pictures: the YUV formats */
    EXPECT(pic(JMI_I420, 30, 18, b, b + 1024, b + 2048, 30, 15, 15) == 0);
    EXPECT(pic(JMI_I420, 30, 18, b + 1, b + 1025, b + 2047, 31, 16, 17) == 0);          /* any byte address and stride */
    EXPECT(pic(JMI_NV12, 30, 18, b, b + 1024, NULL, 30, 30, 0) == 0);                   /* plane[2] is not read */
    EXPECT(pic(JMI_P010, 30, 18, b, b + 1024, NULL, 60, 60, 0) == 0);
    EXPECT(pic(JMI_I420, 30, 18, b, b + 1024, NULL, 30, 15, 15) != 0);                  /* a null plane */
    EXPECT(pic(JMI_I420, 30, 18, NULL, b, b, 30, 15, 15) != 0);
    EXPECT(pic(JMI_NV12, 30, 18, b, NULL, b, 30, 30, 0) != 0);
    EXPECT(pic(4, 30, 18, b, b, b, 64, 64, 64) != 0 && pic(-1, 30, 18, b, b, b, 64, 64, 64) != 0 && pic(15, 30, 18, b, b, b, 128, 64, 64) != 0);
    EXPECT(pic(JMI_I420 | JMR_BT709, 30, 18, b, b, b, 64, 64, 64) != 0);                /* a flag on a YUV format */
    EXPECT(pic(JMI_NV12 | JMR_FULL_RANGE, 30, 18, b, b, b, 64, 64, 64) != 0);
    EXPECT(pic(JMI_I420, 29, 18, b, b, b, 64, 64, 64) != 0 && pic(JMI_I420, 30, 17, b, b, b, 64, 64, 64) != 0);
    EXPECT(pic(JMI_I420, 0, 18, b, b, b, 64, 64, 64) != 0 && pic(JMI_I420, 30, 0, b, b, b, 64, 64, 64) != 0);
    EXPECT(pic(JMI_I420, 34, 18, b, b, b, 64, 64, 64) != 0 && pic(JMI_I420, 30, 34, b, b, b, 64, 64, 64) != 0);
    EXPECT(pic(JMI_I420, 32, 32, b, b, b, 32, 16, 16) == 0);
    EXPECT(pic(JMI_I420, 30, 18, b, b, b, 29, 15, 15) != 0 && pic(JMI_I420, 30, 18, b, b, b, 30, 14, 15) != 0 && pic(JMI_I420, 30, 18, b, b, b, 30, 15, 14) != 0);
    EXPECT(pic(JMI_NV12, 30, 18, b, b, NULL, 30, 29, 0) != 0);
    EXPECT(pic(JMI_I420, 30, 18, b, b, b, -64, 64, 64) != 0 && pic(JMI_I420, 30, 18, b, b, b, 64, -64, 64) != 0);
    EXPECT(pic(JMI_I010, 30, 18, b, b, b, 60, 30, 30) == 0 && pic(JMI_I010, 30, 18, b, b, b, 59, 30, 30) != 0);
    EXPECT(pic(JMI_I010, 30, 18, b + 1, b, b, 64, 32, 32) != 0 && pic(JMI_I010, 30, 18, b, b, b + 1, 64, 32, 32) != 0);   /* 16-bit planes: 2 */
    EXPECT(pic(JMI_I010, 30, 18, b, b, b, 61, 32, 32) != 0 && pic(JMI_P010, 30, 18, b, b + 3, NULL, 64, 64, 0) != 0);
    /* pictures: RGB */
    for (int f = JMR_BGRA8; f <= JMR_BGR10A2; f++) {
        EXPECT(pic(f, 30, 18, b, NULL, NULL, 120, 0, 0) == 0);                          /* plane[1], plane[2] are not read */
        EXPECT(pic(f | JMR_BT709 | JMR_FULL_RANGE, 30, 18, b + 4, NULL, NULL, 124, -1, -1) == 0);
        EXPECT(pic(f, 30, 18, NULL, b, b, 120, 0, 0) != 0);
        EXPECT(pic(f, 30, 18, b, b, b, 119, 0, 0) != 0 && pic(f, 30, 18, b, b, b, 116, 0, 0) != 0 && pic(f, 30, 18, b, b, b, -128, 0, 0) != 0);
        EXPECT(pic(f, 30, 18, b + 2, b, b, 120, 0, 0) != 0 && pic(f, 30, 18, b, b, b, 122, 0, 0) != 0);      /* RGB: 4 */
        EXPECT(pic(f | 1 << 10, 30, 18, b, b, b, 120, 0, 0) != 0 && pic(f | 1 << 7, 30, 18, b, b, b, 120, 0, 0) != 0);
        EXPECT(pic(f, 29, 18, b, b, b, 128, 0, 0) != 0 && pic(f, 34, 18, b, b, b, 256, 0, 0) != 0 && pic(f, 30, 1, b, b, b, 128, 0, 0) != 0);
    }
    EXPECT(pic(20, 30, 18, b, b, b, 128, 0, 0) != 0);
    /* tensors */
    for (int dt = 0; dt < JMT_NDTYPES; dt++) {
        const int es = jmt_es(dt);
        EXPECT(ten(dt, 0, 30, 18, b, b + 2048, b + 4096, es, 30 * es) == 0);
        EXPECT(ten(dt, JMR_BT709 | JMR_FULL_RANGE, 30, 18, b + es, b + 2 * es, b, 4 * es, 29 * 4 * es + es) == 0);
        EXPECT(ten(dt, 0, 30, 18, b, b, b, es, 30 * es) == 0);
        EXPECT(ten(dt, 0, 30, 18, NULL, b, b, es, 64 * es) != 0 && ten(dt, 0, 30, 18, b, NULL, b, es, 64 * es) != 0 && ten(dt, 0, 30, 18, b, b, NULL, es, 64 * es) != 0);
        EXPECT(ten(dt, 1, 30, 18, b, b, b, es, 64 * es) != 0 && ten(dt, 16, 30, 18, b, b, b, es, 64 * es) != 0 && ten(dt, 1 << 10, 30, 18, b, b, b, es, 64 * es) != 0);
        EXPECT(ten(dt, 0, 29, 18, b, b, b, es, 64 * es) != 0 && ten(dt, 0, 30, 17, b, b, b, es, 64 * es) != 0 && ten(dt, 0, 0, 18, b, b, b, es, 64 * es) != 0);
        EXPECT(ten(dt, 0, 34, 18, b, b, b, es, 64 * es) != 0 && ten(dt, 0, 30, 34, b, b, b, es, 64 * es) != 0);
        EXPECT(ten(dt, 0, 30, 18, b, b, b, 0, 64 * es) != 0 && ten(dt, 0, 30, 18, b, b, b, -es, 64 * es) != 0 && ten(dt, 0, 30, 18, b, b, b, es, -64 * es) != 0);
        EXPECT(ten(dt, 0, 30, 18, b, b, b, es, 29 * es) != 0 && ten(dt, 0, 30, 18, b, b, b, 3 * es, 29 * 3 * es) != 0);
        if (es > 1) {
            EXPECT(ten(dt, 0, 30, 18, b + 1, b, b, es, 64 * es) != 0 && ten(dt, 0, 30, 18, b, b, b + 1, es, 64 * es) != 0);
            EXPECT(ten(dt, 0, 30, 18, b, b, b, es + 1, 64 * es) != 0 && ten(dt, 0, 30, 18, b, b, b, es, 64 * es + 1) != 0);
        }
        if (es > 2) EXPECT(ten(dt, 0, 30, 18, b + 2, b, b, es, 64 * es) != 0 && ten(dt, 0, 30, 18, b, b, b, es, 64 * es + 2) != 0);
    }
    EXPECT(ten(5, 0, 30, 18, b, b, b, 4, 256) != 0 && ten(-1, 0, 30, 18, b, b, b, 4, 256) != 0);
    /* the depth rules */
    EXPECT(jmout_picture_depth_ok(JMI_I420, 8) && jmout_picture_depth_ok(JMI_NV12, 8) && !jmout_picture_depth_ok(JMI_I420, 10) && !jmout_picture_depth_ok(JMI_NV12, 9));
    EXPECT(jmout_picture_depth_ok(JMI_I010, 9) && jmout_picture_depth_ok(JMI_I010, 10) && !jmout_picture_depth_ok(JMI_I010, 8));
    EXPECT(jmout_picture_depth_ok(JMI_P010, 10) && !jmout_picture_depth_ok(JMI_P010, 9) && !jmout_picture_depth_ok(JMI_P010, 8));
    EXPECT(jmout_picture_depth_ok(JMR_BGRA8 | JMR_BT709, 8) && jmout_picture_depth_ok(JMR_RGBA8, 8) && !jmout_picture_depth_ok(JMR_BGRA8, 10) && !jmout_picture_depth_ok(JMR_RGBA8, 9));
    EXPECT(jmout_picture_depth_ok(JMR_RGB10A2, 10) && jmout_picture_depth_ok(JMR_BGR10A2 | JMR_FULL_RANGE, 10) && !jmout_picture_depth_ok(JMR_RGB10A2, 8) && !jmout_picture_depth_ok(JMR_BGR10A2, 9));
    EXPECT(jmout_tensor_depth_ok(JMT_U8, 8) && !jmout_tensor_depth_ok(JMT_U8, 10) && jmout_tensor_depth_ok(JMT_U16, 10) && !jmout_tensor_depth_ok(JMT_U16, 8));
    for (int dt = 0; dt < JMT_NDTYPES; dt++) EXPECT(!jmout_tensor_depth_ok(dt, 9));
    for (int dt = JMT_F16; dt < JMT_NDTYPES; dt++) EXPECT(jmout_tensor_depth_ok(dt, 8) && jmout_tensor_depth_ok(dt, 10));
    /* hand-worked values.  BT.601 limited, 8 bits: black, white, and V at its top over mid grey:
     * (19077 * 110 + 26149 * 127 + 8192) >> 14 = 331 clamps to 255; G = (2098470 - 13320 * 127 + 8192) >> 14 = 25 */
    jmout_coef k;
    int32_t rgb[3];
    jmout_coefficients(0, 8, &k);
    EXPECT(k.iy == 19077 && k.irv == 26149 && k.igu == -6419 && k.igv == -13320 && k.ibu == 33050 && k.yo == 16 && k.co == 128 && k.maxv == 255);
    jmout_rgb(&k, 16, 128, 128, rgb);
    EXPECT(rgb[0] == 0 && rgb[1] == 0 && rgb[2] == 0);
    jmout_rgb(&k, 235, 128, 128, rgb);
    EXPECT(rgb[0] == 255 && rgb[1] == 255 && rgb[2] == 255);
    jmout_rgb(&k, 126, 128, 255, rgb);
    EXPECT(rgb[0] == 255 && rgb[1] == 25 && rgb[2] == 128);
    jmout_rgb(&k, 0, 0, 0, rgb);                                                        /* below black: G = (-305232 + 821632 + 1704960 + 8192) >> 14 = 136 */
    EXPECT(rgb[0] == 0 && rgb[1] == 136 && rgb[2] == 0);
    jmout_coefficients(JMR_BT709 | JMR_FULL_RANGE, 10, &k);
    EXPECT(k.iy == 16384 && k.irv == 25802 && k.igu == -3069 && k.igv == -7670 && k.ibu == 30402 && k.yo == 0 && k.co == 512 && k.maxv == 1023);
    jmout_rgb(&k, 700, 512, 512, rgb);
    EXPECT(rgb[0] == 700 && rgb[1] == 700 && rgb[2] == 700);
    const int32_t c123[3] = {1, 2, 3};
    EXPECT(jmout_pack(JMR_BGRA8, c123) == 0xff010203u && jmout_pack(JMR_RGBA8, c123) == 0xff030201u);
    EXPECT(jmout_pack(JMR_RGB10A2, c123) == (0xc0000000u | 3u << 20 | 2u << 10 | 1u) && jmout_pack(JMR_BGR10A2, c123) == (0xc0000000u | 1u << 20 | 2u << 10 | 3u));
    EXPECT(jmout_yuv_value(JMI_P010, 1023) == 0xffc0u && jmout_yuv_value(JMI_I010, 1023) == 1023 && jmout_yuv_value(JMI_NV12, 255) == 255);
    /* 1/3 = 85/255 = 341/1023: float32 0x3eaaaaab, float16 0x3555, bfloat16 0x3eab; 1 and 0 */
    EXPECT(jmout_dequant(JMT_F32, 85, 255) == 0x3eaaaaabu && jmout_dequant(JMT_F16, 341, 1023) == 0x3555u && jmout_dequant(JMT_BF16, 85, 255) == 0x3eabu);
    EXPECT(jmout_dequant(JMT_F32, 255, 255) == 0x3f800000u && jmout_dequant(JMT_F16, 1023, 1023) == 0x3c00u && jmout_dequant(JMT_BF16, 1023, 1023) == 0x3f80u);
    EXPECT(jmout_dequant(JMT_F32, 0, 255) == 0 && jmout_dequant(JMT_F16, 0, 255) == 0 && jmout_dequant(JMT_BF16, 0, 1023) == 0);
    EXPECT(jmout_dequant(JMT_U8, 200, 255) == 200 && jmout_dequant(JMT_U16, 1000, 1023) == 1000);
    EXPECT(jmout_dequant(JMT_F16, 1, 1023) == 0x1401u);                                 /* the smallest level: 2^-10 (1 + 1/1023), a normal half */
    printf("output rules: %ld checks, %ld differ\n", s_checks, s_bad);
    return s_bad != 0;
}

static int walk(const char *cases, const char *out) {
    FILE *in = fopen(cases, "rb"), *of = fopen(out, "wb");
    if (!in || !of) { fprintf(stderr, "cannot open %s / %s\n", cases, out); return 2; }
    long n = 0;
    int64_t r[24];
    while (fread(r, sizeof(r), 1, in) == 1) {
        const int kind = (int)r[0], fmt = (int)r[1], flags = (int)r[2], bd = (int)r[3], W = (int)r[4], H = (int)r[5], w = (int)r[6], h = (int)r[7];
        const size_t nbytes = (size_t)r[14], sbytes = (size_t)W * H * 3 / 2 * (bd > 8 ? 2 : 1);
        uint8_t *src = (uint8_t *)malloc(sbytes), *dst = (uint8_t *)malloc(nbytes);
        if (!src || !dst || fread(src, 1, sbytes, in) != sbytes) { fprintf(stderr, "case %ld: short record\n", n); return 2; }
        memset(dst, 0xA5, nbytes);
        uint8_t *p[3];
        const void *cp[3];
        for (int i = 0; i < 3; i++) { p[i] = r[8 + i] >= 0 ? dst + r[8 + i] : NULL; cp[i] = p[i]; }
        if (kind == 0) {
            const int64_t stride[3] = {r[11], r[12], r[13]};
            if (jmout_check_picture(fmt, w, h, W, H, cp, stride) || !jmout_picture_depth_ok(fmt, bd)) { fprintf(stderr, "case %ld: refused\n", n); return 1; }
            jmout_picture(fmt, bd, src, W, H, w, h, p, stride);
        } else {
            if (jmout_check_tensor(fmt, flags, w, h, W, H, cp, r[11], r[12]) || !jmout_tensor_depth_ok(fmt, bd)) { fprintf(stderr, "case %ld: refused\n", n); return 1; }
            jmout_tensor(fmt, flags, bd, src, W, H, w, h, p, r[11], r[12]);
        }
        if (fwrite(dst, 1, nbytes, of) != nbytes) return 2;
        free(src);
        free(dst);
        n++;
    }
    fclose(in);
    if (fclose(of)) return 2;
    printf("output walk: %ld cases\n", n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "rules")) return rules();
    if (argc == 4 && !strcmp(argv[1], "walk")) return walk(argv[2], argv[3]);
    fprintf(stderr, "usage: output_check rules | output_check walk <cases> <out>\n");
    return 2;
}
