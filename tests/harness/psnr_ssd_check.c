/*
 * psnr_ssd_check.c — jm_psnr_from_ssd (what DeviceWriterAsync=1 prints from the device's SSDs) against
 * psnr_pl (what every other path computes from the two pictures), on random 8- and 10-bit planes:
 * the doubles must be identical, so the printed digits are.  A stand-alone program built with ASan +
 * UBSan by psnr_ssd.mk (tests/test_coded_cfg.py); psnr_pl is static, so the frame loop's source is
 * included here.
 */
#include "encoder.c"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static int check(int w, int h, int cw, int ch, int bd, int spread) {
    jm_pic a, b;
    if (jm_pic_alloc_bd(&a, w, h, bd) || jm_pic_alloc_bd(&b, w, h, bd)) return 2;
    const size_t n = (size_t)w * h * 3 / 2;
    const uint32_t maxv = (1u << bd) - 1;
    for (size_t i = 0; i < n; i++) {
        const uint32_t x = rnd() & maxv;
        uint32_t y = spread < 0 ? rnd() & maxv : x + rnd() % (uint32_t)(spread + 1);
        if (y > maxv) y = maxv;
        if (bd > 8) { a.Y[i] = (uint16_t)x; b.Y[i] = (uint16_t)y; }
        else { a.y[i] = (uint8_t)x; b.y[i] = (uint8_t)y; }
    }
    int bad = 0;
    for (int pl = 0; pl < 3; pl++) {
        const int pw = pl ? w / 2 : w, ww = pl ? cw / 2 : cw, hh = pl ? ch / 2 : ch;
        const size_t off = pl == 0 ? 0 : (size_t)w * h + (size_t)(pl - 1) * (w / 2) * (h / 2);
        uint64_t ssd = 0;
        for (int y = 0; y < hh; y++)
            for (int x = 0; x < ww; x++) {
                const size_t k = off + (size_t)y * pw + x;
                const int64_t d = bd > 8 ? (int64_t)a.Y[k] - b.Y[k] : (int64_t)a.y[k] - b.y[k];
                ssd += (uint64_t)(d * d);
            }
        const double want = psnr_pl(&a, &b, pl, ww, hh), got = jm_psnr_from_ssd(ssd, ww, hh, bd);
        printf("%dx%d crop %dx%d bd %d plane %d: ssd %llu psnr_pl %.17g from ssd %.17g\n", w, h, cw, ch, bd, pl,
               (unsigned long long)ssd, want, got);
        if (memcmp(&want, &got, sizeof(want))) bad = 1;
    }
    jm_pic_free(&a);
    jm_pic_free(&b);
    return bad;
}

int main(void) {
    int bad = 0;
    bad |= check(64, 48, 64, 48, 8, -1);
    bad |= check(48, 32, 46, 30, 8, 3);
    bad |= check(176, 144, 174, 142, 8, 1);
    bad |= check(64, 48, 64, 48, 10, -1);
    bad |= check(48, 32, 46, 30, 10, 5);
    bad |= check(32, 32, 32, 32, 9, -1);
    bad |= check(32, 32, 32, 32, 8, 0);       /* equal pictures: 99.0 */
    bad |= check(32, 32, 30, 30, 10, 0);
    if (bad) { printf("MISMATCH\n"); return 1; }
    printf("ok\n");
    return 0;
}
