/*
 * nal_core_check.c — the device NAL stage's shared core (csrc/jmh_nal.h, the text the kernels of
 * csrc/jmh_nal.hip compile) against the product's serial packaging: host/bitstream.c › jm_write_nal
 * and the cabac_zero_words loop of host/encoder.c › encode_picture_slices.  A stand-alone program,
 * built with -fsanitize=address,undefined (nal_core.mk), driven by tests/test_nal_core.py.
 *
 * The core's passes run serially as the kernels run them: plan (chunks per unit), count (a record
 * per chunk from its tiles' ballots, carry 0 assumed), scan (every chunk's carry from the chunks
 * before it in the unit, the lead's escapes in closed form, offsets, zero words), write (the same
 * predicate under the chunk's carry).  Bytes, unit offsets and sizes must equal the reference.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jmhost.h"
#include "../../h264-jm-commentary_amd/csrc/jmh_nal.h"

typedef struct unit { int ref_idc, type; uint8_t *head; int hn; uint8_t *pay; long pn; } unit_t;

static long census_tile, census_chunk, census_junction, census_zero_chunk, n_escapes;
static long n_units, n_aus, n_differ, n_zero_cases;

static uint8_t unit_byte(const unit_t *u, long i) { return i < u->hn ? u->head[i] : u->pay[i - u->hn]; }

/* a tile's ballots as the lanes would cast them */
static void tile_ballots(const unit_t *u, long pos, int n, uint64_t *nz, uint64_t *le3) {
    *nz = 0; *le3 = 0;
    for (int lane = 0; lane < n; lane++) {
        const uint8_t v = unit_byte(u, pos + lane);
        if (v) *nz |= 1ull << lane;
        if (v <= 3) *le3 |= 1ull << lane;
    }
}
static uint64_t tile_escapes(uint64_t nz, uint64_t le3, int32_t carry) {
    uint64_t esc = 0;
    for (int lane = 0; lane < 64; lane++)
        if (jmn_escape((uint32_t)((le3 >> lane) & 1), jmn_lane_L(nz, lane, carry))) esc |= 1ull << lane;
    return esc;
}

/* the access unit through the core; returns its bytes */
static long core_wrap(const unit_t *us, int n, long bins, int bd, long nmb, uint8_t *out, long *uoff, long *usz) {
    /* plan */
    int *cs = (int *)malloc((n + 1) * sizeof(int));
    long nch = 0;
    for (int u = 0; u < n; u++) { cs[u] = (int)nch; nch += jmn_unit_chunks(us[u].hn + us[u].pn); }
    cs[n] = (int)nch;
    jmn_chunk *ch = (jmn_chunk *)calloc(nch, sizeof(jmn_chunk));
    /* count */
    for (int u = 0; u < n; u++)
        for (int c = cs[u]; c < cs[u + 1]; c++) {
            const long start = (long)(c - cs[u]) * JMN_CHUNK, left = us[u].hn + us[u].pn - start;
            const int len = (int)(left < JMN_CHUNK ? left : JMN_CHUNK);
            jmn_count s;
            jmn_count_begin(&s);
            for (int p = 0; p < len; p += JMN_TILE) {
                const int tn = len - p < JMN_TILE ? len - p : JMN_TILE;
                uint64_t nz, le3;
                tile_ballots(&us[u], start + p, tn, &nz, &le3);
                jmn_count_tile(&s, nz, le3, tile_escapes(nz, le3, s.carry), tn);
            }
            jmn_count_end(&s, &ch[c]);
        }
    /* scan */
    for (int u = 0; u < n; u++)
        for (int c = cs[u]; c < cs[u + 1]; c++) {
            int32_t carry = 0;
            for (int j = c - 1; j >= cs[u]; j--) {
                if (ch[j].lead != ch[j].n) { carry += ch[j].trail; break; }
                carry += ch[j].n;
            }
            /* the carry handed on chunk by chunk gives the same */
            if (c > cs[u] && carry != jmn_chunk_carry(&ch[c - 1], ch[c - 1].carry)) { printf("carry mismatch\n"); n_differ++; }
            ch[c].unit = u; ch[c].first = c == cs[u]; ch[c].carry = carry;
            ch[c].outn = ch[c].n + ch[c].cnt + jmn_lead_escapes(carry, ch[c].lead, ch[c].first_le3);
        }
    long o = 0;
    for (long c = 0; c < nch; c++) {
        if (ch[c].first) o += JMN_UNIT_OVERHEAD;
        ch[c].out = o;
        o += ch[c].outn;
    }
    const long z = (long)jmn_zero_words(bins, bd, nmb, o - 4L * n), total = o + 3 * z;
    for (int u = 0; u < n; u++) {
        uoff[u] = (long)ch[cs[u]].out - JMN_UNIT_OVERHEAD;
        usz[u] = (u + 1 < n ? (long)ch[cs[u + 1]].out - JMN_UNIT_OVERHEAD : total) - uoff[u];
    }
    /* write */
    for (long c = 0; c < nch; c++) {
        const int u = ch[c].unit;
        const long start = (long)(c - cs[u]) * JMN_CHUNK;
        long w = (long)ch[c].out;
        if (ch[c].first) {
            out[w - 5] = 0; out[w - 4] = 0; out[w - 3] = 0; out[w - 2] = 1;
            out[w - 1] = (uint8_t)((us[u].ref_idc << 5) | us[u].type);
        }
        int32_t carry = ch[c].carry;
        for (int p = 0; p < ch[c].n; p += JMN_TILE) {
            const int tn = ch[c].n - p < JMN_TILE ? ch[c].n - p : JMN_TILE;
            uint64_t nz, le3;
            tile_ballots(&us[u], start + p, tn, &nz, &le3);
            const uint64_t esc = tile_escapes(nz, le3, carry);
            for (int lane = 0; lane < tn; lane++) {
                const long at = w + jmn_lane_out(esc, lane);
                if ((esc >> lane) & 1) {
                    out[at - 1] = 3;
                    const long L = jmn_lane_L(nz, lane, carry), i = start + p + lane;
                    n_escapes++;
                    if (L > lane) census_tile++;
                    if (L > p + lane) census_chunk++;
                    if (L >= p + lane + JMN_CHUNK) census_zero_chunk++;
                    if (i >= us[u].hn && i - L < us[u].hn) census_junction++;
                }
                out[at] = unit_byte(&us[u], start + p + lane);
            }
            w += tn + __builtin_popcountll(esc);
            carry = jmn_tile_carry(nz, tn, carry);
        }
        if (w != (long)ch[c].out + ch[c].outn) { printf("chunk size mismatch\n"); n_differ++; }
        if (c == nch - 1) for (long i = 0; i < 3 * z; i++) out[w + i] = i % 3 == 2 ? 3 : 0;
    }
    free(cs); free(ch);
    return total;
}

/* the reference: jm_write_nal per unit, then the zero words as encode_picture_slices appends them */
static long ref_wrap(const unit_t *us, int n, long bins, int bd, long nmb, jm_bits *out, long *uoff, long *usz) {
    out->len = 0;
    for (int u = 0; u < n; u++) {
        jm_bits r;
        jm_bits_init(&r);
        jm_bits h = {us[u].head, us[u].hn, us[u].hn, 0, 0}, p = {us[u].pay, us[u].pn, us[u].pn, 0, 0};
        jm_bits_append(&r, &h);
        jm_bits_append(&r, &p);
        uoff[u] = out->len;
        jm_write_nal(out, us[u].ref_idc, us[u].type, &r);
        usz[u] = out->len - uoff[u];
        jm_bits_free(&r);
    }
    if (bins > 0) {
        const long bytes = out->len - 4L * n;
        const int b = bd > 8 ? bd : 8;
        const long excess = 3 * bins - 36L * b * nmb - 32 * bytes;
        for (long z = excess > 0 ? (excess + 95) / 96 : 0; z > 0; z--) {
            static const uint8_t zw[3] = {0, 0, 3};
            jm_bits t = {(uint8_t *)zw, 3, 3, 0, 0};
            jm_bits_append(out, &t);
            usz[n - 1] += 3;
        }
    }
    return out->len;
}

static jm_bits ref_out;
static long check_au(const unit_t *us, int n, long bins, int bd, long nmb) {
    long in = 0;
    for (int u = 0; u < n; u++) in += us[u].hn + us[u].pn;
    long *ro = (long *)malloc(4 * n * sizeof(long)), *rs = ro + n, *co = rs + n, *cz = co + n;
    const long rt = ref_wrap(us, n, bins, bd, nmb, &ref_out, ro, rs);
    uint8_t *big = (uint8_t *)malloc(rt ? rt : 1);     /* exactly the reference's bytes: a store past them is the sanitizer's */
    const long ct = core_wrap(us, n, bins, bd, nmb, big, co, cz);
    int bad = ct != rt || memcmp(big, ref_out.buf, rt < ct ? rt : ct) != 0;
    for (int u = 0; u < n && !bad; u++) bad = ro[u] != co[u] || rs[u] != cz[u];
    if (bad) {
        n_differ++;
        if (n_differ < 5) printf("differ: %d units, %ld input bytes, ref %ld core %ld bytes\n", n, in, rt, ct);
    }
    n_aus++; n_units += n;
    free(big); free(ro);
    return rt;
}

static uint8_t *filled(long n, uint8_t v) { uint8_t *p = (uint8_t *)malloc(n ? n : 1); memset(p, v, n ? n : 1); return p; }

/* one unit: a zero run of r bytes ending at `end`, the follower v behind it, filler elsewhere; the first hn bytes are the head */
static void run_case(long end, int r, int v, int hn) {
    if (end - r < 0) return;
    const long len = end + 3;
    uint8_t *b = filled(len, 0x55);
    memset(b + end - r, 0, r);
    b[end] = (uint8_t)v;
    if (hn > len) hn = (int)len;
    unit_t u = {2, 1, b, hn, b + hn, len - hn};
    check_au(&u, 1, 0, 8, 1);
    free(b);
}

static uint32_t rng = 12345;
static uint32_t rnd(void) { rng = rng * 1664525u + 1013904223u; return rng >> 8; }
static const uint8_t ALPHA[8] = {0, 0, 0, 1, 2, 3, 4, 0xff};

int main(void) {
    static const int FOLLOW[6] = {0, 1, 2, 3, 4, 0xff};
    const long TT[2] = {JMN_TILE, JMN_CHUNK};
    jm_bits_init(&ref_out);
    /* zero runs ending around multiples of the tile and the chunk; all payload, and behind a 7-byte head */
    for (int t = 0; t < 2; t++)
        for (int m = 1; m <= 3; m++)
            for (int d = -3; d <= 3; d++)
                for (int r = 1; r <= 7; r++)
                    for (int f = 0; f < 6; f++) {
                        run_case(m * TT[t] + d, r, FOLLOW[f], 0);
                        run_case(m * TT[t] + d, r, FOLLOW[f], 7);
                    }
    /* the run split by the head / payload junction at every split point (s of its r zeros in the head) */
    for (int r = 1; r <= 7; r++)
        for (int s = 0; s <= r; s++)
            for (int f = 0; f < 6; f++)
                for (int hn = s; hn <= JMH_NAL_HEAD_MAX; hn = hn < s + 9 ? hn + 1 : hn < 58 ? 58 : hn + 1)
                    run_case(hn - s + r, r, FOLLOW[f], hn);
    /* units of 0, 1, T - 1, T, T + 1 bytes */
    for (int t = 0; t < 2; t++) {
        const long L[5] = {0, 1, TT[t] - 1, TT[t], TT[t] + 1};
        for (int k = 0; k < 5; k++)
            for (int rep = 0; rep < 8; rep++) {
                uint8_t *b = filled(L[k], 0);
                for (long i = 0; i < L[k]; i++) b[i] = ALPHA[rnd() & 7];
                const int hn = (int)(rep & 1 ? (L[k] < 5 ? L[k] : 5) : 0);
                unit_t u = {3, 5, b, hn, b + hn, L[k] - hn};
                check_au(&u, 1, 0, 8, 1);
                free(b);
            }
    }
    /* a middle chunk of zeros, and two of them: before it 0..3 zeros end the first chunk, every follower behind */
    for (int zc = 1; zc <= 2; zc++)
        for (int pre = 0; pre <= 3; pre++)
            for (int f = 0; f < 6; f++) {
                const long len = (zc + 2L) * JMN_CHUNK;
                uint8_t *b = filled(len, 0x77);
                memset(b + JMN_CHUNK - pre, 0, pre + (long)zc * JMN_CHUNK);
                b[(zc + 1L) * JMN_CHUNK] = (uint8_t)FOLLOW[f];
                unit_t u = {2, 1, b, 3, b + 3, len - 3};
                check_au(&u, 1, 0, 8, 1);
                free(b);
            }
    /* units in a row: one ends in 00 00, the next begins with 00 xx: no carry may cross units */
    for (int f = 0; f < 6; f++)
        for (int hn = 0; hn <= 2; hn++) {
            uint8_t a[6] = {9, 9, 9, 9, 0, 0}, b[4] = {0, (uint8_t)FOLLOW[f], 0, 0}, c[3] = {0, 0, (uint8_t)FOLLOW[f]}, e[1] = {0};
            unit_t us[5] = {{3, 5, a, hn, a + hn, 6 - hn}, {3, 5, b, hn, b + hn, 4 - hn}, {2, 1, c, hn, c + hn, 3 - hn}, {2, 1, e, 0, e, 0},
                            {2, 1, c, 0, c, 3}};
            check_au(us, 5, 0, 8, 1);
        }
    /* 2,000 random units of 0..3 chunks, in access units of 1..4 */
    for (int done = 0; done < 2000;) {
        unit_t us[4];
        const int n = 1 + (int)(rnd() % 4);
        for (int u = 0; u < n; u++) {
            const uint32_t k = rnd() % 8;
            const long len = k == 0 ? rnd() % 8 : k < 4 ? rnd() % (2 * JMN_TILE + 2) : rnd() % (3 * JMN_CHUNK + 1);
            uint8_t *b = filled(len, 0);
            for (long i = 0; i < len; i++) b[i] = ALPHA[rnd() & 7];
            int hn = (int)(rnd() % (JMH_NAL_HEAD_MAX + 1));
            if (hn > len) hn = (int)len;
            us[u] = (unit_t){(int)(rnd() & 3), 1 + (int)(rnd() % 5), b, hn, b + hn, len - hn};
        }
        check_au(us, n, 0, 8, 1);
        for (int u = 0; u < n; u++) free(us[u].head);
        done += n;
    }
    /* zero words: bins for an excess of 0, 1, 96, 97 and for many words, at bit depths 8 and 10 */
    {
        static const long EXC[6] = {0, 1, 96, 97, -50, 96 * 40 + 1}, WANT[6] = {0, 1, 1, 2, 0, 41};
        const long nmb = 12;
        for (int bd = 8; bd <= 10; bd += 2)
            for (int k = 0; k < 6; k++)
                for (long len = 30; len < 33; len++) {                    /* bytes = 1 + len; 3 | excess + 32 * bytes picks one */
                    const long rhs = EXC[k] + 36L * bd * nmb + 32 * (1 + len);
                    if (rhs % 3) continue;
                    uint8_t *b = filled(len, 0x55);
                    b[len - 1] = 0; b[len - 2] = 0;                          /* the unit ends in zeros: the words follow them */
                    unit_t u = {2, 1, b, 4, b + 4, len - 4};
                    const long before = check_au(&u, 1, 0, bd, nmb), after = check_au(&u, 1, rhs / 3, bd, nmb);
                    if (after - before != 3 * WANT[k]) { printf("zero words: excess %ld gave %ld bytes\n", EXC[k], after - before); n_differ++; }
                    n_zero_cases++;
                    free(b);
                }
    }
    jm_bits_free(&ref_out);
    printf("nal core check: %ld access units, %ld units, %ld escapes, %ld zero-word cases, %ld differ; an escape's zero run crossed "
           "a tile boundary %ld times, a chunk boundary %ld, the junction %ld, a chunk of zeros %ld\n",
           n_aus, n_units, n_escapes, n_zero_cases, n_differ, census_tile, census_chunk, census_junction, census_zero_chunk);
    return n_differ ? 1 : 0;
}
