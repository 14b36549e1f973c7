/*
 * jmh_cabac_split.h -- one CABAC slice coded as many chunks (csrc/jmh_cabac_split.hip, DESIGN.md
 * §5.5).  A slice's bin records (jmh_cabac_write.h) are cut into chunks of L records; every chunk
 * of every slice is coded at once and the chunks' bytes are added up to the bytes the serial coder
 * (k_cabac_code, jmc_enc) writes.  The three kinds of coder state, each resolved without a serial
 * pass over the slice:
 *
 *   contexts  A context's next value depends on its value and the bin only (jms_ctx_next, the ns /
 *             nm of jmc_enc_bin).  Over a span of records (a whole number of chunks, jms_span) a
 *             context undergoes a map on 128 values; the maps of a slice's spans are composed in
 *             order, which gives every span its entry contexts; one more pass over the span then
 *             replaces every regular record's context index by the context's value at that bin
 *             (jms_resolve: a resolved record, pStateIdx << 1 | valMPS in bits 0..6).
 *   range     After every record the range is one of the 256 values 256..511.  jms_range_rec steps
 *             one candidate through one resolved record and counts its renormalisation shifts, so
 *             a chunk is a table entry range -> (exit range, shifts); composed along the slice it
 *             gives every chunk's entry range and the bits T of the code string before it.
 *   low       low is linear in what is added to it, so a chunk coded from low = 0 with its entry
 *             range yields its addend to the code string.  left is preset (jms_left0) so that the
 *             chunk's byte boundaries fall on the slice's byte grid: its first byte is the slice's
 *             byte jms_byte0(T).  Chunk c owns the region [jms_byte0(T_c), jms_byte0(T_c+1)) of
 *             the slice; the bits of low not yet sent at its end (at most 20) leave as three more
 *             bytes, the chunk's tail (jms_enc_tail), which lie on the successor's first bytes.
 *             The last chunk ends with jmc_enc_finish.  Its rbsp_stop_one_bit stands where bit 7
 *             of low is, and a tail may reach that bit (no shift between the chunk boundary and
 *             end_of_slice_flag 1): the serial coder drops bit 7 of the sum, so the last chunk
 *             leaves its own bit 7 there (jms_stop_info), the sum is made, and the stop bit is
 *             set afterwards.
 *   merge     A region's bytes are its own bytes plus the tail bytes of earlier chunks that fall
 *             into it (jms_tail_sum: into its first three bytes at most; a region may be empty,
 *             then a tail reaches the regions behind it) plus the carry from the regions behind.
 *             jms_region_sum adds the tails and states the region's carry-out as a function of
 *             its carry-in x: q + (x >= theta), or x itself for an empty region.  Such functions
 *             compose to one of the same form, so the carry into every region is a suffix
 *             evaluation over the slice's chunks (jms_carry_apply), and jms_region_carry ripples
 *             it through the region's trailing 0xff bytes.  This is what jmc_byte_out's held /
 *             nheld resolve inside one coder, across chunks.
 *
 * The coder codes resolved records with the step functions of jmh_cabac_write.h: this header maps
 * JMC_CTX_GET to the record's own value unless the including file has set the macros (a kernel
 * keeps Table 9-44 in registers).  No table is repeated here.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_CABAC_SPLIT_H
#define JMH_CABAC_SPLIT_H

#ifndef JMC_CTX_GET
#define JMC_CTX_GET(e, i) ((uint32_t)(i))            /* a resolved record carries the context's value */
#define JMC_CTX_SET(e, i, v) ((void)(v))
#define JMC_LPS_GET(e, s, q) ((uint32_t)(e)->lps[(s) * 4 + (q)])
#define JMC_TLPS_GET(e, s) 0
#endif
#include "jmh_cabac_write.h"

#define JMS_NVAL 128                                 /* values of a context: state << 1 | valMPS */
#define JMS_MAP_BYTES (JMR_NCTX * JMS_NVAL)          /* one span's maps: 36,864 bytes */
#define JMS_SPAN_MIN 4096                            /* records of a span at least (the kernels) */
#define JMS_NRANGE 256                               /* entry ranges 256..511 */
#define JMS_THETA_INF 0xffffffffu

/* chunks of a slice of nb records: a slice shorter than L is one chunk, the last chunk may be short */
JMR_FN uint64_t jms_nchunks(uint64_t nb, uint64_t L) { return nb <= L ? 1 : (nb + L - 1) / L; }
/* the span of the context pass: the least multiple of L that is at least JMS_SPAN_MIN */
JMR_FN uint64_t jms_span(uint64_t L) { return L >= JMS_SPAN_MIN ? L : L * ((JMS_SPAN_MIN + L - 1) / L); }

/* ---- contexts ------------------------------------------------------------------------------- */
/* a context's value after a bin; tl: transIdxLPS of its state */
JMR_FN uint32_t jms_ctx_next(uint32_t v, int bin, int tl) {
    const int s = (int)(v >> 1), mps = (int)(v & 1);
    const int lpsbin = bin != mps;
    const int ns = lpsbin ? tl : (s < 62 ? s + 1 : s);
    const int nm = mps ^ (lpsbin & (s == 0));
    return (uint32_t)((ns << 1) | nm);
}
JMR_FN int jms_is_regular(uint32_t rec) { return !(rec & (JMC_BYPASS | JMC_TERM)); }
/* the resolved record of a regular bin whose context holds v */
JMR_FN uint32_t jms_resolve(uint32_t rec, uint32_t v) { return (rec & 0x8000u) | v; }

/* ---- range ---------------------------------------------------------------------------------- */
JMR_FN uint32_t jms_lps_dword(int s) {               /* rangeTabLPS[s][0..3]: all <= 240 */
    return (uint32_t)jmr_lps[s][0] | (uint32_t)jmr_lps[s][1] << 8 | (uint32_t)jmr_lps[s][2] << 16 | (uint32_t)jmr_lps[s][3] << 24;
}
/* one candidate range through one resolved record; lpsdw: jms_lps_dword of the record's state */
JMR_FN void jms_range_rec(uint32_t rr, uint32_t lpsdw, uint32_t *range, uint32_t *shifts) {
    const int bin = (int)JMC_VAL(rr);
    if (rr & JMC_TERM) {
        const uint32_t r = *range - 2;
        const int n = bin ? 7 : jmr_renorm_steps(r);
        *range = bin ? 256u : r << n;
        *shifts += (uint32_t)n;
    } else if (rr & JMC_BYPASS) *shifts += 1;
    else {
        const uint32_t lps = (lpsdw >> (8 * ((*range >> 6) & 3))) & 0xffu;
        const uint32_t r = bin != (int)(rr & 1) ? lps : *range - lps;
        const int n = jmr_renorm_steps(r);
        *range = r << n;
        *shifts += (uint32_t)n;
    }
}
/* a chunk's table entry: exit range and shifts (<= 7 * 65536) of one entry range */
JMR_FN uint32_t jms_rmap_pack(uint32_t range, uint32_t shifts) { return (range - 256u) | shifts << 8; }
JMR_FN uint32_t jms_rmap_range(uint32_t e) { return 256u + (e & 0xffu); }
JMR_FN uint32_t jms_rmap_shifts(uint32_t e) { return e >> 8; }

/* ---- the byte grid --------------------------------------------------------------------------
 * After T shifts the serial coder's left is 23 - T while no byte is whole (T <= 11), then the value
 * in 12..19 congruent to 23 - T modulo 8; the bytes it has taken from low by then: jms_byte0. */
JMR_FN int jms_left0(uint64_t T) { return T <= 11 ? 23 - (int)T : 12 + (int)((11 - T) & 7); }
JMR_FN uint64_t jms_byte0(uint64_t T) { return (T + (uint64_t)jms_left0(T) - 23) >> 3; }

/* ---- code ----------------------------------------------------------------------------------- */
/* a chunk's coder: low = 0, its entry range, left on the slice's grid.  T = 0, range 510 is jmc_enc_start */
JMR_FN void jms_enc_begin(jmc_enc *e, uint32_t range, uint64_t T) {
    e->low = 0; e->range = range; e->left = jms_left0(T);
    e->held = 0xff; e->nheld = 0;
    e->nbytes = 0;
}
/* end of a chunk that is not the slice's last: the unsent bits of low (below bit 32 - left, at
   most 20) as three bytes, then the held bytes; nothing is pending above them (low started at 0) */
JMR_FN void jms_enc_tail(jmc_enc *e) {
    for (int k = 0; k < 3; k++) {
        e->low <<= 8;
        e->left -= 8;
        jmc_byte_out(e);
    }
    if (e->nheld > 0) JMC_EMIT(e, e->held);
    for (; e->nheld > 1; e->nheld--) JMC_EMIT(e, 0xff);
    e->nheld = 0;
}
/* before jmc_enc_finish of the last chunk: bit 3 the chunk's own bit 7 of low, bits 0..2 the bit of
   the slice's last byte that holds the rbsp_stop_one_bit */
JMR_FN uint32_t jms_stop_info(const jmc_enc *e) {
    const int nb = 24 - e->left + 1;
    return ((e->low >> 7) & 1u) << 3 | (uint32_t)((8 - (nb & 7)) & 7);
}
/* the last byte of the slice before the sum (the chunk's own bit in place of the stop bit) and after it */
JMR_FN uint32_t jms_stop_clear(uint32_t byte, uint32_t info) { return (byte & ~(1u << (info & 7))) | ((info >> 3) & 1u) << (info & 7); }
JMR_FN uint32_t jms_stop_set(uint32_t byte, uint32_t info) { return byte | 1u << (info & 7); }

/* ---- merge ---------------------------------------------------------------------------------- */
/* The bytes of the tails of the slice's chunks before chunk c that fall into [B, B + m), m <= 3, as
   a number whose last byte lies at B + m - 1.  T[p]: the shifts before chunk p of this slice (its
   region starts at jms_byte0(T[p]), where chunk p - 1's tail lies); tail[p]: chunk p's three bytes */
JMR_FN uint64_t jms_tail_sum(const uint32_t *tail, const uint64_t *T, uint64_t c, uint64_t B, uint32_t m) {
    uint64_t A = 0;
    for (uint64_t p = c; p > 0; p--) {
        const uint64_t at = jms_byte0(T[p]);
        if (at + 3 <= B) break;                       /* regions ascend: nothing before reaches B */
        for (uint32_t j = 0; j < 3; j++) {
            const uint64_t P = at + j;
            if (P >= B && P < B + m) A += (uint64_t)((tail[p - 1] >> (8 * (2 - j))) & 0xffu) << (8 * (B + m - 1 - P));
        }
    }
    return A;
}
/* Region b[0 .. len): adds A to its first min(len, 3) bytes; carry-out for carry-in x is
   q + (x >= theta), theta >= 1; theta = 0: the region is empty, the carry passes */
JMR_FN void jms_region_sum(uint8_t *b, uint64_t len, uint64_t A, uint32_t *q, uint32_t *theta) {
    *q = 0; *theta = 0;
    if (!len) return;
    const uint32_t m = len < 3 ? (uint32_t)len : 3u;
    uint64_t H = 0;
    for (uint32_t i = 0; i < m; i++) H = H << 8 | b[i];
    H += A;
    for (uint32_t i = m; i > 0; i--) { b[i - 1] = (uint8_t)H; H >>= 8; }
    *q = (uint32_t)H;
    uint32_t last = 0;                                /* the last m bytes */
    for (uint32_t i = 0; i < m; i++) last = last << 8 | b[len - m + i];
    uint64_t k = len - m;
    while (k > 0 && b[k - 1] == 0xff) k--;            /* bounded by the region */
    *theta = k ? JMS_THETA_INF : (1u << (8 * m)) - last;
}
JMR_FN uint32_t jms_carry_apply(uint32_t q, uint32_t theta, uint32_t x) { return theta ? q + (x >= theta) : x; }
/* the carry x into region b[0 .. len) */
JMR_FN void jms_region_carry(uint8_t *b, uint64_t len, uint32_t x) {
    for (uint64_t k = len; k > 0 && x; k--) {
        const uint32_t s = b[k - 1] + x;
        b[k - 1] = (uint8_t)s;
        x = s >> 8;
    }
}

#endif
