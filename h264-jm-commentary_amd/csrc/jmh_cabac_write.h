/*
 * jmh_cabac_write.h -- CABAC slice data as the device writes it (csrc/jmh_cabac.hip, DESIGN.md
 * §5.3), in two halves that share nothing but a sequence of bin records:
 *
 *   1. binarisation and context selection: host/cabac.c › write_mb_body restated as a function of
 *      the picture's jmh_mb_result array (jmw_pic / jmw_slice of jmh_cavlc_write.h).  The host
 *      writes mb_qp_delta = 0 always and the model is fixed (cabac_init_idc 0), so every ctxIdx of
 *      a macroblock depends only on final results of macroblocks of the same slice, never on coder
 *      state.  A neighbour is available iff it lies in the picture and its address lies in
 *      [first_mb, current); what the host keeps of it in `cmb` is recomputed from its result:
 *      kind, cbp, transform_size_8x8_flag (jmc_t8: the syntax conditions of 7.3.5 decide whether
 *      the flag was sent at all), intra_chroma_pred_mode, and the coded_block_flags recounted from
 *      the levels under the cbp / I16 rules (jmc_cbf_luma: an 8x8-transform block infers 1 on its
 *      four 4x4 blocks, the host's 0x33 << ...).
 *      mvd of a neighbouring partition: RECOMPUTED as its mv minus its MVP (jmc_abs_mvd_of), not read
 *      from a per-4x4 array a preparation pass would write.  Why: the header unit of a macroblock
 *      then needs no pass before it and no buffer of the picture's size, so count and store stay
 *      two launches over the same inputs; the price is at most two more jmw_mvp per partition
 *      (three instead of one), paid by one lane of 28 while the residual lanes are still busy.
 *      The host stores mvd in int16_t, so a neighbour's |mvd| is taken after that truncation.
 *   2. the arithmetic encoder of 9.3.4.2 .. 9.3.4.5 with byte output (jmc_enc): the interval's low
 *      end is kept with its carry and bytes leave through one held-back byte plus a count of 0xff
 *      bytes behind it, instead of PutBit's outstanding bits.  The code string is the same (the
 *      spec fixes it); tests/harness/cabac_core_check.c compares bytes with host/cabac.c.
 *
 * Bin record (16 bits): bit 15 the bin value; bits 0..8 the dense context JMR_CTX (< JMR_NCTX = 288)
 * of a regular bin, or JMC_BYPASS / JMC_TERM.  The sink counts (rec == NULL) or stores.
 *
 * Units: a macroblock is cut into the JMW_UNITS = 28 units of the CAVLC core (0 header syntax:
 * end_of_slice_flag 0 of the previous macroblock, mb_skip_flag .. mb_qp_delta; 1 Intra16x16 DC;
 * 2..17 luma 4x4 in coding order -- with the 8x8 transform unit 2 + 4 * b8 holds the whole 8x8
 * block; 18 / 19 chroma DC; 20..27 chroma AC; unit 27 also ends the slice's last macroblock with
 * end_of_slice_flag 1).  The units' records concatenated in unit order are the macroblock's bins;
 * inside one block the bins stay serial (eq1 / gt1).
 *
 * Worst case of one macroblock for arbitrary int16_t levels and motion vectors (JMC_MB_MAX_BINS):
 *   - a level: |level| <= 32768, coeff_abs_level_minus1 <= 32767: 14 regular bins (the prefix TU,
 *     cMax 14), the UEG0 suffix of 32767 - 14 = 32753: 14 ones (2^14 - 1 <= 32753 < 2^15 - 1), a
 *     zero, 14 bits = 29 bypass bins, and the sign: 44 bins;
 *   - a block of n coefficients, all non-zero: coded_block_flag 1 + significant / last flags
 *     2 (n - 1) + 44 n: 735 (n = 16), 689 (n = 15), 183 (chroma DC, n = 4), 2942 (8x8, n = 64, no
 *     coded_block_flag).  A zero coefficient costs 1 bin instead of 46: never more;
 *   - residual: luma max(4 * 2942 = 11768 (8x8), 16 * 735 = 11760, I16 735 + 16 * 689 = 11759)
 *     + chroma 2 * 183 + 8 * 689 = 5878: 17646;
 *   - an mvd component: |mvd| <= 65535: 9 regular bins (prefix TU, uCoff 9), the UEG3 suffix of
 *     65535 - 9 = 65526: 12 ones (8 * (2^12 - 1) <= 65526 < 8 * (2^13 - 1)), a zero, 15 bits = 28,
 *     and the sign: 38 bins;
 *   - header: end_of_slice_flag 1 + mb_skip_flag 1 + inter at most mb_type 3 + four sub_mb_type
 *     3 each + 32 mvd components 1216 + coded_block_pattern 6 + transform flag 1 + mb_qp_delta 1
 *     = 1241 (intra at most 1 + 1 + 8 + 1 + 16 * 4 + 3 + 6 + 1 = 85);
 *   - the slice's closing end_of_slice_flag: 1;
 *   - in all 1241 + 17646 + 1 = 18888 bins: under JMC_MB_MAX_BINS = 18944 (a multiple of 64).
 *
 * Bytes of one slice from its counted bins (JMC_SLICE_MAX_BYTES): every renormalisation step and
 * every bypass bin yields exactly one bit of the code string.  A regular bin renormalises at most
 * 6 steps (the range is >= 6 after an LPS: Table 9-44 without state 63, which no context reaches;
 * >= 128 after an MPS), a bypass bin is one step, end_of_slice_flag 0 at most one, end_of_slice
 * _flag 1 seven (range 2); EncodeFlush adds 3 bits and the first bit is dropped.  So a slice of
 * n bins has at most 7 n + 2 bits, (7 n + 9) / 8 bytes.
 *
 * Written in the common subset of C99 and HIP C++.
 */
#ifndef JMH_CABAC_WRITE_H
#define JMH_CABAC_WRITE_H

#include <stdint.h>
#include "jmh_cabac_rate.h"
#include "jmh_cavlc_write.h"

#define JMC_MB_MAX_BINS 18944
#define JMC_SLICE_MAX_BYTES(nbins) ((7 * (uint64_t)(nbins) + 9) / 8)

#define JMC_BYPASS 0x1000u
#define JMC_TERM 0x2000u
#define JMC_VAL(rec) ((uint32_t)(rec) >> 15)

/* ---- bin sink ---------------------------------------------------------------------------------- */
typedef struct jmc_sink {
    uint16_t *rec;                 /* NULL: only counts */
    uint32_t n;
} jmc_sink;

JMR_FN void jmc_put(jmc_sink *s, uint32_t what, int bin) {
    if (s->rec) s->rec[s->n] = (uint16_t)(what | (bin ? 0x8000u : 0u));
    s->n++;
}
#define jmc_bin(s, ctx, bin) jmc_put((s), (uint32_t)(ctx), (bin))
#define jmc_bypass(s, bin) jmc_put((s), JMC_BYPASS, (bin))
#define jmc_term(s, bin) jmc_put((s), JMC_TERM, (bin))

/* UEGk suffix (9.3.2.3) in bypass bins */
JMR_FN void jmc_eg_bypass(jmc_sink *s, unsigned v, int k) {
    for (;;) {
        if (v >= (1u << k)) { jmc_bypass(s, 1); v -= 1u << k; k++; }
        else {
            jmc_bypass(s, 0);
            while (k--) jmc_bypass(s, (int)((v >> k) & 1));
            return;
        }
    }
}

/* ---- what host/cabac.c keeps of a written macroblock (cmb), from its result ------------------- */
JMR_FN int jmc_kind(const jmh_mb_result *r, int sp) {
    if (jmw_is_skip(r, sp)) return JMR_K_SKIP;
    return r->mb_type == JMH_I16MB ? JMR_K_I16 : jmw_is_nxn(r, sp) ? JMR_K_INXN : JMR_K_INTER;
}
JMR_FN int jmc_cbp(const jmh_mb_result *r, int sp) { return jmw_is_skip(r, sp) ? 0 : (uint8_t)r->cbp; }
JMR_FN int jmc_all8x8(const jmh_mb_result *r) {
    return r->b8mode[0] == 4 && r->b8mode[1] == 4 && r->b8mode[2] == 4 && r->b8mode[3] == 4;
}
/* transform_size_8x8_flag as sent (0 where the syntax does not send it) */
JMR_FN int jmc_t8(const jmw_pic *p, const jmh_mb_result *r, int sp) {
    if (!p->t8mode || jmw_is_skip(r, sp) || r->mb_type == JMH_I16MB) return 0;
    if (jmw_is_nxn(r, sp)) return r->mb_type == JMH_I8MB;
    if (!(r->cbp & 15) || (r->mb_type == JMH_P8x8 && !jmc_all8x8(r))) return 0;
    return r->transform_8x8 != 0;
}
JMR_FN int jmc_cmode(const jmh_mb_result *r, int sp) { return jmw_is_intra(r, sp) ? r->c_ipred_mode : 0; }
/* coded_block_flag of luma 4x4 (x4, y4) as cbf_l holds it (the current macroblock's own included) */
JMR_FN int jmc_cbf_luma(const jmw_pic *p, const jmh_mb_result *r, int sp, int x4, int y4) {
    if (jmw_is_skip(r, sp)) return 0;
    if (!((r->cbp >> ((y4 >> 1) * 2 + (x4 >> 1))) & 1)) return 0;
    if (jmc_t8(p, r, sp)) return 1;                    /* inferred (7.4.5.3.3) */
    return r->mb_type == JMH_I16MB ? jmw_nnz(r->luma[y4 * 4 + x4] + 1, 15) != 0 : jmw_nnz(r->luma[y4 * 4 + x4], 16) != 0;
}
/* condTermFlagN (9.3.3.1.1.9) of a neighbour's luma 4x4; n NULL: not available */
JMR_FN int jmc_luma_term(const jmw_pic *p, const jmh_mb_result *n, int sp, int cur_intra, int x4, int y4) {
    return n ? jmc_cbf_luma(p, n, sp, x4, y4) : cur_intra;
}
JMR_FN int jmc_i16dc_term(const jmh_mb_result *n, int sp) {
    if (!n) return 1;
    return jmc_kind(n, sp) == JMR_K_I16 ? jmw_nnz(n->luma_dc, 16) != 0 : 0;
}
JMR_FN int jmc_cdc_term(const jmh_mb_result *n, int sp, int cur_intra, int uv) {
    if (!n) return cur_intra;
    return (jmc_cbp(n, sp) >> 4) != 0 ? jmw_nnz(n->chroma_dc[uv], 4) != 0 : 0;
}
JMR_FN int jmc_cac_flag(const jmh_mb_result *r, int uv, int k) { return jmw_nnz(r->chroma_ac[uv][k] + 1, 15) != 0; }
JMR_FN int jmc_cac_term(const jmh_mb_result *n, int sp, int cur_intra, int uv, int k) {
    if (!n) return cur_intra;
    return (jmc_cbp(n, sp) >> 4) == 2 ? jmc_cac_flag(n, uv, k) : 0;
}

/* the partition of macroblock r that covers its 4x4 block k (raster) */
JMR_FN void jmc_partition(const jmh_mb_result *r, int k, int *bx, int *by, int *bw, int *bh) {
    const int x = (k & 3) * 4, y = (k >> 2) * 4, mbt = r->mb_type;
    if (mbt == JMH_P16x16) { *bx = 0; *by = 0; *bw = 16; *bh = 16; }
    else if (mbt == JMH_P16x8) { *bx = 0; *by = y & 8; *bw = 16; *bh = 8; }
    else if (mbt == JMH_P8x16) { *bx = x & 8; *by = 0; *bw = 8; *bh = 16; }
    else {
        const int sm = r->b8mode[(y >> 3) * 2 + (x >> 3)];
        *bw = (sm == 4 || sm == 5) ? 8 : 4;
        *bh = (sm == 4 || sm == 6) ? 8 : 4;
        *bx = x & ~(*bw - 1);
        *by = y & ~(*bh - 1);
    }
}
/* mvd_l0 of the partition at (bx, by) of macroblock a: mv - MVP */
JMR_FN void jmc_mvd_part(const jmw_pic *p, const jmw_slice *sl, int a, int bx, int by, int bw, int bh, int *d) {
    int pr[2];
    jmw_mvp(p, sl, a, bx, by, bw, bh, pr);
    const jmh_mb_result *r = p->res + a;
    const int k = (by >> 2) * 4 + (bx >> 2);
    d[0] = r->mv[k][0] - pr[0];
    d[1] = r->mv[k][1] - pr[1];
}
/* absMvdComp of the 4x4 block k of macroblock n as the host's int16_t mvd array holds it (0 for
   P_Skip and intra macroblocks) */
JMR_FN void jmc_abs_mvd_of(const jmw_pic *p, const jmw_slice *sl, const jmh_mb_result *n, int k, int *out) {
    out[0] = 0; out[1] = 0;
    if (!n || jmw_is_skip(n, sl->slice_p) || jmw_is_intra(n, sl->slice_p)) return;
    int bx, by, bw, bh, d[2];
    jmc_partition(n, k, &bx, &by, &bw, &bh);
    jmc_mvd_part(p, sl, (int)(n - p->res), bx, by, bw, bh, d);
    for (int c = 0; c < 2; c++) {
        const int t = (int16_t)d[c];
        out[c] = t < 0 ? -t : t;
    }
}

/* one mvd_l0 component (UEG3, signed, uCoff 9) with absMvdComp(A) + absMvdComp(B) = sum */
JMR_FN void jmc_mvd_comp(jmc_sink *s, int v, int sum, int comp) {
    const int base = comp ? JMR_CTX(47) : JMR_CTX(40), a = v < 0 ? -v : v;
    jmc_bin(s, base + (sum < 3 ? 0 : sum > 32 ? 2 : 1), a != 0);
    if (!a) return;
    int k = 1;
    for (; k < a && k < 9; k++) jmc_bin(s, base + (k < 4 ? k + 2 : 6), 1);
    if (a < 9) jmc_bin(s, base + (k < 4 ? k + 2 : 6), 0);
    else jmc_eg_bypass(s, (unsigned)(a - 9), 3);
    jmc_bypass(s, v < 0);
}
JMR_FN void jmc_mvd(jmc_sink *s, const jmw_pic *p, const jmw_slice *sl, int a, int bx, int by, int bw, int bh) {
    int d[2], sa[2], sb[2], ka = 0, kb = 0;
    jmc_mvd_part(p, sl, a, bx, by, bw, bh, d);
    const jmh_mb_result *A = jmw_nb(p, sl, a, bx - 1, by, &ka), *B = jmw_nb(p, sl, a, bx, by - 1, &kb);
    jmc_abs_mvd_of(p, sl, A, ka, sa);
    jmc_abs_mvd_of(p, sl, B, kb, sb);
    jmc_mvd_comp(s, d[0], sa[0] + sb[0], 0);
    jmc_mvd_comp(s, d[1], sa[1] + sb[1], 1);
}

/* residual_block_cabac (7.3.5.3.3, 9.3.3.1.3): coef[0..n) in scan order, cat 0..4 (ctxBlockCat) or
   5 (luma 8x8, no coded_block_flag: cbf_inc < 0) */
JMR_FN void jmc_residual(jmc_sink *s, const int16_t *coef, int n, int cat, int cbf_inc) {
    uint64_t nzm = 0;
    for (int i = 0; i < n; i++)
        if (coef[i]) nzm |= (uint64_t)1 << i;
    const int last = nzm ? 63 - __builtin_clzll(nzm) : -1;
    if (cbf_inc >= 0) jmc_bin(s, JMR_CTX(85) + 4 * cat + cbf_inc, last >= 0);
    if (last < 0) return;
    const int so = cat == 0 ? 0 : cat == 1 ? 15 : cat == 2 ? 29 : cat == 3 ? 44 : 47;
    const int ao = cat == 0 ? 0 : cat == 1 ? 10 : cat == 2 ? 20 : cat == 3 ? 30 : 39;
    const int sig_base = cat == 5 ? JMR_CTX(402) : JMR_CTX(105) + so, last_base = cat == 5 ? JMR_CTX(417) : JMR_CTX(166) + so;
    const int abs_base = cat == 5 ? JMR_CTX(426) : JMR_CTX(227) + ao;
    for (int i = 0; i < n - 1; i++) {                 /* significance map */
        const int si = cat == 5 ? jmr_sig8x8_inc[i] : cat == 3 ? (i < 2 ? i : 2) : i;
        const int li = cat == 5 ? jmr_last8x8_inc[i] : cat == 3 ? (i < 2 ? i : 2) : i;
        const int sig = (int)((nzm >> i) & 1);
        jmc_bin(s, sig_base + si, sig);
        if (sig) {
            jmc_bin(s, last_base + li, i == last);
            if (i == last) break;
        }
    }
    int eq1 = 0, gt1 = 0;
    const int gmax = 4 - (cat == 3);
    for (uint64_t m = nzm; m;) {                      /* levels, reverse scan order */
        const int i = 63 - __builtin_clzll(m);
        m &= ~((uint64_t)1 << i);
        const int a = coef[i] < 0 ? -coef[i] : coef[i], v = a - 1;
        jmc_bin(s, abs_base + (gt1 ? 0 : (1 + eq1 < 4 ? 1 + eq1 : 4)), v > 0);
        if (v > 0) {
            const int ctx = abs_base + 5 + (gt1 < gmax ? gt1 : gmax);
            for (int k = 1; k < v && k < 14; k++) jmc_bin(s, ctx, 1);
            if (v < 14) jmc_bin(s, ctx, 0);
            else jmc_eg_bypass(s, (unsigned)(v - 14), 0);
        }
        jmc_bypass(s, coef[i] < 0);
        if (a == 1) eq1++;
        else gt1++;
    }
}

/* unit 0 of a coded macroblock: mb_type .. mb_qp_delta (write_mb_body up to the residual) */
JMR_FN void jmc_header(jmc_sink *s, const jmw_pic *p, const jmw_slice *sl, int a, const jmh_mb_result *A, const jmh_mb_result *B) {
    const jmh_mb_result *r = p->res + a;
    const int sp = sl->slice_p, mbt = r->mb_type;
    const int is_i8 = mbt == JMH_I8MB, is_nxn = mbt == JMH_I4MB || is_i8, is_i16 = mbt == JMH_I16MB;
    const int intra = is_nxn || is_i16, cbp = r->cbp, cbpl = cbp & 15, cbpc = cbp >> 4;
    const int ka = A ? jmc_kind(A, sp) : -1, kb = B ? jmc_kind(B, sp) : -1;
    if (intra) {                                      /* mb_type (9.3.2.5, Tables 9-36 / 9-37) */
        int base;
        if (sp) { jmc_bin(s, JMR_CTX(14), 1); base = JMR_CTX(17); }
        else base = JMR_CTX(3);
        const int inc0 = sp ? 0 : (A && ka != JMR_K_INXN) + (B && kb != JMR_K_INXN);
        jmc_bin(s, base + inc0, is_i16);
        if (is_i16) {
            jmc_term(s, 0);                           /* not I_PCM */
            jmc_bin(s, base + 1 + !sp * 2, cbpl != 0);
            jmc_bin(s, base + 2 + !sp * 2, cbpc != 0);
            if (cbpc) jmc_bin(s, base + (sp ? 2 : 5), cbpc == 2);
            jmc_bin(s, base + (sp ? 3 : 6), r->i16mode >> 1);
            jmc_bin(s, base + (sp ? 3 : 7), r->i16mode & 1);
        }
    } else {   /* P_L0_16x16 000, P_L0_L0_16x8 011, P_L0_L0_8x16 010, P_8x8 001 */
        const int b1 = mbt == JMH_P16x8 || mbt == JMH_P8x16, b2 = mbt == JMH_P16x8 || mbt == JMH_P8x8;
        jmc_bin(s, JMR_CTX(14), 0);
        jmc_bin(s, JMR_CTX(15), b1);
        jmc_bin(s, JMR_CTX(16) + b1, b2);
    }
    if (mbt == JMH_P8x8)                              /* sub_mb_type: 8x8 1, 8x4 00, 4x8 011, 4x4 010 */
        for (int i = 0; i < 4; i++) {
            const int sm = r->b8mode[i];
            jmc_bin(s, JMR_CTX(21), sm == JMH_SMB8x8);
            if (sm == JMH_SMB8x8) continue;
            jmc_bin(s, JMR_CTX(22), sm != JMH_SMB8x4);
            if (sm != JMH_SMB8x4) jmc_bin(s, JMR_CTX(23), sm == JMH_SMB4x8);
        }
    const int t8a = A && jmc_t8(p, A, sp), t8b = B && jmc_t8(p, B, sp);
    if (is_nxn && p->t8mode) jmc_bin(s, JMR_CTX(399) + t8a + t8b, is_i8);
    if (is_nxn)
        for (int blk = 0; blk < 16; blk += is_i8 ? 4 : 1) {
            const int x4 = ((blk >> 2) & 1) * 2 + (blk & 1), y4 = (blk >> 3) * 2 + ((blk >> 1) & 1);
            const int pred = jmw_mpm(p, sl, a, x4, y4), mode = r->ipred[y4 * 4 + x4];
            jmc_bin(s, JMR_CTX(68), mode == pred);
            if (mode != pred) {
                const int rem = mode < pred ? mode : mode - 1;
                for (int bit = 0; bit < 3; bit++) jmc_bin(s, JMR_CTX(69), (rem >> bit) & 1);
            }
        }
    if (intra) {                                      /* intra_chroma_pred_mode: TU cMax 3 */
        const int cm = r->c_ipred_mode;
        const int inc = (A && jmc_cmode(A, sp) != 0) + (B && jmc_cmode(B, sp) != 0);
        jmc_bin(s, JMR_CTX(64) + inc, cm > 0);
        if (cm > 0) { jmc_bin(s, JMR_CTX(67), cm > 1); if (cm > 1) jmc_bin(s, JMR_CTX(67), cm > 2); }
    } else if (mbt == JMH_P16x16) jmc_mvd(s, p, sl, a, 0, 0, 16, 16);
    else if (mbt == JMH_P16x8) { jmc_mvd(s, p, sl, a, 0, 0, 16, 8); jmc_mvd(s, p, sl, a, 0, 8, 16, 8); }
    else if (mbt == JMH_P8x16) { jmc_mvd(s, p, sl, a, 0, 0, 8, 16); jmc_mvd(s, p, sl, a, 8, 0, 8, 16); }
    else
        for (int i = 0; i < 4; i++) {
            const int ox = (i & 1) * 8, oy = (i >> 1) * 8, sm = r->b8mode[i];
            const int sw = (sm == 4 || sm == 5) ? 8 : 4, sh = (sm == 4 || sm == 6) ? 8 : 4;
            for (int y = 0; y < 8; y += sh)
                for (int x = 0; x < 8; x += sw) jmc_mvd(s, p, sl, a, ox + x, oy + y, sw, sh);
        }
    if (!is_i16) {                                    /* coded_block_pattern */
        const int cbpa = A ? jmc_cbp(A, sp) : 0, cbpb = B ? jmc_cbp(B, sp) : 0;
        for (int b8 = 0; b8 < 4; b8++) {
            const int bx = b8 & 1, by = b8 >> 1;
            const int ta = bx ? !((cbpl >> (b8 - 1)) & 1) : (A ? !((cbpa >> (b8 + 1)) & 1) : 0);
            const int tb = by ? !((cbpl >> (b8 - 2)) & 1) : (B ? !((cbpb >> (b8 + 2)) & 1) : 0);
            jmc_bin(s, JMR_CTX(73) + ta + 2 * tb, (cbpl >> b8) & 1);
        }
        const int ca = cbpa >> 4, cb = cbpb >> 4;
        jmc_bin(s, JMR_CTX(77) + (ca != 0) + 2 * (cb != 0), cbpc != 0);
        if (cbpc) jmc_bin(s, JMR_CTX(81) + (ca == 2) + 2 * (cb == 2), cbpc == 2);
    }
    if (!intra && cbpl && p->t8mode && (mbt != JMH_P8x8 || jmc_all8x8(r))) jmc_bin(s, JMR_CTX(399) + t8a + t8b, r->transform_8x8 != 0);
    if (cbp > 0 || is_i16) jmc_bin(s, JMR_CTX(60), 0); /* mb_qp_delta = 0 */
}

/* one unit of macroblock a (header comment) */
JMR_FN void jmc_unit(jmc_sink *s, const jmw_pic *p, const jmw_slice *sl, int a, int unit) {
    const jmh_mb_result *r = p->res + a;
    const int sp = sl->slice_p, mx = a % p->mbw, my = a / p->mbw;
    const int last_mb = a == sl->end_mb - 1;
    const jmh_mb_result *A = jmw_mb_ok(p, sl, a, mx - 1, my) ? r - 1 : 0, *B = jmw_mb_ok(p, sl, a, mx, my - 1) ? r - p->mbw : 0;
    const int skip = jmw_is_skip(r, sp);
    if (unit == 0) {
        if (a > sl->first_mb) jmc_term(s, 0);         /* end_of_slice_flag of the previous macroblock */
        if (sp) jmc_bin(s, JMR_CTX(11) + (A && jmc_kind(A, sp) != JMR_K_SKIP) + (B && jmc_kind(B, sp) != JMR_K_SKIP), skip);
        if (!skip) jmc_header(s, p, sl, a, A, B);
        return;
    }
    const int is_i16 = r->mb_type == JMH_I16MB, intra = jmw_is_intra(r, sp), cbpl = r->cbp & 15, cbpc = r->cbp >> 4;
    if (!skip && (r->cbp > 0 || is_i16)) {
        if (unit == 1) {
            if (is_i16) jmc_residual(s, r->luma_dc, 16, 0, jmc_i16dc_term(A, sp) + 2 * jmc_i16dc_term(B, sp));
        } else if (unit < 18) {
            const int blk = unit - 2, b8 = blk >> 2;
            const int x4 = (b8 & 1) * 2 + (blk & 1), y4 = (b8 >> 1) * 2 + ((blk >> 1) & 1);
            if (cbpl & (1 << b8)) {
                if (jmc_t8(p, r, sp)) {               /* 8x8 block (cat 5), flag inferred 1 */
                    if (!(blk & 3)) {
                        int16_t lv[64];
                        for (int j = 0; j < 4; j++) {
                            const int16_t *q = r->luma[(y4 + (j >> 1)) * 4 + x4 + (j & 1)];
                            for (int k = 0; k < 16; k++) lv[4 * k + j] = q[k];
                        }
                        jmc_residual(s, lv, 64, 5, -1);
                    }
                } else {
                    const int ta = x4 ? jmc_cbf_luma(p, r, sp, x4 - 1, y4) : jmc_luma_term(p, A, sp, intra, 3, y4);
                    const int tb = y4 ? jmc_cbf_luma(p, r, sp, x4, y4 - 1) : jmc_luma_term(p, B, sp, intra, x4, 3);
                    if (is_i16) jmc_residual(s, r->luma[y4 * 4 + x4] + 1, 15, 1, ta + 2 * tb);
                    else jmc_residual(s, r->luma[y4 * 4 + x4], 16, 2, ta + 2 * tb);
                }
            }
        } else if (unit < 20) {
            const int uv = unit - 18;
            if (cbpc) jmc_residual(s, r->chroma_dc[uv], 4, 3, jmc_cdc_term(A, sp, intra, uv) + 2 * jmc_cdc_term(B, sp, intra, uv));
        } else if (cbpc == 2) {
            const int uv = (unit - 20) >> 2, k = (unit - 20) & 3;
            const int ta = (k & 1) ? jmc_cac_flag(r, uv, k - 1) : jmc_cac_term(A, sp, intra, uv, k + 1);
            const int tb = (k >> 1) ? jmc_cac_flag(r, uv, k - 2) : jmc_cac_term(B, sp, intra, uv, k + 2);
            jmc_residual(s, r->chroma_ac[uv][k] + 1, 15, 4, ta + 2 * tb);
        }
    }
    if (unit == JMW_UNITS - 1 && last_mb) jmc_term(s, 1);   /* end_of_slice_flag 1 */
}

/* ---- the arithmetic encoder (9.3.4.2 .. 9.3.4.5) with byte output ------------------------------
 * low holds codILow with its carry and the bits not yet sent above it: bit 9 + k of low is the bit
 * PutBit would be given k renormalisation steps ago.  left counts the shifts until the next byte
 * is whole (23 at the start: 8 bits behind the dropped first one).  A whole byte is not sent at
 * once: a later carry may still increment it, and ripple through any 0xff bytes behind it.  So one
 * byte (held) is kept back with the number of 0xff bytes that followed it (nheld counts both); they
 * leave when a byte other than 0xff arrives and settles the carry.  That is PutBit's outstanding
 * count in bytes: a run of 8 or more outstanding bits is a held 0xff.
 * Bytes leave through JMC_EMIT (a kernel stages them in LDS). */
typedef struct jmc_enc {
    uint32_t low, range;
    int32_t left;
    uint32_t held, nheld;
    uint8_t *st;                   /* JMR_NCTX contexts, state << 1 | valMPS */
    const uint8_t *lps, *tlps;     /* Table 9-44: rangeTabLPS [64][4] flat, transIdxLPS */
#ifdef JMC_ENC_EXTRA
    JMC_ENC_EXTRA                  /* a kernel's own home of the contexts and the table (JMC_CTX_GET ..) */
#endif
    uint8_t *out;                  /* byte sink */
    uint32_t nbytes, cap;
    void *spill;                   /* a kernel's: where full stages go */
} jmc_enc;

#ifndef JMC_EMIT
#define JMC_EMIT(e, b) jmc_emit_plain((e), (b))
#endif
/* where the contexts and Table 9-44 live: plain arrays, unless a kernel keeps them elsewhere (a bin
   is a dependent chain context -> rangeTabLPS -> context: k_cabac_code keeps both in registers) */
#ifndef JMC_CTX_GET
#define JMC_CTX_GET(e, i) ((uint32_t)(e)->st[i])
#define JMC_CTX_SET(e, i, v) ((e)->st[i] = (uint8_t)(v))
#define JMC_LPS_GET(e, s, q) ((uint32_t)(e)->lps[(s) * 4 + (q)])
#define JMC_TLPS_GET(e, s) ((int)(e)->tlps[s])
#endif
JMR_FN void jmc_emit_plain(jmc_enc *e, uint32_t b) {
    if (e->nbytes < e->cap) e->out[e->nbytes] = (uint8_t)b;
    e->nbytes++;
}

JMR_FN void jmc_enc_start(jmc_enc *e) {               /* 9.3.4.1 */
    e->low = 0; e->range = 510; e->left = 23;
    e->held = 0xff; e->nheld = 0;
    e->nbytes = 0;
}
JMR_FN void jmc_byte_out(jmc_enc *e) {
    const uint32_t lead = e->low >> (24 - e->left);   /* 8 bits and the carry above them */
    e->left += 8;
    e->low &= 0xffffffffu >> e->left;
    if (lead == 0xff) { e->nheld++; return; }
    if (e->nheld > 0) {
        const uint32_t carry = lead >> 8;
        JMC_EMIT(e, (e->held + carry) & 0xff);
        const uint32_t fill = (0xff + carry) & 0xff;
        for (; e->nheld > 1; e->nheld--) JMC_EMIT(e, fill);
    }
    e->nheld = 1;
    e->held = lead & 0xff;
}
JMR_FN void jmc_enc_bin(jmc_enc *e, int ctx, int bin) {   /* 9.3.4.2, branch-free up to the byte output */
    const uint32_t v = JMC_CTX_GET(e, ctx);
    const int s = (int)(v >> 1), mps = (int)(v & 1);
    const uint32_t lps = JMC_LPS_GET(e, s, (e->range >> 6) & 3);
    const int tl = JMC_TLPS_GET(e, s);
    const int lpsbin = bin != mps;
    const uint32_t rm = e->range - lps;
    const uint32_t r = lpsbin ? lps : rm;
    const int ns = lpsbin ? tl : (s < 62 ? s + 1 : s);
    const int nm = mps ^ (lpsbin & (s == 0));
    JMC_CTX_SET(e, ctx, (ns << 1) | nm);
    const int n = jmr_renorm_steps(r);
    e->low = (e->low + (lpsbin ? rm : 0u)) << n;
    e->range = r << n;
    e->left -= n;
    if (e->left < 12) jmc_byte_out(e);
}
JMR_FN void jmc_enc_bypass(jmc_enc *e, int bin) {         /* 9.3.4.4 */
    e->low = (e->low << 1) + (bin ? e->range : 0u);
    e->left--;
    if (e->left < 12) jmc_byte_out(e);
}
JMR_FN void jmc_enc_term(jmc_enc *e, int bin) {           /* 9.3.4.5; bin 1: EncodeFlush follows (jmc_enc_finish) */
    const uint32_t r = e->range - 2;
    const int n = bin ? 7 : jmr_renorm_steps(r);
    e->low = (e->low + (bin ? r : 0u)) << n;
    e->range = bin ? 256u : r << n;
    e->left -= n;
    if (e->left < 12) jmc_byte_out(e);
}
JMR_FN void jmc_enc_rec(jmc_enc *e, uint32_t rec) {
    const int bin = (int)JMC_VAL(rec);
    if (rec & JMC_TERM) jmc_enc_term(e, bin);
    else if (rec & JMC_BYPASS) jmc_enc_bypass(e, bin);
    else jmc_enc_bin(e, (int)(rec & 0x1ff), bin);
}
/* EncodeFlush after end_of_slice_flag 1: the held bytes, the bits left in low down to codILow's bit
   8, the rbsp_stop_one_bit (codILow's bit 7 | 1) and the alignment zeros.  Returns the bytes. */
JMR_FN uint32_t jmc_enc_finish(jmc_enc *e) {
    if (e->low >> (32 - e->left)) {
        JMC_EMIT(e, (e->held + 1) & 0xff);
        for (; e->nheld > 1; e->nheld--) JMC_EMIT(e, 0x00);
        e->low -= 1u << (32 - e->left);
    } else {
        if (e->nheld > 0) JMC_EMIT(e, e->held);
        for (; e->nheld > 1; e->nheld--) JMC_EMIT(e, 0xff);
    }
    e->nheld = 0;
    int nb = 24 - e->left + 1;                            /* <= 20 */
    uint32_t v = (((e->low >> 8) & ((1u << (nb - 1)) - 1u)) << 1) | 1u;
    const int pad = (8 - (nb & 7)) & 7;
    v <<= pad;
    for (nb += pad; nb > 0; nb -= 8) JMC_EMIT(e, (v >> (nb - 8)) & 0xff);
    return e->nbytes;
}

#endif
