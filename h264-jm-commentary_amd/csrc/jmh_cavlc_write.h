/*
 * jmh_cavlc_write.h -- the code-value half of CAVLC: everything host/bitstream.c › write_mb /
 * write_residual_block / put_mvd / calc_nc / jm_w_mpm / jm_w_mvp emit for one macroblock, as
 * (value, length) pairs put into a bit sink.  jmh_cavlc_rate.h holds the code lengths (shared with
 * the RD kernels); the code values of the same tables (H.264 Tables 9-5, 9-7 .. 9-10) are below.
 *
 * No coder state: nC, the MVPs, the Intra4x4 / 8x8 most-probable mode and mb_skip_run depend only
 * on final per-macroblock results of the same slice, so the neighbour state is read from the
 * picture's jmh_mb_result array (not from a sequential writer context):
 *   - a neighbour macroblock is available iff it lies inside the picture and its address lies in
 *     [slice first_mb, current);
 *   - a P_Skip neighbour contributes its mv, ref 0 and TotalCoeff 0; an intra one ref -1 and mv 0;
 *   - the TotalCoeff of a neighbour's 4x4 block is recounted from its levels under the cbp / I16
 *     rules write_mb applies when it fills tc[24] (jmw_tc).
 *
 * A macroblock is cut into JMW_UNITS independent units (jmw_unit), so that a wave can give every
 * unit a lane: unit 0 is the header syntax (mb_skip_run .. mb_qp_delta), 1 the Intra16x16 DC block,
 * 2..17 the luma 4x4 blocks in coding order, 18 / 19 the chroma DC blocks, 20..27 the chroma AC
 * blocks.  The units' bits concatenated in unit order are the macroblock's bits.
 *
 * Worst case of one macroblock for arbitrary int16_t levels and motion vectors (JMW_MB_MAX_BITS):
 *   - a level costs at most 36 bits: levelCode <= 2 * 32768 - 1, the escape of 9.2.2.1 as
 *     bitstream.c writes it reaches level_prefix 19 (19 zeros, a one, 16 suffix bits); below the
 *     escape a level costs at most 15 + 6 bits;
 *   - a 16-coefficient block: coeff_token <= 16, 16 levels, no total_zeros: 16 + 16 * 36 = 592;
 *     a 15-coefficient block (I16 AC, chroma AC): 16 + 15 * 36 = 556 (a block that is not full
 *     trades a 36-bit level for total_zeros <= 9 and run_before <= 11 bits: less);
 *     a chroma DC block: 8 + 4 * 36 = 152;
 *   - residual: max(I16: 592 + 16 * 556, else 16 * 592) + 2 * 152 + 8 * 556 = 9488 + 304 + 4448
 *     = 14240 (I16), 14224 (other);
 *   - header: mb_skip_run ue(v) <= 63, then inter at most mb_type 5 + four sub_mb_type 5 each +
 *     16 mvd pairs (|mvd| <= 65535: se(v) <= 33 bits) 1056 + me(v) 11 + transform flag 1 +
 *     mb_qp_delta 1 = 1157; intra at most 63 + 9 + 1 + 16 * 4 + 5 + 11 + 1 = 154;
 *   - in all 1157 + 14224 = 15381 bits, and one more for the slice's rbsp_stop_one_bit: under
 *     JMW_MB_MAX_BITS = 15424 (1928 bytes).
 *
 * Written in the common subset of C99 and HIP C++ (csrc/jmh_cavlc.hip and the host: the test
 * program tests/harness/cavlc_core_check.c packs the units serially and compares with bitstream.c).
 */
#ifndef JMH_CAVLC_WRITE_H
#define JMH_CAVLC_WRITE_H

#include <stdint.h>
#include "jmh_cavlc_rate.h"

#define JMW_UNITS 28
#define JMW_MB_MAX_BITS 15424

/* ---- code values (the lengths are jmv_ct, jmv_ctdc, jmv_tz, jmv_tzdc, jmv_rb) ---------------- */
JMV_TABLE uint8_t jmw_ct[3][4][17] = {
    {{1, 5, 7, 7, 7, 7, 15, 11, 8, 15, 11, 15, 11, 15, 11, 7, 4}, {0, 1, 4, 6, 6, 6, 6, 14, 10, 14, 10, 14, 10, 1, 14, 10, 6},
     {0, 0, 1, 5, 5, 5, 5, 5, 13, 9, 13, 9, 13, 9, 13, 9, 5}, {0, 0, 0, 3, 3, 4, 4, 4, 4, 4, 12, 12, 8, 12, 8, 12, 8}},
    {{3, 11, 7, 7, 7, 4, 7, 15, 11, 15, 11, 8, 15, 11, 7, 9, 7}, {0, 2, 7, 10, 6, 6, 6, 6, 14, 10, 14, 10, 14, 10, 11, 8, 6},
     {0, 0, 3, 9, 5, 5, 5, 5, 13, 9, 13, 9, 13, 9, 6, 10, 5}, {0, 0, 0, 5, 4, 6, 8, 4, 4, 4, 12, 8, 12, 12, 8, 1, 4}},
    {{15, 15, 11, 8, 15, 11, 9, 8, 15, 11, 15, 11, 8, 13, 9, 5, 1}, {0, 14, 15, 12, 10, 8, 14, 10, 14, 14, 10, 14, 10, 7, 12, 8, 4},
     {0, 0, 13, 14, 11, 9, 13, 9, 13, 10, 13, 9, 13, 9, 11, 7, 3}, {0, 0, 0, 12, 11, 10, 9, 8, 13, 12, 12, 12, 8, 12, 10, 6, 2}}};
JMV_TABLE uint8_t jmw_ctdc[4][5] = {{1, 7, 4, 3, 2}, {0, 1, 6, 3, 3}, {0, 0, 1, 2, 2}, {0, 0, 0, 5, 0}};
JMV_TABLE uint8_t jmw_tz[15][16] = {
    {1, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 1}, {7, 6, 5, 4, 3, 5, 4, 3, 2, 3, 2, 3, 2, 1, 0}, {5, 7, 6, 5, 4, 3, 4, 3, 2, 3, 2, 1, 1, 0},
    {3, 7, 5, 4, 6, 5, 4, 3, 3, 2, 2, 1, 0}, {5, 4, 3, 7, 6, 5, 4, 3, 2, 1, 1, 0}, {1, 1, 7, 6, 5, 4, 3, 2, 1, 1, 0},
    {1, 1, 5, 4, 3, 3, 2, 1, 1, 0}, {1, 1, 1, 3, 3, 2, 2, 1, 0}, {1, 0, 1, 3, 2, 1, 1, 1}, {1, 0, 1, 3, 2, 1, 1}, {0, 1, 1, 2, 1, 3},
    {0, 1, 1, 1, 1}, {0, 1, 1, 1}, {0, 1, 1}, {0, 1}};
JMV_TABLE uint8_t jmw_tzdc[3][4] = {{1, 1, 1, 0}, {1, 1, 0, 0}, {1, 0, 0, 0}};
JMV_TABLE uint8_t jmw_rb[7][15] = {{1, 0}, {1, 1, 0}, {3, 2, 1, 0}, {3, 2, 1, 1, 0}, {3, 2, 3, 2, 1, 0}, {3, 0, 1, 3, 2, 5, 4},
                                   {7, 6, 5, 4, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1}};

/* ---- bit sink ----------------------------------------------------------------------------------
 * w == NULL: only counts.  Otherwise bit pos of the stream is bit 31 - (pos & 31) of w[pos >> 5]
 * (MSB first, as jm_put produces bytes once every word is stored big endian); words are OR-ed into
 * (zeroed by the caller), so that units which share a word can be written in any order. */
#ifndef JMW_OR
#define JMW_OR(p, v) (*(p) |= (v))
#endif
typedef struct jmw_sink {
    uint32_t *w;
    uint32_t pos;
} jmw_sink;

JMV_FN void jmw_put(jmw_sink *s, uint32_t val, int n) {   /* the low n bits of val, 0 <= n <= 32 */
    if (n > 0 && s->w) {
        const uint64_t v = ((uint64_t)val << (64 - n)) >> (s->pos & 31);
        JMW_OR(&s->w[s->pos >> 5], (uint32_t)(v >> 32));
        if ((uint32_t)v) JMW_OR(&s->w[(s->pos >> 5) + 1], (uint32_t)v);
    }
    s->pos += (uint32_t)n;
}
JMV_FN void jmw_ue(jmw_sink *s, uint32_t v) {
    const uint32_t x = v + 1;
    const int len = 31 - __builtin_clz(x);
    jmw_put(s, 0, len);
    jmw_put(s, x, len + 1);
}
JMV_FN void jmw_se(jmw_sink *s, int v) { jmw_ue(s, v > 0 ? (uint32_t)(2 * v - 1) : (uint32_t)(-2 * v)); }

/* ---- the picture and the slice a macroblock is written in ------------------------------------- */
typedef struct jmw_pic {
    const jmh_mb_result *res;      /* mbw * mbh final results, raster order */
    int mbw, mbh;
    int t8mode, cip;               /* transform_8x8_mode, constrained_intra_pred of the configuration */
} jmw_pic;
typedef struct jmw_slice {
    int first_mb, end_mb;          /* [first_mb, end_mb) */
    int slice_p;
} jmw_slice;

JMV_FN int jmw_is_skip(const jmh_mb_result *r, int slice_p) { return slice_p && r->mb_type == JMH_PSKIP; }
JMV_FN int jmw_is_nxn(const jmh_mb_result *r, int slice_p) {
    return !jmw_is_skip(r, slice_p) && (r->mb_type == JMH_I4MB || r->mb_type == JMH_I8MB);
}
JMV_FN int jmw_is_intra(const jmh_mb_result *r, int slice_p) {
    return !jmw_is_skip(r, slice_p) && (r->mb_type == JMH_I4MB || r->mb_type == JMH_I8MB || r->mb_type == JMH_I16MB);
}

JMV_FN int jmw_nnz(const int16_t *c, int n) {
    int t = 0;
    for (int i = 0; i < n; i++) t += c[i] != 0;
    return t;
}
/* TotalCoeff of a macroblock's 4x4 block as write_mb leaves it in tc[24]: comp 0 luma (x4, y4 in
   0..3), 1 / 2 Cb / Cr AC (0..1) */
JMV_FN int jmw_tc(const jmh_mb_result *r, int slice_p, int comp, int x4, int y4) {
    if (jmw_is_skip(r, slice_p)) return 0;
    if (comp) return (r->cbp >> 4) == 2 ? jmw_nnz(r->chroma_ac[comp - 1][y4 * 2 + x4] + 1, 15) : 0;
    if (!((r->cbp >> ((y4 >> 1) * 2 + (x4 >> 1))) & 1)) return 0;
    return r->mb_type == JMH_I16MB ? jmw_nnz(r->luma[y4 * 4 + x4] + 1, 15) : jmw_nnz(r->luma[y4 * 4 + x4], 16);
}

/* macroblock at (tx, ty) usable as a neighbour of macroblock a (a itself included) */
JMV_FN int jmw_mb_ok(const jmw_pic *p, const jmw_slice *sl, int a, int tx, int ty) {
    if (tx < 0 || ty < 0 || tx >= p->mbw || ty >= p->mbh) return 0;
    const int t = ty * p->mbw + tx;
    return t >= sl->first_mb && t <= a;
}
/* bitstream.c › nb: the 4x4 block covering luma sample (xN, yN) relative to macroblock a; *k its
   raster index inside the macroblock returned (NULL: not available) */
JMV_FN const jmh_mb_result *jmw_nb(const jmw_pic *p, const jmw_slice *sl, int a, int xN, int yN, int *k) {
    const int mx = a % p->mbw, my = a / p->mbw;
    int tx, ty;
    if (yN > 15) return 0;
    if (xN < 0) { tx = mx - 1; ty = yN < 0 ? my - 1 : my; }
    else if (xN <= 15) { tx = mx; ty = yN < 0 ? my - 1 : my; }
    else { if (yN >= 0) return 0; tx = mx + 1; ty = my - 1; }
    if (!jmw_mb_ok(p, sl, a, tx, ty)) return 0;
    *k = (((yN + 16) & 15) >> 2) * 4 + (((xN + 16) & 15) >> 2);
    return p->res + (ty * p->mbw + tx);
}
JMV_FN int jmw_nc(const jmw_pic *p, const jmw_slice *sl, int a, int comp, int x4, int y4) {
    const int mx = a % p->mbw, my = a / p->mbw, lim = comp ? 1 : 3;
    const jmh_mb_result *r = p->res + a;
    int na = -1, nb = -1;
    if (x4 > 0) na = jmw_tc(r, sl->slice_p, comp, x4 - 1, y4);
    else if (mx > 0 && jmw_mb_ok(p, sl, a, mx - 1, my)) na = jmw_tc(r - 1, sl->slice_p, comp, lim, y4);
    if (y4 > 0) nb = jmw_tc(r, sl->slice_p, comp, x4, y4 - 1);
    else if (jmw_mb_ok(p, sl, a, mx, my - 1)) nb = jmw_tc(r - p->mbw, sl->slice_p, comp, x4, lim);
    return na >= 0 && nb >= 0 ? (na + nb + 1) >> 1 : na >= 0 ? na : nb >= 0 ? nb : 0;
}

/* residual_block_cavlc (7.3.5.3.2 / 9.2) as bitstream.c › write_residual_block: coef[0..n) in scan
   order, nC -1: chroma DC.  The non-zero positions come from one bit mask (as jmv_block) */
JMV_FN void jmw_block(jmw_sink *s, const int16_t *coef, int n, int nC) {
    uint32_t nzm = 0;
    for (int i = 0; i < n; i++)
        if (coef[i]) nzm |= 1u << i;
    const int tc = __builtin_popcount(nzm);
    int t1 = 0;
    {
        uint32_t m = nzm;
        while (t1 < 3 && m) {
            const int i = 31 - __builtin_clz(m);
            if (coef[i] != 1 && coef[i] != -1) break;
            m &= ~(1u << i);
            t1++;
        }
    }
    if (nC == -1) jmw_put(s, jmw_ctdc[t1][tc], jmv_ctdc[t1][tc]);
    else if (nC >= 8) jmw_put(s, tc == 0 ? 3u : (uint32_t)(((tc - 1) << 2) | t1), 6);
    else {
        const int t = nC < 2 ? 0 : nC < 4 ? 1 : 2;
        jmw_put(s, jmw_ct[t][t1][tc], jmv_ct[t][t1][tc]);
    }
    if (!tc) return;
    int sl = tc > 10 && t1 < 3;
    uint32_t m = nzm;
    for (int k = 0; k < tc; k++) {
        const int i = 31 - __builtin_clz(m);
        m &= ~(1u << i);
        const int v = coef[i], a = v < 0 ? -v : v;
        if (k < t1) { jmw_put(s, v < 0, 1); continue; }
        int code = 2 * a - 2 + (v < 0);                       /* levelCode */
        if (k == t1 && t1 < 3) code -= 2;
        if (sl == 0 && code < 14) jmw_put(s, 1, code + 1);
        else if (sl == 0 && code < 30) { jmw_put(s, 1, 15); jmw_put(s, (uint32_t)(code - 14), 4); }
        else if (sl > 0 && code < (15 << sl)) { jmw_put(s, 1, (code >> sl) + 1); jmw_put(s, (uint32_t)(code & ((1 << sl) - 1)), sl); }
        else {                                                /* level_prefix >= 15, as bitstream.c */
            int rest = code - (sl == 0 ? 30 : 15 << sl), prefix = 15;
            while (rest >= (1 << (prefix - 3))) { rest -= 1 << (prefix - 3); prefix++; }
            jmw_put(s, 0, prefix); jmw_put(s, 1, 1); jmw_put(s, (uint32_t)rest, prefix - 3);
        }
        if (sl == 0) sl = 1;
        if (a > (3 << (sl - 1)) && sl < 6) sl++;
    }
    const int last = 31 - __builtin_clz(nzm), tz = last + 1 - tc;
    if (tc < n) {
        if (nC == -1) jmw_put(s, jmw_tzdc[tc - 1][tz], jmv_tzdc[tc - 1][tz]);
        else jmw_put(s, jmw_tz[tc - 1][tz], jmv_tz[tc - 1][tz]);
    }
    int zl = tz, prev = last;
    m = nzm & ~(1u << last);
    while (zl > 0 && m) {                                     /* run_before of all but the lowest one */
        const int i = 31 - __builtin_clz(m);
        const int run = prev - i - 1, t = zl > 6 ? 6 : zl - 1;
        jmw_put(s, jmw_rb[t][run], jmv_rb[t][run]);
        zl -= run;
        prev = i;
        m &= ~(1u << i);
    }
}

/* what bitstream.c › jm_w_mark_mb leaves for a 4x4 block: ref (-1 intra, else 0), mv (0 intra) */
JMV_FN int jmw_ref(const jmh_mb_result *r, int slice_p) { return jmw_is_intra(r, slice_p) ? -1 : 0; }

/* normative MVP (8.4.1.3) of the partition at (bx, by) size bw x bh of macroblock a: jm_w_mvp */
JMV_FN void jmw_mvp(const jmw_pic *p, const jmw_slice *sl, int a, int bx, int by, int bw, int bh, int *out) {
    int ka = 0, kb = 0, kc = 0, kd = 0;
    const jmh_mb_result *A = jmw_nb(p, sl, a, bx - 1, by, &ka), *B = jmw_nb(p, sl, a, bx, by - 1, &kb);
    const jmh_mb_result *C = jmw_nb(p, sl, a, bx + bw, by - 1, &kc), *D = jmw_nb(p, sl, a, bx - 1, by - 1, &kd);
    if (by > 0) {                         /* C inside the MB, not yet decoded */
        if (bx < 8) { if (by == 8) { if (bw == 16) C = 0; } else if (bx + bw == 8) C = 0; }
        else if (bx + bw == 16) C = 0;
    }
    if (!C) { C = D; kc = kd; }
    const int sp = sl->slice_p;
    const int rA = A ? jmw_ref(A, sp) : -1, rB = B ? jmw_ref(B, sp) : -1, rC = C ? jmw_ref(C, sp) : -1;
    int type = 0;
    if (rA == 0 && rB != 0 && rC != 0) type = 1;
    else if (rA != 0 && rB == 0 && rC != 0) type = 2;
    else if (rA != 0 && rB != 0 && rC == 0) type = 3;
    if (bw == 8 && bh == 16) { if (bx == 0) { if (rA == 0) type = 1; } else if (rC == 0) type = 3; }
    else if (bw == 16 && bh == 8) { if (by == 0) { if (rB == 0) type = 2; } else if (rA == 0) type = 1; }
    for (int hv = 0; hv < 2; hv++) {
        const int va = A && rA == 0 ? A->mv[ka][hv] : 0, vb = B && rB == 0 ? B->mv[kb][hv] : 0, vc = C && rC == 0 ? C->mv[kc][hv] : 0;
        int v;
        if (type == 1) v = va;
        else if (type == 2) v = vb;
        else if (type == 3) v = vc;
        else if (!B && !C) v = va;
        else {
            int mn = va < vb ? va : vb, mxv = va > vb ? va : vb;
            mn = mn < vc ? mn : vc;
            mxv = mxv > vc ? mxv : vc;
            v = va + vb + vc - mn - mxv;
        }
        out[hv] = v;
    }
}
JMV_FN void jmw_mvd(jmw_sink *s, const jmw_pic *p, const jmw_slice *sl, int a, int bx, int by, int bw, int bh) {
    int pr[2];
    jmw_mvp(p, sl, a, bx, by, bw, bh, pr);
    const jmh_mb_result *r = p->res + a;
    const int k = (by >> 2) * 4 + (bx >> 2);
    jmw_se(s, r->mv[k][0] - pr[0]);
    jmw_se(s, r->mv[k][1] - pr[1]);
}

/* predIntra4x4PredMode / predIntra8x8PredMode: jm_w_mpm */
JMV_FN int jmw_mpm(const jmw_pic *p, const jmw_slice *sl, int a, int x4, int y4) {
    int ka = 0, kb = 0;
    const jmh_mb_result *A = jmw_nb(p, sl, a, 4 * x4 - 1, 4 * y4, &ka), *B = jmw_nb(p, sl, a, 4 * x4, 4 * y4 - 1, &kb);
    if (!A || !B) return 2;
    const int sp = sl->slice_p;
    if (p->cip && (jmw_ref(A, sp) >= 0 || jmw_ref(B, sp) >= 0)) return 2;
    const int ma = jmw_is_nxn(A, sp) && A->ipred[ka] >= 0 ? A->ipred[ka] : 2;
    const int mb = jmw_is_nxn(B, sp) && B->ipred[kb] >= 0 ? B->ipred[kb] : 2;
    return ma < mb ? ma : mb;
}

/* unit 0: mb_skip_run (P slices; skip_run = P_Skip macroblocks of the slice right before a) and
   macroblock_layer up to mb_qp_delta */
JMV_FN void jmw_header(jmw_sink *s, const jmw_pic *p, const jmw_slice *sl, int a, int skip_run) {
    const jmh_mb_result *r = p->res + a;
    const int mbt = r->mb_type, cbp = r->cbp, slice_p = sl->slice_p;
    const int is_i8 = mbt == JMH_I8MB, is_i4 = mbt == JMH_I4MB || is_i8, is_i16 = mbt == JMH_I16MB;
    const int is_intra = is_i4 || is_i16, cbpl = cbp & 15, cbpc = cbp >> 4;
    if (slice_p) jmw_ue(s, (uint32_t)skip_run);
    int ue_type;
    if (is_i16) {
        const int t = 1 + r->i16mode + 4 * cbpc + (cbpl ? 12 : 0);
        ue_type = slice_p ? 5 + t : t;
    } else if (is_i4) ue_type = slice_p ? 5 : 0;
    else if (mbt == JMH_P8x8) ue_type = 3;
    else ue_type = mbt - 1;
    jmw_ue(s, (uint32_t)ue_type);
    if (mbt == JMH_P8x8)
        for (int i = 0; i < 4; i++) jmw_ue(s, (uint32_t)(r->b8mode[i] - 4));
    if (is_i4 && p->t8mode) jmw_put(s, (uint32_t)is_i8, 1);   /* transform_size_8x8_flag */
    if (is_i4)
        for (int blk = 0; blk < 16; blk += is_i8 ? 4 : 1) {
            const int x4 = ((blk >> 2) & 1) * 2 + (blk & 1), y4 = (blk >> 3) * 2 + ((blk >> 1) & 1);
            const int pred = jmw_mpm(p, sl, a, x4, y4), m = r->ipred[y4 * 4 + x4];
            if (m == pred) jmw_put(s, 1, 1);
            else { jmw_put(s, 0, 1); jmw_put(s, (uint32_t)(m < pred ? m : m - 1), 3); }
        }
    if (is_intra) jmw_ue(s, (uint32_t)r->c_ipred_mode);
    else if (mbt == JMH_P16x16) jmw_mvd(s, p, sl, a, 0, 0, 16, 16);
    else if (mbt == JMH_P16x8) { jmw_mvd(s, p, sl, a, 0, 0, 16, 8); jmw_mvd(s, p, sl, a, 0, 8, 16, 8); }
    else if (mbt == JMH_P8x16) { jmw_mvd(s, p, sl, a, 0, 0, 8, 16); jmw_mvd(s, p, sl, a, 8, 0, 8, 16); }
    else
        for (int i = 0; i < 4; i++) {
            const int ox = (i & 1) * 8, oy = (i >> 1) * 8, sm = r->b8mode[i];
            const int sw = (sm == 4 || sm == 5) ? 8 : 4, sh = (sm == 4 || sm == 6) ? 8 : 4;
            for (int y = 0; y < 8; y += sh)
                for (int x = 0; x < 8; x += sw) jmw_mvd(s, p, sl, a, ox + x, oy + y, sw, sh);
        }
    if (!is_i16) jmw_ue(s, is_i4 ? jmv_cbp_i[cbp] : jmv_cbp_p[cbp]);
    /* transform_size_8x8_flag of inter MBs: luma coded, no sub-8x8 partitions (7.3.5) */
    if (!is_intra && cbpl && p->t8mode &&
        (mbt != JMH_P8x8 || (r->b8mode[0] == 4 && r->b8mode[1] == 4 && r->b8mode[2] == 4 && r->b8mode[3] == 4)))
        jmw_put(s, (uint32_t)r->transform_8x8, 1);
    if (cbp > 0 || is_i16) jmw_se(s, 0);                      /* mb_qp_delta */
}

/* one unit of macroblock a (header comment).  A P_Skip macroblock writes nothing, except as the
   slice's last macroblock: the pending run, itself included, as close_slice_data does; skip_run
   counts the P_Skip macroblocks of the slice right before a */
JMV_FN void jmw_unit(jmw_sink *s, const jmw_pic *p, const jmw_slice *sl, int a, int unit, int skip_run) {
    const jmh_mb_result *r = p->res + a;
    if (jmw_is_skip(r, sl->slice_p)) {
        if (unit == 0 && a == sl->end_mb - 1) jmw_ue(s, (uint32_t)skip_run + 1u);
        return;
    }
    if (unit == 0) { jmw_header(s, p, sl, a, skip_run); return; }
    const int is_i16 = r->mb_type == JMH_I16MB, cbpl = r->cbp & 15, cbpc = r->cbp >> 4;
    if (!(r->cbp > 0 || is_i16)) return;
    if (unit == 1) {
        if (is_i16) jmw_block(s, r->luma_dc, 16, jmw_nc(p, sl, a, 0, 0, 0));
    } else if (unit < 18) {
        const int blk = unit - 2, b8 = blk >> 2;
        const int x4 = (b8 & 1) * 2 + (blk & 1), y4 = (b8 >> 1) * 2 + ((blk >> 1) & 1);
        if (!(cbpl & (1 << b8))) return;
        const int nC = jmw_nc(p, sl, a, 0, x4, y4);
        if (is_i16) jmw_block(s, r->luma[y4 * 4 + x4] + 1, 15, nC);
        else jmw_block(s, r->luma[y4 * 4 + x4], 16, nC);
    } else if (unit < 20) {
        if (cbpc) jmw_block(s, r->chroma_dc[unit - 18], 4, -1);
    } else if (cbpc == 2) {
        const int uv = (unit - 20) >> 2, k = (unit - 20) & 3;
        jmw_block(s, r->chroma_ac[uv][k] + 1, 15, jmw_nc(p, sl, a, 1 + uv, k & 1, k >> 1));
    }
}

#endif
