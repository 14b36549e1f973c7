/*
 * deblock_ref.c — the host deblocker (deblock.c) behind flat arguments: a reconstructed picture,
 * its macroblock results and the slice's filter parameters, without mirroring jm_pic / jm_seq in
 * a test.  deblock.c is run as it is (jm_deblock_picture, in place on the caller's planes).
 */
#include <stdlib.h>
#include <string.h>
#include "jmhost.h"

/* y, u, v: contiguous planes of 16 mbw x 16 mbh (chroma: half each way), uint8_t at bit depth 8,
   uint16_t at 9 / 10; res[mbw * mbh] in raster order.  disable_deblocking_filter_idc 0.
   Returns 0, JMH_E_INVALID_ARG or JMH_E_OOM */
int jm_deblock_ref(void *y, void *u, void *v, const jmh_mb_result *res, int mbw, int mbh, int qp, int chroma_qp_offset,
                   int alpha_div2, int beta_div2, int bit_depth) {
    if (!y || !u || !v || !res || mbw <= 0 || mbh <= 0 || qp < 0 || qp > 51 || bit_depth < 8 || bit_depth > 10) return JMH_E_INVALID_ARG;
    if (chroma_qp_offset < -12 || chroma_qp_offset > 12 || alpha_div2 < -6 || alpha_div2 > 6 || beta_div2 < -6 || beta_div2 > 6)
        return JMH_E_INVALID_ARG;
    const int n = mbw * mbh;
    const jmh_mb_result **rp = malloc((size_t)n * sizeof(*rp));
    if (!rp) return JMH_E_OOM;
    for (int i = 0; i < n; i++) rp[i] = &res[i];
    jm_seq s;
    memset(&s, 0, sizeof(s));
    s.width = s.disp_w = 16 * mbw; s.height = s.disp_h = 16 * mbh;
    s.mbw = mbw; s.mbh = mbh;
    s.chroma_qp_offset = chroma_qp_offset;
    s.lf_params_flag = 1; s.lf_disable = 0; s.lf_alpha = alpha_div2; s.lf_beta = beta_div2;
    s.bit_depth = bit_depth;
    jm_pic p;
    memset(&p, 0, sizeof(p));
    p.w = s.width; p.h = s.height; p.bd = bit_depth;
    if (bit_depth > 8) { p.Y = y; p.U = u; p.V = v; }
    else { p.y = y; p.u = u; p.v = v; }
    jm_deblock_picture(&p, &s, rp, qp);
    free(rp);
    return JMH_OK;
}
