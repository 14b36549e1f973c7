/*
 * cabac_ref.c — the host CABAC writer (bitstream.c / cabac.c) behind the calling convention of the
 * device CABAC writer (include/jmhip_cabac.h: jmh_cabac_write_results), with flat arguments: the
 * reference the device bytes are compared with, without mirroring jm_seq / jm_slice in a test.
 *
 * bitstream.c and cabac.c are run as they are (jm_slice_begin / jm_slice_write_mb / jm_slice_restart
 * / jm_slice_end with entropy_coding = 1 and sl.qp = slice_qp, each slice into an RBSP of its own,
 * behind a slice header of this file's choosing).  jm_cabac_slice_start pads the header with
 * cabac_alignment_one_bits, so a slice's bytes behind that point are the device's bytes.
 */
#include <stdlib.h>
#include <string.h>
#include "jmhost.h"

static int last_max_outstanding;
int jm_cabac_ref_max_outstanding(void) { return last_max_outstanding; }

/* returns 0, JMH_E_INVALID_ARG (descriptors, cap) or JMH_E_OOM; where[n] is filled when the
   descriptors are valid (also when cap is too small; out is then untouched) */
int jm_cabac_ref(int width, int height, int transform_8x8_mode, int constrained_intra, const jmh_mb_result *res, int n,
                 const jmh_cabac_slice_desc *d, uint8_t *out, size_t cap, jmh_cabac_slice_bytes *where) {
    if (width <= 0 || height <= 0 || (width & 15) || (height & 15) || !res || n <= 0 || !d || !where) return JMH_E_INVALID_ARG;
    const int mbw = width / 16, mbh = height / 16, nmb = mbw * mbh;
    int next = 0;
    for (int i = 0; i < n; i++) {
        if (d[i].first_mb != next || d[i].n_mb <= 0 || d[i].n_mb > nmb - next) return JMH_E_INVALID_ARG;
        if (d[i].slice_type != JMH_P_SLICE && d[i].slice_type != JMH_I_SLICE) return JMH_E_INVALID_ARG;
        if (d[i].slice_qp < 0 || d[i].slice_qp > 51) return JMH_E_INVALID_ARG;
        next += d[i].n_mb;
    }
    if (next != nmb) return JMH_E_INVALID_ARG;
    jm_seq s;
    memset(&s, 0, sizeof(s));
    s.width = s.disp_w = width; s.height = s.disp_h = height;
    s.mbw = mbw; s.mbh = mbh;
    s.profile_idc = transform_8x8_mode ? 100 : 77;
    s.level_idc = 40;
    s.num_ref_frames = 1;
    s.log2_max_frame_num = 4; s.log2_max_poc_lsb = 4;
    s.constrained_intra = constrained_intra;
    s.transform_8x8_mode = transform_8x8_mode;
    s.entropy_coding = 1;
    jm_bits *rb = calloc((size_t)n, sizeof(jm_bits));
    long *hdr = calloc((size_t)n, sizeof(long));
    if (!rb || !hdr) { free(rb); free(hdr); return JMH_E_OOM; }
    jm_slice_writer *sw = NULL;
    long bins = 0;
    for (int i = 0; i < n; i++) {
        jm_slice sl;
        memset(&sl, 0, sizeof(sl));
        sl.slice_type = d[i].slice_type;
        sl.qp = d[i].slice_qp;
        sl.first_mb = d[i].first_mb;
        if (i == 0) {
            sw = jm_slice_begin(&rb[0], &s, &sl);
            if (!sw) { free(rb); free(hdr); return JMH_E_OOM; }
        } else {
            jm_slice_restart(sw, &rb[i], &sl);
            where[i - 1].nbins = jm_slice_bins(sw) - bins;
            bins = jm_slice_bins(sw);
        }
        hdr[i] = rb[i].len;                      /* byte aligned: the header and its alignment bits */
        for (int a = d[i].first_mb; a < d[i].first_mb + d[i].n_mb; a++) jm_slice_write_mb(sw, a, &res[a]);
    }
    last_max_outstanding = jm_slice_max_outstanding(sw);
    where[n - 1].nbins = jm_slice_end(sw) - bins;
    int64_t off = 0;
    for (int i = 0; i < n; i++) {
        where[i].nbytes = rb[i].len - hdr[i];
        where[i].offset = off;
        off += where[i].nbytes;
    }
    int st = JMH_OK;
    if (!out || (size_t)off > cap) st = JMH_E_INVALID_ARG;
    else
        for (int i = 0; i < n; i++) memcpy(out + where[i].offset, rb[i].buf + hdr[i], (size_t)where[i].nbytes);
    for (int i = 0; i < n; i++) jm_bits_free(&rb[i]);
    free(rb); free(hdr);
    return st;
}
