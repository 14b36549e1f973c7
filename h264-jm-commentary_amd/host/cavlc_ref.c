/*
 * cavlc_ref.c — the host writer (bitstream.c) behind the calling convention of the device CAVLC
 * writer (include/jmhip_cavlc.h: jmh_cavlc_write_results), with flat arguments: the reference the
 * device bytes are compared with, without mirroring jm_seq / jm_slice in a test.
 *
 * bitstream.c is run as it is (jm_slice_begin / jm_slice_write_mb / jm_slice_restart /
 * jm_slice_end, each slice into an RBSP of its own, behind a slice header of this file's choosing);
 * a slice's bits between the end of that header and its rbsp_stop_one_bit are then copied behind
 * the caller's lead bits and closed with rbsp_trailing_bits.  jm_put is a plain bit writer, so the
 * bits written for a macroblock do not depend on where the header ended.
 */
#include <stdlib.h>
#include <string.h>
#include "jmhost.h"

static int get_bit(const jm_bits *b, long i) { return (b->buf[i >> 3] >> (7 - (i & 7))) & 1; }

/* returns 0, JMH_E_INVALID_ARG (descriptors, cap) or JMH_E_OOM; where[n] is filled when the
   descriptors are valid (also when cap is too small; out is then untouched) */
int jm_cavlc_ref(int width, int height, int transform_8x8_mode, int constrained_intra, const jmh_mb_result *res, int n,
                 const jmh_slice_desc *d, uint8_t *out, size_t cap, jmh_slice_bytes *where) {
    if (width <= 0 || height <= 0 || (width & 15) || (height & 15) || !res || n <= 0 || !d || !where) return JMH_E_INVALID_ARG;
    const int mbw = width / 16, mbh = height / 16, nmb = mbw * mbh;
    int next = 0;
    for (int i = 0; i < n; i++) {
        if (d[i].first_mb != next || d[i].n_mb <= 0 || d[i].n_mb > nmb - next) return JMH_E_INVALID_ARG;
        if (d[i].slice_type != JMH_P_SLICE && d[i].slice_type != JMH_I_SLICE) return JMH_E_INVALID_ARG;
        if (d[i].lead_nbits < 0 || d[i].lead_nbits > 7) return JMH_E_INVALID_ARG;
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
    jm_bits *rb = calloc((size_t)n, sizeof(jm_bits));
    long *hdr = calloc((size_t)n, sizeof(long));
    if (!rb || !hdr) { free(rb); free(hdr); return JMH_E_OOM; }
    jm_slice_writer *sw = NULL;
    for (int i = 0; i < n; i++) {
        jm_slice sl;
        memset(&sl, 0, sizeof(sl));
        sl.slice_type = d[i].slice_type;
        sl.qp = 26;
        sl.first_mb = d[i].first_mb;
        if (i == 0) {
            sw = jm_slice_begin(&rb[0], &s, &sl);
            if (!sw) { free(rb); free(hdr); return JMH_E_OOM; }
        } else jm_slice_restart(sw, &rb[i], &sl);
        hdr[i] = 8 * rb[i].len + rb[i].nacc;
        for (int a = d[i].first_mb; a < d[i].first_mb + d[i].n_mb; a++) jm_slice_write_mb(sw, a, &res[a]);
    }
    jm_slice_end(sw);
    int64_t off = 0;
    for (int i = 0; i < n; i++) {
        long stop = 8 * rb[i].len - 1;               /* rbsp_stop_one_bit: the last 1 */
        while (!get_bit(&rb[i], stop)) stop--;
        where[i].nbits = d[i].lead_nbits + (stop - hdr[i]);
        where[i].nbytes = where[i].nbits / 8 + 1;
        where[i].offset = off;
        off += where[i].nbytes;
    }
    int st = JMH_OK;
    if (!out || (size_t)off > cap) st = JMH_E_INVALID_ARG;
    else
        for (int i = 0; i < n; i++) {
            jm_bits b;
            jm_bits_init(&b);
            jm_put(&b, d[i].lead_bits, d[i].lead_nbits);
            const long end = hdr[i] + (where[i].nbits - d[i].lead_nbits);
            for (long k = hdr[i]; k < end; k++) jm_put(&b, (uint32_t)get_bit(&rb[i], k), 1);
            jm_trailing_bits(&b);
            if (b.len != where[i].nbytes) st = JMH_E_STATE;
            else memcpy(out + where[i].offset, b.buf, (size_t)b.len);
            jm_bits_free(&b);
        }
    for (int i = 0; i < n; i++) jm_bits_free(&rb[i]);
    free(rb); free(hdr);
    return st;
}
