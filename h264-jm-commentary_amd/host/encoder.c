/*
 * encoder.c — sequence / picture driver, restating JM 8.6 lencod.c › main frame loop and
 * image.c › encode_one_frame [J]: read (or synthesise) the picture, choose I/P, run the
 * macroblock hot path through the backend (encode_one_macroblock for every MB), write the
 * slice (CAVLC), deblock the reconstruction, make it the reference (UnifiedOneForthPix runs in
 * the backend), write the recon, print JM's per-frame report line.
 */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "jmhost.h"

static double now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

int jm_lambda_rdo_off(int qp) {
    static const int QP2QUANT[40] = {1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4,
                                     5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 23,
                                     25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91};
    int i = qp - 12;
    return QP2QUANT[i < 0 ? 0 : i];
}

/* RDOptimization 1 (rdopt.c encode_one_macroblock [J], no B pictures): lambda_mode = 0.85 *
   2^((QP - SHIFT_QP) / 3) at QP + QpBdOffsetY (JM >= 13 init_lambda's bitdepth_luma_qp_scale),
   lambda_motion = sqrt(lambda_mode), LAMBDA_FACTOR = (int)(65536 * lambda_motion + 0.5) */
double jm_lambda_rdo_on(int qp, int bit_depth, int *lambda_factor) {
    const int qpbd = bit_depth > 8 ? 6 * (bit_depth - 8) : 0;
    const double lam = 0.85 * pow(2.0, (double)(qp + qpbd - 12) / 3.0);
    if (lambda_factor) *lambda_factor = (int)(65536.0 * sqrt(lam) + 0.5);
    return lam;
}

/* squared error summed in integers (per row in 32 bits: 65025 * w < 2^32 for w < 66051; 64-bit
   rows at High 10), so the value equals JM's double accumulation of integer squares exactly; the
   peak is (1 << bit depth) - 1 (JM >= 10 img->max_imgpel_value [J]) */
double jm_psnr_from_ssd(uint64_t se, int w, int h, int bit_depth) {
    if (se == 0) return 99.0;
    const double peak = bit_depth > 8 ? (double)((1 << bit_depth) - 1) : 255.0;
    return 10.0 * log10(peak * peak * w * h / (double)se);
}
static double psnr_pl(const jm_pic *a, const jm_pic *b, int pl, int w, int h) {
    uint64_t se = 0;
    const int st = pl ? a->w / 2 : a->w;
    const size_t off = pl == 0 ? 0 : (size_t)a->w * a->h + (size_t)(pl - 1) * (a->w / 2) * (a->h / 2);
    for (int y = 0; y < h; y++) {
        uint64_t r = 0;
        if (a->bd > 8) {
            const uint16_t *pa = a->Y + off + (size_t)y * st, *pb = b->Y + off + (size_t)y * st;
            for (int x = 0; x < w; x++) { const int d = pa[x] - pb[x]; r += (uint64_t)(d * d); }
        } else {
            const uint8_t *pa = a->y + off + (size_t)y * st, *pb = b->y + off + (size_t)y * st;
            uint32_t r32 = 0;
            for (int x = 0; x < w; x++) { const int d = pa[x] - pb[x]; r32 += (uint32_t)(d * d); }
            r = r32;
        }
        se += r;
    }
    return jm_psnr_from_ssd(se, w, h, a->bd);
}

/* slice.c › encode_one_slice [J]: the macroblock loop of one slice through the JM 8.6 call
 * surface (host/jm86.c): start_macroblock, encode_one_macroblock, write_one_macroblock.
 * image.c › code_a_picture [J] runs it for every slice of the picture (SliceMode 1: SliceArgument
 * MBs each, raster order); each slice is its own NAL unit, appended to out.  One slice writer
 * serves the picture (jm_slice_restart between slices). */
static void encode_one_slice(const jm_seq *s, int first) {
    const int nmb = s->mbw * s->mbh, end = s->slice_mbs > 0 && first + s->slice_mbs < nmb ? first + s->slice_mbs : nmb;
    img->slice_first = first;
    for (int a = first; a < end; a++) {
        img->current_mb_nr = a;
        start_macroblock();
        encode_one_macroblock();
        write_one_macroblock();
    }
}
static int encode_picture_slices(jm86_img *im, const jm_seq *s, const jm_slice *sl0, const jmh_frame_params *fp,
                                 const jm_pic *cur, const jm_pic *ref, jm_bits *out) {
    const int nmb = s->mbw * s->mbh, step = s->slice_mbs > 0 ? s->slice_mbs : nmb;
    const long len0 = out->len;
    jm_slice sl = *sl0;
    sl.first_mb = 0;
    jm_bits rbsp[2];             /* the slice being written and the next one (alternating) */
    int k = 0, nslices = 0;
    long bins = 0;
    jm_bits_init(&rbsp[0]);
    jm_slice_writer *w = jm_slice_begin(&rbsp[0], s, &sl);
    if (!w) { jm_bits_free(&rbsp[0]); return JMH_E_OOM; }
    int r = jm86_start_picture(im, fp, cur, ref, w);
    if (r) { jm_slice_end(w); jm_bits_free(&rbsp[0]); return r; }
    for (int first = 0; first < nmb; first += step) {
        encode_one_slice(s, first);
        if (first + step >= nmb) {
            long chk, bad;
            jm_slice_rate_check(w, &chk, &bad);
            im->rate_checked += chk;
            im->rate_mismatches += bad;
            bins = jm_slice_end(w);
        } else {
            jm_bits_init(&rbsp[k ^ 1]);
            sl.first_mb = first + step;
            jm_slice_restart(w, &rbsp[k ^ 1], &sl);
        }
        jm_write_nal(out, sl0->idr ? 3 : 2, sl0->idr ? 5 : 1, &rbsp[k]);
        jm_bits_free(&rbsp[k]);
        nslices++;
        k ^= 1;
    }
    im->writer = NULL;
    if (s->entropy_coding) {
        /* cabac_zero_words (7.4.2.10, 9.3.4.6): BinCountsInNALunits <= 32/3 * NumBytesInVclNALunits
           + RawMbBits * PicSizeInMbs / 32 (4:2:0: RawMbBits = 256 * BitDepthY + 128 * BitDepthC, 3072 at
           8 bits, 3840 at High 10); scaled by 3, so 3 * RawMbBits / 32 = 36 * BitDepth per MB.  Each word
           appended to the last slice is 0x000003 in the byte stream (emulation prevention). */
        const long bytes = out->len - len0 - 4L * nslices;          /* NAL units, no start codes */
        const int bd = s->bit_depth > 8 ? s->bit_depth : 8;
        const long excess = 3 * bins - 36L * bd * nmb - 32 * bytes;
        for (long z = excess > 0 ? (excess + 95) / 96 : 0; z > 0; z--) {
            static const uint8_t zw[3] = {0, 0, 3};
            jm_bits t = {(uint8_t *)zw, 3, 3, 0, 0};
            jm_bits_append(out, &t);
        }
    }
    return JMH_OK;
}

/* ---- DeviceCAVLC 1 / DeviceCABAC 1: image.c › code_a_picture [J] with the slice data written on
 * the device.  The slice headers are written here (jm_write_slice_header).
 * CAVLC: the bits of each header's last, partial byte go to the device with the slice's macroblock
 * range, and the device returns slice_data() + rbsp_trailing_bits behind them (jmh_cavlc_write
 * _slices).  CABAC: the header is padded with cabac_alignment_one_bits here, the device returns the
 * coded slice_data() up to the rbsp_stop_one_bit and the slice's bins (jmh_cabac_write_slices); the
 * cabac_zero_words rule of encode_picture_slices is then applied to the summed bins.
 * Header bytes + device bytes are the slice's RBSP, wrapped by jm_write_nal as ever.  No
 * jm_slice_write_mb, no writer threads, no rate cross-check. */
static jm_cavlc_slices_fn device_cavlc_fn;
void jm_set_device_cavlc(jm_cavlc_slices_fn fn) { device_cavlc_fn = fn; }
static jm_cabac_slices_fn device_cabac_fn;
void jm_set_device_cabac(jm_cabac_slices_fn fn) { device_cabac_fn = fn; }
static jm_cabac_split_fn device_cabac_split_fn;
void jm_set_device_cabac_split(jm_cabac_split_fn fn) { device_cabac_split_fn = fn; }
/* DeviceWriterAsync 1: the same writers queued behind each pipelined picture (jmh_frame_push_coded /
 * jmh_frame_pop_coded).  The headers are written when the picture is pushed (device_slice_headers:
 * frame_num, slice type, QP and first_mb are known then) and kept with the picture; its pop brings
 * the device bytes, which device_slice_assemble joins to them exactly as the synchronous path does. */
static jm_coded_push_fn device_coded_push_fn;
static jm_coded_pop_fn device_coded_pop_fn;
void jm_set_device_coded(jm_coded_push_fn push, jm_coded_pop_fn pop) { device_coded_push_fn = push; device_coded_pop_fn = pop; }
/* DeviceNAL 1: the whole bytes of each header go down with the push as the slice's head (device_slice
 * _heads), the device finishes the NAL units behind the writer, and the pop brings the picture's
 * access unit, which goes to the stream in one copy: no device_slice_assemble on this path. */
static jm_nal_heads_fn device_nal_fn;
void jm_set_device_nal(jm_nal_heads_fn fn) { device_nal_fn = fn; }

typedef struct dcavlc {
    int n;                       /* slices per picture */
    int cabac;                   /* DeviceCABAC: cd / cwhere instead of d / where */
    jmh_slice_desc *d;
    jmh_slice_bytes *where;
    jmh_cabac_slice_desc *cd;
    jmh_cabac_slice_bytes *cwhere;
    jmh_coded_slice *cs;         /* the descriptors of either coder (the coded push takes these) */
    jmh_coded_bytes *cw;         /* where of either coder: what device_slice_assemble reads */
    jm_bits *hdr;                /* per slice: the header, then the whole RBSP */
    jmh_nal_head *nh;            /* DeviceNAL: per slice, the header's whole bytes as the NAL unit's head */
    uint8_t *buf;                /* the device bytes (NULL in a pending picture's own dcavlc_t: they share one) */
    size_t cap;
} dcavlc_t;

static void dcavlc_free(dcavlc_t *dc) {
    if (dc->hdr) for (int i = 0; i < dc->n; i++) jm_bits_free(&dc->hdr[i]);
    free(dc->d); free(dc->where); free(dc->cd); free(dc->cwhere); free(dc->cs); free(dc->cw); free(dc->hdr); free(dc->nh); free(dc->buf);
    memset(dc, 0, sizeof(*dc));
}
static int dcavlc_init(dcavlc_t *dc, const jm_seq *s, int cabac, int with_buf) {
    const int nmb = s->mbw * s->mbh, step = s->slice_mbs > 0 ? s->slice_mbs : nmb;
    memset(dc, 0, sizeof(*dc));
    dc->n = (nmb + step - 1) / step;
    dc->cabac = cabac;
    dc->d = (jmh_slice_desc *)calloc(dc->n, sizeof(*dc->d));
    dc->where = (jmh_slice_bytes *)calloc(dc->n, sizeof(*dc->where));
    dc->cd = (jmh_cabac_slice_desc *)calloc(dc->n, sizeof(*dc->cd));
    dc->cwhere = (jmh_cabac_slice_bytes *)calloc(dc->n, sizeof(*dc->cwhere));
    dc->hdr = (jm_bits *)calloc(dc->n, sizeof(*dc->hdr));
    dc->cs = (jmh_coded_slice *)calloc(dc->n, sizeof(*dc->cs));
    dc->cw = (jmh_coded_bytes *)calloc(dc->n, sizeof(*dc->cw));
    dc->nh = (jmh_nal_head *)calloc(dc->n, sizeof(*dc->nh));
    dc->cap = with_buf ? (size_t)nmb * 64 + 1024 : 0;
    dc->buf = with_buf ? (uint8_t *)malloc(dc->cap) : NULL;
    if (!dc->d || !dc->where || !dc->cd || !dc->cwhere || !dc->cs || !dc->cw || !dc->hdr || !dc->nh || (with_buf && !dc->buf)) { dcavlc_free(dc); return JMH_E_OOM; }
    return JMH_OK;
}
static int device_call(dcavlc_t *dc, jm_backend *be) {
    return dc->cabac ? device_cabac_fn(be->ctx, dc->n, dc->cd, dc->buf, dc->cap, dc->cwhere)
                     : device_cavlc_fn(be->ctx, dc->n, dc->d, dc->buf, dc->cap, dc->where);
}
/* the header / descriptor half: every slice's header into hdr[], its descriptor for either entry point */
static void device_slice_headers(dcavlc_t *dc, const jm_seq *s, const jm_slice *sl0) {
    const int nmb = s->mbw * s->mbh, step = s->slice_mbs > 0 ? s->slice_mbs : nmb;
    for (int i = 0; i < dc->n; i++) {
        jm_slice sl = *sl0;
        sl.first_mb = i * step;
        jm_bits *h = &dc->hdr[i];
        h->len = 0; h->acc = 0; h->nacc = 0;
        jm_write_slice_header(h, s, &sl);
        const int n_mb = sl.first_mb + step < nmb ? step : nmb - sl.first_mb;
        if (dc->cabac) while (h->nacc) jm_put(h, 1, 1);    /* cabac_alignment_one_bit */
        dc->cs[i].first_mb = sl.first_mb; dc->cs[i].n_mb = n_mb; dc->cs[i].slice_type = sl0->slice_type;
        dc->cs[i].slice_qp = sl0->qp; dc->cs[i].lead_nbits = h->nacc; dc->cs[i].lead_bits = (uint32_t)h->acc;
        if (dc->cabac) {
            dc->cd[i].first_mb = sl.first_mb;
            dc->cd[i].n_mb = n_mb;
            dc->cd[i].slice_type = sl0->slice_type;
            dc->cd[i].slice_qp = sl0->qp;
            continue;
        }
        dc->d[i].first_mb = sl.first_mb;
        dc->d[i].n_mb = n_mb;
        dc->d[i].slice_type = sl0->slice_type;
        dc->d[i].lead_nbits = h->nacc;
        dc->d[i].lead_bits = (uint32_t)h->acc;
    }
}
/* DeviceNAL: the headers of device_slice_headers as heads (for CAVLC the partial last byte travels as
   lead bits and comes back as the first device byte); JMH_E_INVALID_ARG: a header too long for a head */
static int device_slice_heads(dcavlc_t *dc, const jm_slice *sl0) {
    for (int i = 0; i < dc->n; i++) {
        const jm_bits *h = &dc->hdr[i];
        if (h->len > JMH_NAL_HEAD_MAX) return JMH_E_INVALID_ARG;
        dc->nh[i].nal_ref_idc = sl0->idr ? 3 : 2; dc->nh[i].nal_unit_type = sl0->idr ? 5 : 1;
        dc->nh[i].nbytes = (int32_t)h->len;
        memcpy(dc->nh[i].bytes, h->buf, (size_t)h->len);
    }
    return JMH_OK;
}
/* the assemble half: header bytes + the device bytes that cw[] places in buf, per slice through
   jm_write_nal; the cabac_zero_words rule on the summed bins */
static void device_slice_assemble(dcavlc_t *dc, const jm_seq *s, const jm_slice *sl0, const uint8_t *buf, jm_bits *out) {
    const int nmb = s->mbw * s->mbh;
    const long len0 = out->len;
    long bins = 0;
    for (int i = 0; i < dc->n; i++) {
        jm_bits *h = &dc->hdr[i];
        jm_bits t = {(uint8_t *)buf + dc->cw[i].offset, dc->cw[i].nbytes, dc->cw[i].nbytes, 0, 0};
        h->acc = 0; h->nacc = 0;                /* CAVLC: the partial byte comes back as the first device byte */
        jm_bits_append(h, &t);
        jm_write_nal(out, sl0->idr ? 3 : 2, sl0->idr ? 5 : 1, h);
        if (dc->cabac) bins += (long)dc->cw[i].nbins;
    }
    if (dc->cabac) {                            /* cabac_zero_words: as encode_picture_slices */
        const long bytes = out->len - len0 - 4L * dc->n;
        const int bd = s->bit_depth > 8 ? s->bit_depth : 8;
        const long excess = 3 * bins - 36L * bd * nmb - 32 * bytes;
        for (long z = excess > 0 ? (excess + 95) / 96 : 0; z > 0; z--) {
            static const uint8_t zw[3] = {0, 0, 3};
            jm_bits t = {(uint8_t *)zw, 3, 3, 0, 0};
            jm_bits_append(out, &t);
        }
    }
}
static int device_picture_slices(dcavlc_t *dc, jm_backend *be, const jm_seq *s, const jm_slice *sl0, jm_bits *out) {
    device_slice_headers(dc, s, sl0);
    memset(dc->where, 0, dc->n * sizeof(*dc->where));
    memset(dc->cwhere, 0, dc->n * sizeof(*dc->cwhere));
    int r = device_call(dc, be);
    const size_t total = dc->cabac ? (size_t)(dc->cwhere[dc->n - 1].offset + dc->cwhere[dc->n - 1].nbytes)
                                   : (size_t)(dc->where[dc->n - 1].offset + dc->where[dc->n - 1].nbytes);
    if (r == JMH_E_INVALID_ARG && total > dc->cap) {   /* the counted size: grow and write again */
        uint8_t *nb = (uint8_t *)realloc(dc->buf, 2 * total);
        if (!nb) return JMH_E_OOM;
        dc->buf = nb; dc->cap = 2 * total;
        r = device_call(dc, be);
    }
    if (r) return r;
    for (int i = 0; i < dc->n; i++) {
        dc->cw[i].offset = dc->cabac ? dc->cwhere[i].offset : dc->where[i].offset;
        dc->cw[i].nbytes = dc->cabac ? dc->cwhere[i].nbytes : dc->where[i].nbytes;
        dc->cw[i].nbits = dc->cabac ? 0 : dc->where[i].nbits;
        dc->cw[i].nbins = dc->cabac ? dc->cwhere[i].nbins : 0;
    }
    device_slice_assemble(dc, s, sl0, dc->buf, out);
    return JMH_OK;
}
/* DeviceWriterAsync: the pop of the oldest coded picture into the shared buffer of dc (grown to the
   picture's bytes when the device says so), its where into the picture's own pdc */
static int device_coded_pop(dcavlc_t *dc, dcavlc_t *pdc, jm_backend *be, jmh_coded_stats *stats) {
    int r = device_coded_pop_fn(be->ctx, dc->buf, dc->cap, pdc->cw, stats);
    const size_t total = (size_t)(pdc->cw[pdc->n - 1].offset + pdc->cw[pdc->n - 1].nbytes);
    if (r == JMH_E_INVALID_ARG && total > dc->cap) {
        uint8_t *nb = (uint8_t *)realloc(dc->buf, 2 * total);
        if (!nb) return JMH_E_OOM;
        dc->buf = nb; dc->cap = 2 * total;
        r = device_coded_pop_fn(be->ctx, dc->buf, dc->cap, pdc->cw, stats);
    }
    return r;
}

/* ---- parallel slice writing (WriterThreads > 0, pipelined device backend) -------------------
 * The slices of different pictures are independent once their macroblock results exist (one
 * slice per picture, device deblocking), so popped pictures are written by a pool of threads,
 * each with its own JM state (img is thread-local), and emitted in picture order.  The main
 * thread keeps the device busy: pop, copy the results and the deblocked picture into a job,
 * push the next picture. */
typedef struct wjob {
    jm86_img im;                 /* the job's JM state; im.mb_data holds the picture's results   */
    jm_pic rec;                  /* its deblocked reconstruction                                 */
    const jm_pic *cur;           /* its source (pend slot, not refilled before the job is flushed) */
    jmh_frame_params fp;
    jm_slice sl;
    int f, is_i;
    double met;                  /* backend time charged to the picture (report line)           */
    jm_bits out;                 /* NAL unit                                                     */
    long pic_bits;
    double py, pu, pv, write_ms;
    int status, state;           /* state: 0 idle, 1 queued, 2 running, 3 done                   */
} wjob_t;

typedef struct wpool {
    pthread_mutex_t mu;
    pthread_cond_t cv_work, cv_done;
    wjob_t *jobs;
    int nj, stop;
    int *queue, qh, qt;          /* job indices, FIFO */
    const jm_seq *s;
    const jm_input *inp;
    pthread_t *th;
    int nth;
} wpool_t;

static int encode_picture_slices(jm86_img *im, const jm_seq *s, const jm_slice *sl0, const jmh_frame_params *fp,
                                 const jm_pic *cur, const jm_pic *ref, jm_bits *out);

static void job_run(wpool_t *P, wjob_t *j) {
    const jm_seq *s = P->s;
    const jm_input *inp = P->inp;
    const int W = s->width;
    double t0 = now_ms();
    j->out.len = 0;
    j->status = encode_picture_slices(&j->im, s, &j->sl, &j->fp, j->cur, &j->rec, &j->out);
    j->pic_bits = j->out.len * 8;
    j->py = psnr_pl(j->cur, &j->rec, 0, inp->width, inp->height);
    j->pu = psnr_pl(j->cur, &j->rec, 1, inp->width / 2, inp->height / 2);
    j->pv = psnr_pl(j->cur, &j->rec, 2, inp->width / 2, inp->height / 2);
    (void)W;
    j->write_ms = now_ms() - t0;
}

static void *writer_main(void *arg) {
    wpool_t *P = (wpool_t *)arg;
    for (;;) {
        pthread_mutex_lock(&P->mu);
        while (!P->stop && P->qh == P->qt) pthread_cond_wait(&P->cv_work, &P->mu);
        if (P->qh == P->qt) { pthread_mutex_unlock(&P->mu); return NULL; }   /* stop, queue drained */
        wjob_t *j = &P->jobs[P->queue[P->qh % P->nj]];
        P->qh++;
        j->state = 2;
        pthread_mutex_unlock(&P->mu);
        job_run(P, j);
        pthread_mutex_lock(&P->mu);
        j->state = 3;
        pthread_cond_broadcast(&P->cv_done);
        pthread_mutex_unlock(&P->mu);
    }
}

static void pool_submit(wpool_t *P, int k) {
    pthread_mutex_lock(&P->mu);
    P->jobs[k].state = 1;
    P->queue[P->qt % P->nj] = k;
    P->qt++;
    pthread_cond_signal(&P->cv_work);
    pthread_mutex_unlock(&P->mu);
}

static void pool_wait(wpool_t *P, int k) {
    pthread_mutex_lock(&P->mu);
    while (P->jobs[k].state != 3) pthread_cond_wait(&P->cv_done, &P->mu);
    pthread_mutex_unlock(&P->mu);
}

/* job state is shared with the writer threads: read and reset it under the pool lock only */
static int job_busy(wpool_t *P, int k) {
    pthread_mutex_lock(&P->mu);
    const int st = P->jobs[k].state;
    pthread_mutex_unlock(&P->mu);
    return st != 0;
}
static void job_release(wpool_t *P, int k) {
    pthread_mutex_lock(&P->mu);
    P->jobs[k].state = 0;
    pthread_mutex_unlock(&P->mu);
}

/* DeviceReconFormat / DeviceReconTensor: the current picture pulled on the device and appended to ReconFile */
typedef struct { jm_device_output_fn fn; int format, tensor, flags, w, h; size_t bytes; uint8_t *buf; FILE *f; } drec_t;
static int device_recon_write(const drec_t *d, const jm_backend *be) {
    const int r = d->fn(be->ctx, d->format, d->tensor, d->flags, d->w, d->h, d->buf);
    if (r) { fprintf(stderr, "device recon pull failed: %d\n", r); return r; }
    return fwrite(d->buf, 1, d->bytes, d->f) == d->bytes ? 0 : JMH_E_INVALID_ARG;
}

int jm_encode_sequence(const jm_input *inp, jm_backend *be, jm_stats *st, FILE *log) {
    memset(st, 0, sizeof(*st));
    if (inp->device_nal && !device_nal_fn) {
        fprintf(stderr, "DeviceNAL=1 needs the device backend (backend '%s' finishes its NAL units on the host: DeviceNAL=0)\n", be->name);
        return JMH_E_UNSUPPORTED_CFG;
    }
    if (inp->device_cavlc && !device_cavlc_fn) {
        fprintf(stderr, "DeviceCAVLC=1 needs the device backend (backend '%s' writes its slices on the host: DeviceCAVLC=0)\n", be->name);
        return JMH_E_UNSUPPORTED_CFG;
    }
    if (inp->device_cabac_split && !device_cabac_split_fn) {
        fprintf(stderr, "DeviceCABACSplit=%d with DeviceCABAC=1 needs the device backend (backend '%s' writes its slices on the host: DeviceCABAC=0)\n",
                inp->device_cabac_split, be->name);
        return JMH_E_UNSUPPORTED_CFG;
    }
    if (inp->device_cabac && !device_cabac_fn) {
        fprintf(stderr, "DeviceCABAC=1 needs the device backend (backend '%s' writes its slices on the host: DeviceCABAC=0)\n", be->name);
        return JMH_E_UNSUPPORTED_CFG;
    }
    const int device_writer = inp->device_cavlc || inp->device_cabac;
    if (inp->device_cabac_split) {               /* once, before the first picture: every writer call and coded picture follows it */
        const int r = device_cabac_split_fn(be->ctx, inp->device_cabac_split);
        if (r) { fprintf(stderr, "DeviceCABACSplit=%d: the backend refused it (%d)\n", inp->device_cabac_split, r); return r; }
    }
    const jm_device_push_fn device_input_fn = inp->device_input ? jm_device_input() : NULL;
    if (inp->device_input && !device_input_fn) {
        fprintf(stderr, "DeviceInput=1 needs the device backend (backend '%s' has no device input: DeviceInput=0)\n", be->name);
        return JMH_E_UNSUPPORTED_CFG;
    }
    /* the source the backend pushes: 4:2:0 planes under DeviceInput alone, else the layout its key names.  The keys in
       the order they are checked, each with its value, the source's code and flags and its refusals: without DeviceInput
       on the device backend or beside a key before it, without DeviceWriterAsync, with the synthetic source */
    const int rgb_flags = (inp->device_input_matrix ? JMH_PIX_BT709 : 0) | (inp->device_input_full ? JMH_PIX_FULL_RANGE : 0);
    const struct { int val, kind, code, flags; const char *needs, *async, *synthetic; } src_keys[3] = {
        {inp->device_input_format, JM_SRC_RGB, inp->device_input_format | rgb_flags, 0,
         "DeviceInputFormat=%d needs DeviceInput=1 on the device backend (backend '%s' has no RGB device input: DeviceInputFormat=0)\n",
         "DeviceInputFormat=%d needs DeviceWriterAsync=1 (no YUV source on the host: the distortion is the device's)\n",
         "DeviceInputFormat=%d reads RGB frames from InputFile: the synthetic source is YUV\n"},
        {inp->device_input_tensor, JM_SRC_TENSOR, inp->device_input_tensor, rgb_flags,
         "DeviceInputTensor=%d needs DeviceInput=1 on the device backend and DeviceInputFormat=0 (backend '%s')\n",
         "DeviceInputTensor=%d needs DeviceWriterAsync=1 (no YUV source on the host: the distortion is the device's)\n",
         "DeviceInputTensor=%d reads RGB frames from InputFile: the synthetic source is YUV\n"},
        {inp->device_input_yuv, JM_SRC_YUV,
         inp->device_input_yuv | (inp->device_input_chroma_left && jm_yuv_is444(inp->device_input_yuv) ? JMH_PIX_CHROMA_LEFT : 0), 0,
         "DeviceInputYUV=%d needs DeviceInput=1 on the device backend, DeviceInputFormat=0 and DeviceInputTensor=0 (backend '%s')\n",
         "DeviceInputYUV=%d needs DeviceWriterAsync=1 (no 4:2:0 source on the host: the distortion is the device's)\n",
         "DeviceInputYUV=%d reads 4:2:2 or 4:4:4 frames from InputFile: the synthetic source is 4:2:0\n"},
    };
    jm_device_source src = {JM_SRC_PLANES, 0, 0, NULL, NULL, 0, 0};
    int src_key = -1;                            /* the key that names the layout of InputFile, if one does */
    for (int k = 0; k < 3; k++) {
        if (!src_keys[k].val) continue;
        if (src_key >= 0 || !device_input_fn) { fprintf(stderr, src_keys[k].needs, src_keys[k].val, be->name); return JMH_E_UNSUPPORTED_CFG; }
        if (!inp->device_writer_async) { fprintf(stderr, src_keys[k].async, src_keys[k].val); return JMH_E_UNSUPPORTED_CFG; }
        src.kind = src_keys[k].kind; src.code = src_keys[k].code; src.flags = src_keys[k].flags;
        src_key = k;
    }
    const int scale = inp->device_input_scale;
    const jm_device_scale_fn device_scale_fn = scale ? jm_device_input_scale() : NULL;
    if (scale && (!device_input_fn || !device_scale_fn || !inp->device_writer_async)) {
        fprintf(stderr, "DeviceInputScale=%d needs DeviceInput=1 and DeviceWriterAsync=1 on the device backend (backend '%s')\n", scale, be->name);
        return JMH_E_UNSUPPORTED_CFG;
    }
    /* the frames of InputFile: DeviceInputWidth x DeviceInputHeight under DeviceInputScale, else the display size */
    const int src_w = scale ? inp->device_input_width : inp->width, src_h = scale ? inp->device_input_height : inp->height;
    src.w = src_w; src.h = src_h;
    if (inp->device_writer_async && !(device_coded_push_fn && device_coded_pop_fn)) {
        fprintf(stderr, "DeviceWriterAsync=1 needs the device backend (backend '%s' has no coded push / pop: DeviceWriterAsync=0)\n", be->name);
        return JMH_E_UNSUPPORTED_CFG;
    }
    jmh_config cfg;
    jm_fill_config(inp, &cfg);
    int W = cfg.width, H = cfg.height;
    jm_seq s;
    memset(&s, 0, sizeof(s));
    s.width = W; s.height = H; s.disp_w = inp->width; s.disp_h = inp->height;
    s.mbw = W / 16; s.mbh = H / 16;
    s.profile_idc = inp->profile_idc; s.level_idc = inp->level_idc;
    s.num_ref_frames = inp->num_ref_frames;
    s.log2_max_frame_num = 8; s.log2_max_poc_lsb = 8;
    s.chroma_qp_offset = inp->chroma_qp_offset;
    s.lf_params_flag = inp->lf_params_flag; s.lf_disable = inp->lf_disable;
    s.slice_mbs = inp->slice_mode == 1 ? inp->slice_arg : 0;
    s.lf_alpha = inp->lf_alpha; s.lf_beta = inp->lf_beta;
    s.constrained_intra = inp->constrained_intra;
    s.transform_8x8_mode = inp->transform_8x8_mode;
    s.entropy_coding = inp->symbol_mode;
    s.bit_depth = inp->bit_depth_luma;
    const int bd = inp->bit_depth_luma;
    s.cabac_init_idc = inp->model_number;
    s.rdo = inp->rdopt;

    FILE *fin = NULL, *fout = NULL, *frec = NULL;
    uint64_t seed = 0;
    int synthetic = !strncmp(inp->infile, "synthetic:", 10);
    if (synthetic && src_key >= 0) { fprintf(stderr, src_keys[src_key].synthetic, src_keys[src_key].val); return JMH_E_UNSUPPORTED_CFG; }
    if (synthetic && scale) { fprintf(stderr, "DeviceInputScale=%d reads frames of DeviceInputWidth x DeviceInputHeight from InputFile: the synthetic source has the coded size\n", scale); return JMH_E_UNSUPPORTED_CFG; }
    if (synthetic) seed = strtoull(inp->infile + 10, NULL, 10);
    else if (!(fin = fopen(inp->infile, "rb"))) { fprintf(stderr, "Input file %s does not exist\n", inp->infile); return JMH_E_INVALID_ARG; }
    if (!(fout = fopen(inp->outfile, "wb"))) { fprintf(stderr, "Cannot open output file %s\n", inp->outfile); if (fin) fclose(fin); return JMH_E_INVALID_ARG; }
    if (inp->reconfile[0] && !(frec = fopen(inp->reconfile, "wb"))) { fprintf(stderr, "Cannot open recon file %s\n", inp->reconfile); fclose(fout); if (fin) fclose(fin); return JMH_E_INVALID_ARG; }

    /* pictures waiting for their results: depth > 1 when the backend pipelines (jmh_frame_push /
       jmh_frame_pop, lencod.c); their sources stay here for the PSNR */
    const int dev_dbk = be->read_deblocked && be->reference_deblocked;
    /* DeviceReconFormat / DeviceReconTensor: ReconFile holds the picture converted on the device, pulled right
       after its pop (while it is the current picture) and written then: pops come in picture order */
    drec_t drec;
    memset(&drec, 0, sizeof(drec));
    if (inp->device_recon_format || inp->device_recon_tensor) {
        drec.fn = jm_device_output();
        drec.flags = (inp->device_recon_matrix ? JMH_PIX_BT709 : 0) | (inp->device_recon_full ? JMH_PIX_FULL_RANGE : 0);
        drec.format = inp->device_recon_format ? inp->device_recon_format | drec.flags : 0;
        drec.tensor = inp->device_recon_tensor;
        drec.w = inp->width; drec.h = inp->height;
        drec.bytes = jm_recon_frame_bytes(drec.tensor, drec.w, drec.h);
        drec.f = frec;
        if (!drec.fn || !frec || !dev_dbk || !(drec.buf = (uint8_t *)malloc(drec.bytes))) {
            fprintf(stderr, "DeviceRecon%s=%d needs ReconFile and the device backend with device deblocking (backend '%s')\n",
                    drec.tensor ? "Tensor" : "Format", drec.tensor ? drec.tensor : inp->device_recon_format, be->name);
            if (fin) fclose(fin);
            fclose(fout);
            if (frec) fclose(frec);
            free(drec.buf);
            return JMH_E_UNSUPPORTED_CFG;
        }
    }
    const int pipelined = dev_dbk && be->push && be->pop && be->depth > 1;
    const int depth = pipelined ? be->depth : 1;
    const int async = inp->device_writer_async;
    const int nal = async && inp->device_nal;
    if ((async || device_input_fn) && !pipelined) {
        fprintf(stderr, "%s=1 needs the pipelined path (device deblocking, more than one picture in flight)\n", async ? "DeviceWriterAsync" : "DeviceInput");
        if (fin) fclose(fin);
        fclose(fout);
        if (frec) fclose(frec);
        free(drec.buf);
        return JMH_E_UNSUPPORTED_CFG;
    }
    /* parallel slice writing: pipelined device backend, not with the call surface's per-MB
       device searches (those share the context with the frame loop) */
    const int nwr = (pipelined && !inp->jm_call_surface && !device_writer) ? inp->writer_threads : 0;
    const int nj = nwr ? 2 * nwr : 0;                  /* jobs in flight: queued + running + done */
    const int plen = depth + nj + 1;                   /* source slots: a job's source stays put */
    typedef struct { jm_pic cur; jmh_frame_params fp; int f, is_i, frame_num; } pend_t;
    pend_t *pend = (pend_t *)calloc(plen, sizeof(pend_t));
    jm_pic rec;
    memset(&rec, 0, sizeof(rec));
    /* DeviceInputFormat: one frame as read, height rows of 4 * width bytes (free again when its upload returns);
       DeviceInputTensor: one frame of its file, in the same buffer; DeviceInputYUV: one frame of its layout, likewise */
    const int raw_source = src.kind != JM_SRC_PLANES;
    const size_t rgb_bytes = jm_source_frame_bytes(&src);
    uint8_t *rgb = raw_source ? (uint8_t *)malloc(rgb_bytes) : NULL;
    src.frame = rgb;
    /* DeviceInputScale with a YUV file: one frame as read, at its own size (free again when its upload returns) */
    jm_pic big;
    memset(&big, 0, sizeof(big));
    int alloc_fail = !pend || (raw_source && !rgb) || jm_pic_alloc_bd(&rec, W, H, bd) || (scale && !raw_source && jm_pic_alloc_bd(&big, src_w, src_h, bd));
    for (int k = 0; k < plen && !alloc_fail; k++) alloc_fail = jm_pic_alloc_bd(&pend[k].cur, W, H, bd);
    if (alloc_fail) {
        if (pend) for (int k = 0; k < plen; k++) jm_pic_free(&pend[k].cur);
        free(pend);
        free(rgb);
        jm_pic_free(&rec);
        jm_pic_free(&big);
        if (fin) fclose(fin);
        fclose(fout);
        if (frec) fclose(frec);
        free(drec.buf);
        return JMH_E_OOM;
    }
    if (device_input_fn) {   /* the readers write the display size only: what lies outside is the device's to pad, never this */
        jm_source_padding(0);
        for (int k = 0; k < plen; k++) memset(bd > 8 ? (void *)pend[k].cur.Y : (void *)pend[k].cur.y, 0x5A, (size_t)W * H * 3 / 2 * (bd > 8 ? 2 : 1));
    }
    int nmb = s.mbw * s.mbh;
    const jmh_mb_result **res = (const jmh_mb_result **)malloc(sizeof(*res) * nmb);
    jm86_img im;
    memset(&im, 0, sizeof(im));
    wpool_t pool;
    memset(&pool, 0, sizeof(pool));
    dcavlc_t dc;
    memset(&dc, 0, sizeof(dc));
    dcavlc_t *pdc = NULL;        /* DeviceWriterAsync: per pending picture, its headers and descriptors */
    int st_ret = 0, njobs_init = 0, nstarted = 0, pool_sync = 0;
    long jseq = 0, jflushed = 0;   /* jobs submitted / emitted (picture order) */
    double copy_ms = 0, write_ms = 0;
    double read_ms = 0, push_ms = 0, pop_ms = 0, flush_ms = 0;   /* main thread, for the summary */
    jm_bits out, rbsp;
    jm_bits_init(&out); jm_bits_init(&rbsp);
    if (!res || jm86_init(&im, inp, be, W, H)) { st_ret = JMH_E_OOM; goto cleanup; }
    if (device_writer && dcavlc_init(&dc, &s, inp->device_cabac, 1)) { st_ret = JMH_E_OOM; goto cleanup; }
    if (async) {
        if (!(pdc = (dcavlc_t *)calloc(plen, sizeof(*pdc)))) { st_ret = JMH_E_OOM; goto cleanup; }
        for (int k = 0; k < plen; k++)
            if (dcavlc_init(&pdc[k], &s, inp->device_cabac, 0)) { st_ret = JMH_E_OOM; goto cleanup; }
    }
    if (nwr) {
        pool.nj = nj; pool.s = &s; pool.inp = inp; pool.nth = nwr;
        pool.jobs = (wjob_t *)calloc(nj, sizeof(wjob_t));
        pool.queue = (int *)calloc(nj, sizeof(int));
        pool.th = (pthread_t *)calloc(nwr, sizeof(pthread_t));
        if (!pool.jobs || !pool.queue || !pool.th) { st_ret = JMH_E_OOM; goto cleanup; }
        for (; njobs_init < nj; njobs_init++) {
            wjob_t *j = &pool.jobs[njobs_init];
            jm_bits_init(&j->out);
            if (jm86_init(&j->im, inp, be, W, H) || jm_pic_alloc_bd(&j->rec, W, H, bd)) { njobs_init++; st_ret = JMH_E_OOM; goto cleanup; }
            j->im.res = j->im.mb_data;   /* results copied in at pop */
        }
        img = &im;   /* jm86_init of the jobs set this thread's img */
        pthread_mutex_init(&pool.mu, NULL);
        pthread_cond_init(&pool.cv_work, NULL);
        pthread_cond_init(&pool.cv_done, NULL);
        pool_sync = 1;
        for (; nstarted < nwr; nstarted++)
            if (pthread_create(&pool.th[nstarted], NULL, writer_main, &pool)) { st_ret = JMH_E_OOM; goto cleanup; }
    }
    jm_write_sps(&rbsp, &s); jm_write_nal(&out, 3, 7, &rbsp); jm_bits_free(&rbsp);
    jm_write_pps(&rbsp, &s); jm_write_nal(&out, 3, 8, &rbsp); jm_bits_free(&rbsp);
    long header_bits = out.len * 8;
    fwrite(out.buf, 1, out.len, fout);
    st->bits += header_bits;
    out.len = 0;
    if (log) {
        fprintf(log, "------------------------------- MI355X jm-hot-path lencod (%s) -------------------------------\n", be->name);
        if (pipelined) fprintf(log, " (%d pictures in flight%s)\n", depth, nwr ? ", parallel slice writing" : "");
        if (nwr) fprintf(log, " (%d slice-writer threads)\n", nwr);
        if (inp->device_cavlc) fprintf(log, " (CAVLC slice data written on the device)\n");
        if (inp->device_cabac && inp->device_cabac_split)
            fprintf(log, " (CABAC slice data written on the device, every slice in chunks of %d bins: no writer threads, no per-macroblock rate check)\n",
                    inp->device_cabac_split);
        else if (inp->device_cabac) fprintf(log, " (CABAC slice data written on the device: no writer threads, no per-macroblock rate check)\n");
        if (src.kind == JM_SRC_RGB)
            fprintf(log, " (the source is RGB, format %d: converted on the device with the BT.%s matrix at %s range; the stream does not signal either)\n",
                    inp->device_input_format, inp->device_input_matrix ? "709" : "601", inp->device_input_full ? "full" : "limited");
        if (src.kind == JM_SRC_TENSOR)
            fprintf(log, " (the source is an RGB tensor, %s: quantised and converted on the device with the BT.%s matrix at %s range; the stream does not signal either)\n",
                    src.code == 1 ? "rgb24" : src.code == 2 ? "gbrp" : src.code == 3 ? "gbrp10le" : "gbrpf32le",
                    inp->device_input_matrix ? "709" : "601", inp->device_input_full ? "full" : "limited");
        if (src.kind == JM_SRC_YUV)
            fprintf(log, " (the source is %s, format %d: its chroma is reduced to 4:2:0 on the device%s)\n", jm_yuv_is444(inp->device_input_yuv) ? "4:4:4" : "4:2:2",
                    inp->device_input_yuv, src.code & JMH_PIX_CHROMA_LEFT ? ", left-sited" : "");
        if (drec.fn)
            fprintf(log, " (ReconFile holds %s %s: the display-size picture converted on the device with the BT.%s matrix at %s range and downloaded)\n",
                    drec.tensor ? "an RGB tensor," : "RGB, format",
                    drec.tensor == 1 ? "rgb24" : drec.tensor == 2 ? "gbrp" : drec.tensor == 3 ? "gbrp10le" : drec.tensor == 4 ? "gbrpf32le"
                    : inp->device_recon_format == 16 ? "16" : inp->device_recon_format == 17 ? "17" : inp->device_recon_format == 18 ? "18" : "19",
                    inp->device_recon_matrix ? "709" : "601", inp->device_recon_full ? "full" : "limited");
        if (scale)
            fprintf(log, " (the source has %dx%d samples: resampled on the device to %dx%d, %s, chroma %s)\n", src_w, src_h, inp->width, inp->height,
                    scale == 1 ? "bilinear" : scale == 2 ? "bicubic" : "Lanczos3", inp->device_input_chroma_left ? "left-sited" : "centred");
        if (device_input_fn) fprintf(log, " (the source is uploaded as read and pushed from device memory: the device pads it to the coded size)\n");
        if (async) fprintf(log, " (the slice writer is queued behind each picture: its pop returns the slice bytes and the SSDs)\n");
        if (nal) fprintf(log, " (NAL units finished on the device: the pop returns the picture's access unit)\n");
        fprintf(log, " Frame  Bit/pic  QP   SnrY    SnrU    SnrV    Time(ms) MET(ms) Frm/Fld  I D\n");
    }
    if (scale) {                                 /* once, before the first picture: every push follows it */
        const int r = device_scale_fn(be->ctx, scale, inp->device_input_chroma_left ? JMH_SCALE_CHROMA_LEFT : 0, inp->width, inp->height);
        if (r) { fprintf(stderr, "DeviceInputScale=%d to %dx%d: the backend refused it (%d)\n", scale, inp->width, inp->height, r); st_ret = r; goto cleanup; }
    }
    double t_start = now_ms();
    int frame_num = 0, head = 0, count = 0;
    /* the rest of encode_one_frame for a picture whose macroblock results are available:
       slice (CAVLC), deblocking / next reference, recon file, PSNR, report line */
    /* emit a finished job: NAL unit, recon, statistics, report line (picture order) */
    #define FLUSH_JOB(J)                                                                           \
    do {                                                                                           \
        wjob_t *fj_ = (J);                                                                          \
        double tf_ = now_ms();                                                                      \
        pool_wait(&pool, (int)(fj_ - pool.jobs));                                                   \
        if (fj_->status) { st_ret = fj_->status; break; }                                           \
        fwrite(fj_->out.buf, 1, fj_->out.len, fout);                                                 \
        if (frec && !drec.fn) jm_write_yuv_frame(frec, &fj_->rec, inp->width, inp->height);         \
        st->psnr_y += fj_->py; st->psnr_u += fj_->pu; st->psnr_v += fj_->pv;                          \
        st->bits += fj_->pic_bits;                                                                  \
        im.rate_checked += fj_->im.rate_checked; im.rate_mismatches += fj_->im.rate_mismatches;     \
        fj_->im.rate_checked = fj_->im.rate_mismatches = 0;                                         \
        st->frames++;                                                                              \
        st->entropy_ms += fj_->write_ms;                                                            \
        write_ms += fj_->write_ms;                                                                  \
        if (log)                                                                                   \
            fprintf(log, "%4d(%s) %8ld   %2d %7.4f %7.4f %7.4f %9.1f %7.1f    FRM\n", fj_->f,          \
                    fj_->is_i ? "IDR" : " P ", fj_->pic_bits, fj_->fp.qp, fj_->py, fj_->pu, fj_->pv,       \
                    fj_->write_ms + fj_->met, fj_->met);                                              \
        job_release(&pool, (int)(fj_ - pool.jobs));                                                 \
        jflushed++;                                                                                \
        flush_ms += now_ms() - tf_;                                                                 \
    } while (0)
    /* hand a popped picture to the writer pool: its results and deblocked picture into a job */
    #define SUBMIT(P, MET_MS)                                                                      \
    do {                                                                                           \
        pend_t *p_ = (P);                                                                          \
        wjob_t *j_ = &pool.jobs[jseq % nj];                                                       \
        if (job_busy(&pool, (int)(j_ - pool.jobs))) { FLUSH_JOB(j_); if (st_ret) break; }          \
        double t1 = now_ms();                                                                      \
        const jmh_mb_result *r0_ = be->mb_result(be->ctx, 0);                                      \
        if (nmb > 1 && be->mb_result(be->ctx, nmb - 1) != r0_ + (nmb - 1)) { st_ret = JMH_E_STATE; break; } \
        memcpy(j_->im.mb_data, r0_, (size_t)nmb * sizeof(jmh_mb_result));                         \
        int r_ = be->read_deblocked(be->ctx, &j_->rec);                                            \
        if (r_) { fprintf(stderr, "read_deblocked failed: %d\n", r_); st_ret = r_; break; }       \
        if (drec.fn && (r_ = device_recon_write(&drec, be))) { st_ret = r_; break; }               \
        copy_ms += now_ms() - t1;                                                                  \
        st->deblock_ms += now_ms() - t1;                                                           \
        j_->cur = &p_->cur; j_->fp = p_->fp; j_->f = p_->f; j_->is_i = p_->is_i; j_->met = (MET_MS); \
        j_->sl.idr = p_->f == 0; j_->sl.slice_type = p_->fp.slice_type; j_->sl.frame_num = p_->frame_num; \
        j_->sl.poc_lsb = 2 * p_->f; j_->sl.idr_pic_id = 0; j_->sl.qp = p_->fp.qp; j_->sl.first_mb = 0; \
        pool_submit(&pool, (int)(j_ - pool.jobs));                                                 \
        jseq++;                                                                                    \
    } while (0)
    #define EMIT(P, MET_MS)                                                                          \
    do {                                                                                           \
        if (nwr) { SUBMIT(P, MET_MS); break; }                                                     \
        pend_t *p_ = (P);                                                                          \
        double t1 = now_ms();                                                                      \
        for (int a = 0; a < nmb; a++) res[a] = be->mb_result(be->ctx, a);                          \
        jm_slice sl;                                                                               \
        sl.idr = p_->f == 0; sl.slice_type = p_->fp.slice_type; sl.frame_num = p_->frame_num;      \
        sl.poc_lsb = 2 * p_->f; sl.idr_pic_id = 0; sl.qp = p_->fp.qp;                              \
        sl.first_mb = 0;                                                                           \
        { int e_ = device_writer ? device_picture_slices(&dc, be, &s, &sl, &out)                \
                                     : encode_picture_slices(&im, &s, &sl, &p_->fp, &p_->cur, &rec, &out); \
          if (e_) { if (device_writer) fprintf(stderr, "device slice writer failed: status %d\n", e_); st_ret = e_; break; } } \
        double t2 = now_ms();                                                                      \
        st->entropy_ms += t2 - t1;                                                                 \
        long pic_bits = out.len * 8;                                                               \
        fwrite(out.buf, 1, out.len, fout);                                                         \
        out.len = 0;                                                                               \
        int r_;                                                                                    \
        if (dev_dbk) r_ = be->read_deblocked(be->ctx, &rec);                                       \
        else {                                                                                     \
            be->read_recon(be->ctx, &rec);                                                         \
            jm_deblock_picture(&rec, &s, res, p_->fp.qp);                                          \
            r_ = be->set_reference(be->ctx, &rec);                                                 \
        }                                                                                          \
        double t3 = now_ms();                                                                      \
        st->deblock_ms += t3 - t2;                                                                 \
        if (r_) { fprintf(stderr, "set_reference failed: %d\n", r_); st_ret = r_; break; }         \
        if (drec.fn) { if ((r_ = device_recon_write(&drec, be))) { st_ret = r_; break; } }         \
        else if (frec) jm_write_yuv_frame(frec, &rec, inp->width, inp->height);                    \
        double py = psnr_pl(&p_->cur, &rec, 0, inp->width, inp->height);                           \
        double pu = psnr_pl(&p_->cur, &rec, 1, inp->width / 2, inp->height / 2);                   \
        double pv = psnr_pl(&p_->cur, &rec, 2, inp->width / 2, inp->height / 2);                   \
        st->psnr_y += py; st->psnr_u += pu; st->psnr_v += pv;                                      \
        st->bits += pic_bits;                                                                      \
        st->frames++;                                                                              \
        if (log)                                                                                   \
            fprintf(log, "%4d(%s) %8ld   %2d %7.4f %7.4f %7.4f %9.1f %7.1f    FRM\n", p_->f,          \
                    p_->is_i ? "IDR" : " P ", pic_bits, p_->fp.qp, py, pu, pv, t3 - t1 + (MET_MS), (MET_MS)); \
    } while (0)
    #define PEND_SLICE(P, SL)                                                                      \
    do {                                                                                           \
        (SL).idr = (P)->f == 0; (SL).slice_type = (P)->fp.slice_type; (SL).frame_num = (P)->frame_num; \
        (SL).poc_lsb = 2 * (P)->f; (SL).idr_pic_id = 0; (SL).qp = (P)->fp.qp; (SL).first_mb = 0;      \
    } while (0)
    /* DeviceWriterAsync: the oldest picture's slice bytes and SSDs; headers + bytes to the stream, the
       PSNR from the SSDs, the picture itself only for the recon file */
    #define EMIT_CODED(SLOT, MET_MS)                                                               \
    do {                                                                                           \
        pend_t *p_ = &pend[(SLOT)];                                                                \
        double t1 = now_ms();                                                                      \
        jm_slice sl;                                                                               \
        PEND_SLICE(p_, sl);                                                                        \
        if (nal) {                                                                                 \
            const dcavlc_t *d_ = &pdc[(SLOT)];                                                     \
            jm_bits_append_bytes(&out, dc.buf, (long)(d_->cw[d_->n - 1].offset + d_->cw[d_->n - 1].nbytes)); \
        } else device_slice_assemble(&pdc[(SLOT)], &s, &sl, dc.buf, &out);                         \
        double t2 = now_ms();                                                                      \
        st->entropy_ms += t2 - t1;                                                                 \
        long pic_bits = out.len * 8;                                                               \
        fwrite(out.buf, 1, out.len, fout);                                                         \
        out.len = 0;                                                                               \
        if (drec.fn) { int r_ = device_recon_write(&drec, be); if (r_) { st_ret = r_; break; } }   \
        else if (frec) {                                                                           \
            int r_ = be->read_deblocked(be->ctx, &rec);                                            \
            if (r_) { fprintf(stderr, "read_deblocked failed: %d\n", r_); st_ret = r_; break; }    \
            jm_write_yuv_frame(frec, &rec, inp->width, inp->height);                               \
        }                                                                                          \
        double t3 = now_ms();                                                                      \
        st->deblock_ms += t3 - t2;                                                                 \
        double py = jm_psnr_from_ssd(cstats.ssd[0], inp->width, inp->height, bd);                  \
        double pu = jm_psnr_from_ssd(cstats.ssd[1], inp->width / 2, inp->height / 2, bd);          \
        double pv = jm_psnr_from_ssd(cstats.ssd[2], inp->width / 2, inp->height / 2, bd);          \
        st->psnr_y += py; st->psnr_u += pu; st->psnr_v += pv;                                      \
        st->bits += pic_bits;                                                                      \
        st->frames++;                                                                              \
        coded_fallbacks += cstats.fallback;                                                        \
        if (log)                                                                                   \
            fprintf(log, "%4d(%s) %8ld   %2d %7.4f %7.4f %7.4f %9.1f %7.1f    FRM\n", p_->f,          \
                    p_->is_i ? "IDR" : " P ", pic_bits, p_->fp.qp, py, pu, pv, t3 - t1 + (MET_MS), (MET_MS)); \
    } while (0)
    jmh_coded_stats cstats;
    memset(&cstats, 0, sizeof(cstats));
    int coded_fallbacks = 0;
    for (int f = 0; f < inp->frames && !st_ret; f++) {
        if (pipelined && count == depth) {   /* the oldest picture's results */
            double t0 = now_ms();
            int r = async ? device_coded_pop(&dc, &pdc[head], be, &cstats) : be->pop(be->ctx);
            double met = now_ms() - t0;
            if (r) { fprintf(stderr, "hot path backend '%s' failed: status %d\n", be->name, r); st_ret = r; break; }
            st->me_tq_ms += met;
            pop_ms += met;
            if (async) EMIT_CODED(head, met);
            else EMIT(&pend[head], met);
            if (st_ret) break;
            head = (head + 1) % plen;
            count--;
        }
        pend_t *p = &pend[(head + count) % plen];
        int idx = inp->start_frame + f;
        double tr = now_ms();
        if (raw_source) {
            if (fseek(fin, (long)rgb_bytes * idx, SEEK_SET) || fread(rgb, 1, rgb_bytes, fin) != rgb_bytes) { fprintf(stderr, "ReadOneFrame: cannot read %s frame %d\n", src.kind == JM_SRC_YUV ? "YUV" : "RGB", idx); st_ret = JMH_E_INVALID_ARG; break; }
        } else
        if (synthetic) jm_synth_frame(&p->cur, inp->width, inp->height, seed, idx);
        else if (jm_read_yuv_frame(fin, scale ? &big : &p->cur, src_w, src_h, idx)) { fprintf(stderr, "ReadOneFrame: cannot read frame %d\n", idx); st_ret = JMH_E_INVALID_ARG; break; }
        read_ms += now_ms() - tr;
        src.pic = raw_source ? NULL : scale ? &big : &p->cur;   /* 4:2:0 planes: the picture just read */
        p->f = f;
        p->is_i = f == 0 || (inp->intra_period && f % inp->intra_period == 0);
        p->frame_num = frame_num++;
        jmh_frame_params *fp = &p->fp;
        memset(fp, 0, sizeof(*fp));
        fp->slice_type = p->is_i ? JMH_I_SLICE : JMH_P_SLICE;
        fp->qp = p->is_i ? inp->qp_i : inp->qp_p;
        fp->lambda_mode = fp->lambda_motion = jm_lambda_rdo_off(fp->qp);
        if (inp->rdopt) fp->lambda_rd = jm_lambda_rdo_on(fp->qp, inp->bit_depth_luma, &fp->lambda_factor_rd);
        fp->chroma_qp_offset = inp->chroma_qp_offset;
        if (dev_dbk) {   /* same parameters jm_deblock_picture derives from the slice header */
            fp->deblock = 1;
            fp->lf_disable = s.lf_params_flag ? s.lf_disable : 0;
            fp->lf_alpha_div2 = s.lf_params_flag ? s.lf_alpha : 0;
            fp->lf_beta_div2 = s.lf_params_flag ? s.lf_beta : 0;
        }
        double t0 = now_ms();
        int r = 0;
        if (dev_dbk && !p->is_i) r = be->reference_deblocked(be->ctx);   /* previous picture, on the device */
        if (!r && async) {   /* the slice headers now: everything they carry is known at the push */
            dcavlc_t *d = &pdc[(head + count) % plen];
            jm_slice sl;
            PEND_SLICE(p, sl);
            device_slice_headers(d, &s, &sl);
            if (nal && !(r = device_slice_heads(d, &sl))) r = device_nal_fn(be->ctx, d->n, d->nh);
            if (!r) r = device_input_fn ? device_input_fn(be->ctx, &src, fp, d->n, d->cs, inp->width, inp->height)
                                        : device_coded_push_fn(be->ctx, &p->cur, fp, d->n, d->cs, inp->width, inp->height);
        } else
        if (!r) r = device_input_fn ? device_input_fn(be->ctx, &src, fp, 0, NULL, 0, 0)
                  : pipelined ? be->push(be->ctx, &p->cur, fp) : be->encode_frame(be->ctx, &p->cur, fp);
        double met = now_ms() - t0;
        if (r) { fprintf(stderr, "hot path backend '%s' failed: status %d\n", be->name, r); st_ret = r; break; }
        st->me_tq_ms += met;
        push_ms += met;
        if (pipelined) count++;
        else EMIT(p, met);
    }
    while (pipelined && count && !st_ret) {
        double t0 = now_ms();
        int r = async ? device_coded_pop(&dc, &pdc[head], be, &cstats) : be->pop(be->ctx);
        double met = now_ms() - t0;
        if (r) { fprintf(stderr, "hot path backend '%s' failed: status %d\n", be->name, r); st_ret = r; break; }
        st->me_tq_ms += met;
        if (async) EMIT_CODED(head, met);
        else EMIT(&pend[head], met);
        head = (head + 1) % plen;
        count--;
    }
    while (nwr && jflushed < jseq && !st_ret) FLUSH_JOB(&pool.jobs[jflushed % nj]);
    if (log && async && coded_fallbacks)
        fprintf(log, " (%d pictures exceeded the writer's queued capacity and were coded by the synchronous call)\n", coded_fallbacks);
    #undef EMIT
    #undef EMIT_CODED
    #undef PEND_SLICE
    #undef SUBMIT
    #undef FLUSH_JOB
    st->total_ms = now_ms() - t_start;
cleanup:
    jm_source_padding(1);
    /* one teardown for every exit: stop and join the writer threads that started, free what
       was allocated (also after a partial setup) */
    if (nstarted) {
        pthread_mutex_lock(&pool.mu);
        pool.stop = 1;
        pthread_cond_broadcast(&pool.cv_work);
        pthread_mutex_unlock(&pool.mu);
        for (int k = 0; k < nstarted; k++) pthread_join(pool.th[k], NULL);
    }
    for (int k = 0; k < njobs_init; k++) { jm86_free(&pool.jobs[k].im); jm_pic_free(&pool.jobs[k].rec); jm_bits_free(&pool.jobs[k].out); }
    if (pool_sync) {
        pthread_mutex_destroy(&pool.mu);
        pthread_cond_destroy(&pool.cv_work);
        pthread_cond_destroy(&pool.cv_done);
    }
    free(pool.jobs); free(pool.queue); free(pool.th);
    dcavlc_free(&dc);
    if (pdc) for (int k = 0; k < plen; k++) dcavlc_free(&pdc[k]);
    free(pdc);
    img = &im;
    st->surface_checked = im.surface_checked;
    st->surface_searches = im.surface_searches;
    st->surface_mismatches = im.surface_mismatches;
    if (log && inp->jm_call_surface)
        fprintf(log, " JM call surface: %d P macroblocks through PartitionMotionSearch / BlockMotionSearch (%d backend "
                     "searches), %d inconsistent with the wavefront decision\n",
                im.surface_checked, im.surface_searches, im.surface_mismatches);
    if (!st_ret && im.surface_mismatches) st_ret = JMH_E_STATE;
    st->rate_checked = im.rate_checked;
    st->rate_mismatches = im.rate_mismatches;
    if (log && inp->rdopt)
        fprintf(log, " RD rate check: %ld macroblocks, %ld whose RD rate differs from the bits written (CABAC or CAVLC)\n",
                im.rate_checked, im.rate_mismatches);
    if (!st_ret && im.rate_mismatches) st_ret = JMH_E_STATE;
    jm86_free(&im);
    if (st->frames) { st->psnr_y /= st->frames; st->psnr_u /= st->frames; st->psnr_v /= st->frames; }
    if (log && st->frames)
        fprintf(log, " Total encoding time for the seq.  : %.3f sec\n Total ME+TQ time (backend)        : %.3f sec\n"
                     " SNR Y(dB) %.4f U %.4f V %.4f   bits %ld\n",
                st->total_ms / 1e3, st->me_tq_ms / 1e3, st->psnr_y, st->psnr_u, st->psnr_v, st->bits);
    if (log && st->frames)
        fprintf(log, " Host per picture: slice writing + PSNR %.2f ms (%s), results + readback (+ host deblocking) %.2f ms, wall %.2f ms\n",
                st->entropy_ms / st->frames, nwr ? "writer threads" : device_writer ? "the device call, no PSNR" : "main thread", st->deblock_ms / st->frames,
                st->total_ms / st->frames);
    if (log && st->frames)
        fprintf(log, " Main thread per picture: read %.2f ms, push %.2f, pop (wait) %.2f, results to writer %.2f, flush %.2f\n",
                read_ms / st->frames, push_ms / st->frames, pop_ms / st->frames, copy_ms / st->frames, flush_ms / st->frames);
    jm_bits_free(&out);
    free(res);
    for (int k = 0; k < plen; k++) jm_pic_free(&pend[k].cur);
    free(pend);
    free(rgb);
    jm_pic_free(&rec);
    jm_pic_free(&big);
    if (fin) fclose(fin);
    fclose(fout);
    if (frec) fclose(frec);
    free(drec.buf);
    return st_ret;
}
