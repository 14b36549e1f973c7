// jmhip_io.hip — device memory handed in or out by the caller, behind the extern "C" boundary (include/jmhip_input.h,
// jmhip_rgb.h, jmhip_yuv.h, jmhip_tensor.h, jmhip_scale.h, jmhip_output.h): the sources of the device pushes and
// their ingest seams, the scaler's tables and scratch picture, the pulls and converts, the caller's buffers and
// streams.  Host code only: the kernels are behind jmh_launch.h.  The scheduler (jmhip_abi.hip) asks three things
// of it: devsrc_check, devsrc_depth and ingest_queue (jmh_ctx.h).
#include "jmh_ctx.h"
#include "jmh_ingest.h"
#include "jmh_scale.h"
#include "jmh_rgb.h"
#include "jmh_tensor.h"
#include "jmh_output.h"

static_assert(JMS_INVALID == JMH_E_INVALID_ARG && JMS_UNSUPPORTED == JMH_E_UNSUPPORTED_CFG && JMS_TAPS_MAX == JMH_SCALE_TAPS_MAX &&
              JMS_SRC_MAX == JMH_SCALE_SRC_MAX && JMS_LANCZOS3 == JMH_SCALE_LANCZOS3 && JMS_CHROMA_LEFT == JMH_SCALE_CHROMA_LEFT, "jmh_scale.h restates jmhip_scale.h");
static_assert(JMY_I422 == JMH_PIX_I422 && JMY_NV16 == JMH_PIX_NV16 && JMY_YUYV == JMH_PIX_YUYV && JMY_UYVY == JMH_PIX_UYVY && JMY_I444 == JMH_PIX_I444 &&
              JMY_VUYA8 == JMH_PIX_VUYA8 && JMY_I210 == JMH_PIX_I210 && JMY_P210 == JMH_PIX_P210 && JMY_Y210 == JMH_PIX_Y210 && JMY_I410 == JMH_PIX_I410 &&
              JMY_Y410 == JMH_PIX_Y410 && JMY_CHROMA_LEFT == JMH_PIX_CHROMA_LEFT, "jmh_yuv.h restates jmhip_yuv.h");

// ---- device sources ----
// the argument rules of jmhip_input.h (formats 0..3, no flag), of jmhip_rgb.h (16..19 with their flags), of
// jmhip_yuv.h (32..37 and 40..44 with their flag) and of jmhip_tensor.h
int devsrc_check(const jmh_ctx *c, const DevSrc &s) {
    if (!s) return JMH_E_INVALID_ARG;
    const bool sc = c->scale.filter != JMH_SCALE_OFF;   // the source bound is the scaler's, not the coded size
    const int BW = sc ? JMS_SRC_MAX : c->W, BH = sc ? JMS_SRC_MAX : c->H;
    const jmh_device_picture *p = s.pic;
    const jmh_device_tensor *t = s.ten;
    if (t                         ? jmt_check(t->dtype, t->flags, t->width, t->height, BW, BH, t->chan, t->stride_x, t->stride_y)
        : jmr_is_rgb(p->format)   ? jmr_check(p->format, p->width, p->height, BW, BH, p->plane, p->stride)
        : jmy_is_yuv(p->format)   ? jmy_check(p->format, p->width, p->height, BW, BH, p->plane, p->stride)
                                  : jmi_check(p->format, p->width, p->height, BW, BH, p->plane, p->stride)) return JMH_E_INVALID_ARG;
    return sc ? jms_check(s.width(), s.height(), c->scale.out_width, c->scale.out_height, c->scale.filter) : JMH_OK;
}
int devsrc_depth(const jmh_ctx *c, const DevSrc &s) {
    const int f = s.pic ? s.pic->format : 0;
    const bool ok = s.ten ? jmt_depth_ok(s.ten->dtype, c->bd)
                          : jmr_is_rgb(f) ? jmr_depth_ok(f, c->bd) : jmy_is_yuv(f) ? jmy_depth_ok(f, c->bd) : jmi_depth_ok(f, c->bd);
    return ok ? JMH_OK : JMH_E_UNSUPPORTED_CFG;
}

// The tables of a w x h source under the current setting: the cached ones, or built and uploaded on st.  The entry
// given up for them is the one used longest ago: its device memory is released in stream order behind its last
// reader, its host copy after the upload out of it
static int scale_tables(jmh_ctx *c, int w, int h, ScaleTab **out) {
    const jmh_scale &s = c->scale;
    const int key[6] = {w, h, s.out_width, s.out_height, s.filter, s.flags};
    c->scale_tick++;
    ScaleTab *slot = nullptr;
    for (ScaleTab &t : c->scale_tabs)
        if (t.d && !memcmp(t.key, key, sizeof key)) { t.used = c->scale_tick; *out = &t; return JMH_OK; }
    if ((int)c->scale_tabs.size() < SCALE_TABS) {
        c->scale_tabs.reserve(SCALE_TABS);               // entries are referred to by address
        c->scale_tabs.emplace_back();
        slot = &c->scale_tabs.back();
    } else {
        for (ScaleTab &t : c->scale_tabs) if (!slot || t.used < slot->used) slot = &t;
        if (slot->up) HCHK(hipEventSynchronize(slot->up));
        if (slot->d) HCHK(hipFreeAsync(slot->d, c->st));
        slot->d = nullptr;
    }
    if (!slot->up && hipEventCreateWithFlags(&slot->up, hipEventDisableTiming) != hipSuccess) { slot->up = nullptr; return JMH_E_HIP; }
    size_t end = 0;
    std::vector<int32_t> first[2][2];
    std::vector<int16_t> taps[2][2];
    for (int pc = 0; pc < 2; pc++) {
        const int ns[2] = {pc ? w / 2 : w, pc ? h / 2 : h}, nd[2] = {pc ? s.out_width / 2 : s.out_width, pc ? s.out_height / 2 : s.out_height};
        for (int ax = 0; ax < 2; ax++) {
            first[pc][ax].resize(nd[ax]);
            taps[pc][ax].resize((size_t)nd[ax] * JMS_TAPS_MAX);
            const int r = jms_taps(ns[ax], nd[ax], s.filter, pc && !ax && (s.flags & JMH_SCALE_CHROMA_LEFT), first[pc][ax].data(), taps[pc][ax].data(),
                                   &slot->T[pc][ax]);
            if (r) return r;
        }
        // the intermediate rows of k_scale's tallest tile fit its LDS (they do for every T <= JMS_TAPS_MAX)
        if (jms_span(first[pc][1].data(), nd[1], slot->T[pc][1], pc ? c->H / 2 : c->H) > JMS_SPAN_MAX) return JMH_E_UNSUPPORTED_CFG;
        const size_t bytes[4] = {(size_t)nd[0] * 4, (size_t)nd[1] * 4, (size_t)nd[0] * JMS_HPAIRS * 4, (size_t)nd[1] * JMS_VPAIRS * 4};
        for (int i = 0; i < 4; i++) { slot->off[pc][i] = end; end += (bytes[i] + 15) & ~(size_t)15; }
    }
    slot->h.assign(end, 0);
    for (int pc = 0; pc < 2; pc++) {
        memcpy(slot->h.data() + slot->off[pc][0], first[pc][0].data(), first[pc][0].size() * 4);
        memcpy(slot->h.data() + slot->off[pc][1], first[pc][1].data(), first[pc][1].size() * 4);
        jms_pack_axis(first[pc][0].data(), taps[pc][0].data(), (int)first[pc][0].size(), slot->T[pc][0], 0, (uint32_t *)(slot->h.data() + slot->off[pc][2]));
        jms_pack_axis(first[pc][1].data(), taps[pc][1].data(), (int)first[pc][1].size(), slot->T[pc][1], 1, (uint32_t *)(slot->h.data() + slot->off[pc][3]));
    }
    if (hipMallocAsync((void **)&slot->d, end, c->st) != hipSuccess) { slot->d = nullptr; return JMH_E_OOM; }
    HCHK(hipMemcpyAsync(slot->d, slot->h.data(), end, hipMemcpyHostToDevice, c->st));
    HCHK(hipEventRecord(slot->up, c->st));
    memcpy(slot->key, key, sizeof key);
    slot->used = c->scale_tick;
    *out = slot;
    return JMH_OK;
}

// With a scale set an ingest kernel packs its w x h source at its own size, rounded up to macroblocks, into the
// context's scratch picture (scale_begin: where, and its size), and k_scale resamples that into dst (scale_end).
// The scratch picture grows by a release and an allocation in stream order: behind its last reader
static int scale_begin(jmh_ctx *c, int w, int h, uint8_t **out, int *W, int *H, ScaleTab **tab) {
    int r = scale_tables(c, w, h, tab);
    if (r) return r;
    const int sW = (w + 15) & ~15, sH = (h + 15) & ~15;
    const size_t need = (size_t)sW * sH * 3 / 2 * c->ps;
    if (need > c->scl_cap) {
        if (c->d_scl) HCHK(hipFreeAsync(c->d_scl, c->st));
        c->d_scl = nullptr; c->scl_cap = 0;
        if (hipMallocAsync((void **)&c->d_scl, need, c->st) != hipSuccess) { c->d_scl = nullptr; return JMH_E_OOM; }
        c->scl_cap = need;
    }
    *out = c->d_scl; *W = sW; *H = sH;
    return JMH_OK;
}
static int scale_end(jmh_ctx *c, const ScaleTab *t, int w, int h, int sW, int sH, uint8_t *dst) {
    ScaleArgs a;
    a.src = c->d_scl; a.dst = dst;
    a.w = w; a.h = h; a.sW = sW; a.sH = sH; a.ow = t->key[2]; a.oh = t->key[3]; a.W = c->W; a.H = c->H;
    for (int pc = 0; pc < 2; pc++) {
        a.fh[pc] = (const int32_t *)(t->d + t->off[pc][0]); a.fv[pc] = (const int32_t *)(t->d + t->off[pc][1]);
        a.th[pc] = (const uint32_t *)(t->d + t->off[pc][2]); a.tv[pc] = (const uint32_t *)(t->d + t->off[pc][3]);
        a.nph[pc] = t->T[pc][0] / 2; a.npv[pc] = t->T[pc][1] / 2 + 1; a.tv_taps[pc] = t->T[pc][1];
    }
    a.maxv = c->maxv; a.P = 14 - c->bd;
    HCHK(jmh_launch_scale(a, c->st));
    return JMH_OK;
}

int ingest_queue(jmh_ctx *c, const DevSrc &s, uint8_t *dst, int slot, hipEvent_t ev) {
    if (s.stream()) {
        HCHK(hipEventRecord(ev, (hipStream_t)s.stream()));
        HCHK(hipStreamWaitEvent(c->st, ev, 0));
    }
    const int w = s.width(), h = s.height();
    uint8_t *out = dst;
    int W = c->W, H = c->H, r;
    ScaleTab *tab = nullptr;
    if (c->scale.filter != JMH_SCALE_OFF && (r = scale_begin(c, w, h, &out, &W, &H, &tab))) return r;
    unsigned long long *clamped = nullptr;
    if (s.counts()) {
        const size_t nb = (size_t)(c->nring + 1) * sizeof(unsigned long long);
        if (!c->d_clamp && hipMalloc((void **)&c->d_clamp, nb) != hipSuccess) { c->d_clamp = nullptr; return JMH_E_OOM; }
        if (!c->h_clamp && hipHostMalloc((void **)&c->h_clamp, nb, hipHostMallocDefault) != hipSuccess) { c->h_clamp = nullptr; return JMH_E_OOM; }
        clamped = c->d_clamp + slot;
        HCHK(hipMemsetAsync(clamped, 0, sizeof(unsigned long long), c->st));
    }
    const jmh_device_picture *p = s.pic;
    if (const jmh_device_tensor *t = s.ten) {   // k_ingest_tensor: quantised and converted, nothing counted
        TensorArgs g;
        for (int i = 0; i < 3; i++) g.chan[i] = (const uint8_t *)t->chan[i];
        g.sx = t->stride_x; g.sy = t->stride_y;
        g.dst = out; g.w = w; g.h = h; g.W = W; g.H = H;
        jmr_coefficients(t->flags, c->bd, &g.k);
        HCHK(jmh_launch_ingest_tensor(t->dtype, g, c->st));
    } else if (jmr_is_rgb(p->format)) {   // k_ingest_rgb: one plane, nothing counted
        RgbArgs g;
        g.src = (const uint8_t *)p->plane[0]; g.stride = p->stride[0];
        g.dst = out; g.w = w; g.h = h; g.W = W; g.H = H;
        jmr_coefficients(p->format, c->bd, &g.k);
        HCHK(jmh_launch_ingest_rgb(p->format, g, c->st));
    } else if (jmy_is_yuv(p->format)) {   // k_ingest_yuv: 4:2:2 / 4:4:4 reduced to 4:2:0 (planes the layout does not read stay null)
        YuvArgs g;
        for (int i = 0; i < 3; i++) {
            const bool read = i < jmy_planes(jmy_layout(p->format));
            g.plane[i] = read ? (const uint8_t *)p->plane[i] : nullptr; g.stride[i] = read ? p->stride[i] : 0;
        }
        g.dst = out; g.w = w; g.h = h; g.W = W; g.H = H; g.maxv = (uint32_t)c->maxv; g.clamped = clamped;
        HCHK(jmh_launch_ingest_yuv(p->format, g, c->st));
    } else {
        IngestArgs a;
        for (int i = 0; i < 3; i++) { a.plane[i] = (const uint8_t *)p->plane[i]; a.stride[i] = p->stride[i]; }
        a.dst = out; a.w = w; a.h = h; a.W = W; a.H = H; a.maxv = (uint32_t)c->maxv; a.clamped = clamped;
        HCHK(jmh_launch_ingest(p->format, a, c->st));
    }
    if (clamped) HCHK(hipMemcpyAsync(c->h_clamp + slot, clamped, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->st));
    return tab ? scale_end(c, tab, w, h, W, H, dst) : JMH_OK;
}

// the unit seam of the ingest kernels: the source's kernel into a scratch picture, the packed planes to the host
static int ingest_seam(jmh_ctx *c, const DevSrc &s, void *y, void *u, void *v, int sy, int sc) {
    if (!c || !y || !u || !v || sy < c->W || sc < c->Wc) return JMH_E_INVALID_ARG;
    int r = devsrc_check(c, s);
    if (r || (r = devsrc_depth(c, s))) return r;
    HCHK(hipSetDevice(c->dev));
    DevTemps t;
    uint8_t *d = nullptr;
    if (t.alloc(&d, c->fsize) != hipSuccess) return JMH_E_OOM;
    hipEvent_t ev = nullptr;
    if (s.stream()) HCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    r = ingest_queue(c, s, d, c->nring, ev);
    if (!r && s.stream() && (hipEventRecord(ev, c->st) != hipSuccess || hipStreamWaitEvent((hipStream_t)s.stream(), ev, 0) != hipSuccess))
        r = JMH_E_HIP;
    const hipError_t se = hipStreamSynchronize(c->st);
    if (ev) (void)hipEventDestroy(ev);
    if (r) return r;
    HCHK(se);
    std::vector<uint8_t> h(c->fsize);
    HCHK(hipMemcpy(h.data(), d, c->fsize, hipMemcpyDeviceToHost));
    unpack_planes(h.data(), c->W, c->H, y, u, v, sy, sc, c->ps);
    c->last_clamped = s.counts() ? c->h_clamp[c->nring] : 0;
    return JMH_OK;
}

// ---- decoded pictures pulled on the device (include/jmhip_output.h) ----
// the destination of a pull: a picture or a tensor
struct PullDst { const jmh_device_picture_out *pic; const jmh_device_tensor_out *ten; };

// the argument rules, then the context's bit depth
static int check_pull_dst(const jmh_ctx *c, const PullDst &d) {
    if (d.pic) {
        const jmh_device_picture_out *p = d.pic;
        if (jmout_check_picture(p->format, p->width, p->height, c->W, c->H, p->plane, p->stride)) return JMH_E_INVALID_ARG;
        return jmout_picture_depth_ok(p->format, c->bd) ? JMH_OK : JMH_E_UNSUPPORTED_CFG;
    }
    const jmh_device_tensor_out *t = d.ten;
    if (!t || jmout_check_tensor(t->dtype, t->flags, t->width, t->height, c->W, c->H, t->chan, t->stride_x, t->stride_y)) return JMH_E_INVALID_ARG;
    return jmout_tensor_depth_ok(t->dtype, c->bd) ? JMH_OK : JMH_E_UNSUPPORTED_CFG;
}
static int output_stream(jmh_ctx *c) {
    if (!c->ost && hipStreamCreateWithFlags(&c->ost, hipStreamNonBlocking) != hipSuccess) { c->ost = nullptr; return JMH_E_HIP; }
    return JMH_OK;
}
// the one kernel of a (checked) destination, reading the packed picture at src, on st
static int pull_launch(jmh_ctx *c, const PullDst &d, const uint8_t *src, hipStream_t st) {
    OutArgs a;
    a.src = src; a.W = c->W; a.H = c->H;
    if (d.pic) {
        const jmh_device_picture_out *p = d.pic;
        for (int i = 0; i < 3; i++) { a.dst[i] = (uint8_t *)p->plane[i]; a.stride[i] = p->stride[i]; }
        a.w = p->width; a.h = p->height;
        jmout_coefficients(p->format, c->bd, &a.k);   // a YUV format reads none of them
        HCHK(jmh_launch_pull_picture(p->format, a, st));
    } else {
        const jmh_device_tensor_out *t = d.ten;
        for (int i = 0; i < 3; i++) a.dst[i] = (uint8_t *)t->chan[i];
        a.stride[0] = t->stride_x; a.stride[1] = t->stride_y; a.stride[2] = 0;
        a.w = t->width; a.h = t->height;
        jmout_coefficients(t->flags, c->bd, &a.k);
        HCHK(jmh_launch_pull_tensor(t->dtype, a, st));
    }
    return JMH_OK;
}
// jmh_pull_picture / jmh_pull_tensor.  The current picture is complete (its pop waited for it), so the
// kernel waits for nothing but its stream: the caller's, where it is ordered behind the destination's
// last consumer and in front of its next one, or the context's own, waited for here.  The entry's
// event then holds the pull, for the claim that rewrites the entry (claim_entry) and for output_wait;
// an earlier pull of the entry on another stream is chained in front, so one event holds them all.
static int pull_any(jmh_ctx *c, int which, const PullDst &d, void *stream) {
    if (which != JMOUT_DEBLOCKED && which != JMOUT_RECON) return JMH_E_INVALID_ARG;
    int r = check_pull_dst(c, d);
    if (r) return r;
    if (c->cur_entry < 0) return JMH_E_STATE;
    PicBuf &b = c->ring[c->cur_entry];
    if (which == JMOUT_DEBLOCKED && !b.deblocked) return JMH_E_STATE;
    HCHK(hipSetDevice(c->dev));
    hipStream_t st = (hipStream_t)stream;
    if (!st) { if ((r = output_stream(c))) return r; st = c->ost; }
    if (b.ev_out) HCHK(hipStreamWaitEvent(st, b.ev_out, 0));
    else if (hipEventCreateWithFlags(&b.ev_out, hipEventDisableTiming) != hipSuccess) { b.ev_out = nullptr; return JMH_E_HIP; }
    if ((r = pull_launch(c, d, which == JMOUT_DEBLOCKED ? b.dbk : b.rec, st))) return r;
    HCHK(hipEventRecord(b.ev_out, st));
    if (!stream) HCHK(hipStreamSynchronize(st));
    return JMH_OK;
}
// jmh_convert_picture / jmh_convert_tensor: the host planes packed, uploaded to a scratch picture, the
// same kernel, everything on the context's output stream and waited for
static int convert_any(jmh_ctx *c, const void *y, const void *u, const void *v, int sy, int sc, const PullDst &d, void *stream) {
    int r = check_pull_dst(c, d);
    if (r) return r;
    if (!y || !u || !v || sy < c->W || sc < c->Wc) return JMH_E_INVALID_ARG;
    HCHK(hipSetDevice(c->dev));
    if ((r = output_stream(c))) return r;
    std::vector<uint8_t> h(c->fsize);
    if (!pack_planes(h.data(), c->W, c->H, y, u, v, sy, sc, c->ps, c->maxv)) return JMH_E_INVALID_ARG;
    DevTemps tmp;
    uint8_t *src = nullptr;
    if (tmp.alloc(&src, c->fsize) != hipSuccess) return JMH_E_OOM;
    if (stream) HCHK(hipStreamSynchronize((hipStream_t)stream));   // the destination's last consumer
    hipError_t e = hipMemcpyAsync(src, h.data(), c->fsize, hipMemcpyHostToDevice, c->ost);
    if (e == hipSuccess) r = pull_launch(c, d, src, c->ost);
    const hipError_t se = hipStreamSynchronize(c->ost);   // before src and h are freed, whatever happened
    HCHK(e);
    if (r) return r;
    HCHK(se);
    return JMH_OK;
}

extern "C" {

// ---- the ingest seams (include/jmhip_input.h, jmhip_tensor.h) ----
int jmh_ingest_picture(jmh_ctx *c, const jmh_device_picture *pic, void *y, void *u, void *v, int sy, int sc) {
    return ingest_seam(c, DevSrc{pic, nullptr}, y, u, v, sy, sc);
}
int jmh_ingest_tensor(jmh_ctx *c, const jmh_device_tensor *t, void *y, void *u, void *v, int sy, int sc) {
    return ingest_seam(c, DevSrc{nullptr, t}, y, u, v, sy, sc);
}

// ---- jmhip_scale.h: the sticky setting of the device pushes, its tables on the host, the setting read back ----
int jmh_input_scale(jmh_ctx *c, const jmh_scale *s) {
    if (!c) return JMH_E_INVALID_ARG;
    if (!s || s->filter == JMH_SCALE_OFF) { c->scale = jmh_scale{0, 0, 0, 0}; return JMH_OK; }
    if (jms_check_setting(s->filter, s->flags, s->out_width, s->out_height, c->W, c->H)) return JMH_E_INVALID_ARG;
    c->scale = *s;
    return JMH_OK;
}
int jmh_scale_taps(int n_src, int n_dst, int filter, int chroma_left, int32_t *first, int16_t *taps, int *ntaps) {
    return jms_taps(n_src, n_dst, filter, chroma_left != 0, first, taps, ntaps);
}
int jmh_scale_info(const jmh_ctx *c, jmh_scale *s, int *active) {
    if (!c || !s || !active) return JMH_E_INVALID_ARG;
    *s = c->scale;
    *active = c->scale.filter != JMH_SCALE_OFF;
    return JMH_OK;
}

// ---- the caller's side of a device push (include/jmhip_input.h) ----
int jmh_device_input_wait(jmh_ctx *c) {
    if (!c) return JMH_E_INVALID_ARG;
    if (c->last_dev_entry < 0) return JMH_OK;
    HCHK(hipSetDevice(c->dev));
    HCHK(hipEventSynchronize(c->ring[c->last_dev_entry].ev_src));   // (a later occupant's event has passed the picture's too)
    return JMH_OK;
}
int jmh_device_input_clamped(const jmh_ctx *c, uint64_t *n) {
    if (!c || !n) return JMH_E_INVALID_ARG;
    *n = c->last_clamped;
    return JMH_OK;
}
int jmh_device_malloc(jmh_ctx *c, size_t n, void **p) {
    if (!c || !p || !n) return JMH_E_INVALID_ARG;
    HCHK(hipSetDevice(c->dev));
    if (hipMalloc(p, n) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return JMH_E_OOM; }
    return JMH_OK;
}
int jmh_device_free(jmh_ctx *c, void *p) {
    if (!c) return JMH_E_INVALID_ARG;
    HCHK(hipSetDevice(c->dev));
    if (p) HCHK(hipFree(p));
    return JMH_OK;
}
int jmh_device_upload(jmh_ctx *c, void *dst, const void *src, size_t n, void *stream) {
    if (!c || !dst || !src) return JMH_E_INVALID_ARG;
    if (!n) return JMH_OK;
    HCHK(hipSetDevice(c->dev));
    if (!stream) {
        HCHK(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
        return JMH_OK;
    }
    // through the context's pinned buffer: src is free on return, the copy itself runs on the stream
    if (!c->ev_up) { if (hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming) != hipSuccess) { c->ev_up = nullptr; return JMH_E_HIP; } }
    else HCHK(hipEventSynchronize(c->ev_up));
    if (n > c->up_cap) {
        if (c->up_h) (void)hipHostFree(c->up_h);
        c->up_h = nullptr; c->up_cap = 0;
        if (hipHostMalloc((void **)&c->up_h, n, hipHostMallocDefault) != hipSuccess) { c->up_h = nullptr; return JMH_E_OOM; }
        c->up_cap = n;
    }
    memcpy(c->up_h, src, n);
    HCHK(hipMemcpyAsync(dst, c->up_h, n, hipMemcpyHostToDevice, (hipStream_t)stream));
    HCHK(hipEventRecord(c->ev_up, (hipStream_t)stream));
    return JMH_OK;
}
int jmh_device_stream_create(jmh_ctx *c, void **stream) {
    if (!c || !stream) return JMH_E_INVALID_ARG;
    HCHK(hipSetDevice(c->dev));
    hipStream_t st = nullptr;
    HCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = st;
    return JMH_OK;
}
int jmh_device_stream_destroy(jmh_ctx *c, void *stream) {
    if (!c || !stream) return JMH_E_INVALID_ARG;
    HCHK(hipSetDevice(c->dev));
    HCHK(hipStreamSynchronize((hipStream_t)stream));
    HCHK(hipStreamDestroy((hipStream_t)stream));
    return JMH_OK;
}

// ---- pulls, converts and downloads (include/jmhip_output.h) ----
int jmh_pull_picture(jmh_ctx *c, int which, const jmh_device_picture_out *dst) {
    if (!c || !dst) return JMH_E_INVALID_ARG;
    return pull_any(c, which, PullDst{dst, nullptr}, dst->stream);
}
int jmh_pull_tensor(jmh_ctx *c, int which, const jmh_device_tensor_out *dst) {
    if (!c || !dst) return JMH_E_INVALID_ARG;
    return pull_any(c, which, PullDst{nullptr, dst}, dst->stream);
}
int jmh_convert_picture(jmh_ctx *c, const void *y, const void *u, const void *v, int sy, int sc, const jmh_device_picture_out *dst) {
    if (!c || !dst) return JMH_E_INVALID_ARG;
    return convert_any(c, y, u, v, sy, sc, PullDst{dst, nullptr}, dst->stream);
}
int jmh_convert_tensor(jmh_ctx *c, const void *y, const void *u, const void *v, int sy, int sc, const jmh_device_tensor_out *dst) {
    if (!c || !dst) return JMH_E_INVALID_ARG;
    return convert_any(c, y, u, v, sy, sc, PullDst{nullptr, dst}, dst->stream);
}
int jmh_device_output_wait(jmh_ctx *c) {
    if (!c) return JMH_E_INVALID_ARG;
    HCHK(hipSetDevice(c->dev));
    return output_wait(c);
}
int jmh_device_download(jmh_ctx *c, void *dst, const void *src, size_t n, void *stream) {
    if (!c || !dst || !src) return JMH_E_INVALID_ARG;
    if (!n) return JMH_OK;
    HCHK(hipSetDevice(c->dev));
    hipStream_t st = (hipStream_t)stream;
    if (!st) { int r = output_stream(c); if (r) return r; st = c->ost; }
    HCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    return JMH_OK;
}

// ---- helpers that need no context ----
// the quantiser of a tensor's elements (include/jmhip_tensor.h) on the host
int jmh_tensor_quantise(int dtype, int bit_depth, const void *elems, size_t n, int32_t *q) {
    if (dtype < 0 || dtype >= JMT_NDTYPES || (n && (!elems || !q))) return JMH_E_INVALID_ARG;
    if (!jmt_depth_ok(dtype, bit_depth)) return JMH_E_UNSUPPORTED_CFG;
    const int32_t M = (1 << bit_depth) - 1;
    const uint8_t *p = (const uint8_t *)elems;
    for (size_t i = 0; i < n; i++) q[i] = jmt_quant(dtype, jmt_load(dtype, p + i * jmt_es(dtype)), M);
    return JMH_OK;
}
// the dequantiser of a tensor's elements on the host
int jmh_tensor_dequantise(int dtype, int bit_depth, const int32_t *q, size_t n, void *elems) {
    if (dtype < 0 || dtype >= JMT_NDTYPES || (n && (!elems || !q))) return JMH_E_INVALID_ARG;
    if (!jmt_depth_ok(dtype, bit_depth)) return JMH_E_UNSUPPORTED_CFG;
    const int32_t M = (1 << bit_depth) - 1;
    uint8_t *p = (uint8_t *)elems;
    for (size_t i = 0; i < n; i++) jmout_put(p + i * jmt_es(dtype), jmt_es(dtype), jmout_dequant(dtype, jmr_clip(q[i], M), M));
    return JMH_OK;
}
// the conversion of an RGB format (include/jmhip_rgb.h)
int jmh_rgb_coefficients(int format, int bit_depth, int32_t out[12]) {
    if (!out || !jmr_is_rgb(format)) return JMH_E_INVALID_ARG;
    if (!jmr_depth_ok(format, bit_depth)) return JMH_E_UNSUPPORTED_CFG;
    jmr_coef k;
    jmr_coefficients(format, bit_depth, &k);
    memcpy(out, k.c, sizeof(k.c));
    out[9] = k.yo; out[10] = k.co; out[11] = k.maxv;
    return JMH_OK;
}
// the inverse conversion of the flags (include/jmhip_output.h)
int jmh_yuv_coefficients(int flags, int bit_depth, int32_t out[8]) {
    if (!out || (flags & ~JMR_FLAGS) || (bit_depth != 8 && bit_depth != 10)) return JMH_E_INVALID_ARG;
    jmout_coef k;
    jmout_coefficients(flags, bit_depth, &k);
    const int32_t w[8] = {k.iy, k.irv, k.igu, k.igv, k.ibu, k.yo, k.co, k.maxv};
    memcpy(out, w, sizeof(w));
    return JMH_OK;
}

}  // extern "C"
