/*
 * lencod.c — product encoder binary: JM 8.6 lencod.c › main [J] with the macroblock hot path
 * bound to the MI355X C ABI (libjmhip.so).  There is no CPU fallback: if no HIP device is
 * usable the run fails with the jmh_* status, as JM's error() would.
 */
#include <stdlib.h>
#include <string.h>
#include "jmhost.h"

/* 8-bit pictures through the uint8_t entry points, High 10 ones through the _u16 ones */
static int gpu_set_ref(void *ctx, const jm_pic *p) {
    if (p->bd > 8) return jmh_set_reference_u16((jmh_ctx *)ctx, 0, 0, p->Y, p->U, p->V, p->w, p->w / 2);
    return jmh_set_reference((jmh_ctx *)ctx, 0, 0, p->y, p->u, p->v, p->w, p->w / 2);
}
static int gpu_encode(void *ctx, const jm_pic *cur, const jmh_frame_params *fp) {
    int r = cur->bd > 8 ? jmh_frame_submit_u16((jmh_ctx *)ctx, cur->Y, cur->U, cur->V, cur->w, cur->w / 2, fp)
                        : jmh_frame_submit((jmh_ctx *)ctx, cur->y, cur->u, cur->v, cur->w, cur->w / 2, fp);
    return r ? r : jmh_frame_wait((jmh_ctx *)ctx);
}
static const jmh_mb_result *gpu_res(void *ctx, int a) { return jmh_get_mb_result((const jmh_ctx *)ctx, a); }
static int gpu_recon(void *ctx, jm_pic *p) {
    if (p->bd > 8) return jmh_read_recon_u16((jmh_ctx *)ctx, p->Y, p->U, p->V, p->w, p->w / 2);
    return jmh_read_recon((jmh_ctx *)ctx, p->y, p->u, p->v, p->w, p->w / 2);
}
static void gpu_destroy(void *ctx) { jmh_destroy((jmh_ctx *)ctx); }
static int gpu_deblocked(void *ctx, jm_pic *p) {
    if (p->bd > 8) return jmh_read_deblocked_u16((jmh_ctx *)ctx, p->Y, p->U, p->V, p->w, p->w / 2);
    return jmh_read_deblocked((jmh_ctx *)ctx, p->y, p->u, p->v, p->w, p->w / 2);
}
static int gpu_ref_deblocked(void *ctx) { return jmh_set_reference_slot((jmh_ctx *)ctx, -2); }
static int gpu_push(void *ctx, const jm_pic *cur, const jmh_frame_params *fp) {
    if (cur->bd > 8) return jmh_frame_push_u16((jmh_ctx *)ctx, cur->Y, cur->U, cur->V, cur->w, cur->w / 2, fp);
    return jmh_frame_push((jmh_ctx *)ctx, cur->y, cur->u, cur->v, cur->w, cur->w / 2, fp);
}
static int gpu_pop(void *ctx) { return jmh_frame_pop((jmh_ctx *)ctx); }
static int gpu_search_pictures(void *ctx, const jm_pic *cur, const jm_pic *ref) {
    return jmh_search_pictures((jmh_ctx *)ctx, cur->y, ref->y, cur->w);
}
static int gpu_block_search(void *ctx, int n, const jmh_block_search *q, jmh_block_result *r) {
    return jmh_block_motion_search((jmh_ctx *)ctx, n, q, r);
}
static int gpu_tq4x4(void *ctx, int n, const int16_t *resid, const uint8_t *pred, int qp, int intra, int16_t *lev, uint8_t *rec,
                     int32_t *cc, int32_t *nz) {
    return jmh_tq4x4_batch((jmh_ctx *)ctx, n, resid, pred, qp, intra, lev, rec, cc, nz);
}
static int gpu_cavlc_slices(void *ctx, int n, const jmh_slice_desc *d, uint8_t *out, size_t cap, jmh_slice_bytes *where) {
    return jmh_cavlc_write_slices((jmh_ctx *)ctx, n, d, out, cap, where);
}
static int gpu_cabac_slices(void *ctx, int n, const jmh_cabac_slice_desc *d, uint8_t *out, size_t cap, jmh_cabac_slice_bytes *where) {
    return jmh_cabac_write_slices((jmh_ctx *)ctx, n, d, out, cap, where);
}
static int gpu_cabac_split(void *ctx, int chunk_bins) { return jmh_cabac_set_split((jmh_ctx *)ctx, chunk_bins); }
static int gpu_push_coded(void *ctx, const jm_pic *cur, const jmh_frame_params *fp, int n, const jmh_coded_slice *sl, int cw, int ch) {
    if (cur->bd > 8) return jmh_frame_push_coded_u16((jmh_ctx *)ctx, cur->Y, cur->U, cur->V, cur->w, cur->w / 2, fp, n, sl, cw, ch);
    return jmh_frame_push_coded((jmh_ctx *)ctx, cur->y, cur->u, cur->v, cur->w, cur->w / 2, fp, n, sl, cw, ch);
}
static int gpu_nal_heads(void *ctx, int n, const jmh_nal_head *heads) { return jmh_coded_nal_heads((jmh_ctx *)ctx, n, heads); }
static int gpu_pop_coded(void *ctx, uint8_t *out, size_t cap, jmh_coded_bytes *where, jmh_coded_stats *stats) {
    return jmh_frame_pop_coded((jmh_ctx *)ctx, out, cap, where, stats);
}
/* a frame of a tensor file (DeviceInputTensor / DeviceReconTensor 1..4) as a device tensor: the offsets of R, G, B,
   the strides, the element type.  rgb24 (1): pixels of R, G, B; gbrp, gbrp10le, gbrpf32le (2..4): planes G, B, R */
typedef struct { size_t off[3]; int64_t stride_x, stride_y; int dtype; } gpu_tensor_layout;
static gpu_tensor_layout gpu_tensor_frame(int kind, int dw, int dh) {
    const size_t es = (size_t)jm_tensor_elem_bytes(kind), plane = es * dw * dh;
    const gpu_tensor_layout packed = {{0, 1, 2}, 3, (int64_t)3 * dw, JMH_T_U8};
    const gpu_tensor_layout planar = {{2 * plane, 0, plane}, (int64_t)es, (int64_t)es * dw, kind == 4 ? JMH_T_F32 : kind == 3 ? JMH_T_U16 : JMH_T_U8};
    return kind == 1 ? packed : planar;
}
/* DeviceInput 1: the frame as read uploaded raw into one device buffer and pushed from there.  The upload and the
   push share a stream of the caller's, so the next picture's upload follows this picture's packing kernel. */
static struct { void *buf, *stream; size_t bytes; } gpu_in;
static int gpu_in_upload(void *ctx, size_t bytes, const void *data) {
    int r;
    if (!gpu_in.stream && (r = jmh_device_stream_create((jmh_ctx *)ctx, &gpu_in.stream))) return r;
    if (gpu_in.bytes < bytes) {
        if ((r = jmh_device_free((jmh_ctx *)ctx, gpu_in.buf)) || (r = jmh_device_malloc((jmh_ctx *)ctx, bytes, &gpu_in.buf))) return r;
        gpu_in.bytes = bytes;
    }
    return jmh_device_upload((jmh_ctx *)ctx, gpu_in.buf, data, bytes, gpu_in.stream);
}
/* the source described as the library takes it: 4:2:0 planes (display size, the coded picture's strides, unpadded),
   packed RGB and 4:2:2 / 4:4:4 layouts (its planes one after the other, rows tight) as a device picture, a tensor
   file's frame as a device tensor; the device pads, converts, reduces or quantises it */
static int gpu_push_source(void *ctx, const jm_device_source *src, const jmh_frame_params *fp, int n, const jmh_coded_slice *sl, int cw, int ch) {
    const jm_pic *cur = src->pic;
    const size_t ps = cur && cur->bd > 8 ? 2 : 1, luma = cur ? (size_t)cur->w * cur->h * ps : 0;
    int r;
    if ((r = cur ? gpu_in_upload(ctx, luma * 3 / 2, cur->bd > 8 ? (const void *)cur->Y : (const void *)cur->y)
                 : gpu_in_upload(ctx, jm_source_frame_bytes(src), src->frame))) return r;
    const uint8_t *base = (const uint8_t *)gpu_in.buf;
    if (src->kind == JM_SRC_TENSOR) {
        const gpu_tensor_layout l = gpu_tensor_frame(src->code, src->w, src->h);
        jmh_device_tensor t;
        memset(&t, 0, sizeof(t));
        t.dtype = l.dtype; t.flags = src->flags;
        t.width = src->w; t.height = src->h;
        for (int i = 0; i < 3; i++) t.chan[i] = base + l.off[i];
        t.stride_x = l.stride_x; t.stride_y = l.stride_y;
        t.stream = gpu_in.stream;
        return jmh_frame_push_coded_tensor((jmh_ctx *)ctx, &t, fp, n, sl, cw, ch);
    }
    jmh_device_picture pic;
    memset(&pic, 0, sizeof(pic));
    pic.width = src->w; pic.height = src->h;
    pic.stream = gpu_in.stream;
    if (src->kind == JM_SRC_PLANES) {
        pic.format = cur->bd > 8 ? JMH_PIX_I010 : JMH_PIX_I420;
        pic.plane[0] = base; pic.plane[1] = base + luma; pic.plane[2] = base + luma + luma / 4;
        pic.stride[0] = (int64_t)cur->w * ps; pic.stride[1] = pic.stride[2] = (int64_t)(cur->w / 2) * ps;
        if (!n) return jmh_frame_push_device((jmh_ctx *)ctx, &pic, fp);
    } else if (src->kind == JM_SRC_RGB) {
        pic.format = src->code;
        pic.plane[0] = base;
        pic.stride[0] = (int64_t)4 * src->w;
    } else {
        const int layout = src->code & ~JMH_PIX_CHROMA_LEFT;
        size_t off = 0;
        pic.format = src->code;
        for (int sp = 0; sp < 3 && jm_yuv_row_bytes(layout, sp, src->w); sp++) {
            pic.plane[sp] = base + off;
            pic.stride[sp] = (int64_t)jm_yuv_row_bytes(layout, sp, src->w);
            off += jm_yuv_row_bytes(layout, sp, src->w) * src->h;
        }
    }
    return jmh_frame_push_coded_device((jmh_ctx *)ctx, &pic, fp, n, sl, cw, ch);
}
/* DeviceReconFormat 16..19 / DeviceReconTensor 1..4: the current picture, deblocked, pulled at the display size into
   one device buffer in the file's layout, on a stream of the caller's, and downloaded behind it */
static struct { void *buf, *stream; size_t bytes; } gpu_out;
static int gpu_pull_recon(void *ctx, int format, int tensor, int flags, int dw, int dh, void *dst) {
    const size_t bytes = jm_recon_frame_bytes(tensor, dw, dh);
    int r;
    if (!gpu_out.stream && (r = jmh_device_stream_create((jmh_ctx *)ctx, &gpu_out.stream))) return r;
    if (gpu_out.bytes < bytes) {
        if ((r = jmh_device_free((jmh_ctx *)ctx, gpu_out.buf)) || (r = jmh_device_malloc((jmh_ctx *)ctx, bytes, &gpu_out.buf))) return r;
        gpu_out.bytes = bytes;
    }
    uint8_t *base = (uint8_t *)gpu_out.buf;
    if (!tensor) {
        jmh_device_picture_out pic;
        memset(&pic, 0, sizeof(pic));
        pic.format = format;
        pic.width = dw; pic.height = dh;
        pic.plane[0] = base;
        pic.stride[0] = (int64_t)4 * dw;
        pic.stream = gpu_out.stream;
        r = jmh_pull_picture((jmh_ctx *)ctx, JMH_OUT_DEBLOCKED, &pic);
    } else {
        const gpu_tensor_layout l = gpu_tensor_frame(tensor, dw, dh);
        jmh_device_tensor_out t;
        memset(&t, 0, sizeof(t));
        t.dtype = l.dtype; t.flags = flags;
        t.width = dw; t.height = dh;
        for (int i = 0; i < 3; i++) t.chan[i] = base + l.off[i];
        t.stride_x = l.stride_x; t.stride_y = l.stride_y;
        t.stream = gpu_out.stream;
        r = jmh_pull_tensor((jmh_ctx *)ctx, JMH_OUT_DEBLOCKED, &t);
    }
    return r ? r : jmh_device_download((jmh_ctx *)ctx, dst, gpu_out.buf, bytes, gpu_out.stream);
}
/* DeviceInputScale 1..3: the sticky setting of the pushes above */
static int gpu_input_scale(void *ctx, int filter, int flags, int ow, int oh) {
    const jmh_scale s = {filter, flags, ow, oh};
    return jmh_input_scale((jmh_ctx *)ctx, &s);
}
static void gpu_input_release(void *ctx) {
    if (gpu_in.stream) (void)jmh_device_stream_destroy((jmh_ctx *)ctx, gpu_in.stream);
    if (gpu_in.buf) (void)jmh_device_free((jmh_ctx *)ctx, gpu_in.buf);
    memset(&gpu_in, 0, sizeof(gpu_in));
    if (gpu_out.stream) (void)jmh_device_stream_destroy((jmh_ctx *)ctx, gpu_out.stream);
    if (gpu_out.buf) (void)jmh_device_free((jmh_ctx *)ctx, gpu_out.buf);
    memset(&gpu_out, 0, sizeof(gpu_out));
}

int main(int argc, char **argv) {
    jm_input inp;
    char err[1024];
    jm_input_defaults(&inp);
    jm_set_device_input(gpu_push_source);   /* before PatchInp: it rejects DeviceInput on a backend without one */
    jm_set_device_input_scale(gpu_input_scale);
    jm_set_device_output(gpu_pull_recon);
    if (jm_configure(&inp, argc, argv, err, sizeof(err))) { fprintf(stderr, "%s\n", err); return 1; }
    jmh_config cfg;
    jm_fill_config(&inp, &cfg);
    /* device deblocking: only the deblocked picture comes back (the recon file, PSNR and the
       next reference are the filtered picture, as in JM) */
    if (!getenv("JMH_HOST_DEBLOCK")) cfg.flags |= JMH_FLAG_NO_RECON_READBACK;
    jmh_ctx *ctx = NULL;
    int r = jmh_create(&cfg, inp.hip_device, &ctx);
    if (r) { fprintf(stderr, "jmh_create failed: %s\n", jmh_strerror(r)); return 2; }
    jm_backend be = {"mi355x-hip", ctx, gpu_set_ref, gpu_encode, gpu_res, gpu_recon, gpu_destroy,
                     gpu_deblocked, gpu_ref_deblocked, gpu_push, gpu_pop, jmh_pipeline_depth(ctx),
                     gpu_search_pictures, gpu_block_search, gpu_tq4x4};
    jm_set_device_cavlc(gpu_cavlc_slices);
    jm_set_device_cabac(gpu_cabac_slices);
    jm_set_device_cabac_split(gpu_cabac_split);
    jm_set_device_coded(gpu_push_coded, gpu_pop_coded);
    jm_set_device_nal(gpu_nal_heads);
    if (getenv("JMH_HOST_DEBLOCK")) be.read_deblocked = NULL, be.reference_deblocked = NULL;
    jm_stats st;
    r = jm_encode_sequence(&inp, &be, &st, stdout);
    double mp = (double)inp.width * inp.height * st.frames / 1e6;
    if (!r && st.me_tq_ms > 0)
        printf(" ME+TQ throughput (host-observed, incl. PCIe): %.2f MP/s\n", mp / (st.me_tq_ms / 1e3));
    gpu_input_release(ctx);
    be.destroy(ctx);
    return r ? 3 : 0;
}
