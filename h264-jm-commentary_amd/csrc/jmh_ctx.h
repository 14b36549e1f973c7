// jmh_ctx.h — the context behind include/jmhip.h, for the two host-only files that share it: jmhip_abi.hip (the
// context's life, the scheduler, coded pictures, references, the coder's unit seams) and jmhip_io.hip (device
// memory handed in or out by the caller: sources, the scaler, pulls).  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <deque>
#include <vector>
#include "jmh_launch.h"
#include "jmh_cavlc.h"
#include "jmh_cabac.h"
#include "jmh_cabac_rate.h"
#include "jmh_yuv.h"
#include "jmh_nal.h"

// ring of begin/end event pairs; completed pairs are folded into `sum` (ms)
struct EvRing {
    std::vector<hipEvent_t> a, b;
    int cap = 0, head = 0, count = 0, n = 0;
    float sum = 0;
};

// NAL units finished on the device (jmhip_nal.h): the buffers of one access unit, a
// ring entry's or the synchronous seam's
struct NalBuf {
    uint8_t *h, *d;                      // pinned / device: heads, where, chunk starts, chunk records, unit places, meta (NalLayout)
    int ucap, maxch;                     //   the units and chunks they hold
    uint8_t *out;                        // device: the access unit
    size_t out_cap;
};
// offsets into NalBuf::h / d (each a multiple of 8)
struct NalLayout {
    size_t heads, where, cs, ch, uout, meta, bytes;
    NalLayout(int ucap, int maxch) {
        auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
        heads = 0;
        where = up8((size_t)ucap * sizeof(jmh_nal_head));
        cs = where + (size_t)ucap * 3 * sizeof(int64_t);
        ch = up8(cs + ((size_t)ucap + 1) * sizeof(int32_t));
        uout = ch + (size_t)maxch * sizeof(jmn_chunk);
        meta = uout + (size_t)ucap * 2 * sizeof(int64_t);
        bytes = meta + JMN_META_WORDS * sizeof(uint64_t);
    }
};
static_assert(sizeof(jmn_chunk) % 8 == 0 && sizeof(jmh_nal_range) == 2 * sizeof(int64_t), "NalLayout");

// one ring entry: everything one picture in flight owns
struct PicBuf {
    uint8_t *src, *rec, *dbk;            // device: source (jmh_frame_push), recon, deblocked recon
    int16_t *mv;
    int8_t *refidx, *ipred;
    jmh_mb_result *res;
    MbScratch *scr;
    jmh_mb_result *h_res;                // pinned host copies (allocated on first readback use)
    uint8_t *h_src, *h_rec, *h_dbk;
    hipEvent_t ev_src, ev_t0, ev_done;   // staging reuse / push..done timing
    hipEvent_t ev_fin;                   // the picture's last tick (the copy stream's readback waits)
    uint8_t *cab;                        // RDOptimization 1: the slices' context states,
    uint32_t *range;                     //   codIRange, the MBs' context-selection records
    jmr_mbinfo *mbi;
    RdoPic *h_rp;                        //   pinned staging of the entry's RdoPic (after scr)
    hipEvent_t ev_rp;                    //   its H2D copy (h_rp is rewritten only after it completes)
    int recon_read;                      // h_rec holds the occupant's reconstruction
    int unpopped;                        // readback picture not yet popped
    int deblocked;                       // the occupant was deblocked on the device (dbk valid)
    uint32_t gen;                        // dataflow: occupants so far (the flag value of its MBs)
    // coded pictures (jmhip_coded.h): the entry's own writer buffers, on its first coded picture
    int coded;                           // the occupant is a coded picture: no readback, its writer queued behind it
    int cd_n, cd_cw, cd_ch;              //   its slices, its crop
    uint8_t *cd_h, *cd_d;                // pinned / device: descriptors [nmb], where [nmb], meta (CodedLayout)
    jmh_coded_slice *cd_sl;              // pinned (inside cd_h): the caller's descriptors, for the synchronous fallback
    uint8_t *cd_out;                     // device: the picture's output region
    size_t cd_cap;                       //   its bytes
    int nal_armed;                       // the occupant was armed (jmh_coded_nal_heads): its pop returns the access unit
    NalBuf nal;                          //   the entry's NAL buffers, on its first armed picture
    // device pictures (jmhip_input.h)
    int dev_fmt;                         // the occupant was pushed as a device picture: its format + 1, else 0 (a host picture, a tensor)
    hipEvent_t ev_in;                    //   the caller's stream at the push (created on first use)
    // pulled pictures (jmhip_output.h)
    hipEvent_t ev_out;                   // the last pull that read rec / dbk (created on first use); the next claim waits for it
};

// offsets into PicBuf::cd_h / cd_d (each a multiple of 8)
struct CodedLayout {
    size_t sl, where, meta, user, bytes;
    explicit CodedLayout(size_t nmb) {
        sl = 0;
        where = sl + nmb * 24;           // jmh_slice_desc is 20 bytes, jmh_cabac_slice_desc 16
        meta = where + nmb * sizeof(jmh_slice_bytes);
        user = meta + JMH_WRITER_META_BYTES;
        bytes = user + nmb * sizeof(jmh_coded_slice);   // (host only)
    }
};
static_assert(sizeof(jmh_slice_bytes) == sizeof(jmh_cabac_slice_bytes) && sizeof(jmh_slice_desc) <= 24 && sizeof(jmh_cabac_slice_desc) <= 24,
              "CodedLayout");

// a picture in flight (not yet fully issued)
struct Flight {
    int id, entry, ref_entry;            // ref_entry: ring entry read as reference (-1: d_ref / none)
    int tmv_entry;                       // ring entry whose motion field EPZS reads (-1: none)
    int pred_id;                         // picture it must trail by PIPE_LAG diagonals (-1: none)
    int stage, started, readback;
    PicParams pp;
};

// the tables of one geometry of the scaler (jmh_scale.h, jms_pack_axis) on the device; h: what was uploaded, kept
// while the copy may be pending (up)
#define SCALE_TABS 8
struct ScaleTab {
    int key[6];                          // source w, h, output w, h, filter, flags
    uint8_t *d = nullptr;
    std::vector<uint8_t> h;
    hipEvent_t up = nullptr;
    size_t off[2][4];                    // [luma, chroma][fh, fv, th, tv]: bytes into d
    int T[2][2];                         // [luma, chroma][horizontal, vertical]
    uint64_t used = 0;
};

struct jmh_ctx {
    jmh_config cfg;
    int dev;
    hipStream_t st;                      // the wavefront ticks (and source uploads)
    hipStream_t cst;                     // readback of finished pictures, overlapping later ticks
    hipStream_t sst = nullptr;           // RDO on: k_rdo_intra beside k_rdo_inter
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int W, H, Wc, Hc, mbw, mbh, sr, side, npos, qstride, qplane, nd;
    size_t fsize, n4, nmb;               // bytes of one 4:2:0 picture (Y then U then V)
    uint8_t *d_ref, *d_qpel, *d_slots;   // explicit reference (set_reference), a1 seam, slots
    struct { void *cur, *ref; } spic[2]; // luma pictures of the per-block searches, by sample width: [0] 8-bit
                                         //   (jmh_search_pictures), [1] 16-bit, the High 10 seams (..._u16)
    uint32_t *d_ordtab;                  // FFS order keys of the analysis threads' strips (ordtab_fill)
    int bd, ps, maxv;                    // picture bit depth, bytes per sample (1, 2), (1 << bd) - 1
    int hbd_bits;                        // bit depth of the 16-bit search pictures
    int nslots;
    int depth, nring;
    std::vector<PicBuf> ring;
    std::deque<Flight> fl;               // issued-incompletely pictures, oldest first
    std::deque<int> popq;                // readback pictures (ring entries) not yet popped
    int next_id, next_entry;
    int last_id, last_entry;             // the last pushed picture
    int ref_kind, ref_entry;             // the reference of the next pushed picture
    int cur_entry;                       // results visible through get_mb_result / read_*
    unsigned long long *d_prof;          // JMH_PHASE_PROF=<mb>: per-phase wall clock of one MB
    int prof_mb;
    unsigned long long *d_bprof;         // JMH_BLOCK_PROF=<tick>: k_mb_analyse block start/end/role
    int bprof_tick, bprof_blocks;
    uint8_t *h_stage_ref;
    EvRing ring_interp, ring_mb, ring_an, ring_fin;   // ring_an / ring_fin: JMH_FLAG_KERNEL_TIMING
    jmh_timing timing;
    int ticks_total;
    std::vector<int> dcount, dymin;
    int lag;                             // stages a picture trails its reference picture by
    // RDOptimization 1: the RD stage schedule (MB addresses in stage order, offsets per stage),
    // the tick's candidate scratch, slices per picture
    int32_t *d_sched, *d_soff;
    void *d_rscr;
    void *d_ffs;                         // RDO + SearchMode 0: the tick MBs' SAD tables (k_rdo_inter)
    int nslice;
    // dataflow wavefront (k_mb_flow): ticks are not launched one by one but
    // collected into a segment of macroblocks in tick order, launched as one grid on a flush
    bool flow = false;
    int seg_max = 0;                     // ticks per segment before a flush (JMH_FLOW_SEG)
    int seg_min = 8;                     // ... or, once the device is idle, this many (2 / 4 / 16 within
                                         //   noise: profiles/r10h_flow_bench20_ab.txt)
    hipEvent_t ev_flow = nullptr;        // the last segment launch's end: a segment of >= seg_min ticks
                                         //   is flushed as soon as the device has run out of work
    std::vector<FlowPic> fpic;           // per ring entry: parameters + flag generations
    std::vector<uint32_t> seg;           // the pending segment's macroblocks (FLOW_ITEM)
    unsigned long long seg_mask = 0;     // ring entries the pending segment reads or writes
    int seg_ticks = 0;
    size_t seg_cap = 0;                  // items the device / staging buffers hold
    // segment buffers, alternating: pinned staging -> device on the upload stream, beside the
    // previous segment's launch (a buffer is rewritten once the launch that read it has ended)
    uint8_t *d_seg[2] = {nullptr, nullptr};   // device: FlowPic[nring], then the items
    uint8_t *h_seg[2] = {nullptr, nullptr};   // pinned staging
    hipEvent_t ev_seg[2] = {nullptr, nullptr};   // the upload out of h_seg[i] / into d_seg[i] done
    hipEvent_t ev_kseg[2] = {nullptr, nullptr};  // the launch that read d_seg[i] done
    hipStream_t ust = nullptr;           // the segment uploads
    int seg_slot = 0;
    uint32_t *d_flags = nullptr;         // [nring][nmb] generations of the finished MBs
    unsigned *d_head = nullptr;          // ticket counter
    unsigned head_base = 0;
    unsigned *h_err = nullptr;           // pinned, device-written: a dependency wait timed out
    int fprof_launch = -1, flow_count = 0;   // debug: JMH_FLOW_PROF=<launch> -> JMH_FLOW_PROF_OUT (raw u64)
    unsigned long long *d_fprof = nullptr;
    size_t fprof_n = 0;
    std::vector<uint32_t> fprof_items;
    jmh_cavlc_state *cavlc = nullptr;    // device CAVLC writer (jmh_cavlc.hip): its own stream, created on first use
    int cabac_split = 0;                 // jmh_cabac_set_split: bins per chunk of the split coder, 0 off
    jmh_cabac_state *cabac = nullptr;    // device CABAC writer (jmh_cabac.hip): the same
    size_t coded_cap = 0;                // coded pictures: bytes of output per macroblock queued with a picture
    std::vector<void *> coded_retired;   //   outgrown output regions: freed with the context
    uint8_t *h_coded_pic = nullptr;      //   pinned: jmh_read_recon / jmh_read_deblocked of a coded picture
    bool nal_armed = false;              // jmh_coded_nal_heads: the next coded push takes nal_arm
    std::vector<jmh_nal_head> nal_arm;
    NalBuf nalw = {};                    // jmh_nal_wrap: its buffers,
    uint8_t *nalw_pay = nullptr;         //   the payload on the device
    size_t nalw_pay_cap = 0;
    // device pictures: the I010 clamp counts, a word per ring entry and one for the unit seam (on the
    // first I010 picture), the count of the picture last popped, the last device push
    unsigned long long *d_clamp = nullptr, *h_clamp = nullptr;
    uint64_t last_clamped = 0;
    int last_dev_entry = -1;
    uint8_t *up_h = nullptr;             // jmh_device_upload on a stream: its pinned buffer,
    size_t up_cap = 0;
    hipEvent_t ev_up = nullptr;          //   the last copy out of it
    hipStream_t ost = nullptr;           // pulls without a caller's stream, the convert seams, downloads (created on first use)
    // jmh_input_scale (jmhip_scale.h): the setting (filter 0: off), the tables of the geometries last used and the
    // scratch picture the ingest kernels pack into.  All of it is allocated, written, read and released on st
    jmh_scale scale = {0, 0, 0, 0};
    std::vector<ScaleTab> scale_tabs;
    uint64_t scale_tick = 0;
    uint8_t *d_scl = nullptr;
    size_t scl_cap = 0;
};

#define HCHK(x)                                                                  \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            fprintf(stderr, "jmhip: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return JMH_E_HIP;                                                    \
        }                                                                        \
    } while (0)

// device temporaries of the unit seams: freed on every return path
struct DevTemps {
    std::vector<void *> p;
    ~DevTemps() { for (void *q : p) if (q) (void)hipFree(q); }
    template <class T> hipError_t alloc(T **out, size_t n) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, n);
        if (e == hipSuccess) p.push_back(q);
        *out = (T *)q;
        return e;
    }
};

// ---- jmhip_abi.hip, for jmhip_io.hip: planar 4:2:0 packing of ps-byte samples, the wait for every pull ----
bool pack_planes(uint8_t *dst, int W, int H, const void *yv, const void *uv, const void *vv, int sy, int sc, int ps, int maxv);
void unpack_planes(const uint8_t *src, int W, int H, void *yv, void *uv, void *vv, int sy, int sc, int ps);
int output_wait(jmh_ctx *c);

// ---- jmhip_io.hip, for the push of jmhip_abi.hip ----
// whether the packing kernel of the (checked) format counts samples above maxv (jmh_device_input_clamped)
static inline bool device_format_counts(int format) { return format == JMH_PIX_I010 || (jmy_is_yuv(format) && jmy_clamps(jmy_layout(format))); }
// A source in device memory, the counterpart of PullDst: a picture or a tensor.  What the host code asks of a
// source it asks here; a new kind of source is one more branch in these questions and one more launcher
struct DevSrc {
    const jmh_device_picture *pic;
    const jmh_device_tensor *ten;
    explicit operator bool() const { return pic || ten; }
    int width() const { return pic ? pic->width : ten->width; }
    int height() const { return pic ? pic->height : ten->height; }
    void *stream() const { return pic ? pic->stream : ten->stream; }   // the caller's
    bool counts() const { return pic && device_format_counts(pic->format); }   // (a tensor never counts)
};
// the argument rules of the source's header, then the scaler's when a scale is set
int devsrc_check(const jmh_ctx *c, const DevSrc &s);
// JMH_E_UNSUPPORTED_CFG unless a context of this bit depth takes the (checked) source
int devsrc_depth(const jmh_ctx *c, const DevSrc &s);
// the (checked) source packed into dst on the context's stream, behind the work queued on the caller's stream so
// far (ev: that stream's event); slot: the clamp word of a source that counts
int ingest_queue(jmh_ctx *c, const DevSrc &s, uint8_t *dst, int slot, hipEvent_t ev);
