// jmh_device.h — device-side types and constants shared by the MI355X kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/jmhip.h"
#include "jmh_rgb.h"
#include "jmh_tensor.h"
#include "jmh_output.h"

#define SRMAX 32                         // LDS-resident FFS window: SearchRange <= 32
#define SIDE_MAX (2 * SRMAX + 1)
#define NPOS_MAX (SIDE_MAX * SIDE_MAX)   // 4225 search positions
#define QPAD 4                           // quarter-pel plane padding (== oracle JMO_PAD)
#define NT 256                           // threads per finalize / unit workgroup
#define NTA 512                          // threads per analysis workgroup (8 waves, 2 per SIMD)
// (a P macroblock's Intra4x4 steps ride in the search stages' sub-pel phases on waves 6 and 7; a
// variant with the intra decisions on a wave of their own measured slower)
#define NPK 10                           // FFS search positions per thread (a column strip):
                                         //   65 x ceil(65 / NPK) strips <= NTA
#define NPK2 ((NPK + 1) / 2)             // packed order-key pairs per thread
#define ORDTAB_SPOS (NPK2 * NTA)         // ordtab: the spiral-index -> position table after the keys
#define BIGCOST (1 << 20)
#define PMAX 33                          // pictures per wavefront tick (pipelined pictures in flight;
                                         // 2160p needs 508 / PIPE_LAG + 1 = 33)
// A picture's macroblock (x, y) reads its reference (the previous picture, deblocked) at pixel
// offsets -68..+83 from the MB origin: window centre |MVP/4| <= SR, positions +-SR around it,
// +-3/4 sub-pel, the 6-tap support and the LDS window margin (SR 32).  The farthest samples, rows
// and columns 0..3 of MB (x+5, y+5), are final once that MB's own final kernel (DeblockMb of its
// left and top edges) has run; samples 13..15 of MBs x+4 / y+4 wait for the same MB.  So picture q
// may run diagonal d once picture q-1 has completed diagonal (x+5) + 2(y+5) = d + 15: a lag of
// PIPE_LAG diagonals (tests/test_gpu_parity.py checks pipelined == sequential at the window edge).
#define PIPE_LAG 16
// SearchRange > 32 (EPZS only, up to 64): the same argument with the reach 16 + 2 SR + 3 pixels, i.e.
// MB (x + R, y + R), R = (19 + 2 SR) / 16 (5 at SR 32, 9 at SR 64): a lag of 3 R + 1 diagonals (the
// RD stage schedule's lag follows the same reach, jmhip_abi.hip rdo_schedule)
__host__ __device__ __forceinline__ int ref_reach(int sr) { return sr <= SRMAX ? 5 : (19 + 2 * sr) / 16; }
__host__ __device__ __forceinline__ int pipe_lag(int sr) { return sr <= SRMAX ? PIPE_LAG : 3 * ref_reach(sr) + 1; }

// Per-macroblock analysis results, written by k_mb_analyse (three roles on separate
// workgroups) and consumed by k_mb_final on the same wavefront diagonal.
struct MbScratch {
    int16_t all_mv[8][16][2];            // best MV per block type (1..7) and 4x4 block
    uint16_t fpc[7][16];                 // EPZS: each search's full-pel cost per block type 1..7 and
                                         //   4x4, saturated (the neighbours' distortion of item 61)
    int32_t motion_cost[8][4];           // per block type: partition cost (16x8/8x16 block, P8x8 b8)
    int32_t best8x8;                     // P8x8 sub-mode per b8, 4 bits each
    int32_t cost8x8;
    int32_t skipx, skipy;                // FindSkipModeMotionVector
    int32_t i4cost, i4cbp, i4blk;        // Intra4x4 decision (with its reconstruction)
    int32_t i16cost, i16mode, c_mode;
    int8_t ipred[16];
    int16_t i4lev[16][16];               // Intra4x4 levels in scan order
    alignas(4) uint8_t i4rec[512];       // Intra4x4 reconstruction of the MB (256 samples of pel)
    // Intra8x8 decision (k_mb_intra8, Transform8x8Mode only)
    int32_t i8cost, i8cbp, i8modes;      // i8modes: 4 bits per 8x8 block
    int16_t i8lev[16][16];               // levels in the CAVLC interleave (jmh_mb_result.luma)
    alignas(4) uint8_t i8rec[512];
};

// k_mb_flow hands a macroblock's analysis to its final inside the workgroup, in LDS: the MVs, costs,
// Intra4x4 modes and reconstruction stay where the analysis computed them (MeS, IntraS), the
// Intra4x4 levels go straight into the final's level array, and these words carry the scalars that
// have no other LDS home (the MbScratch members of the same names).  The analysis functions take
// either struct as their destination (scr_global: which one).
struct MbCarry {
    int32_t best8x8, cost8x8;
    int32_t skipx, skipy;
    int32_t i4cost, i4cbp, i4blk;
    int32_t i16cost, i16mode, c_mode;
};
template <class SC> struct ScrKind { static constexpr bool global = false; };
template <> struct ScrKind<MbScratch> { static constexpr bool global = true; };
template <class SC> constexpr bool scr_global = ScrKind<SC>::global;

// RDOptimization 1: the per-picture RD state, stored right after the picture's MbScratch array
// (PicParams.scr + mbw * mbh) so that the kernel arguments stay within 4 KB: the lambdas from the
// host, the slices' CABAC states (contexts + codIRange, jmh_cabac_rate.h) and what every coded
// macroblock leaves for its neighbours' context selection
struct jmr_mbinfo;
struct RdoPic {
    double lambda;                       // lambda_mode (jmh_frame_params.lambda_rd)
    int32_t lf;                          // LAMBDA_FACTOR(sqrt(lambda_mode)) of the motion searches
    int32_t pad;
    uint8_t *cab;                        // [slice][JMR_NCTX] context states (state << 1 | valMPS)
    uint32_t *range;                     // [slice] codIRange (CAVLC: the mb_skip_run so far)
    jmr_mbinfo *mbi;                     // [MB]
};

// byte offset of the RdoPic in a picture's MbScratch allocation (16-aligned)
__host__ __device__ __forceinline__ size_t rdo_pic_offset(size_t nmb) { return (nmb * sizeof(MbScratch) + 15) & ~(size_t)15; }

// A pointer to global memory (HBM) with the address space in its type: an access through it is a
// global_load / global_store whatever the compiler can prove about where the pointer came from.  A
// generic pointer loaded from memory (k_mb_flow's PicParams come from a device table) compiles to
// flat_* accesses, which count on the LDS counter as well and are ordered against every ds_write.
// Only tick_params and flow_params make one from a generic pointer (to_global); a pointer into LDS
// does not convert, so it cannot be read as global by mistake (the other way is implicit).
// The type is in force in k_mb_flow's translation unit (JMH_FLOW_TU), which compiles every helper
// the dataflow path shares with the tick kernels.  In the tick kernels' own units the alias is a
// generic pointer: theirs come from kernel arguments, which the compiler knows to be global (no
// flat_* there), and with the typed form their register allocation moved (a few spilled SGPRs more
// or less per kernel, 4 B more scratch in k_mb_intra) for nothing.
#if defined(__HIP_DEVICE_COMPILE__) && defined(JMH_FLOW_TU)
template <class T> using gptr = __attribute__((address_space(1))) T *;
#define JMH_TYPED_GPTR 1
#else
template <class T> using gptr = T *;
#endif
template <class T> __host__ __device__ __forceinline__ gptr<T> to_global(T *p) { return (gptr<T>)p; }

struct DevParams {
    int W, H, Wc, Hc, mbw, mbh;
    int sr, side, npos;
    int search_mode, use_hadamard, restrict_sr;
    int isr;                    // InterSearch16x16..4x4 as bits 1..7 (a mask: a per-thread array
                                // indexed at run time would put the whole DevParams in scratch)
    int t8;                     // Transform8x8Mode (High profile)
    int epzs_dual;              // EPZSDualRefinement (SearchMode 3)
    int epzs_subpel;            // EPZSSubPelME (item 62) and its EPZSSubPelThresScale
    int epzs_spts;
    int epzs_mints, epzs_maxts; // EPZSMinThresScale / EPZSMaxThresScale (item 61; maxts 0: off)
    int slice_mbs;              // SliceMode 1: MBs per slice (the whole picture for one slice)
    int maxv, qpbd;             // (1 << bit depth) - 1 (Clip1), QpBdOffsetY = QpBdOffsetC = 6 (bit depth - 8)
    // plane pointers are byte addresses of uint8_t (bit depth 8) or uint16_t (9 / 10) samples:
    // the kernels templated on the sample type cast them (spl<pel>)
    gptr<const uint8_t> orgY, orgU, orgV;
    gptr<const uint8_t> refY, refU, refV;
    gptr<uint8_t> recY, recU, recV;
    gptr<uint8_t> dbkY, dbkU, dbkV;   // deblocked reconstruction (null: no deblocking on the device)
    int lf_disable, lf_offA, lf_offB;   // disable_deblocking_filter_idc, FilterOffsetA/B (= 2 x div2)
    gptr<int16_t> mv;
    gptr<int8_t> refidx;
    gptr<int8_t> ipred;
    const int16_t *tmv;         // EPZS temporal predictors: the previous picture's MVs / ref_idx
    const int8_t *tref;         //   (null: no previous picture)
    const uint32_t *ordtab;     // FFS: JM order keys of every thread's positions (ordtab_fill)
    gptr<jmh_mb_result> res;
    MbScratch *scr;             // (tick kernels only, like tmv / tref / rp: generic, from kernel arguments)
    gptr<unsigned long long> prof;   // debug phase timestamps (null: off)
    int prof_mb;
    int slice_type, qp, lambda_mode, lambda_motion, cqp_off;
    int qsel;                   // quantisation rounding selector of this slice (q_round, jmh_common.h)
    int diag, y_min;            // wavefront diagonal of this picture in the launch: mbx + 2*mby == diag
                                //   (RDOptimization 1: diag = the stage of the RD schedule)
    int rdo;                    // RDOptimization 1 (the RD kernels; no 16x16 zero-vector biases)
    int lf;                     // LAMBDA_FACTOR of the motion searches: 65536 * lambda_motion (RDO
                                //   off, integer lambda), the host's RDO one (RDOptimization 1)
    double lambda_rd;           // RDOptimization 1: lambda_mode
    int cavlc;                  // RDOptimization 1 with SymbolMode 0: CAVLC rates (jmh_cavlc_rate.h, item 64);
                                //   RdoPic.range[slice] then holds the slice's mb_skip_run so far
    const RdoPic *rp;           // RDOptimization 1: the picture's RD state
    int cip;                    // UseConstrainedIntraPred: intra prediction from intra neighbours only (intra_avail)
    int i16c;                   // k_mb_flow: the P macroblock's Intra16x16 / chroma decisions run on
                                //   me_mb's idle waves (intra slot 11); 0: k_mb_analyse's intra roles do them
};

// Neighbour MB availability (6.4.8 / JM getNeighbour): inside the picture and in the current
// slice.  Slices are runs of slice_mbs MBs in raster order and every neighbour precedes the MB,
// so "same slice" is "address >= the slice's first MB".  One slice: the picture-edge rules.
struct MbAvail { bool L, T, TL, TR; };
__device__ __forceinline__ MbAvail mb_avail(const DevParams &d, int mbx, int mby) {
    const int a = mby * d.mbw + mbx, first = a - a % d.slice_mbs;
    MbAvail v;
    v.L = mbx > 0 && a - 1 >= first;
    v.T = mby > 0 && a - d.mbw >= first;
    v.TL = mbx > 0 && mby > 0 && a - d.mbw - 1 >= first;
    v.TR = mby > 0 && mbx + 1 < d.mbw && a - d.mbw + 1 >= first;
    return v;
}
// ... for intra prediction (samples and the Intra4x4 / 8x8 mode prediction): with
// UseConstrainedIntraPred an inter (or skipped) neighbour is "not available for Intra prediction"
// (8.3.1.1 dcPredModePredictedFlag, 8.3.1.2, 8.3.2, 8.3.3, 8.3.4); its refidx (-1: intra) is final
// by the time the MB's intra analysis runs
__device__ __forceinline__ MbAvail intra_avail(const DevParams &d, int mbx, int mby) {
    MbAvail v = mb_avail(d, mbx, mby);
    if (d.cip && d.slice_type == JMH_P_SLICE) {
        const int W4 = d.W >> 2, a = 4 * mby * W4 + 4 * mbx;   // the MB's top-left 4x4
        v.L = v.L && d.refidx[a - 1] < 0;
        v.T = v.T && d.refidx[a - W4] < 0;
        v.TL = v.TL && d.refidx[a - W4 - 1] < 0;
        v.TR = v.TR && d.refidx[a - W4 + 4] < 0;
    }
    return v;
}

// One wavefront tick: the same diagonal step for up to PMAX pictures in flight, each on its own
// diagonal (kernel argument, by value; ~2.4 KB).  Entries [0, nP) are P pictures.
struct PicParams {
    const uint8_t *org, *ref;            // 4:2:0 pictures, Y then U then V
    uint8_t *rec, *dbk;                  // dbk null: no deblocking
    int16_t *mv;
    int8_t *refidx, *ipred;
    const int16_t *tmv;                  // previous picture's motion field (EPZS temporal predictors)
    const int8_t *tref;
    jmh_mb_result *res;
    MbScratch *scr;
    int32_t lambda_mode, lambda_motion;
    int16_t diag, y_min;
    int16_t qsel;                        // q_round selector (JM 8.6 !P / JM >= 10 2 + quant_offset)
    int8_t slice_type, qp, cqp_off, lf_disable, lf_offA, lf_offB;   // packed: PMAX entries fit 4 KB
};
struct TickArgs {
    int W, H, mbw, mbh, sr, search_mode, use_hadamard, restrict_sr;
    int inter_search[8];
    unsigned long long *prof;
    int prof_mb;
    unsigned long long *bprof;           // debug (JMH_BLOCK_PROF): per-block start / end / role
    unsigned long long *bprof_fin;       //   ... of k_mb_final (role 3)
    int me_in_analyse;                   // 1: k_mb_analyse runs the FFS searches; 0: k_mb_me_full did
                                         //   (full search, SearchMode -1, or EPZS, SearchMode 3)
    int t8;                              // Transform8x8Mode: k_mb_intra8 ran, k_mb_final decides 4x4 / 8x8
    int epzs_dual;                       // EPZSDualRefinement (k_mb_epzs)
    int epzs_subpel, epzs_spts;          // EPZSSubPelME, EPZSSubPelThresScale
    int epzs_mints, epzs_maxts;          // EPZSMinThresScale, EPZSMaxThresScale
    int slice_mbs;                       // SliceMode 1: MBs per slice (>= 1; mbw * mbh for one slice)
    int cip;                             // UseConstrainedIntraPred
    int bd;                              // bit depth: 8 (uint8_t samples) or 9 / 10 (uint16_t, High 10)
    int rdo;                             // RDOptimization 1: k_rdo_inter + k_rdo_intra + k_rdo_final on the stage
                                         //   (1: CABAC rates, 2: CAVLC rates, SymbolMode 0)
    const int32_t *sched, *soff;         //   schedule: MB addresses in stage order, offsets per stage
    void *rscr;                          //   the tick's candidate scratch (RdoScr per tick MB)
    void *ffs;                           //   SearchMode 0: the tick MBs' SAD tables (null: the searches scan)
    unsigned long long ffs_slot;         //   ... bytes per tick MB (ffs_slot_bytes)
    const uint32_t *ordtab;              // FFS order keys, [NPK2][NTA] packed pairs (jmh_create)
    int npic, nP;
    int pre[PMAX + 1];                   // MB prefix sums over the entries
    PicParams p[PMAX];
};
// RDOptimization 1 + SearchMode 0: bytes of one tick MB's SAD table (jmh_epzs.h ffs_table_build)
__host__ __device__ __forceinline__ size_t ffs_slot_bytes(int sr) {
    const size_t np = (size_t)(2 * sr + 1) * (2 * sr + 1);
    return np * 5 * 8;                   // five phases of four u16 SADs per position
}
static_assert(sizeof(TickArgs) <= 4096, "TickArgs is passed by value in the kernel argument segment");

// ---------------------------------------------------------------------------------------------
//  Dataflow wavefront (k_mb_flow, SearchMode 0 with 8-bit samples, RDO off): one launch per
//  segment of ticks, one workgroup per macroblock.  The host flattens the segment's ticks into a list
//  of macroblocks in tick order; a workgroup claims the next one with an atomic ticket when it
//  starts, waits until the macroblocks it depends on are done (per-MB flags), and runs its whole
//  encode_one_macroblock -- motion search, intra decisions, the final -- before publishing its own
//  flag.  Every dependency precedes the MB in tick order, and every claimed ticket belongs to a
//  resident workgroup, so the wait always ends.
// ---------------------------------------------------------------------------------------------
// per ring entry, copied to the device with each segment: the picture's parameters and the flag
// generations that mark its macroblocks (and its reference picture's) done
struct FlowPic {
    PicParams pp;
    uint32_t gen;                        // flags[entry][mb] >= gen: MB done (the entry's use count)
    int32_t ref_entry;                   // ring entry of the reference picture (-1: none / explicit buffer)
    uint32_t ref_gen;
    int32_t pad;
};
struct FlowArgs {
    int W, H, mbw, mbh, sr, search_mode, use_hadamard, restrict_sr;
    int isr;                             // InterSearch bits 1..7
    int slice_mbs;
    const uint32_t *ordtab;
    unsigned long long *prof;
    int prof_mb;
    const FlowPic *pics;                 // [nring]
    const uint32_t *items;               // the segment's MBs in tick order: entry << 24 | mby << 12 | mbx
    int nitems;
    int nmb, nring;
    unsigned *head;                      // ticket counter (monotonic over launches)
    unsigned base;                       // its value at this launch's first ticket
    uint32_t *flags;                     // [nring][nmb] generations
    unsigned *err;                       // host-visible: [0] 1 = a dependency wait timed out, 2 = a ticket /
                                         //   item out of range ([1] ticket, [2] item)
    unsigned long long *fprof;           // debug (JMH_FLOW_PROF=<launch>): per ticket 6 words -- start,
                                         //   dependencies met, analysis done, final done, flag stored,
                                         //   hardware id << 32 | item (null: off)
};
#define FLOW_ITEM(e, x, y) (((uint32_t)(e) << 24) | ((uint32_t)(y) << 12) | (uint32_t)(x))

// k_ingest (jmh_ingest.hip): a device picture of w x h luma samples into the packed W x H source
struct IngestArgs {
    const uint8_t *plane[3];             // device planes of the caller (jmhip_input.h), [2] unused when UV is interleaved
    int64_t stride[3];                   // bytes per row
    uint8_t *dst;                        // Y, U, V of the coded size, samples of 1 or 2 bytes
    int w, h, W, H;
    uint32_t maxv;
    unsigned long long *clamped;         // I010: samples above maxv are added here
};

// k_ingest_rgb (jmh_rgb.hip): an RGB device picture of w x h pixels converted into the packed W x H source
struct RgbArgs {
    const uint8_t *src;                  // plane[0] of the caller (jmhip_rgb.h): one dword per pixel
    int64_t stride;                      // bytes per row
    uint8_t *dst;                        // Y, U, V of the coded size, samples of 1 or 2 bytes
    int w, h, W, H;
    jmr_coef k;                          // the conversion of the format's flags at the context's bit depth
};

// k_ingest_yuv (jmh_yuv.hip): a 4:2:2 or 4:4:4 device picture of w x h luma samples reduced into the packed W x H source
struct YuvArgs {
    const uint8_t *plane[3];             // device planes of the caller (jmhip_yuv.h), those the layout reads
    int64_t stride[3];                   // bytes per row
    uint8_t *dst;                        // Y, U, V of the coded size, samples of 1 or 2 bytes
    int w, h, W, H;
    uint32_t maxv;
    unsigned long long *clamped;         // I210, I410: samples above maxv are added here
};

// k_ingest_tensor (jmh_tensor.hip): a device tensor of w x h pixels quantised and converted into the packed W x H source
struct TensorArgs {
    const uint8_t *chan[3];              // R, G, B of the caller (jmhip_tensor.h) at pixel (0, 0)
    int64_t sx, sy;                      // bytes between pixels / rows
    uint8_t *dst;                        // Y, U, V of the coded size, samples of 1 or 2 bytes
    int w, h, W, H;
    jmr_coef k;                          // the conversion of the flags at the context's bit depth (maxv: M of the quantiser)
};

// k_pull_picture / k_pull_tensor (jmh_output.hip): the w x h crop of a packed W x H picture written into the caller's memory
struct OutArgs {
    const uint8_t *src;                  // Y, U, V of the coded size, samples of 1 or 2 bytes (k.maxv > 255: 2)
    uint8_t *dst[3];                     // planes of the caller (jmhip_output.h) / R, G, B of its tensor at pixel (0, 0)
    int64_t stride[3];                   // a picture: bytes per row of each plane; a tensor: stride_x, stride_y
    int w, h, W, H;
    jmout_coef k;                        // the conversion of the flags at the context's bit depth (a YUV format: maxv only)
};

// k_scale (jmh_scale.hip): the top-left w x h of a packed sW x sH picture resampled to ow x oh and padded into the
// packed W x H source.  The tables of jmh_scale.h (jms_pack_axis), [0] luma, [1] chroma (U and V share them)
struct ScaleArgs {
    const uint8_t *src;                  // Y, U, V of sW x sH, samples of 1 or 2 bytes (maxv > 255: 2)
    uint8_t *dst;                        // Y, U, V of the coded size
    int w, h, sW, sH, ow, oh, W, H;
    const int32_t *fh[2], *fv[2];        // first of every output column / row
    const uint32_t *th[2], *tv[2];       // JMS_HPAIRS dwords per column, JMS_VPAIRS per row
    int nph[2], npv[2];                  // the pairs in use: T / 2 horizontally, T / 2 + 1 vertically
    int tv_taps[2];                      // T of the vertical axis
    int maxv, P;                         // (1 << bit depth) - 1, 14 - bit depth
};

// The stores of the converting ingest kernels (k_ingest_rgb, k_ingest_tensor): 8 luma samples of a row or 4 + 4
// chroma samples, packed little-endian; TEN: 16-bit samples
template <bool TEN>
__device__ __forceinline__ uint32_t ingest_pack(const int32_t *v) {
    return TEN ? (uint32_t)v[0] | (uint32_t)v[1] << 16 : (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
}
template <bool TEN>
__device__ __forceinline__ void ingest_store_luma(uint8_t *o, const int32_t *y) {
    if (TEN) *reinterpret_cast<uint4 *>(o) = make_uint4(ingest_pack<true>(y), ingest_pack<true>(y + 2), ingest_pack<true>(y + 4), ingest_pack<true>(y + 6));
    else *reinterpret_cast<uint2 *>(o) = make_uint2(ingest_pack<false>(y), ingest_pack<false>(y + 4));
}
template <bool TEN>
__device__ __forceinline__ void ingest_store_chroma(uint8_t *o, const int32_t *c) {
    if (TEN) *reinterpret_cast<uint2 *>(o) = make_uint2(ingest_pack<true>(c), ingest_pack<true>(c + 2));
    else *reinterpret_cast<uint32_t *>(o) = ingest_pack<false>(c);
}

// XCD-aware block order.  Workgroups are dispatched round-robin over the 8 XCDs (hardware block b
// runs on XCD b % 8), each with its own L2.  A launch of n logical blocks uses 8 * ceil(n / 8)
// hardware blocks and gives every XCD one contiguous run of the logical list, whose consecutive
// entries are neighbouring MBs of one picture's diagonal (search windows and MC reads overlap), so
// they share that XCD's L2.  Returns the logical block (>= n: idle).
#define NXCD 8
__device__ __forceinline__ int xcd_block(int b, int n) { return (b % NXCD) * ((n + NXCD - 1) / NXCD) + b / NXCD; }
__host__ __device__ __forceinline__ int xcd_grid(int n) { return NXCD * ((n + NXCD - 1) / NXCD); }

// entry of MB index idx (pre[e] <= idx < pre[e + 1]); uniform scalar loop
__device__ __forceinline__ int tick_entry(const TickArgs &t, int idx) {
    int e = 0;
    while (e + 1 < t.npic && t.pre[e + 1] <= idx) e++;
    return e;
}
// the picture's planes, side arrays and results as global pointers (ls / lc: bytes of a luma / chroma
// plane): the one place where DevParams' typed pointers are made
__device__ __forceinline__ void set_pic_pointers(DevParams &d, const PicParams &q, int ls, int lc) {
    const gptr<const uint8_t> org = to_global(q.org), ref = to_global(q.ref);
    const gptr<uint8_t> rec = to_global(q.rec), dbk = to_global(q.dbk);
    d.orgY = org; d.orgU = org + ls; d.orgV = org + ls + lc;
    d.refY = ref; d.refU = ref + ls; d.refV = ref + ls + lc;
    d.recY = rec; d.recU = rec + ls; d.recV = rec + ls + lc;
    d.dbkY = dbk; d.dbkU = dbk ? dbk + ls : nullptr; d.dbkV = dbk ? dbk + ls + lc : nullptr;
    d.mv = to_global(q.mv); d.refidx = to_global(q.refidx); d.ipred = to_global(q.ipred); d.res = to_global(q.res);
}
__device__ __forceinline__ bool inter_on(int isr, int mode) { return (isr >> mode) & 1; }
__device__ __forceinline__ DevParams tick_params(const TickArgs &t, int e) {
    DevParams d;
    const PicParams &q = t.p[e];
    d.W = t.W; d.H = t.H; d.Wc = t.W >> 1; d.Hc = t.H >> 1; d.mbw = t.mbw; d.mbh = t.mbh;
    d.sr = t.sr; d.side = 2 * t.sr + 1; d.npos = d.side * d.side;
    d.search_mode = t.search_mode; d.use_hadamard = t.use_hadamard; d.restrict_sr = t.restrict_sr;
    d.isr = 0;
#pragma unroll
    for (int i = 1; i < 8; i++) d.isr |= (t.inter_search[i] != 0) << i;
    d.t8 = t.t8;
    d.epzs_dual = t.epzs_dual;
    d.epzs_subpel = t.epzs_subpel; d.epzs_spts = t.epzs_spts;
    d.epzs_mints = t.epzs_mints; d.epzs_maxts = t.epzs_maxts;
    d.slice_mbs = t.slice_mbs;
    d.maxv = (1 << t.bd) - 1; d.qpbd = 6 * (t.bd - 8);
    const int ps = t.bd > 8 ? 2 : 1, ls = t.W * t.H * ps, lc = ls >> 2;
    set_pic_pointers(d, q, ls, lc);
    d.lf_disable = q.lf_disable; d.lf_offA = q.lf_offA; d.lf_offB = q.lf_offB;
    d.scr = q.scr;
    d.tmv = q.tmv; d.tref = q.tref; d.ordtab = t.ordtab;
    d.prof = e == 0 ? to_global(t.prof) : nullptr; d.prof_mb = t.prof_mb;
    d.slice_type = q.slice_type; d.qp = q.qp; d.lambda_mode = q.lambda_mode; d.lambda_motion = q.lambda_motion;
    d.cqp_off = q.cqp_off; d.qsel = q.qsel; d.diag = q.diag; d.y_min = q.y_min;
    d.rdo = t.rdo;
    d.cavlc = t.rdo == 2;
    d.i16c = 0;
    d.cip = t.cip;
    d.lf = q.lambda_motion << 16;
    d.lambda_rd = 0;
    d.rp = nullptr;
    if (t.rdo) {
        d.rp = reinterpret_cast<const RdoPic *>(reinterpret_cast<const uint8_t *>(q.scr) + rdo_pic_offset((size_t)t.mbw * t.mbh));
        d.lf = d.rp->lf;
        d.lambda_rd = d.rp->lambda;
    }
    return d;
}

// the macroblock of tick MB index m (entry e): the diagonal mbx + 2 mby == diag of the RDO-off
// wavefront, or the RD stage schedule's list (RDOptimization 1)
__device__ __forceinline__ void tick_mb(const TickArgs &t, const DevParams &d, int e, int m, int &mbx, int &mby) {
    if (t.rdo) {
        const int a = t.sched[t.soff[d.diag] + (m - t.pre[e])];
        mby = a / d.mbw;
        mbx = a - mby * d.mbw;
    } else {
        mby = d.y_min + (m - t.pre[e]);
        mbx = d.diag - 2 * mby;
    }
}

// sample-typed view of a DevParams plane pointer (bytes of uint8_t or uint16_t samples), in the
// pointer's address space; the generic forms serve MbScratch's byte arrays
template <class pel> __device__ __forceinline__ pel *spl(uint8_t *p) { return reinterpret_cast<pel *>(p); }
template <class pel> __device__ __forceinline__ const pel *spl(const uint8_t *p) { return reinterpret_cast<const pel *>(p); }
#ifdef JMH_TYPED_GPTR
template <class pel> __device__ __forceinline__ gptr<pel> spl(gptr<uint8_t> p) { return (gptr<pel>)p; }
template <class pel> __device__ __forceinline__ gptr<const pel> spl(gptr<const uint8_t> p) { return (gptr<const pel>)p; }
#endif
