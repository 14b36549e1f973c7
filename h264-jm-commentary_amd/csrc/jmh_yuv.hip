// jmh_yuv.hip — k_ingest_yuv: a 4:2:2 or 4:4:4 device picture (include/jmhip_yuv.h)
// reduced to 4:2:0, packed and padded into a ring entry's source, where k_ingest moves a 4:2:0 one.
//
// One launch for the three planes, in the shape of k_ingest.  The picture is H luma row tasks and
// H / 2 chroma row tasks (a chroma task reads its two source rows and writes the U row and the V
// row); a wave takes whole tasks, a lane 16 output bytes of the row per step.  Where a sample lies,
// what it is worth and how chroma is reduced is jmh_yuv.h's; this file only loads the runs of a
// source row whose fields are consecutive as vectors and picks the fields out of registers:
//   - a vector whose source samples all lie inside the source row loads their run whole: 16-byte
//     loads when every plane base and stride is 16-byte aligned (a wave-uniform test), else aligned
//     dwords funnelled with v_alignbyte (and one more only where the address is not dword aligned,
//     which then holds the run's last bytes).  Packed luma is de-interleaved with v_perm_b32
//     (jmi_deint), every other field is a constant bit field of a register (v_bfe_u32).  The left
//     neighbour of a left-sited vector is the one sample before its run, read by itself: steps of
//     a row task have different trip counts per lane, so there is no lane to hand it over;
//   - the vector that straddles the source width, and those beyond it, take every sample through
//     jmy_coded_sample (the clamped column); rows below the source height read the clamped rows.
// So of every row only aligned dwords that hold one of the row's bytes are read.  Output rows are
// 16-byte aligned (the coded width is a multiple of 16) but for 8-bit chroma of an odd number of
// macroblock columns, whose rows are 8-byte aligned: those are stored as 8-byte halves.
// All address arithmetic is 64-bit.  No LDS, no scratch.  I210 / I410 samples above maxv are counted
// per lane (each source sample by the one vector that owns it), summed over the wave, one atomic
// per wave that has any.
#include <hip/hip_runtime.h>
#include "jmh_launch.h"
#include "jmh_yuv.h"

#define YUV_WAVES 4

struct YuvVec { uint32_t d[4]; };

// 4 * N bytes at any address: aligned dwords + v_alignbyte
template <int N>
__device__ __forceinline__ void yuv_load(const uint8_t *p, bool al16, uint32_t *out) {
    if (al16) {
#pragma unroll
        for (int i = 0; i < N / 4; i++) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            out[4 * i] = v.x; out[4 * i + 1] = v.y; out[4 * i + 2] = v.z; out[4 * i + 3] = v.w;
        }
        return;
    }
    const uint32_t sel = (uint32_t)(uintptr_t)p & 3u;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sel);
    uint32_t w[N + 1];
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = q[i];
    w[N] = sel ? q[N] : 0u;             // holds the last sel bytes of the run; not read otherwise
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sel);
}

// 16 bytes (or the row's last 8) at out + b0 of a row of ob bytes; R16: the rows are 16-byte aligned
template <bool R16>
__device__ __forceinline__ void yuv_store(uint8_t *out, int64_t b0, int ob, const YuvVec &v) {
    if (R16) {
        *reinterpret_cast<uint4 *>(out + b0) = make_uint4(v.d[0], v.d[1], v.d[2], v.d[3]);
    } else {
        *reinterpret_cast<uint2 *>(out + b0) = make_uint2(v.d[0], v.d[1]);
        if (b0 + 8 < ob) *reinterpret_cast<uint2 *>(out + b0 + 8) = make_uint2(v.d[2], v.d[3]);
    }
}

// the raw field of sample k of a run held in registers (k counted from the run's first sample; a
// field never straddles a dword)
__device__ __forceinline__ uint32_t yuv_field(jmy_field f, const uint32_t *s, int k) {
    const int bit = k * f.pitch + f.first;
    return s[bit >> 5] >> (bit & 31) & ((1u << f.bits) - 1u);
}
// sample i (ES bytes) of an output vector
template <int ES>
__device__ __forceinline__ void yuv_put(YuvVec &v, int i, uint32_t val) {
    if ((i * ES & 3) == 0) v.d[i * ES / 4] = val;
    else v.d[i * ES / 4] |= val << (8 * (i * ES & 3));
}

// the vector at sample x0 of row y of plane pl, sample by sample (PW: the coded row's samples;
// samples beyond it are not read and not stored)
template <int FORMAT>
__device__ __forceinline__ void yuv_edge(const YuvArgs &a, int pl, int x0, int y, int PW, YuvVec &v, uint32_t *over) {
    constexpr int ES = jmy_wide(jmy_layout(FORMAT)) ? 2 : 1, NS = 16 / ES;
    v.d[0] = v.d[1] = v.d[2] = v.d[3] = 0;
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const int x = x0 + i;
        if (x >= PW) break;
        const uint32_t val = jmy_coded_sample(FORMAT, a.plane, a.stride, pl, x, y, a.w, a.h, a.maxv, over);
        v.d[i * ES / 4] |= val << (8 * (i * ES & 3));
    }
}

// a luma vector whose NS samples lie inside the source row
template <int FMT>
__device__ __forceinline__ void yuv_luma(const uint8_t *row, int x0, bool al16, uint32_t maxv, YuvVec &v, uint32_t *over) {
    constexpr jmy_field F = jmy_comp(FMT, 0);
    constexpr int ES = jmy_wide(FMT) ? 2 : 1, NS = 16 / ES, ND = NS * F.pitch / 32;
    uint32_t s[ND];
    yuv_load<ND>(row + (int64_t)x0 * (F.pitch / 8), al16, s);
    if constexpr (F.pitch == F.bits && !jmy_wide(FMT)) {                        // planar bytes: moved untouched
#pragma unroll
        for (int i = 0; i < 4; i++) v.d[i] = s[i];
    } else if constexpr (F.pitch == 2 * F.bits && F.bits >= 8) {                // Y0 U Y1 V: every other byte or word
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t d = jmi_deint(s[2 * i], s[2 * i + 1], F.first / F.bits, F.bits == 16);
            v.d[i] = F.bits == 16 ? d >> F.shift & 0x03ff03ffu : d;   // (the only such 16-bit layout is Y210)
        }
    } else {
#pragma unroll
        for (int i = 0; i < NS; i++) yuv_put<ES>(v, i, jmy_value(FMT, F, yuv_field(F, s, i), maxv, over));
    }
}

// The sums of one source row for NS output chroma samples from i0 on (all inside the source row):
// added to hu, hv.  row1: the row of U's plane, row2: of V's (the same row where they share a plane)
template <int FMT, bool LEFT>
__device__ __forceinline__ void yuv_chroma_row(const uint8_t *row1, const uint8_t *row2, int i0, bool al16, uint32_t maxv, uint32_t *hu, uint32_t *hv,
                                               uint32_t *over) {
    constexpr jmy_field FU = jmy_comp(FMT, 1), FV = jmy_comp(FMT, 2);
    constexpr bool IS444 = jmy_444(FMT), SHARED = FU.sp == FV.sp;
    constexpr int ES = jmy_wide(FMT) ? 2 : 1, NS = 16 / ES, NSRC = IS444 ? 2 * NS : NS, ND = NSRC * FU.pitch / 32;
    const int k0 = IS444 ? 2 * i0 : i0;                               // the run's first source sample
    const int64_t b0 = (int64_t)k0 * (FU.pitch / 8);
    uint32_t su[ND], sv[SHARED ? 1 : ND];
    yuv_load<ND>(row1 + b0, al16, su);
    if constexpr (!SHARED) yuv_load<ND>(row2 + b0, al16, sv);
    const uint32_t *pv = SHARED ? su : sv;
    uint32_t lu = 0, lv = 0, none = 0;
    if (LEFT) {                                                       // C[max(2 i0 - 1, 0)]: counted by the vector before
        lu = jmy_sample(FMT, FU, row1, k0 ? k0 - 1 : 0, maxv, &none);
        lv = jmy_sample(FMT, FV, row2, k0 ? k0 - 1 : 0, maxv, &none);
    }
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const int k = IS444 ? 2 * i : i;
        const uint32_t au = jmy_value(FMT, FU, yuv_field(FU, su, k), maxv, over), av = jmy_value(FMT, FV, yuv_field(FV, pv, k), maxv, over);
        const uint32_t bu = IS444 ? jmy_value(FMT, FU, yuv_field(FU, su, k + 1), maxv, over) : 0;
        const uint32_t bv = IS444 ? jmy_value(FMT, FV, yuv_field(FV, pv, k + 1), maxv, over) : 0;
        hu[i] += jmy_hsum(IS444, LEFT, lu, au, bu);
        hv[i] += jmy_hsum(IS444, LEFT, lv, av, bv);
        lu = bu; lv = bv;
    }
}

// one row task of a wave: luma row task, or the U and V rows task - a.H
template <int FMT, bool LEFT, bool R16>
__device__ __forceinline__ void yuv_task(const YuvArgs &a, int task, int lane, bool al16, uint32_t &over) {
    constexpr int FORMAT = FMT | (LEFT ? JMY_CHROMA_LEFT : 0);
    constexpr bool IS444 = jmy_444(FMT);
    constexpr int ES = jmy_wide(FMT) ? 2 : 1, NS = 16 / ES;
    const bool chroma = task >= a.H;
    const int y = chroma ? task - a.H : task;
    const int PW = chroma ? a.W / 2 : a.W, pw = chroma ? a.w / 2 : a.w, ph = chroma ? a.h / 2 : a.h;
    const int ob = PW * ES, nvec = (ob + 15) / 16;
    const bool counted = y < ph;                                      // a row of the reduced source, not a replica
    const int cy = jmi_clamp(y, ph);
    if (!chroma) {
        constexpr jmy_field F = jmy_comp(FMT, 0);
        const uint8_t *row = a.plane[F.sp] + (int64_t)cy * a.stride[F.sp];
        uint8_t *o = a.dst + (size_t)y * PW * ES;
        for (int k = lane; k < nvec; k += 64) {
            const int x0 = k * NS;
            YuvVec v;
            if (x0 + NS <= pw) {
                uint32_t ov = 0;
                yuv_luma<FMT>(row, x0, al16, a.maxv, v, &ov);
                if (counted) over += ov;
            } else {
                yuv_edge<FORMAT>(a, 0, x0, y, PW, v, &over);
            }
            yuv_store<R16>(o, (int64_t)16 * k, ob, v);
        }
    } else {
        constexpr jmy_field FU = jmy_comp(FMT, 1), FV = jmy_comp(FMT, 2);
        const uint8_t *ru = a.plane[FU.sp] + (int64_t)(2 * cy) * a.stride[FU.sp], *rv = a.plane[FV.sp] + (int64_t)(2 * cy) * a.stride[FV.sp];
        uint8_t *o1 = a.dst + (jmi_dst_off(1, a.W, a.H) + (size_t)y * PW) * ES;
        uint8_t *o2 = a.dst + (jmi_dst_off(2, a.W, a.H) + (size_t)y * PW) * ES;
        for (int k = lane; k < nvec; k += 64) {
            const int i0 = k * NS;
            YuvVec u, v;
            if (i0 + NS <= pw) {
                uint32_t hu[NS], hv[NS], ov = 0;
#pragma unroll
                for (int i = 0; i < NS; i++) hu[i] = hv[i] = 0;
                yuv_chroma_row<FMT, LEFT>(ru, rv, i0, al16, a.maxv, hu, hv, &ov);
                yuv_chroma_row<FMT, LEFT>(ru + a.stride[FU.sp], rv + a.stride[FV.sp], i0, al16, a.maxv, hu, hv, &ov);
                if (counted) over += ov;
#pragma unroll
                for (int i = 0; i < NS; i++) {
                    yuv_put<ES>(u, i, jmy_round(IS444, LEFT, hu[i], 0));
                    yuv_put<ES>(v, i, jmy_round(IS444, LEFT, hv[i], 0));
                }
            } else {
                yuv_edge<FORMAT>(a, 1, i0, y, PW, u, &over);
                yuv_edge<FORMAT>(a, 2, i0, y, PW, v, &over);
            }
            yuv_store<R16>(o1, (int64_t)16 * k, ob, u);
            yuv_store<R16>(o2, (int64_t)16 * k, ob, v);
        }
    }
}

template <int FMT, bool LEFT>
__global__ __launch_bounds__(64 * YUV_WAVES) void k_ingest_yuv(YuvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntask = a.H + a.H / 2, nblk = (ntask + YUV_WAVES - 1) / YUV_WAVES;
    uint64_t bits = 0;
    for (int sp = 0; sp < jmy_planes(FMT); sp++) bits |= (uint64_t)(uintptr_t)a.plane[sp] | (uint64_t)a.stride[sp];
    const bool al16 = (bits & 15) == 0;
    uint32_t over = 0;
    const int blk = xcd_block(blockIdx.x, nblk);
    const int task = blk * YUV_WAVES + wave;
    if (blk < nblk && task < ntask) {
        // output rows are 16-byte aligned but for 8-bit chroma of an odd number of macroblock columns (wave-uniform)
        if (jmy_wide(FMT) || task < a.H || (a.W & 31) == 0) yuv_task<FMT, LEFT, true>(a, task, lane, al16, over);
        else yuv_task<FMT, LEFT, false>(a, task, lane, al16, over);
    }
    if (jmy_clamps(FMT)) {                                            // the only layouts that clamp
#pragma unroll
        for (int m = 32; m; m >>= 1) over += __shfl_xor(over, m);
        if (lane == 0 && over) atomicAdd(a.clamped, (unsigned long long)over);
    }
}

template <int FMT>
static void yuv_launch(bool left, const YuvArgs &a, dim3 grid, dim3 block, hipStream_t st) {
    if (left && jmy_444(FMT)) hipLaunchKernelGGL((k_ingest_yuv<FMT, jmy_444(FMT)>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_ingest_yuv<FMT, false>), grid, block, 0, st, a);
}

hipError_t jmh_launch_ingest_yuv(int format, const YuvArgs &a, hipStream_t st) {
    const int ntask = a.H + a.H / 2;
    const dim3 grid(xcd_grid((ntask + YUV_WAVES - 1) / YUV_WAVES)), block(64 * YUV_WAVES);
    const bool left = jmy_left(format);
    switch (jmy_layout(format)) {
    case JMY_I422: yuv_launch<JMY_I422>(left, a, grid, block, st); break;
    case JMY_NV16: yuv_launch<JMY_NV16>(left, a, grid, block, st); break;
    case JMY_YUYV: yuv_launch<JMY_YUYV>(left, a, grid, block, st); break;
    case JMY_UYVY: yuv_launch<JMY_UYVY>(left, a, grid, block, st); break;
    case JMY_I444: yuv_launch<JMY_I444>(left, a, grid, block, st); break;
    case JMY_VUYA8: yuv_launch<JMY_VUYA8>(left, a, grid, block, st); break;
    case JMY_I210: yuv_launch<JMY_I210>(left, a, grid, block, st); break;
    case JMY_P210: yuv_launch<JMY_P210>(left, a, grid, block, st); break;
    case JMY_Y210: yuv_launch<JMY_Y210>(left, a, grid, block, st); break;
    case JMY_I410: yuv_launch<JMY_I410>(left, a, grid, block, st); break;
    case JMY_Y410: yuv_launch<JMY_Y410>(left, a, grid, block, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
