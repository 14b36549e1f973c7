// jmh_ingest.hip — k_ingest: a device picture (include/jmhip_input.h) packed and
// padded into a ring entry's source, where a host picture is packed on the CPU and uploaded.
//
// One launch for the three planes.  The picture is H luma row tasks and H / 2 chroma row tasks (a
// chroma task writes the U row and the V row); a wave takes whole tasks, a lane 16 output bytes of
// the row per step.  Where a sample comes from and what is stored for it is jmh_ingest.h's; this
// file only moves the runs of samples whose source bytes are consecutive as vectors:
//   - a vector that lies inside the source row is loaded whole: 16-byte loads when every plane
//     base and stride is 16-byte aligned (a wave-uniform test), else aligned dwords funnelled with
//     v_alignbyte (four or eight, and one more only where the address is not dword aligned, which
//     then holds the vector's last bytes).  An interleaved UV row gives 32 bytes per lane, split
//     into a U and a V vector with v_perm_b32 (jmi_deint);
//   - the vector that straddles the source width, and those beyond it, take every sample through
//     jmi_src (the clamped column); rows below the source height read the clamped row.
// So of every row only aligned dwords that hold one of the row's bytes are read.  Output rows are
// 16-byte aligned (the coded width is a multiple of 16) but for 8-bit chroma of an odd number of
// macroblock columns, whose rows are 8-byte aligned: those are stored as 8-byte halves.
// All address arithmetic is 64-bit.  I010 samples above maxv are counted per lane, summed over the
// wave, one atomic per wave that has any.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "jmh_launch.h"
#include "jmh_ingest.h"

#define ING_WAVES 4

struct Vec16 { uint32_t d[4]; };

// 4 * N bytes at any address (2-byte aligned for 16-bit samples): aligned dwords + v_alignbyte
template <int N>
__device__ __forceinline__ void ing_load(const uint8_t *p, bool al16, uint32_t *out) {
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
__device__ __forceinline__ void ing_store(uint8_t *out, int64_t b0, int ob, const Vec16 &v) {
    if (R16) {
        *reinterpret_cast<uint4 *>(out + b0) = make_uint4(v.d[0], v.d[1], v.d[2], v.d[3]);
    } else {
        *reinterpret_cast<uint2 *>(out + b0) = make_uint2(v.d[0], v.d[1]);
        if (b0 + 8 < ob) *reinterpret_cast<uint2 *>(out + b0 + 8) = make_uint2(v.d[2], v.d[3]);
    }
}

template <int FMT>
__device__ __forceinline__ void ing_values(Vec16 &v, uint32_t maxv, uint32_t *over) {
    if (jmi_wide(FMT))
#pragma unroll
        for (int i = 0; i < 4; i++) v.d[i] = jmi_value_x2(FMT, v.d[i], maxv, over);
}

// the vector at sample x0 of row y of plane pl, sample by sample (the clamped column, PW: the
// coded row's samples; samples beyond it are not read and not stored)
template <int FMT>
__device__ __forceinline__ void ing_edge(const IngestArgs &a, int pl, int x0, int y, int PW, Vec16 &v, uint32_t *over) {
    constexpr int ES = jmi_wide(FMT) ? 2 : 1, NS = 16 / ES;
    v.d[0] = v.d[1] = v.d[2] = v.d[3] = 0;
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const int x = x0 + i;
        if (x >= PW) break;
        int sp;
        int64_t off;
        jmi_src(FMT, pl, x, y, a.w, a.h, a.stride, &sp, &off);
        const uint8_t *p = a.plane[sp] + off;
        const uint32_t raw = ES == 2 ? *reinterpret_cast<const uint16_t *>(p) : *p;
        uint32_t o = 0;
        const uint32_t val = jmi_value(FMT, raw, a.maxv, &o);
        if (jmi_in_source(pl, x, y, a.w, a.h)) *over += o;
        v.d[i * ES / 4] |= val << (8 * (i * ES & 3));
    }
}

// one row task of a wave: luma row task, or the U and V rows task - a.H
template <int FMT, bool R16>
__device__ __forceinline__ void ing_task(const IngestArgs &a, int task, int lane, bool al16, uint32_t &over) {
    constexpr bool SEMI = jmi_semi(FMT);
    constexpr int ES = jmi_wide(FMT) ? 2 : 1, NS = 16 / ES;
    {
        const bool chroma = task >= a.H;
        const int y = chroma ? task - a.H : task;
        const int PW = chroma ? a.W / 2 : a.W, pw = chroma ? a.w / 2 : a.w, ph = chroma ? a.h / 2 : a.h;
        const int ob = PW * ES, nvec = (ob + 15) / 16;
        const bool counted = y < ph;                         // a row of the source, not a replica
        uint8_t *o1 = a.dst + (jmi_dst_off(chroma ? 1 : 0, a.W, a.H) + (size_t)y * PW) * ES;
        uint8_t *o2 = a.dst + (jmi_dst_off(2, a.W, a.H) + (size_t)y * PW) * ES;
        int sp0;
        int64_t r0;
        jmi_src(FMT, chroma ? 1 : 0, 0, y, a.w, a.h, a.stride, &sp0, &r0);   // the clamped row's start
        if (chroma && SEMI) {
            const uint8_t *row = a.plane[sp0] + r0;
            for (int k = lane; k < nvec; k += 64) {
                const int x0 = k * NS;
                Vec16 u, v;
                uint32_t ov = 0;
                if (x0 + NS <= pw) {
                    uint32_t s[8];
                    ing_load<8>(row + (int64_t)32 * k, al16, s);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        u.d[i] = jmi_deint(s[2 * i], s[2 * i + 1], 0, ES == 2);
                        v.d[i] = jmi_deint(s[2 * i], s[2 * i + 1], 1, ES == 2);
                    }
                    ing_values<FMT>(u, a.maxv, &ov);
                    ing_values<FMT>(v, a.maxv, &ov);
                    if (counted) over += ov;
                } else {
                    ing_edge<FMT>(a, 1, x0, y, PW, u, &over);
                    ing_edge<FMT>(a, 2, x0, y, PW, v, &over);
                }
                ing_store<R16>(o1, (int64_t)16 * k, ob, u);
                ing_store<R16>(o2, (int64_t)16 * k, ob, v);
            }
        } else {
            for (int pl = chroma ? 1 : 0; pl <= (chroma ? 2 : 0); pl++) {
                int sp;
                int64_t r;
                jmi_src(FMT, pl, 0, y, a.w, a.h, a.stride, &sp, &r);
                const uint8_t *row = a.plane[sp] + r;
                uint8_t *o = pl == 2 ? o2 : o1;
                for (int k = lane; k < nvec; k += 64) {
                    const int x0 = k * NS;
                    Vec16 v;
                    uint32_t ov = 0;
                    if (x0 + NS <= pw) {
                        ing_load<4>(row + (int64_t)16 * k, al16, v.d);
                        ing_values<FMT>(v, a.maxv, &ov);
                        if (counted) over += ov;
                    } else {
                        ing_edge<FMT>(a, pl, x0, y, PW, v, &over);
                    }
                    ing_store<R16>(o, (int64_t)16 * k, ob, v);
                }
            }
        }
    }
}

template <int FMT>
__global__ __launch_bounds__(64 * ING_WAVES) void k_ingest(IngestArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntask = a.H + a.H / 2, nblk = (ntask + ING_WAVES - 1) / ING_WAVES;
    uint64_t bits = 0;
    for (int sp = 0; sp < jmi_planes(FMT); sp++) bits |= (uint64_t)(uintptr_t)a.plane[sp] | (uint64_t)a.stride[sp];
    const bool al16 = (bits & 15) == 0;
    uint32_t over = 0;
    const int blk = xcd_block(blockIdx.x, nblk);
    const int task = blk * ING_WAVES + wave;
    if (blk < nblk && task < ntask) {
        // output rows are 16-byte aligned but for 8-bit chroma of an odd number of macroblock columns (wave-uniform)
        if (jmi_wide(FMT) || task < a.H || (a.W & 31) == 0) ing_task<FMT, true>(a, task, lane, al16, over);
        else ing_task<FMT, false>(a, task, lane, al16, over);
    }
    if (FMT == JMI_I010) {                                   // the only format that clamps
#pragma unroll
        for (int m = 32; m; m >>= 1) over += __shfl_xor(over, m);
        if (lane == 0 && over) atomicAdd(a.clamped, (unsigned long long)over);
    }
}

hipError_t jmh_launch_ingest(int format, const IngestArgs &a, hipStream_t st) {
    const int ntask = a.H + a.H / 2;
    const dim3 grid(xcd_grid((ntask + ING_WAVES - 1) / ING_WAVES)), block(64 * ING_WAVES);
    switch (format) {
    case JMI_I420: hipLaunchKernelGGL(k_ingest<JMI_I420>, grid, block, 0, st, a); break;
    case JMI_NV12: hipLaunchKernelGGL(k_ingest<JMI_NV12>, grid, block, 0, st, a); break;
    case JMI_I010: hipLaunchKernelGGL(k_ingest<JMI_I010>, grid, block, 0, st, a); break;
    case JMI_P010: hipLaunchKernelGGL(k_ingest<JMI_P010>, grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
