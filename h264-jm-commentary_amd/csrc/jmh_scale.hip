// jmh_scale.hip — k_scale: the packed 4:2:0 picture an ingest kernel wrote at the source's size
// resampled to the setting's output size and padded into a ring entry's source
// (include/jmhip_scale.h).
//
// One launch for the three planes.  A workgroup of four waves owns a JMS_TILE_W x JMS_TILE_H tile of
// one plane of the coded size; the padding is the clamp of the tile's output coordinates, so a lane
// beyond the output size computes the last column or row again.  What a tap is, where it reads and
// how a sum is rounded is jmh_scale.h's; the tables are those of jms_pack_axis.
//   Pass 1.  A lane owns an output column and keeps its taps as packed pairs in registers; the waves
//     share the source rows the tile's vertical taps reach (from the even row at or below the first
//     one).  Every row is filtered with v_dot2 into LDS as int16, rows 2m and 2m + 1 in one dword.
//   Pass 2.  A wave owns four output rows.  A row's taps are wave-uniform (scalar loads), paired as
//     the rows are paired in LDS; a lane reads one dword per pair, consecutive lanes consecutive
//     banks.  The samples go to a small LDS tile,
//   from which the tile's rows are stored as 16-byte vectors (8-byte ones where the plane's rows are
//     only 8-byte aligned: 8-bit chroma of an odd number of macroblock columns).
// All address arithmetic on the pictures is 64-bit.
#include <hip/hip_runtime.h>
#include "jmh_launch.h"
#include "jmh_scale.h"

#define SCL_WAVES 4

typedef short scl_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int32_t scl_dot2(uint32_t a, uint32_t b, int32_t c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(scl_s2, a), __builtin_bit_cast(scl_s2, b), c, false);
}
__device__ __forceinline__ int scl_min(int a, int b) { return a < b ? a : b; }

template <class pel>
__global__ __launch_bounds__(64 * SCL_WAVES) void k_scale(ScaleArgs a) {
    constexpr int ES = sizeof(pel);
    __shared__ uint32_t mid[JMS_SPAN_MAX / 2][JMS_TILE_W];
    __shared__ __attribute__((aligned(16))) pel tile[JMS_TILE_H][JMS_TILE_W];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ltx = (a.W + JMS_TILE_W - 1) / JMS_TILE_W, lty = (a.H + JMS_TILE_H - 1) / JMS_TILE_H;
    const int ctx = (a.W / 2 + JMS_TILE_W - 1) / JMS_TILE_W, cty = (a.H / 2 + JMS_TILE_H - 1) / JMS_TILE_H;
    const int nl = ltx * lty, nc = ctx * cty, ntile = nl + 2 * nc;
    int t = xcd_block(blockIdx.x, ntile);
    if (t >= ntile) return;
    int pl = 0, tx, ty;
    if (t < nl) { tx = t % ltx; ty = t / ltx; }
    else { t -= nl; pl = 1 + t / nc; t %= nc; tx = t % ctx; ty = t / ctx; }
    const int c = pl ? 1 : 0;
    const int sw = c ? a.w / 2 : a.w, sh = c ? a.h / 2 : a.h, dw = c ? a.ow / 2 : a.ow, dh = c ? a.oh / 2 : a.oh;
    const int SPW = c ? a.sW / 2 : a.sW, PW = c ? a.W / 2 : a.W, PH = c ? a.H / 2 : a.H;
    const pel *__restrict__ sp = reinterpret_cast<const pel *>(a.src) + jmi_dst_off(pl, a.sW, a.sH);
    pel *__restrict__ dp = reinterpret_cast<pel *>(a.dst) + jmi_dst_off(pl, a.W, a.H);
    const int32_t *__restrict__ fv = a.fv[c];

    const int y0 = ty * JMS_TILE_H, y1 = scl_min(y0 + JMS_TILE_H - 1, PH - 1);
    const int r_base = fv[jmi_clamp(y0, dh)] & ~1;
    const int nr = scl_min(fv[jmi_clamp(y1, dh)] + a.tv_taps[c] - r_base, JMS_SPAN_MAX);

    // pass 1: the rows r_base .. r_base + nr - 1 of the source (clamped), this lane's column
    {
        const int xc = jmi_clamp(tx * JMS_TILE_W + lane, dw);
        const int fx = a.fh[c][xc];
        uint32_t tp[JMS_HPAIRS];
        const uint4 *__restrict__ q = reinterpret_cast<const uint4 *>(a.th[c] + (size_t)xc * JMS_HPAIRS);
#pragma unroll
        for (int i = 0; i < JMS_HPAIRS / 4; i++) {
            const uint4 v = q[i];
            tp[4 * i] = v.x; tp[4 * i + 1] = v.y; tp[4 * i + 2] = v.z; tp[4 * i + 3] = v.w;
        }
        const int nph = a.nph[c];
        int16_t *m16 = reinterpret_cast<int16_t *>(&mid[0][0]);
        for (int i = wave; i < nr; i += SCL_WAVES) {
            const pel *__restrict__ row = sp + (size_t)jms_tap_at(r_base + i, sh) * SPW;
            int32_t acc = 0;
#pragma unroll
            for (int p = 0; p < JMS_HPAIRS; p++)
                if (p < nph) {
                    const uint32_t s0 = row[jms_tap_at(fx + 2 * p, sw)], s1 = row[jms_tap_at(fx + 2 * p + 1, sw)];
                    acc = scl_dot2(s0 | s1 << 16, tp[p], acc);
                }
            m16[((i >> 1) * JMS_TILE_W + lane) * 2 + (i & 1)] = (int16_t)jms_hpass(acc, a.P);
        }
    }
    __syncthreads();

    // pass 2: four output rows of the tile per wave
    {
        const int npv = a.npv[c];
        for (int k = 0; k < JMS_TILE_H / SCL_WAVES; k++) {
            const int ry = wave * (JMS_TILE_H / SCL_WAVES) + k;
            if (y0 + ry > y1) break;
            const int yc = jmi_clamp(y0 + ry, dh);
            const int m0 = ((fv[yc] & ~1) - r_base) >> 1;
            const uint32_t *__restrict__ tv = a.tv[c] + (size_t)yc * JMS_VPAIRS;
            int32_t acc = 0;
#pragma unroll
            for (int p = 0; p < JMS_VPAIRS; p++)
                if (p < npv) acc = scl_dot2(mid[scl_min(m0 + p, JMS_SPAN_MAX / 2 - 1)][lane], tv[p], acc);
            tile[ry][lane] = (pel)jms_vpass(acc, a.P, a.maxv);
        }
    }
    __syncthreads();

    // the tile's rows as vectors: 16 bytes where the plane's rows are 16-byte aligned, else 8
    {
        const int rows = y1 - y0 + 1, x0 = tx * JMS_TILE_W;
        const int tb = scl_min(JMS_TILE_W, PW - x0) * ES;      // a multiple of 8: PW is one
        const bool r16 = ((PW * ES) & 15) == 0;
        const int vb = r16 ? 16 : 8, nv = tb / vb;
        for (int i = threadIdx.x; i < rows * nv; i += 64 * SCL_WAVES) {
            const int ry = i / nv, vx = i % nv;
            const uint8_t *s = reinterpret_cast<const uint8_t *>(&tile[ry][0]) + vx * vb;
            uint8_t *d = reinterpret_cast<uint8_t *>(dp + (size_t)(y0 + ry) * PW + x0) + vx * vb;
            if (r16) *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(s);
            else *reinterpret_cast<uint2 *>(d) = *reinterpret_cast<const uint2 *>(s);
        }
    }
}

hipError_t jmh_launch_scale(const ScaleArgs &a, hipStream_t st) {
    const int nl = ((a.W + JMS_TILE_W - 1) / JMS_TILE_W) * ((a.H + JMS_TILE_H - 1) / JMS_TILE_H);
    const int nc = ((a.W / 2 + JMS_TILE_W - 1) / JMS_TILE_W) * ((a.H / 2 + JMS_TILE_H - 1) / JMS_TILE_H);
    const dim3 grid(xcd_grid(nl + 2 * nc)), block(64 * SCL_WAVES);
    if (a.maxv > 255) hipLaunchKernelGGL(k_scale<uint16_t>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_scale<uint8_t>, grid, block, 0, st, a);
    return hipGetLastError();
}
