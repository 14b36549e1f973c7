// jmh_rgb.hip — k_ingest_rgb: an RGB device picture (include/jmhip_rgb.h) converted
// to 4:2:0, packed and padded into a ring entry's source, where k_ingest moves a YUV one.
//
// One launch per picture.  A task is a pair of luma rows with their U row and V row (H / 2 tasks); a
// wave takes whole tasks, a lane 8 pixels x 2 rows per step: four 16-byte loads when the base and
// the stride are 16-byte aligned (a wave-uniform test), else sixteen dword loads (pixels are dword
// aligned by the argument rule, so no byte funnel is needed).  What a pixel's dword means and every
// sample's value is jmh_rgb.h's (jmr_unpack, jmr_luma, jmr_chroma); the coefficients arrive in the
// kernel arguments, wave-uniform.  A lane stores 8 luma samples per row (8 bytes, or 16 in a 10-bit
// context) and 4 U and 4 V samples (4 bytes each, or 8): no byte or short stores, and none wider
// than the alignment of any output row (8-bit chroma rows of an odd number of macroblock columns
// are 8-byte aligned; a lane's 4 bytes of them are dword aligned).
//   - the vector that straddles the source width, and those beyond it, go block by block through
//     the clamped column: only dwords of source pixels are read, never beyond 4 * w in a row;
//   - a row pair below the source height reads the last pair of the source: its chroma is that
//     block row's, both its luma rows are the last source row's.
// All address arithmetic is 64-bit.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include "jmh_launch.h"
#include "jmh_rgb.h"

#define RGB_WAVES 4

// the 2x2 block of dwords p00 p01 / p10 p11: its four luma samples and its U and V
template <int FMT>
__device__ __forceinline__ void rgb_block(const jmr_coef &k, uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int32_t *y0, int32_t *y1,
                                          int32_t *u, int32_t *v) {
    int32_t r[4], g[4], b[4];
    jmr_unpack(FMT, p00, &r[0], &g[0], &b[0]);
    jmr_unpack(FMT, p01, &r[1], &g[1], &b[1]);
    jmr_unpack(FMT, p10, &r[2], &g[2], &b[2]);
    jmr_unpack(FMT, p11, &r[3], &g[3], &b[3]);
    y0[0] = jmr_luma(&k, r[0], g[0], b[0]);
    y0[1] = jmr_luma(&k, r[1], g[1], b[1]);
    y1[0] = jmr_luma(&k, r[2], g[2], b[2]);
    y1[1] = jmr_luma(&k, r[3], g[3], b[3]);
    const int32_t rs = r[0] + r[1] + r[2] + r[3], gs = g[0] + g[1] + g[2] + g[3], bs = b[0] + b[1] + b[2] + b[3];
    *u = jmr_chroma(&k, 0, rs, gs, bs);
    *v = jmr_chroma(&k, 1, rs, gs, bs);
}

// 8 pixels of a row that lie inside the source
__device__ __forceinline__ void rgb_load8(const uint8_t *p, bool al16, uint32_t *d) {
    if (al16) {
        const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = reinterpret_cast<const uint32_t *>(p)[i];
    }
}

template <int FMT>
__global__ __launch_bounds__(64 * RGB_WAVES) void k_ingest_rgb(RgbArgs a) {
    constexpr bool TEN = jmr_ten(FMT);
    constexpr int ES = TEN ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntask = a.H / 2, nblk = (ntask + RGB_WAVES - 1) / RGB_WAVES;
    const bool al16 = (((uint64_t)(uintptr_t)a.src | (uint64_t)a.stride) & 15) == 0;
    const int blk = xcd_block(blockIdx.x, nblk);
    const int task = blk * RGB_WAVES + wave;
    if (blk >= nblk || task >= ntask) return;
    const jmr_coef &k = a.k;
    const int W = a.W, w = a.w, CW = W / 2;
    const int sy = jmi_clamp(task, a.h / 2) * 2;                  // the source row pair (the last one below the source)
    const bool below = 2 * task >= a.h;                           // both luma rows are the last source row's
    const uint8_t *row0 = a.src + jmr_src_off(0, sy, a.stride), *row1 = row0 + a.stride;
    uint8_t *oy0 = a.dst + (size_t)(2 * task) * W * ES, *oy1 = oy0 + (size_t)W * ES;
    uint8_t *ou = a.dst + (jmi_dst_off(1, W, a.H) + (size_t)task * CW) * ES;
    uint8_t *ov = a.dst + (jmi_dst_off(2, W, a.H) + (size_t)task * CW) * ES;
    for (int x0 = 8 * lane; x0 < W; x0 += 8 * 64) {
        int32_t y0[8], y1[8], u[4], v[4];
        if (x0 + 8 <= w) {
            uint32_t p0[8], p1[8];
            rgb_load8(row0 + (int64_t)4 * x0, al16, p0);
            rgb_load8(row1 + (int64_t)4 * x0, al16, p1);
#pragma unroll
            for (int j = 0; j < 4; j++) rgb_block<FMT>(k, p0[2 * j], p0[2 * j + 1], p1[2 * j], p1[2 * j + 1], y0 + 2 * j, y1 + 2 * j, &u[j], &v[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int bx = jmi_clamp(x0 / 2 + j, w / 2);      // the clamped block column
                const int64_t o = (int64_t)8 * bx;
                rgb_block<FMT>(k, jmr_load(row0 + o), jmr_load(row0 + o + 4), jmr_load(row1 + o), jmr_load(row1 + o + 4), y0 + 2 * j, y1 + 2 * j,
                               &u[j], &v[j]);
                if (x0 + 2 * j >= w) { y0[2 * j] = y0[2 * j + 1]; y1[2 * j] = y1[2 * j + 1]; }   // beyond the source: the last column's
            }
        }
        if (below) {
#pragma unroll
            for (int i = 0; i < 8; i++) y0[i] = y1[i];
        }
        ingest_store_luma<TEN>(oy0 + (size_t)x0 * ES, y0);
        ingest_store_luma<TEN>(oy1 + (size_t)x0 * ES, y1);
        ingest_store_chroma<TEN>(ou + (size_t)(x0 / 2) * ES, u);
        ingest_store_chroma<TEN>(ov + (size_t)(x0 / 2) * ES, v);
    }
}

hipError_t jmh_launch_ingest_rgb(int format, const RgbArgs &a, hipStream_t st) {
    const int ntask = a.H / 2;
    const dim3 grid(xcd_grid((ntask + RGB_WAVES - 1) / RGB_WAVES)), block(64 * RGB_WAVES);
    switch (jmr_layout(format)) {
    case JMR_BGRA8: hipLaunchKernelGGL(k_ingest_rgb<JMR_BGRA8>, grid, block, 0, st, a); break;
    case JMR_RGBA8: hipLaunchKernelGGL(k_ingest_rgb<JMR_RGBA8>, grid, block, 0, st, a); break;
    case JMR_RGB10A2: hipLaunchKernelGGL(k_ingest_rgb<JMR_RGB10A2>, grid, block, 0, st, a); break;
    case JMR_BGR10A2: hipLaunchKernelGGL(k_ingest_rgb<JMR_BGR10A2>, grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
