// jmh_tensor.hip — k_ingest_tensor: a device tensor (include/jmhip_tensor.h) quantised,
// converted to 4:2:0, packed and padded into a ring entry's source, where k_ingest_rgb converts a
// picture of packed dwords.
//
// One launch per picture.  A task is a pair of luma rows with their U row and V row (H / 2 tasks), in
// xcd_block order; a wave takes whole tasks, a lane 8 pixels x 2 rows per step: 8 elements of each of
// the three channels in both rows.  What an element's bits mean and every sample's value is
// jmh_tensor.h's and jmh_rgb.h's (jmt_quant, jmr_luma, jmr_chroma); the coefficients arrive in the
// kernel arguments, wave-uniform, and their maxv is the quantiser's M.  U8 writes 8-bit samples, U16
// 16-bit ones; a float instance serves both contexts and picks its stores by maxv (wave-uniform).
//   - PLANAR (stride_x == the element size: CHW) loads a channel's 8 elements of a row as one run of
//     8 / 16 / 32 bytes with the widest loads the three bases and the row stride allow (a wave-uniform
//     test): 16-byte loads (one 8-byte load for U8), else dword loads, else element by element;
//   - the general instance (HWC, any stride_x) loads element by element.
// A lane stores 8 luma samples per row (8 bytes, or 16 in a 10-bit context) and 4 U and 4 V samples
// (4 bytes each, or 8): no byte or short stores, and none wider than the alignment of any output row
// (8-bit chroma rows of an odd number of macroblock columns are 8-byte aligned; a lane's 4 bytes of
// them are dword aligned).
//   - the vector that straddles the source width, and those beyond it, go block by block through the
//     clamped column: only bytes of source elements are read;
//   - a row pair below the source height reads the last pair of the source: its chroma is that block
//     row's, both its luma rows are the last source row's.
// All address arithmetic is 64-bit.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include "jmh_launch.h"
#include "jmh_tensor.h"

#define TNS_WAVES 4

// the 2x2 block of quantised pixels 0 1 / 2 3: its four luma samples and its U and V
__device__ __forceinline__ void tns_block(const jmr_coef &k, const int32_t *r, const int32_t *g, const int32_t *b, int32_t *y0, int32_t *y1,
                                          int32_t *u, int32_t *v) {
    y0[0] = jmr_luma(&k, r[0], g[0], b[0]);
    y0[1] = jmr_luma(&k, r[1], g[1], b[1]);
    y1[0] = jmr_luma(&k, r[2], g[2], b[2]);
    y1[1] = jmr_luma(&k, r[3], g[3], b[3]);
    const int32_t rs = r[0] + r[1] + r[2] + r[3], gs = g[0] + g[1] + g[2] + g[3], bs = b[0] + b[1] + b[2] + b[3];
    *u = jmr_chroma(&k, 0, rs, gs, bs);
    *v = jmr_chroma(&k, 1, rs, gs, bs);
}

// how a PLANAR run of 8 elements may be loaded: the alignment every run of the picture shares
enum { TNS_ELEM = 0, TNS_DWORD = 1, TNS_WIDE = 2 };

// 8 consecutive elements of a channel's row that lie inside the source: their raw bits
template <int DT>
__device__ __forceinline__ void tns_load8(const uint8_t *p, int tier, uint32_t *e) {
    constexpr int ES = jmt_es(DT), NW = 2 * ES;   // the run is 2, 4 or 8 dwords
    if (tier == TNS_ELEM) {
#pragma unroll
        for (int i = 0; i < 8; i++) e[i] = jmt_load(DT, p + i * ES);
        return;
    }
    uint32_t w[NW];
    if (tier == TNS_WIDE) {
        if constexpr (ES == 1) {
            const uint2 a = *reinterpret_cast<const uint2 *>(p);
            w[0] = a.x; w[1] = a.y;
        } else {
#pragma unroll
            for (int i = 0; i < NW / 4; i++) {
                const uint4 a = reinterpret_cast<const uint4 *>(p)[i];
                w[4 * i] = a.x; w[4 * i + 1] = a.y; w[4 * i + 2] = a.z; w[4 * i + 3] = a.w;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; i++) w[i] = reinterpret_cast<const uint32_t *>(p)[i];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if constexpr (ES == 1) e[i] = w[i >> 2] >> 8 * (i & 3) & 0xffu;
        else if constexpr (ES == 2) e[i] = w[i >> 1] >> 16 * (i & 1) & 0xffffu;
        else e[i] = w[i];
    }
}

// one task: luma rows 2 * task and 2 * task + 1 with their chroma rows
template <int DT, bool PLANAR, bool TEN>
__device__ __forceinline__ void tns_task(const TensorArgs &a, int task, int lane, int tier) {
    constexpr int ES = TEN ? 2 : 1;
    const jmr_coef &k = a.k;
    const int W = a.W, w = a.w, CW = W / 2;
    const int32_t M = k.maxv;
    const int sy = jmi_clamp(task, a.h / 2) * 2;                  // the source row pair (the last one below the source)
    const bool below = 2 * task >= a.h;                           // both luma rows are the last source row's
    const uint8_t *row[3][2];
#pragma unroll
    for (int c = 0; c < 3; c++) { row[c][0] = a.chan[c] + jmt_src_off(0, sy, a.sx, a.sy); row[c][1] = row[c][0] + a.sy; }
    uint8_t *oy0 = a.dst + (size_t)(2 * task) * W * ES, *oy1 = oy0 + (size_t)W * ES;
    uint8_t *ou = a.dst + (jmi_dst_off(1, W, a.H) + (size_t)task * CW) * ES;
    uint8_t *ov = a.dst + (jmi_dst_off(2, W, a.H) + (size_t)task * CW) * ES;
    for (int x0 = 8 * lane; x0 < W; x0 += 8 * 64) {
        int32_t y0[8], y1[8], u[4], v[4];
        if (x0 + 8 <= w) {
            int32_t q[3][2][8];
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    uint32_t e[8];
                    if (PLANAR) tns_load8<DT>(row[c][r] + (int64_t)x0 * jmt_es(DT), tier, e);
                    else {
#pragma unroll
                        for (int i = 0; i < 8; i++) e[i] = jmt_load(DT, row[c][r] + (int64_t)(x0 + i) * a.sx);
                    }
#pragma unroll
                    for (int i = 0; i < 8; i++) q[c][r][i] = jmt_quant(DT, e[i], M);
                }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int32_t p[3][4];
#pragma unroll
                for (int c = 0; c < 3; c++) { p[c][0] = q[c][0][2 * j]; p[c][1] = q[c][0][2 * j + 1]; p[c][2] = q[c][1][2 * j]; p[c][3] = q[c][1][2 * j + 1]; }
                tns_block(k, p[0], p[1], p[2], y0 + 2 * j, y1 + 2 * j, &u[j], &v[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int bx = jmi_clamp(x0 / 2 + j, w / 2);      // the clamped block column
                const int64_t o = (int64_t)(2 * bx) * a.sx;
                int32_t p[3][4];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    p[c][0] = jmt_quant(DT, jmt_load(DT, row[c][0] + o), M);
                    p[c][1] = jmt_quant(DT, jmt_load(DT, row[c][0] + o + a.sx), M);
                    p[c][2] = jmt_quant(DT, jmt_load(DT, row[c][1] + o), M);
                    p[c][3] = jmt_quant(DT, jmt_load(DT, row[c][1] + o + a.sx), M);
                }
                tns_block(k, p[0], p[1], p[2], y0 + 2 * j, y1 + 2 * j, &u[j], &v[j]);
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

template <int DT, bool PLANAR>
__global__ __launch_bounds__(64 * TNS_WAVES) void k_ingest_tensor(TensorArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntask = a.H / 2, nblk = (ntask + TNS_WAVES - 1) / TNS_WAVES;
    const int blk = xcd_block(blockIdx.x, nblk);
    const int task = blk * TNS_WAVES + wave;
    if (blk >= nblk || task >= ntask) return;
    // what every run of 8 elements is aligned to: the three bases and the row stride (x0 * es is a multiple of 8 * es)
    const uint64_t low = (uint64_t)(uintptr_t)a.chan[0] | (uint64_t)(uintptr_t)a.chan[1] | (uint64_t)(uintptr_t)a.chan[2] | (uint64_t)a.sy;
    const int tier = !(low & (jmt_es(DT) == 1 ? 7 : 15)) ? TNS_WIDE : !(low & 3) ? TNS_DWORD : TNS_ELEM;
    if (DT == JMT_U8) tns_task<DT, PLANAR, false>(a, task, lane, tier);
    else if (DT == JMT_U16 || a.k.maxv > 255) tns_task<DT, PLANAR, true>(a, task, lane, tier);
    else tns_task<DT, PLANAR, false>(a, task, lane, tier);
}

template <int DT>
static void tns_launch(const TensorArgs &a, dim3 grid, dim3 block, hipStream_t st) {
    if (a.sx == jmt_es(DT)) hipLaunchKernelGGL((k_ingest_tensor<DT, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_ingest_tensor<DT, false>), grid, block, 0, st, a);
}

hipError_t jmh_launch_ingest_tensor(int dtype, const TensorArgs &a, hipStream_t st) {
    const int ntask = a.H / 2;
    const dim3 grid(xcd_grid((ntask + TNS_WAVES - 1) / TNS_WAVES)), block(64 * TNS_WAVES);
    switch (dtype) {
    case JMT_U8: tns_launch<JMT_U8>(a, grid, block, st); break;
    case JMT_U16: tns_launch<JMT_U16>(a, grid, block, st); break;
    case JMT_F16: tns_launch<JMT_F16>(a, grid, block, st); break;
    case JMT_BF16: tns_launch<JMT_BF16>(a, grid, block, st); break;
    case JMT_F32: tns_launch<JMT_F32>(a, grid, block, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
