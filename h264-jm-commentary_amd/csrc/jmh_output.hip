// jmh_output.hip — k_pull_picture and k_pull_tensor: the top-left w x h crop of a packed 4:2:0
// picture of the coded size (a ring entry's reconstruction or deblocked picture) written into device
// memory of the caller (include/jmhip_output.h): YUV planes, packed RGB dwords or an
// RGB tensor.  k_ingest_tensor turned round.
//
// One launch per picture.  A task is a pair of luma rows with their chroma row (h / 2 tasks), in
// xcd_block order; a wave takes whole tasks, a lane 8 pixels x 2 rows per step, so that the U and V of
// a 2x2 block are loaded once: 8 bytes of each luma row and 4 of each chroma row in an 8-bit context,
// 16 and 8 in a 16-bit one, each load as wide as the lane's samples and aligned to its size (luma rows
// are multiples of 16 samples; 8-bit chroma rows of an odd number of macroblock columns are 8-byte
// aligned, a lane's 4 bytes of them dword aligned).  x0 < w <= W, so every load lies inside the source.
// What a sample becomes is jmh_output.h's (jmout_chroma_terms, jmout_rgb_terms, jmout_dequant,
// jmout_pack, jmout_yuv_value); the coefficients arrive in the kernel arguments, wave-uniform.
//   - A run of consecutive elements (a plane's row, a channel's row of a planar tensor, the dwords of
//     an RGB row) is stored with the widest stores the bases and the row strides allow, a wave-uniform
//     test: 16-byte stores (or the run's size where that is less), else dwords, else element by element.
//   - Interleaved and strided tensors (HWC, any stride_x) store element by element: the fourth
//     channel of HWC4 is not the kernel's to write.  BGRA / RGBA dwords define all four bytes.
//   - The vector that straddles w goes element by element up to w; nothing is stored beyond the crop.
// All address arithmetic is 64-bit.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include "jmh_launch.h"
#include "jmh_output.h"

#define OUT_WAVES 4

enum { OUT_ELEM = 0, OUT_DWORD = 1, OUT_WIDE = 2 };

// how runs of `bytes` bytes (a power of two, every run at a multiple of it from a row's start) may be
// stored, given the OR of the bases and row strides they start from
__device__ __forceinline__ int out_tier(uint64_t low, int bytes) {
    const int al = bytes < 16 ? bytes : 16;
    return !(low & (uint64_t)(al - 1)) ? OUT_WIDE : !(low & 3) ? OUT_DWORD : OUT_ELEM;
}

template <int ES>
__device__ __forceinline__ void out_store_elem(uint8_t *p, uint32_t v) {
    if constexpr (ES == 1) *p = (uint8_t)v;
    else if constexpr (ES == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    else *reinterpret_cast<uint32_t *>(p) = v;
}

// N (4 or 8) consecutive elements of ES bytes at p, the first n of them inside the crop
template <int ES, int N>
__device__ __forceinline__ void out_store_run(uint8_t *p, const uint32_t *e, int n, int tier) {
    constexpr int NW = N * ES / 4;   // dwords of the run: 1, 2, 4 or 8
    if (n < N || tier == OUT_ELEM) {
#pragma unroll
        for (int i = 0; i < N; i++)
            if (i < n) out_store_elem<ES>(p + i * ES, e[i]);
        return;
    }
    uint32_t w[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) {
        if constexpr (ES == 1) w[i] = e[4 * i] | e[4 * i + 1] << 8 | e[4 * i + 2] << 16 | e[4 * i + 3] << 24;
        else if constexpr (ES == 2) w[i] = e[2 * i] | e[2 * i + 1] << 16;
        else w[i] = e[i];
    }
    if (tier == OUT_WIDE) {
        if constexpr (NW == 1) *reinterpret_cast<uint32_t *>(p) = w[0];
        else if constexpr (NW == 2) *reinterpret_cast<uint2 *>(p) = make_uint2(w[0], w[1]);
        else {
#pragma unroll
            for (int i = 0; i < NW / 4; i++) reinterpret_cast<uint4 *>(p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; i++) reinterpret_cast<uint32_t *>(p)[i] = w[i];
    }
}

// the lane's samples of a task: 8 luma samples of both rows and the 4 U and 4 V of their blocks,
// from column x0 (a multiple of 8) of the packed source; SES: bytes of a source sample
template <int SES>
__device__ __forceinline__ void out_load(const OutArgs &a, int task, int x0, uint32_t (*y)[8], uint32_t *u, uint32_t *v) {
    const int W = a.W, CW = W / 2;
    const uint8_t *py = a.src + ((size_t)(2 * task) * W + x0) * SES;
    const uint8_t *pu = a.src + (jmi_dst_off(1, W, a.H) + (size_t)task * CW + x0 / 2) * SES;
    const uint8_t *pv = a.src + (jmi_dst_off(2, W, a.H) + (size_t)task * CW + x0 / 2) * SES;
    if constexpr (SES == 1) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint2 t = *reinterpret_cast<const uint2 *>(py + (size_t)r * W);
#pragma unroll
            for (int i = 0; i < 4; i++) { y[r][i] = t.x >> 8 * i & 0xffu; y[r][4 + i] = t.y >> 8 * i & 0xffu; }
        }
        const uint32_t tu = *reinterpret_cast<const uint32_t *>(pu), tv = *reinterpret_cast<const uint32_t *>(pv);
#pragma unroll
        for (int i = 0; i < 4; i++) { u[i] = tu >> 8 * i & 0xffu; v[i] = tv >> 8 * i & 0xffu; }
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint4 t = *reinterpret_cast<const uint4 *>(py + (size_t)r * W * 2);
            const uint32_t d[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int i = 0; i < 4; i++) { y[r][2 * i] = d[i] & 0xffffu; y[r][2 * i + 1] = d[i] >> 16; }
        }
        const uint2 tu = *reinterpret_cast<const uint2 *>(pu), tv = *reinterpret_cast<const uint2 *>(pv);
        u[0] = tu.x & 0xffffu; u[1] = tu.x >> 16; u[2] = tu.y & 0xffffu; u[3] = tu.y >> 16;
        v[0] = tv.x & 0xffffu; v[1] = tv.x >> 16; v[2] = tv.y & 0xffffu; v[3] = tv.y >> 16;
    }
}

// R, G, B of the lane's 8 x 2 pixels
__device__ __forceinline__ void out_convert(const jmout_coef &k, const uint32_t (*y)[8], const uint32_t *u, const uint32_t *v, int32_t (*rgb)[8][3]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int32_t t[3];
        jmout_chroma_terms(&k, (int32_t)u[j], (int32_t)v[j], t);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            jmout_rgb_terms(&k, (int32_t)y[r][2 * j], t, rgb[r][2 * j]);
            jmout_rgb_terms(&k, (int32_t)y[r][2 * j + 1], t, rgb[r][2 * j + 1]);
        }
    }
}

// the task of this wave, or -1
__device__ __forceinline__ int out_task(const OutArgs &a) {
    const int ntask = a.h / 2, nblk = (ntask + OUT_WAVES - 1) / OUT_WAVES;
    const int blk = xcd_block(blockIdx.x, nblk);
    const int task = blk * OUT_WAVES + (threadIdx.x >> 6);
    return blk >= nblk || task >= ntask ? -1 : task;
}

// ---- a picture: FMT one of the layouts of jmhip_input.h / jmhip_rgb.h (flags stripped) ----
template <int FMT>
__global__ __launch_bounds__(64 * OUT_WAVES) void k_pull_picture(OutArgs a) {
    constexpr bool RGB = FMT >= JMR_BGRA8;
    constexpr int SES = RGB ? (jmr_ten(FMT) ? 2 : 1) : (jmi_wide(FMT) ? 2 : 1);   // the context's sample: the depth rule
    const int task = out_task(a), lane = threadIdx.x & 63;
    if (task < 0) return;
    const int w = a.w;
    if constexpr (RGB) {
        const int tier = out_tier((uint64_t)(uintptr_t)a.dst[0] | (uint64_t)a.stride[0], 32);
        uint8_t *row0 = a.dst[0] + (int64_t)(2 * task) * a.stride[0];
        for (int x0 = 8 * lane; x0 < w; x0 += 8 * 64) {
            uint32_t y[2][8], u[4], v[4];
            int32_t rgb[2][8][3];
            out_load<SES>(a, task, x0, y, u, v);
            out_convert(a.k, y, u, v, rgb);
            const int n = w - x0 < 8 ? w - x0 : 8;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                uint32_t e[8];
#pragma unroll
                for (int i = 0; i < 8; i++) e[i] = jmout_pack(FMT, rgb[r][i]);
                out_store_run<4, 8>(row0 + (int64_t)r * a.stride[0] + (int64_t)4 * x0, e, n, tier);
            }
        }
    } else {
        constexpr int ES = SES;
        constexpr bool SEMI = jmi_semi(FMT);
        const int ty = out_tier((uint64_t)(uintptr_t)a.dst[0] | (uint64_t)a.stride[0], 8 * ES);
        const int tc = SEMI ? out_tier((uint64_t)(uintptr_t)a.dst[1] | (uint64_t)a.stride[1], 8 * ES)
                            : out_tier((uint64_t)(uintptr_t)a.dst[1] | (uint64_t)(uintptr_t)a.dst[2] | (uint64_t)a.stride[1] | (uint64_t)a.stride[2], 4 * ES);
        uint8_t *oy = a.dst[0] + (int64_t)(2 * task) * a.stride[0];
        uint8_t *ou = a.dst[1] + (int64_t)task * a.stride[1];
        uint8_t *ov = SEMI ? nullptr : a.dst[2] + (int64_t)task * a.stride[2];
        for (int x0 = 8 * lane; x0 < w; x0 += 8 * 64) {
            uint32_t y[2][8], u[4], v[4];
            out_load<SES>(a, task, x0, y, u, v);
            const int n = w - x0 < 8 ? w - x0 : 8;
#pragma unroll
            for (int r = 0; r < 2; r++) {
#pragma unroll
                for (int i = 0; i < 8; i++) y[r][i] = jmout_yuv_value(FMT, y[r][i]);
                out_store_run<ES, 8>(oy + (int64_t)r * a.stride[0] + (int64_t)x0 * ES, y[r], n, ty);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) { u[i] = jmout_yuv_value(FMT, u[i]); v[i] = jmout_yuv_value(FMT, v[i]); }
            if constexpr (SEMI) {
                uint32_t e[8];
#pragma unroll
                for (int i = 0; i < 4; i++) { e[2 * i] = u[i]; e[2 * i + 1] = v[i]; }
                out_store_run<ES, 8>(ou + (int64_t)x0 * ES, e, n, tc);
            } else {
                out_store_run<ES, 4>(ou + (int64_t)(x0 / 2) * ES, u, n / 2, tc);
                out_store_run<ES, 4>(ov + (int64_t)(x0 / 2) * ES, v, n / 2, tc);
            }
        }
    }
}

// ---- a tensor: DT its element type, PLANAR: stride_x == the element size ----
template <int DT, bool PLANAR, int SES>
__device__ __forceinline__ void out_tensor_task(const OutArgs &a, int task, int lane) {
    constexpr int ES = jmt_es(DT);
    const int w = a.w;
    const int32_t M = a.k.maxv;
    const int64_t sx = a.stride[0], sy = a.stride[1];
    const int tier = out_tier((uint64_t)(uintptr_t)a.dst[0] | (uint64_t)(uintptr_t)a.dst[1] | (uint64_t)(uintptr_t)a.dst[2] | (uint64_t)sy, 8 * ES);
    for (int x0 = 8 * lane; x0 < w; x0 += 8 * 64) {
        uint32_t y[2][8], u[4], v[4];
        int32_t rgb[2][8][3];
        out_load<SES>(a, task, x0, y, u, v);
        out_convert(a.k, y, u, v, rgb);
        const int n = w - x0 < 8 ? w - x0 : 8;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int r = 0; r < 2; r++) {
                uint8_t *p = a.dst[c] + jmt_src_off(x0, 2 * task + r, sx, sy);
                uint32_t e[8];
#pragma unroll
                for (int i = 0; i < 8; i++) e[i] = jmout_dequant(DT, rgb[r][i][c], M);
                if constexpr (PLANAR) out_store_run<ES, 8>(p, e, n, tier);
                else {
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        if (i < n) out_store_elem<ES>(p + (int64_t)i * sx, e[i]);
                }
            }
    }
}

template <int DT, bool PLANAR>
__global__ __launch_bounds__(64 * OUT_WAVES) void k_pull_tensor(OutArgs a) {
    const int task = out_task(a), lane = threadIdx.x & 63;
    if (task < 0) return;
    // U8 lives in 8-bit contexts and U16 in 10-bit ones; a float instance serves both (wave-uniform)
    if (DT == JMT_U8) out_tensor_task<DT, PLANAR, 1>(a, task, lane);
    else if (DT == JMT_U16 || a.k.maxv > 255) out_tensor_task<DT, PLANAR, 2>(a, task, lane);
    else out_tensor_task<DT, PLANAR, 1>(a, task, lane);
}

static dim3 out_grid(const OutArgs &a) { return dim3(xcd_grid((a.h / 2 + OUT_WAVES - 1) / OUT_WAVES)); }

hipError_t jmh_launch_pull_picture(int format, const OutArgs &a, hipStream_t st) {
    const dim3 grid = out_grid(a), block(64 * OUT_WAVES);
    switch (jmr_is_rgb(format) ? jmr_layout(format) : format) {
    case JMI_I420: hipLaunchKernelGGL((k_pull_picture<JMI_I420>), grid, block, 0, st, a); break;
    case JMI_NV12: hipLaunchKernelGGL((k_pull_picture<JMI_NV12>), grid, block, 0, st, a); break;
    case JMI_I010: hipLaunchKernelGGL((k_pull_picture<JMI_I010>), grid, block, 0, st, a); break;
    case JMI_P010: hipLaunchKernelGGL((k_pull_picture<JMI_P010>), grid, block, 0, st, a); break;
    case JMR_BGRA8: hipLaunchKernelGGL((k_pull_picture<JMR_BGRA8>), grid, block, 0, st, a); break;
    case JMR_RGBA8: hipLaunchKernelGGL((k_pull_picture<JMR_RGBA8>), grid, block, 0, st, a); break;
    case JMR_RGB10A2: hipLaunchKernelGGL((k_pull_picture<JMR_RGB10A2>), grid, block, 0, st, a); break;
    case JMR_BGR10A2: hipLaunchKernelGGL((k_pull_picture<JMR_BGR10A2>), grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int DT>
static void out_launch_tensor(const OutArgs &a, dim3 grid, dim3 block, hipStream_t st) {
    if (a.stride[0] == jmt_es(DT)) hipLaunchKernelGGL((k_pull_tensor<DT, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_pull_tensor<DT, false>), grid, block, 0, st, a);
}

hipError_t jmh_launch_pull_tensor(int dtype, const OutArgs &a, hipStream_t st) {
    const dim3 grid = out_grid(a), block(64 * OUT_WAVES);
    switch (dtype) {
    case JMT_U8: out_launch_tensor<JMT_U8>(a, grid, block, st); break;
    case JMT_U16: out_launch_tensor<JMT_U16>(a, grid, block, st); break;
    case JMT_F16: out_launch_tensor<JMT_F16>(a, grid, block, st); break;
    case JMT_BF16: out_launch_tensor<JMT_BF16>(a, grid, block, st); break;
    case JMT_F32: out_launch_tensor<JMT_F32>(a, grid, block, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
