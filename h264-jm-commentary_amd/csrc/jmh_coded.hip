// jmh_coded.hip — k_plane_ssd: the distortion of a coded picture (include/jmhip_coded.h, DESIGN.md
// §5.4): the sum of squared differences between the source as pushed and the picture's output, per
// plane, over the crop.  It runs behind the slice writer on the writer's stream, so the picture
// itself never crosses PCIe for the PSNR.
//
// One launch for the three planes (blockIdx.y).  A wave takes whole rows; a lane loads one dword of
// each picture per step (four u8 or two u16 samples: rows are dword aligned, the coded width is a
// multiple of 16), lanes below the row's remainder take the scalar tail.  Every dword's sum (four
// squares of at most 255^2, or two of at most 65535^2 taken in 64 bits: a 10-bit square is up to
// 1,046,529) is added to a 64-bit lane total at once, so no 32-bit partial is ever carried from one
// dword to the next.  The wave total comes from a DPP reduction of three 26-bit limbs
// (64 lanes add 6 bits: each limb's sum fits 32 bits), then one 64-bit atomic add per wave.  Integer
// sums do not depend on the order: the result is exact.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "jmh_coded.h"

#define SSD_WAVES 4

// sum over the wave of a value below 2^26: row_shr 1, 2, 4, 8 leave each row's sum in its lane 15
// (lanes shifted in from outside the row read 0), the four row sums are read with v_readlane
__device__ __forceinline__ uint32_t ssd_wave_sum26(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 15) + (uint32_t)__builtin_amdgcn_readlane((int)v, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 47) + (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ uint32_t ssd_dword(uint32_t x, uint32_t y, uint8_t) {
    uint32_t s = 0;
    for (int i = 0; i < 4; i++) {
        const int d = (int)((x >> (8 * i)) & 255u) - (int)((y >> (8 * i)) & 255u);
        s += (uint32_t)(d * d);
    }
    return s;
}
// two u16 samples: each square is below 2^32, their sum may not be
__device__ __forceinline__ uint64_t ssd_dword(uint32_t x, uint32_t y, uint16_t) {
    const int64_t d0 = (int64_t)(x & 0xffffu) - (int64_t)(y & 0xffffu), d1 = (int64_t)(x >> 16) - (int64_t)(y >> 16);
    return (uint64_t)(d0 * d0) + (uint64_t)(d1 * d1);
}

template <class T>
__global__ __launch_bounds__(64 * SSD_WAVES) void k_plane_ssd(const T *a, const T *b, int W, int H, int crop_w, int crop_h,
                                                              unsigned long long *ssd) {
    constexpr int PER = 4 / (int)sizeof(T);                      // samples per dword
    const int pl = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pw = pl ? W >> 1 : W, cw = pl ? crop_w >> 1 : crop_w, ch = pl ? crop_h >> 1 : crop_h;
    const size_t base = pl == 0 ? 0 : (size_t)W * H + (pl == 2 ? (size_t)(W >> 1) * (H >> 1) : 0);
    const T *pa = a + base, *pb = b + base;
    const int nd = cw / PER, tail = cw - nd * PER;
    uint64_t acc = 0;
    for (int r = blockIdx.x * SSD_WAVES + wave; r < ch; r += gridDim.x * SSD_WAVES) {
        const T *ra = pa + (size_t)r * pw, *rb = pb + (size_t)r * pw;
        const uint32_t *da = (const uint32_t *)ra, *db = (const uint32_t *)rb;
        for (int k = lane; k < nd; k += 64) acc += ssd_dword(da[k], db[k], T());
        if (lane < tail) {
            const int64_t d = (int64_t)ra[nd * PER + lane] - (int64_t)rb[nd * PER + lane];
            acc += (uint64_t)(d * d);
        }
    }
    const uint32_t m = (1u << 26) - 1;
    const uint64_t s0 = ssd_wave_sum26((uint32_t)acc & m), s1 = ssd_wave_sum26((uint32_t)(acc >> 26) & m),
                   s2 = ssd_wave_sum26((uint32_t)(acc >> 52));
    const uint64_t total = s0 + (s1 << 26) + (s2 << 52);
    if (lane == 0 && total) atomicAdd(&ssd[pl], (unsigned long long)total);
}

int jmh_plane_ssd(hipStream_t st, const uint8_t *a, const uint8_t *b, int W, int H, int crop_w, int crop_h, int ps, uint64_t *ssd) {
    if (crop_w <= 0 || crop_h <= 0 || crop_w > W || crop_h > H) return JMH_E_INVALID_ARG;
    const int gx = (crop_h + SSD_WAVES - 1) / SSD_WAVES;         // a wave per luma row, at most 256 workgroups per plane
    const dim3 grid(gx < 256 ? gx : 256, 3), block(64 * SSD_WAVES);
    if (ps == 1) hipLaunchKernelGGL(k_plane_ssd<uint8_t>, grid, block, 0, st, a, b, W, H, crop_w, crop_h, (unsigned long long *)ssd);
    else hipLaunchKernelGGL(k_plane_ssd<uint16_t>, grid, block, 0, st, (const uint16_t *)a, (const uint16_t *)b, W, H, crop_w, crop_h,
                            (unsigned long long *)ssd);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fprintf(stderr, "jmhip: k_plane_ssd launch failed: %s\n", hipGetErrorString(e));
        return JMH_E_HIP;
    }
    return JMH_OK;
}
