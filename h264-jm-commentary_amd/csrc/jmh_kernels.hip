// jmh_kernels.hip — gfx950 kernels outside the macroblock wavefront:
//
//  k_interp      UnifiedOneForthPix [J] / H.264 8.4.2.2.1: 16 quarter-pel phase planes of the
//                reference (HBM-bound; one thread per padded integer position, all 16 phases),
//                for the jmh_read_qpel seam (a1).  The macroblock kernels interpolate on the fly
//                (LDS planes in k_mb_analyse, qpel_direct in k_mb_final), so a picture can be
//                searched while its reference is still being reconstructed (pipelining).
//  k_sad_table / k_tq4x4 / k_tq8x8   unit seams, one template each on the sample type: uint8_t, and
//                uint16_t for the High 10 seams (9 / 10-bit luma, config 5; include/jmhip.h
//                jmh_*_u16; JM >= 10 FRExt with imgpel = unsigned short [J]):
//    k_sad_table  SetupFastFullPelSearch's 4x4 BlockSAD table: one thread per (macroblock, window
//                 position); a 4x4 SAD <= 16 * 1023 fits the u16 table at 10 bits as at 8
//    k_tq4x4      dct_luma at qp + QpBdOffsetY on 16-lane groups (the macroblock kernels'
//                 lane_fwd4x4 / lane_quant / lane_inv4x4), reconstruction clipped to 2^bd - 1
//    k_tq8x8      dct_luma8x8 likewise on one wave per block; int32 headroom at 10 bits: the
//                 largest |coefficient| x quant_coef8 is 64 * 1023 * 20972 + (1 << 26) / 3 < 2^31
//                The per-block search seam is k_block_search (jmh_block.hip).
//  k_spiral_positions   unit seam of the searches' spiral decode (jmh_spiral.h, jmhip_spiral.h)
//
// The macroblock wavefront itself is k_mb_analyse (jmh_analyse.hip) + k_mb_final (jmh_final.hip).
#include "jmh_common.h"
#include "jmh_launch.h"
#include "jmh_spiral.h"

// ======================================================================================
//  quarter-pel interpolation (H.264 8.4.2.2.1), spec coordinate clamping
// ======================================================================================
// rpx / hb1 / vh1: jmh_common.h

__global__ __launch_bounds__(256) void k_interp(const uint8_t *__restrict__ ref, int W, int H, uint8_t *__restrict__ qpel, int qstride,
                                                int qplane) {
    int px = blockIdx.x * 64 + (threadIdx.x & 63);
    int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= qstride || py >= H + 2 * QPAD) return;
    int x = px - QPAD, y = py - QPAD;
    int G = rpx(ref, W, H, x, y), Hn = rpx(ref, W, H, x + 1, y), M = rpx(ref, W, H, x, y + 1);
    int b = clip255((hb1(ref, W, H, x, y) + 16) >> 5);
    int hh = clip255((vh1(ref, W, H, x, y) + 16) >> 5);
    int s = clip255((hb1(ref, W, H, x, y + 1) + 16) >> 5);
    int m = clip255((vh1(ref, W, H, x + 1, y) + 16) >> 5);
    int j1 = tap6(vh1(ref, W, H, x - 2, y), vh1(ref, W, H, x - 1, y), vh1(ref, W, H, x, y), vh1(ref, W, H, x + 1, y), vh1(ref, W, H, x + 2, y),
                  vh1(ref, W, H, x + 3, y));
    int j = clip255((j1 + 512) >> 10);
    uint8_t v[16];
    v[0] = G;                  v[1] = (G + b + 1) >> 1;   v[2] = b;                  v[3] = (Hn + b + 1) >> 1;
    v[4] = (G + hh + 1) >> 1;  v[5] = (b + hh + 1) >> 1;  v[6] = (b + j + 1) >> 1;   v[7] = (b + m + 1) >> 1;
    v[8] = hh;                 v[9] = (hh + j + 1) >> 1;  v[10] = j;                 v[11] = (j + m + 1) >> 1;
    v[12] = (M + hh + 1) >> 1; v[13] = (hh + s + 1) >> 1; v[14] = (j + s + 1) >> 1;  v[15] = (m + s + 1) >> 1;
    size_t o = (size_t)py * qstride + px;
#pragma unroll
    for (int ph = 0; ph < 16; ph++) qpel[(size_t)ph * qplane + o] = v[ph];
}

// ======================================================================================
//  unit seams (pel: uint8_t or uint16_t samples; qpb = qp + QpBdOffset, maxv = 2^bd - 1)
// ======================================================================================
template <class pel>
__global__ __launch_bounds__(256) void k_sad_table(const pel *__restrict__ org, const pel *__restrict__ ref, int W, int H, int sr,
                                                   const int32_t *mb_xy, const int32_t *centres, uint16_t *out) {
    int i = blockIdx.y;
    int side = 2 * sr + 1, npos = side * side;
    int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= npos) return;
    int px = 16 * mb_xy[2 * i], py = 16 * mb_xy[2 * i + 1];
    int dx = r % side - sr + centres[2 * i], dy = r / side - sr + centres[2 * i + 1];
    for (int b = 0; b < 16; b++) {
        int ox = (b & 3) * 4, oy = (b >> 2) * 4, sad = 0;
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++)
                sad += abs(org[(py + oy + y) * W + px + ox + x] - ref[iclip(0, H - 1, py + dy + oy + y) * W + iclip(0, W - 1, px + dx + ox + x)]);
        out[((size_t)i * 16 + b) * npos + r] = (uint16_t)sad;
    }
}

// the macroblock kernel's 16-lane dct_luma on independent blocks (16 lanes per block)
template <class pel>
__global__ __launch_bounds__(256) void k_tq4x4(int n, const int16_t *resid, const pel *pred, int qpb, int qsel, int maxv, int16_t *levels,
                                               pel *recon, int32_t *coeff_cost, int32_t *nonzero) {
    const int blk = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    const bool act = blk < n;
    const int bi = act ? blk : 0;
    const int c = lane_fwd4x4(resid[16 * bi + l], l);
    int lev, dq, cc;
    const int q_bits = 15 + qpb / 6;
    unsigned nz = lane_quant(c, l, qpb, q_round(qsel, q_bits), false, lev, dq, cc);
    const int rv = lane_inv4x4(dq, l, pred[16 * bi + l], maxv);
    if (act) {
        levels[16 * blk + l] = (int16_t)lev;
        recon[16 * blk + l] = (pel)rv;
        if (l == 0) { coeff_cost[blk] = cc; nonzero[blk] = nz != 0; }
    }
}

// the macroblock kernels' one-wave dct_luma8x8 on independent blocks (4 blocks per workgroup)
template <class pel>
__global__ __launch_bounds__(256) void k_tq8x8(int n, const int16_t *resid, const pel *pred, int qpb, int qsel, int maxv, int16_t *levels,
                                               pel *recon, int32_t *coeff_cost, int32_t *nonzero) {
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (blk >= n) return;                        // whole waves only: no workgroup barrier below
    const int q_bits = 16 + qpb / 6;
    const int c = wave_fwd8x8(resid[64 * blk + l], l);
    int lev, dq, cc;
    const unsigned long long nz = wave_quant8(c, l, qpb, q_round(qsel, q_bits), lev, dq, cc);
    recon[64 * blk + l] = (pel)wave_inv8x8(dq, l, pred[64 * blk + l], maxv);
    levels[64 * blk + l] = (int16_t)lev;
    if (l == 0) { coeff_cost[blk] = cc; nonzero[blk] = nz != 0; }
}

// unit seam of the searches' spiral decode (jmhip_spiral.h): jms_decode_dev, the function
// subpel_wave calls, on every index n < count; out_xy holds 2 * count words
__global__ __launch_bounds__(256) void k_spiral_positions(int count, int32_t *__restrict__ out_xy) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= count) return;
    int x, y;
    jms_decode_dev(n, x, y);
    out_xy[2 * n] = x;
    out_xy[2 * n + 1] = y;
}

// ---- launchers (host side, same translation unit) --------------------------------------
hipError_t jmh_launch_spiral_positions(int count, int32_t *out_xy, hipStream_t st) {
    hipLaunchKernelGGL(k_spiral_positions, dim3((count + 255) / 256), dim3(256), 0, st, count, out_xy);
    return hipGetLastError();
}
hipError_t jmh_launch_interp(const uint8_t *ref, int W, int H, uint8_t *qpel, int qstride, int qplane, hipStream_t st) {
    dim3 grid((qstride + 63) / 64, (H + 2 * QPAD + 3) / 4);
    hipLaunchKernelGGL(k_interp, grid, dim3(256), 0, st, ref, W, H, qpel, qstride, qplane);
    return hipGetLastError();
}
template <class pel>
hipError_t jmh_launch_sad_table(const pel *org, const pel *ref, int W, int H, int sr, int n_mb, const int32_t *mb_xy, const int32_t *centres,
                                uint16_t *out, hipStream_t st) {
    int side = 2 * sr + 1, npos = side * side;
    hipLaunchKernelGGL(k_sad_table<pel>, dim3((npos + 255) / 256, n_mb), dim3(256), 0, st, org, ref, W, H, sr, mb_xy, centres, out);
    return hipGetLastError();
}
template <class pel>
hipError_t jmh_launch_tq4x4(int n, const int16_t *resid, const pel *pred, int qpb, int qsel, int maxv, int16_t *levels, pel *recon,
                            int32_t *cc, int32_t *nz, hipStream_t st) {
    hipLaunchKernelGGL(k_tq4x4<pel>, dim3((n + 15) / 16), dim3(256), 0, st, n, resid, pred, qpb, qsel, maxv, levels, recon, cc, nz);
    return hipGetLastError();
}
template <class pel>
hipError_t jmh_launch_tq8x8(int n, const int16_t *resid, const pel *pred, int qpb, int qsel, int maxv, int16_t *levels, pel *recon,
                            int32_t *cc, int32_t *nz, hipStream_t st) {
    hipLaunchKernelGGL(k_tq8x8<pel>, dim3((n + 3) / 4), dim3(256), 0, st, n, resid, pred, qpb, qsel, maxv, levels, recon, cc, nz);
    return hipGetLastError();
}
#define JMH_SEAMS(pel)                                                                                                                  \
    template hipError_t jmh_launch_sad_table<pel>(const pel *, const pel *, int, int, int, int, const int32_t *, const int32_t *, uint16_t *, \
                                                  hipStream_t);                                                                         \
    template hipError_t jmh_launch_tq4x4<pel>(int, const int16_t *, const pel *, int, int, int, int16_t *, pel *, int32_t *, int32_t *, hipStream_t); \
    template hipError_t jmh_launch_tq8x8<pel>(int, const int16_t *, const pel *, int, int, int, int16_t *, pel *, int32_t *, int32_t *, hipStream_t);
JMH_SEAMS(uint8_t)
JMH_SEAMS(uint16_t)
#undef JMH_SEAMS
