// jmh_spiral.h — JM's spiral order of the full-pel search positions (Init_Motion_Search_Module [J],
// docs/JM_SEMANTICS.md item 5), stated once: index -> position and position -> index.  One text
// that the host (ordtab_fill of jmhip_abi.hip), the kernels (subpel_wave of jmh_analyse.hip) and the
// host harness (tests/harness/spiral_check.c) compile.  C99 and HIP.
//
// Index 0 is (0, 0).  Ring l >= 1 (the positions with max(|x|, |y|) == l) starts at index
// (2l - 1)^2 and holds, in this order,
//   2 (2l - 1) top / bottom entries: x = -l+1 .. l-1, each as the pair (x, -l), (x, +l);
//   2 (2l + 1) left / right entries: y = -l .. l,     each as the pair (-l, y), (+l, y).
// The order does not depend on the search range: a range sr uses indices 0 .. (2 sr + 1)^2 - 1.
#ifndef JMH_SPIRAL_H
#define JMH_SPIRAL_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JMS_FN __host__ __device__ static __forceinline__
#else
#define JMS_FN static inline
#endif

// position -> index
JMS_FN int jms_index(int x, int y) {
    const int ax = x < 0 ? -x : x, ay = y < 0 ? -y : y, l = ax > ay ? ax : ay;
    if (l == 0) return 0;
    const int base = (2 * l - 1) * (2 * l - 1);
    if (ay == l && ax < l) return base + 2 * (x + l - 1) + (y > 0);
    return base + 2 * (2 * l - 1) + 2 * (y + l) + (x > 0);
}

// the ring of index n >= 0 from a candidate that is right or off by one either way: the ring is
// the l with (2l - 1)^2 <= n < (2l + 1)^2 (l == 0: n == 0).  Integers only, so what produced the
// candidate (a square root of any rounding) does not matter
JMS_FN int jms_ring_fix(int n, int l) {
    if ((2 * l + 1) * (2 * l + 1) <= n) return l + 1;
    if (l > 0 && (2 * l - 1) * (2 * l - 1) > n) return l - 1;
    return l;
}

// the ring of index n >= 0, integers only (the host's; the kernels take a candidate from the
// device's square root instruction, jms_decode_dev)
JMS_FN int jms_ring(int n) {
    int l = 0;
    while ((2 * l + 1) * (2 * l + 1) <= n) l++;
    return l;
}

// index n of ring l -> position.  Ring 0 needs no case of its own: base = 1, t = -1, m = -2, so
// the side branch runs with u = 1 and gives y = (1 >> 1) - 0 = 0, x = +-0
JMS_FN void jms_ring_pos(int n, int l, int *x, int *y) {
    const int t = n - (2 * l - 1) * (2 * l - 1), m = 2 * (2 * l - 1);
    if (t < m) { *x = (t >> 1) - l + 1; *y = (t & 1) ? l : -l; }
    else { const int u = t - m; *y = (u >> 1) - l; *x = (u & 1) ? l : -l; }
}

// index -> position
JMS_FN void jms_decode(int n, int *x, int *y) { jms_ring_pos(n, jms_ring(n), x, y); }

// The per-context table d_ordtab for search range sr (2 sr + 1 = side), three parts:
//   [((npk + 1) / 2) * nta]  order keys of the FFS analysis threads: thread t of nta owns window
//                   column t % side, rows (t / side) * npk .. + npk - 1; key = spiral index + 1 (0 is
//                   the (0,0) pre-check, set per MB in the kernel), 0xFFFF outside the window; packed
//                   pairs [k / 2][t], the even slot in the low half
//   [side * side]   spiral index -> position, x & 0xFFFF | y << 16
//   [side * side]   raster position (y + sr) * side + x + sr -> spiral index (the RDO FFS table's
//                   tie order, jmh_epzs.h ffs_table_min)
// tab: jms_ordtab_len words, zeroed
JMS_FN size_t jms_ordtab_len(int sr, int npk, int nta) {
    const size_t side = 2 * (size_t)sr + 1;
    return (size_t)((npk + 1) / 2) * nta + 2 * side * side;
}
JMS_FN void jms_ordtab_fill(uint32_t *tab, int sr, int npk, int nta) {
    const int side = 2 * sr + 1, nstrips = (side + npk - 1) / npk;
    const size_t spos = (size_t)((npk + 1) / 2) * nta;
    for (int n = 0; n < side * side; n++) {
        int x, y;
        jms_decode(n, &x, &y);
        tab[spos + n] = ((uint32_t)x & 0xFFFFu) | (uint32_t)y << 16;
        tab[spos + (size_t)side * side + (size_t)(y + sr) * side + x + sr] = (uint32_t)n;
    }
    for (int t = 0; t < nta; t++) {
        const int sact = t < side * nstrips;
        const int dx = sact ? t % side : 0, dy0 = sact ? (t / side) * npk : 0;
        for (int k = 0; k < npk; k++) {
            const int dy = dy0 + k;
            const uint32_t o = (!sact || dy >= side) ? 0xFFFFu : (uint32_t)(jms_index(dx - sr, dy - sr) + 1);
            tab[(size_t)(k >> 1) * nta + t] |= o << (16 * (k & 1));
        }
    }
}

#if defined(__HIPCC__)
// index -> position on the device: the ring candidate (floor(sqrt n) + 1) / 2 from one raw
// v_sqrt_f32 (no IEEE fix-up sequence, no libm), repaired by jms_ring_fix.  For n < 2^24 the
// conversion is exact and the instruction's error of about one ulp moves floor(sqrt n) by at most
// one, hence the candidate by at most one
__device__ __forceinline__ int jms_ring_candidate_dev(int n) {
    return ((int)__builtin_amdgcn_sqrtf((float)n) + 1) >> 1;
}
__device__ __forceinline__ void jms_decode_dev(int n, int &x, int &y) {
    jms_ring_pos(n, jms_ring_fix(n, jms_ring_candidate_dev(n)), &x, &y);
}
#endif

#endif  // JMH_SPIRAL_H
