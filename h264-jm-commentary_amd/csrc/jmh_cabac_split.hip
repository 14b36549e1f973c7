// jmh_cabac_split.hip — one CABAC slice coded on many waves (include/jmhip_cabac_split.h, DESIGN.md
// §5.5): the shared core jmh_cabac_split.h in ten launches that stand in k_cabac_code's place, between
// k_cabac_bins and k_cabac_where, on the writer's stream.  Chunks are L records, spans jms_span(L).
//
//   k_split_plan     one workgroup: every slice's chunks and map slots (a span that has a successor
//                    holds one), their scans, the slice of every chunk and slot.
//   k_split_maps     one wave per slot: the span's 288 maps on 128 values in LDS (36,864 bytes; lane l
//                    holds the values 2 l and 2 l + 1 of every map), then to the slot.
//   k_split_ctx      one workgroup per slice, a thread per context: the slots' maps composed in order;
//                    leaves every later span's entry contexts (288 bytes per slot).
//   k_split_resolve  one wave per span: the contexts in registers as in k_cabac_code; every regular
//                    record's context index replaced, in place, by the context's value at that bin.
//   k_split_range    one wave per chunk that has a successor: the 256 entry ranges, four per lane,
//                    through the chunk's records (wave-uniform); leaves exit range and shifts of each.
//   k_split_along    one wave per slice: the tables composed in order, eight rows in flight: every
//                    chunk's entry range and the shifts before it.
//   k_split_code     one wave per chunk: jmc_enc from low = 0 on the slice's byte grid; own bytes staged
//                    in LDS and stored into the chunk's region of the slice's scratch, the tail kept.
//   k_split_sum      a thread per chunk: earlier tails into the region's first bytes, the region's
//                    carry function.
//   k_split_carry    one wave per slice: the carry into every region, from the slice's end, 64 chunks
//                    per fetch.
//   k_split_apply    a thread per chunk: the carry through the region's trailing 0xff bytes; the stop bit.
//
// k_cabac_code's discipline holds: the overflow word is read first by every launch, grids are sized
// from capacities and every wave compares its index with the counted totals, every loop is bounded
// by a counted size, no workgroup waits on another, and a bin's dependent chain touches no memory but
// the prefetched records (k_split_maps: and the LDS maps).  Region bytes are stored bytewise: regions
// of neighbouring chunks share dwords.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

struct jmc_enc;
__host__ __device__ static inline void sp_emit(jmc_enc *e, uint32_t b);
__host__ __device__ static inline uint32_t sp_lps_get(const jmc_enc *e, int s, uint32_t q);
#define JMC_EMIT(e, b) sp_emit((e), (b))
// k_split_code: rangeTabLPS[s][0..3] packed in lane s of tl (as k_cabac_code); the last three bytes of
// a chunk that has a successor collect in tailv
#define JMC_ENC_EXTRA uint32_t tl, tailv;
#define JMC_CTX_GET(e, i) ((uint32_t)(i))
#define JMC_CTX_SET(e, i, v) ((void)(v))
#define JMC_LPS_GET(e, s, q) sp_lps_get((e), (s), (q))
#define JMC_TLPS_GET(e, s) 0
#include "jmh_cabac_split.h"
#include "jmh_cabac.h"

#define SP_STAGE 256                                 // staged bytes of a chunk: four per lane
#define SP_ROWS 8                                    // range tables in flight in k_split_along

// a byte of a chunk: below cap (the region's length) into the LDS stage, and the full stage into the
// region; at and above cap into the tail
__host__ __device__ static inline void sp_emit(jmc_enc *e, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (e->nbytes >= e->cap) { e->tailv = e->tailv << 8 | (b & 0xffu); e->nbytes++; return; }
    e->out[e->nbytes & (SP_STAGE - 1)] = (uint8_t)b;
    e->nbytes++;
    if ((e->nbytes & (SP_STAGE - 1)) == 0)
        for (int i = 0; i < 4; i++) ((uint8_t *)e->spill)[e->nbytes - SP_STAGE + 64 * i + threadIdx.x] = e->out[64 * i + threadIdx.x];
#else
    jmc_emit_plain(e, b);
#endif
}
__host__ __device__ static inline uint32_t sp_lps_get(const jmc_enc *e, int s, uint32_t q) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((uint32_t)__builtin_amdgcn_readlane((int)e->tl, __builtin_amdgcn_readfirstlane(s)) >> (8 * q)) & 0xffu;
#else
    return e->lps[s * 4 + q];
#endif
}

struct SpArgs {
    const jmh_cabac_slice_desc *sl;
    int nslices;
    const uint64_t *mb_off, *sl_soff;    // the writer's: record offset of every macroblock, scratch offset of every slice
    uint16_t *rec;                       // the records; resolved in place
    uint8_t *scratch;
    int64_t *sl_bytes;
    const uint32_t *ovf;                 // may be null
    uint32_t L, span;
    uint64_t chunks_cap, slots_cap;
    uint64_t *sl_coff, *sl_poff;         // [nslices + 1]: first chunk / first slot of every slice
    uint32_t *ch_slice, *sp_slice;       // the slice of every chunk / slot
    uint64_t *tot;                       // chunks, slots, the most chunks of one slice
    uint8_t *maps, *centry;              // per slot: JMS_MAP_BYTES; the entry contexts of the span behind it
    uint32_t *rmap;                      // per chunk: JMS_NRANGE entries
    uint64_t *ch_T;                      // per chunk: shifts before it
    uint32_t *ch_range, *tail, *cin, *sl_stop;
    uint2 *fn;                           // per chunk: q, theta
};

__device__ __forceinline__ uint64_t sp_slice_bins(const SpArgs &a, int si, uint64_t *r0) {
    const jmh_cabac_slice_desc d = a.sl[si];
    *r0 = a.mb_off[d.first_mb];
    return a.mb_off[d.first_mb + d.n_mb] - *r0;
}

// exclusive scan over the 1024 threads of the workgroup (as k_cabac_scan's)
__device__ uint64_t sp_block_scan(uint64_t v, uint64_t *buf, uint64_t *total) {
    const int t = threadIdx.x;
    int cur = 0;
    buf[t] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint64_t x = buf[cur * 1024 + t] + (t >= o ? buf[cur * 1024 + t - o] : 0);
        buf[(cur ^ 1) * 1024 + t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const uint64_t incl = buf[cur * 1024 + t];
    *total = buf[cur * 1024 + 1023];
    __syncthreads();
    return incl - v;
}

// the largest i < n with off[i] <= g (off ascends, off[0] = 0)
__device__ __forceinline__ uint32_t sp_find(const uint64_t *off, int n, uint64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return (uint32_t)lo;
}

__global__ __launch_bounds__(1024) void k_split_plan(SpArgs a) {
    __shared__ uint64_t buf[2048];
    __shared__ unsigned long long longest;
    const int t = threadIdx.x;
    if (a.ovf && *a.ovf) return;                                 // every thread, before the first barrier
    if (t == 0) longest = 0;
    const int per = (a.nslices + 1023) / 1024, b0 = min(t * per, a.nslices), b1 = min(b0 + per, a.nslices);
    uint64_t sc = 0, ss = 0, most = 0, r0, tc, ts;
    for (int i = b0; i < b1; i++) {
        const uint64_t nb = sp_slice_bins(a, i, &r0), nc = jms_nchunks(nb, a.L);
        sc += nc; ss += jms_nchunks(nb, a.span) - 1;
        most = nc > most ? nc : most;
    }
    uint64_t ec = sp_block_scan(sc, buf, &tc), es = sp_block_scan(ss, buf, &ts);
    atomicMax(&longest, (unsigned long long)most);
    for (int i = b0; i < b1; i++) {
        const uint64_t nb = sp_slice_bins(a, i, &r0), nc = jms_nchunks(nb, a.L), ns = jms_nchunks(nb, a.span) - 1;
        a.sl_coff[i] = ec; a.sl_poff[i] = es;
        ec += nc; es += ns;
    }
    __syncthreads();                                             // sl_coff, sl_poff: written by this workgroup, read below
    // the slice of every chunk and slot: the last slice whose first chunk / slot is not behind it (a slice
    // without slots shares its offset with the next one, which the search passes over)
    for (uint64_t g = t; g < tc && g < a.chunks_cap; g += 1024) a.ch_slice[g] = sp_find(a.sl_coff, a.nslices, g);
    for (uint64_t g = t; g < ts && g < a.slots_cap; g += 1024) a.sp_slice[g] = sp_find(a.sl_poff, a.nslices, g);
    if (t == 0) {
        a.sl_coff[a.nslices] = tc; a.sl_poff[a.nslices] = ts;
        // the capacities hold every count that the record capacity admits (jmh_split_enqueue): never more
        a.tot[0] = tc <= a.chunks_cap ? tc : 0; a.tot[1] = ts <= a.slots_cap && tc <= a.chunks_cap ? ts : 0; a.tot[2] = longest;
    }
}

__global__ __launch_bounds__(64) void k_split_maps(SpArgs a) {
    __shared__ uint16_t map[JMR_NCTX * 64];                      // map[c * 64 + l]: the values 2 l (low byte) and 2 l + 1 of context c
    __shared__ uint8_t nxt[2 * JMS_NVAL];                        // a value after bin 0 / 1
    const int lane = threadIdx.x;
    const uint64_t slot = blockIdx.x;
    if (a.ovf && *a.ovf) return;
    if (slot >= a.tot[1]) return;
    const int si = (int)a.sp_slice[slot];
    uint64_t r0;
    sp_slice_bins(a, si, &r0);
    r0 += (slot - a.sl_poff[si]) * a.span;                       // a span with a successor is whole
    for (int i = lane; i < 2 * JMS_NVAL; i += 64) nxt[i] = (uint8_t)jms_ctx_next((uint32_t)(i & 127), i >> 7, jmr_trans_lps[(i & 127) >> 1]);
    for (int c = 0; c < JMR_NCTX; c++) map[c * 64 + lane] = (uint16_t)(2 * lane | (2 * lane + 1) << 8);
    __syncthreads();
    const uint32_t nb = a.span;
    uint32_t nx = (uint32_t)lane < nb ? a.rec[r0 + lane] : 0u;
    for (uint32_t base = 0; base < nb; base += 64) {
        const int cnt = nb - base < 64 ? (int)(nb - base) : 64;
        const uint32_t cur = nx;
        nx = base + 64 + lane < nb ? a.rec[r0 + base + 64 + lane] : 0u;
        for (int i = 0; i < cnt; i++) {
            const uint32_t rec = (uint32_t)__builtin_amdgcn_readlane((int)cur, i);
            if (!jms_is_regular(rec) || (rec & 0x1ff) >= JMR_NCTX) continue;   // wave-uniform; the second: no record holds one
            uint16_t *m = map + (rec & 0x1ff) * 64 + lane;
            const uint8_t *n = nxt + JMC_VAL(rec) * JMS_NVAL;
            const uint32_t v = *m;
            *m = (uint16_t)(n[v & 0xff] | n[v >> 8] << 8);
        }
    }
    __syncthreads();
    uint32_t *dst = (uint32_t *)(a.maps + slot * JMS_MAP_BYTES);
    for (int i = lane; i < JMS_MAP_BYTES / 4; i += 64) dst[i] = ((const uint32_t *)map)[i];
}

__global__ __launch_bounds__(320) void k_split_ctx(SpArgs a) {
    const int c = threadIdx.x, si = blockIdx.x;
    if (a.ovf && *a.ovf) return;
    if (c >= JMR_NCTX || a.tot[0] == 0) return;
    const jmh_cabac_slice_desc d = a.sl[si];
    const uint64_t s0 = a.sl_poff[si], s1 = a.sl_poff[si + 1];
    uint32_t v = jmr_init_one(c, d.slice_type == JMH_I_SLICE, d.slice_qp);
    for (uint64_t s = s0; s < s1 && s < a.slots_cap; s++) {
        v = a.maps[s * JMS_MAP_BYTES + (uint64_t)c * JMS_NVAL + v];
        a.centry[s * JMR_NCTX + c] = (uint8_t)v;
    }
}

// block b < nslices: the first span of slice b; behind them one block per slot: the span behind the slot
__global__ __launch_bounds__(64) void k_split_resolve(SpArgs a) {
    const int lane = threadIdx.x;
    if (a.ovf && *a.ovf) return;
    if (a.tot[0] == 0) return;
    int si;
    uint64_t j;
    const uint8_t *entry = nullptr;
    if ((int)blockIdx.x < a.nslices) { si = blockIdx.x; j = 0; }
    else {
        const uint64_t slot = blockIdx.x - a.nslices;
        if (slot >= a.tot[1]) return;
        si = (int)a.sp_slice[slot]; j = slot - a.sl_poff[si] + 1;
        entry = a.centry + slot * JMR_NCTX;
    }
    const jmh_cabac_slice_desc d = a.sl[si];
    uint64_t r0;
    const uint64_t all = sp_slice_bins(a, si, &r0);
    r0 += j * a.span;
    const uint32_t nb = all - j * a.span < a.span ? (uint32_t)(all - j * a.span) : a.span;
    uint32_t cv[5];                                              // context i in lane i & 63 of cv[i >> 6] (k_cabac_code)
    for (int k = 0; k < 5; k++) {
        const int c = 64 * k + lane;
        cv[k] = c < JMR_NCTX ? (entry ? entry[c] : jmr_init_one(c, d.slice_type == JMH_I_SLICE, d.slice_qp)) : 0u;
    }
    const uint32_t tt = jmr_trans_lps[lane];
    uint32_t nx = (uint32_t)lane < nb ? a.rec[r0 + lane] : 0u;
    for (uint32_t base = 0; base < nb; base += 64) {
        const int cnt = nb - base < 64 ? (int)(nb - base) : 64;
        const uint32_t cur = nx;
        nx = base + 64 + lane < nb ? a.rec[r0 + base + 64 + lane] : 0u;
        uint32_t mine = cur;
        for (int i = 0; i < cnt; i++) {
            const uint32_t rec = (uint32_t)__builtin_amdgcn_readlane((int)cur, i);
            if (!jms_is_regular(rec)) continue;                  // wave-uniform
            const int c = (int)(rec & 0x1ff), l = c & 63;
            uint32_t v;
            switch (c >> 6) {
            case 0: v = (uint32_t)__builtin_amdgcn_readlane((int)cv[0], l); break;
            case 1: v = (uint32_t)__builtin_amdgcn_readlane((int)cv[1], l); break;
            case 2: v = (uint32_t)__builtin_amdgcn_readlane((int)cv[2], l); break;
            case 3: v = (uint32_t)__builtin_amdgcn_readlane((int)cv[3], l); break;
            default: v = (uint32_t)__builtin_amdgcn_readlane((int)cv[4], l); break;
            }
            mine = lane == i ? jms_resolve(rec, v) : mine;
            const uint32_t w = jms_ctx_next(v, (int)JMC_VAL(rec), __builtin_amdgcn_readlane((int)tt, (int)(v >> 1)));
            const int at = c - lane;
            for (int k = 0; k < 5; k++) cv[k] = at == 64 * k ? w : cv[k];
        }
        if (lane < cnt) a.rec[r0 + base + lane] = (uint16_t)mine;
    }
}

// chunk g of the grid: its slice, its index in the slice, its records; false: nothing to do
__device__ __forceinline__ bool sp_chunk(const SpArgs &a, uint64_t g, int *si, uint64_t *j, uint64_t *nc, uint64_t *r0, uint32_t *nb) {
    if (g >= a.tot[0]) return false;
    *si = (int)a.ch_slice[g];
    *j = g - a.sl_coff[*si];
    const uint64_t all = sp_slice_bins(a, *si, r0);
    *nc = jms_nchunks(all, a.L);
    *r0 += *j * a.L;
    *nb = *j + 1 < *nc ? a.L : (uint32_t)(all - *j * a.L);
    return true;
}

__global__ __launch_bounds__(64) void k_split_range(SpArgs a) {
    const int lane = threadIdx.x;
    const uint64_t g = blockIdx.x;
    if (a.ovf && *a.ovf) return;
    int si; uint64_t j, nc, r0; uint32_t nb;
    if (!sp_chunk(a, g, &si, &j, &nc, &r0, &nb) || j + 1 == nc) return;   // the last chunk has no successor to tell
    const uint32_t tl = jms_lps_dword(lane);
    uint32_t range[4], shifts[4];
    for (int k = 0; k < 4; k++) { range[k] = 256u + 4u * lane + k; shifts[k] = 0; }
    uint32_t nx = (uint32_t)lane < nb ? a.rec[r0 + lane] : 0u;
    for (uint32_t base = 0; base < nb; base += 64) {
        const int cnt = nb - base < 64 ? (int)(nb - base) : 64;
        const uint32_t cur = nx;
        nx = base + 64 + lane < nb ? a.rec[r0 + base + 64 + lane] : 0u;
        for (int i = 0; i < cnt; i++) {
            const uint32_t rr = (uint32_t)__builtin_amdgcn_readlane((int)cur, i);
            const uint32_t lpsdw = (uint32_t)__builtin_amdgcn_readlane((int)tl, (int)((rr >> 1) & 63));
            for (int k = 0; k < 4; k++) jms_range_rec(rr, lpsdw, &range[k], &shifts[k]);
        }
    }
    uint4 o;
    o.x = jms_rmap_pack(range[0], shifts[0]); o.y = jms_rmap_pack(range[1], shifts[1]);
    o.z = jms_rmap_pack(range[2], shifts[2]); o.w = jms_rmap_pack(range[3], shifts[3]);
    ((uint4 *)(a.rmap + g * JMS_NRANGE))[lane] = o;
}

__global__ __launch_bounds__(64) void k_split_along(SpArgs a) {
    const int lane = threadIdx.x, si = blockIdx.x;
    if (a.ovf && *a.ovf) return;
    if (a.tot[0] == 0) return;
    const uint64_t g0 = a.sl_coff[si], nc = a.sl_coff[si + 1] - g0;
    uint32_t range = 510;
    uint64_t T = 0;
    for (uint64_t base = 0; base < nc; base += SP_ROWS) {
        uint4 row[SP_ROWS];
#pragma unroll
        for (int b = 0; b < SP_ROWS; b++)                        // the last chunk's row is not written and not used
            row[b] = base + b + 1 < nc ? ((const uint4 *)(a.rmap + (g0 + base + b) * JMS_NRANGE))[lane] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int b = 0; b < SP_ROWS; b++) {
            if (base + b >= nc) break;                           // wave-uniform
            if (lane == 0) { a.ch_range[g0 + base + b] = range; a.ch_T[g0 + base + b] = T; }
            const uint32_t idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(range - 256u)), k = idx & 3;
            const uint32_t comp = k == 0 ? row[b].x : k == 1 ? row[b].y : k == 2 ? row[b].z : row[b].w;
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)comp, (int)(idx >> 2));
            if (base + b + 1 < nc) { range = jms_rmap_range(e); T += jms_rmap_shifts(e); }
        }
    }
}

__global__ __launch_bounds__(64) void k_split_code(SpArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[SP_STAGE];
    const int lane = threadIdx.x;
    const uint64_t g = blockIdx.x;
    if (a.ovf && *a.ovf) return;
    int si; uint64_t j, nc, r0; uint32_t nb;
    if (!sp_chunk(a, g, &si, &j, &nc, &r0, &nb)) return;
    const bool last = j + 1 == nc;
    const uint64_t T = a.ch_T[g], B = jms_byte0(T), bound = a.sl_soff[si + 1] - a.sl_soff[si];
    if (B > bound) {                                             // cannot happen: the bound holds the slice's bytes
        if (last && lane == 0) { a.sl_bytes[si] = -1; a.sl_stop[si] = 0; }
        return;
    }
    const uint64_t len = last ? bound - B : jms_byte0(a.ch_T[g + 1]) - B;
    jmc_enc e;
    e.tl = jms_lps_dword(lane); e.tailv = 0;
    e.st = nullptr; e.lps = nullptr; e.tlps = nullptr; e.out = stage;
    e.cap = (uint32_t)(len < bound - B ? len : bound - B);      // a slice's bound is below 2^32 (k_cabac_code)
    e.spill = a.scratch + a.sl_soff[si] + B;
    jms_enc_begin(&e, a.ch_range[g], T);
    uint32_t nx = (uint32_t)lane < nb ? a.rec[r0 + lane] : 0u;
    for (uint32_t base = 0; base < nb; base += 64) {
        const int cnt = nb - base < 64 ? (int)(nb - base) : 64;
        const uint32_t cur = nx;
        nx = base + 64 + lane < nb ? a.rec[r0 + base + 64 + lane] : 0u;
        for (int i = 0; i < cnt; i++) jmc_enc_rec(&e, (uint32_t)__builtin_amdgcn_readlane((int)cur, i));
    }
    uint32_t stop = 0;
    if (last) { stop = jms_stop_info(&e); jmc_enc_finish(&e); }
    else jms_enc_tail(&e);
    const uint32_t own = e.nbytes < e.cap ? e.nbytes : e.cap;   // the bytes that went to the stage
    const uint32_t rem = own & (SP_STAGE - 1), done = own - rem;
    for (int i = 0; i < 4; i++)
        if (64u * i + lane < rem) ((uint8_t *)e.spill)[done + 64 * i + lane] = stage[64 * i + lane];
    if (lane == 0) {
        if (last) {
            a.sl_bytes[si] = e.nbytes <= e.cap ? (int64_t)(B + e.nbytes) : -1;   // -1: cannot happen; the host reports it
            a.sl_stop[si] = stop;
        } else a.tail[g] = e.nbytes == e.cap + 3 ? e.tailv & 0xffffffu : 0u;
    }
}

// the region of chunk j of slice si: [*B, *B + *len) of the slice's scratch; false: the slice has no bytes
__device__ __forceinline__ bool sp_region(const SpArgs &a, uint64_t g, int si, uint64_t j, uint64_t nc, uint64_t *B, uint64_t *len) {
    const int64_t total = a.sl_bytes[si];
    if (total <= 0) return false;
    *B = jms_byte0(a.ch_T[g]);
    const uint64_t E = j + 1 < nc ? jms_byte0(a.ch_T[g + 1]) : (uint64_t)total;
    if (*B > E || E > (uint64_t)total) return false;             // cannot happen
    *len = E - *B;
    return true;
}

__global__ __launch_bounds__(256) void k_split_sum(SpArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (a.ovf && *a.ovf) return;
    int si; uint64_t j, nc, r0, B, len; uint32_t nb;
    if (!sp_chunk(a, g, &si, &j, &nc, &r0, &nb)) return;
    a.fn[g] = make_uint2(0, 0);
    if (!sp_region(a, g, si, j, nc, &B, &len)) return;
    uint8_t *b = a.scratch + a.sl_soff[si] + B;
    if (j + 1 == nc && len) b[len - 1] = (uint8_t)jms_stop_clear(b[len - 1], a.sl_stop[si]);
    const uint64_t g0 = g - j;
    uint32_t q, theta;
    jms_region_sum(b, len, jms_tail_sum(a.tail + g0, a.ch_T + g0, j, B, len < 3 ? (uint32_t)len : 3u), &q, &theta);
    a.fn[g] = make_uint2(q, theta);
}

__global__ __launch_bounds__(64) void k_split_carry(SpArgs a) {
    const int lane = threadIdx.x, si = blockIdx.x;
    if (a.ovf && *a.ovf) return;
    if (a.tot[0] == 0) return;
    const uint64_t g0 = a.sl_coff[si], nc = a.sl_coff[si + 1] - g0;
    uint32_t x = 0;
    for (uint64_t left = nc; left > 0;) {                        // from the slice's end, 64 chunks per fetch
        const int cnt = left < 64 ? (int)left : 64;
        const uint2 f = lane < cnt ? a.fn[g0 + left - 1 - lane] : make_uint2(0, 0);
        uint32_t mine = 0;
        for (int i = 0; i < cnt; i++) {
            mine = lane == i ? x : mine;
            x = jms_carry_apply((uint32_t)__builtin_amdgcn_readlane((int)f.x, i), (uint32_t)__builtin_amdgcn_readlane((int)f.y, i), x);
        }
        if (lane < cnt) a.cin[g0 + left - 1 - lane] = mine;
        left -= cnt;
    }
}

__global__ __launch_bounds__(256) void k_split_apply(SpArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (a.ovf && *a.ovf) return;
    int si; uint64_t j, nc, r0, B, len; uint32_t nb;
    if (!sp_chunk(a, g, &si, &j, &nc, &r0, &nb)) return;
    if (!sp_region(a, g, si, j, nc, &B, &len)) return;
    uint8_t *b = a.scratch + a.sl_soff[si] + B;
    jms_region_carry(b, len, a.cin[g]);
    if (j + 1 == nc && len) b[len - 1] = (uint8_t)jms_stop_set(b[len - 1], a.sl_stop[si]);
}

// ---- host side ----------------------------------------------------------------------------------
struct jmh_split_state {
    int nslices_cap = 0;
    uint64_t chunks_cap = 0, slots_cap = 0;
    uint64_t *d_coff = nullptr, *d_poff = nullptr, *d_tot = nullptr, *d_T = nullptr;
    uint32_t *d_chslice = nullptr, *d_spslice = nullptr, *d_rmap = nullptr, *d_range = nullptr, *d_tail = nullptr, *d_cin = nullptr, *d_stop = nullptr;
    uint2 *d_fn = nullptr;
    uint8_t *d_maps = nullptr, *d_centry = nullptr;
    uint64_t *h_tot = nullptr;             // pinned: the three totals of the last synchronous call
    size_t bytes = 0;                      // device memory held
    std::vector<void *> retired;           // outgrown buffers: freed with the state (hipFree would wait for the device)
};

#define SPCHK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "jmhip: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return JMH_E_HIP;                                                     \
        }                                                                         \
    } while (0)

void jmh_split_free(jmh_split_state *s) {
    if (!s) return;
    void *bufs[] = {s->d_coff, s->d_poff, s->d_tot, s->d_T, s->d_chslice, s->d_spslice, s->d_rmap, s->d_range, s->d_tail, s->d_cin, s->d_stop,
                    s->d_fn, s->d_maps, s->d_centry};
    for (void *p : bufs) if (p) (void)hipFree(p);
    for (void *p : s->retired) (void)hipFree(p);
    if (s->h_tot) (void)hipHostFree(s->h_tot);
    delete s;
}

template <class T> static int sp_fit(jmh_split_state *s, T **buf, size_t have, size_t want) {
    if (*buf && have >= want) return JMH_OK;
    if (*buf) { s->retired.push_back(*buf); *buf = nullptr; }
    if (hipMalloc((void **)buf, want * sizeof(T)) != hipSuccess) return JMH_E_OOM;
    s->bytes += want * sizeof(T);
    return JMH_OK;
}

uint64_t jmh_split_bytes(const jmh_split_state *s) { return s ? s->bytes : 0; }
const uint64_t *jmh_split_totals(const jmh_split_state *s) { return s ? s->h_tot : nullptr; }

// The ten launches on st, behind k_cabac_bins and before k_cabac_where.  rec_cap: the records the
// record buffer holds, which bounds the picture's bins: chunks <= rec_cap / L + nslices, slots <=
// rec_cap / span.  The buffers here are sized to exactly that and so grow when the record buffer does.  totals: the synchronous call
// wants the three totals copied to the pinned words behind jmh_split_totals.
int jmh_split_enqueue(jmh_split_state **state, hipStream_t st, const jmh_cabac_slice_desc *d_sl, int nslices, const uint64_t *d_off,
                      const uint64_t *d_soff, uint16_t *d_rec, uint64_t rec_cap, uint8_t *d_scratch, int64_t *d_slbytes, const uint32_t *d_ovf,
                      int chunk_bins, bool totals) {
    if (!*state) *state = new jmh_split_state();
    jmh_split_state *s = *state;
    const uint64_t L = (uint64_t)chunk_bins, span = jms_span(L);
    const uint64_t chunks = rec_cap / L + (uint64_t)nslices, slots = rec_cap / span;
    if (chunks > 0x7fffffffu) return JMH_E_UNSUPPORTED_CFG;      // a grid dimension
    int r = JMH_OK;
    if (!s->h_tot && hipHostMalloc((void **)&s->h_tot, 3 * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) return JMH_E_OOM;
    if (!s->d_tot && (r = sp_fit(s, &s->d_tot, 0, 3))) return r;
    if (nslices > s->nslices_cap) {
        const size_t n = (size_t)nslices + 1;
        if ((r = sp_fit(s, &s->d_coff, 0, n)) || (r = sp_fit(s, &s->d_poff, 0, n)) || (r = sp_fit(s, &s->d_stop, 0, n))) return r;
        s->nslices_cap = nslices;
    }
    if (chunks > s->chunks_cap) {
        const size_t n = (size_t)chunks;                         // rec_cap already grows by halves (cb_grow): no second factor
        if ((r = sp_fit(s, &s->d_chslice, 0, n)) || (r = sp_fit(s, &s->d_T, 0, n + 1)) || (r = sp_fit(s, &s->d_range, 0, n)) ||
            (r = sp_fit(s, &s->d_tail, 0, n)) || (r = sp_fit(s, &s->d_cin, 0, n)) || (r = sp_fit(s, &s->d_fn, 0, n)) ||
            (r = sp_fit(s, &s->d_rmap, 0, n * JMS_NRANGE)))
            return r;
        s->chunks_cap = n;
    }
    if (slots + 1 > s->slots_cap) {
        const size_t n = (size_t)(slots + 1);
        if ((r = sp_fit(s, &s->d_spslice, 0, n)) || (r = sp_fit(s, &s->d_maps, 0, n * JMS_MAP_BYTES)) || (r = sp_fit(s, &s->d_centry, 0, n * JMR_NCTX)))
            return r;
        s->slots_cap = n;
    }
    SpArgs a;
    a.sl = d_sl; a.nslices = nslices; a.mb_off = d_off; a.sl_soff = d_soff; a.rec = d_rec; a.scratch = d_scratch; a.sl_bytes = d_slbytes;
    a.ovf = d_ovf; a.L = (uint32_t)L; a.span = (uint32_t)span; a.chunks_cap = chunks; a.slots_cap = slots;
    a.sl_coff = s->d_coff; a.sl_poff = s->d_poff; a.ch_slice = s->d_chslice; a.sp_slice = s->d_spslice; a.tot = s->d_tot;
    a.maps = s->d_maps; a.centry = s->d_centry; a.rmap = s->d_rmap; a.ch_T = s->d_T; a.ch_range = s->d_range; a.tail = s->d_tail;
    a.cin = s->d_cin; a.sl_stop = s->d_stop; a.fn = s->d_fn;
    const unsigned gc = (unsigned)chunks, gs = (unsigned)slots, gt = (unsigned)((chunks + 255) / 256);
    hipLaunchKernelGGL(k_split_plan, dim3(1), dim3(1024), 0, st, a);
    SPCHK(hipGetLastError());
    if (gs) {
        hipLaunchKernelGGL(k_split_maps, dim3(gs), dim3(64), 0, st, a);
        SPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_split_ctx, dim3(nslices), dim3(320), 0, st, a);
    SPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_resolve, dim3(nslices + gs), dim3(64), 0, st, a);
    SPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_range, dim3(gc), dim3(64), 0, st, a);
    SPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_along, dim3(nslices), dim3(64), 0, st, a);
    SPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_code, dim3(gc), dim3(64), 0, st, a);
    SPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_sum, dim3(gt), dim3(256), 0, st, a);
    SPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_carry, dim3(nslices), dim3(64), 0, st, a);
    SPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_split_apply, dim3(gt), dim3(256), 0, st, a);
    SPCHK(hipGetLastError());
    if (totals) SPCHK(hipMemcpyAsync(s->h_tot, s->d_tot, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return JMH_OK;
}
