// jmh_cabac.hip — CABAC slice data written on the device (include/jmhip_cabac.h): the
// shared core (jmh_cabac_write.h: binarisation + context selection from the result array, and the
// arithmetic encoder with byte output) in six launches on a stream of the writer's own:
//
//   k_cabac_count   one wave per macroblock; lane u < JMW_UNITS counts the bins of unit u with the
//                   counting sink.  Leaves per unit bins, per macroblock bins / slice.
//   k_cabac_scan    one workgroup: exclusive scan of the macroblock bins over the picture; from it
//                   every slice's bins, the bound of its bytes (JMC_SLICE_MAX_BYTES) and the scan of
//                   those bounds: where each slice is coded in the scratch buffer.
//   k_cabac_bins    one wave per macroblock; a wave prefix sum of the unit bins gives every lane its
//                   record offset; the lanes store their unit's bin records.  Macroblocks are in
//                   raster order and slices are raster runs, so a slice's records are contiguous.
//   k_cabac_code    one wave per slice, one wave per workgroup: the serial chain.  Context states
//                   and Table 9-44 live in registers, one entry per lane, read and written through
//                   wave-uniform lane indices; the wave fetches 64 records at a time, one per lane,
//                   and every lane codes them in step (the values are wave-uniform, so the control
//                   flow is scalar); bytes are staged in LDS and leave 256 at a time as one dword per lane.
//   k_cabac_where   one workgroup: scan of the slices' byte counts: where[], the total.
//   k_cabac_pack    copies every slice from the scratch buffer to its place in the output.
//
// Two callers queue these launches.  The synchronous entry points (jmh_cabac_run) learn the bins
// between scan and bins (they size the record and scratch buffers from them) and the bytes between
// where and pack (the capacity check), each by a copy on the writer's stream, which only that stream
// is waited for.  A coded picture (jmh_cabac_enqueue) queues all six behind the
// picture's last macroblock with no host wait: the buffers have capacities decided before, k_cabac_scan
// (bins, scratch) and k_cabac_where (output bytes) set the picture's overflow word when a counted
// size exceeds its capacity, and every later launch of that picture returns at once when it is set
// -- a device-side predicate, no store out of bounds; the host sees the word at the pop.  No workgroup waits on another, every loop is bounded by a
// counted size, and the coder cannot overflow its scratch: it is sized from the bound of its bins.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

struct jmc_enc;
__host__ __device__ static inline void cb_emit(jmc_enc *e, uint32_t b);
__host__ __device__ static inline uint32_t cb_ctx_get(const jmc_enc *e, int i);
__host__ __device__ static inline void cb_ctx_set(jmc_enc *e, int i, uint32_t v);
__host__ __device__ static inline uint32_t cb_lps_get(const jmc_enc *e, int s, uint32_t q);
__host__ __device__ static inline int cb_tlps_get(const jmc_enc *e, int s);
#define JMC_EMIT(e, b) cb_emit((e), (b))
// k_cabac_code: context i in lane i & 63 of register cv[i >> 6]; rangeTabLPS[s][0..3] packed in lane s of
// tl, transIdxLPS[s] in lane s of tt.  Every index is wave-uniform, so a lookup is a v_readlane and an
// update a compare and select: no memory in the dependent chain of a bin
#define JMC_ENC_EXTRA uint32_t cv[5], tl, tt;
#define JMC_CTX_GET(e, i) cb_ctx_get((e), (i))
#define JMC_CTX_SET(e, i, v) cb_ctx_set((e), (i), (uint32_t)(v))
#define JMC_LPS_GET(e, s, q) cb_lps_get((e), (s), (q))
#define JMC_TLPS_GET(e, s) cb_tlps_get((e), (s))
#include "jmh_cabac_write.h"
#include "jmh_cabac.h"

#define CB_WAVES 4                                   // macroblocks (waves) per workgroup
#define CB_STAGE 256                                 // staged output bytes of the coder: one dword per lane
#define CB_PACK_Y 16                                 // workgroups that share the copy of one slice

// a byte of the code string: into the LDS stage, and the stage to the slice's scratch when it is full
__host__ __device__ static inline void cb_emit(jmc_enc *e, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    e->out[e->nbytes & (CB_STAGE - 1)] = (uint8_t)b;
    e->nbytes++;
    if ((e->nbytes & (CB_STAGE - 1)) == 0 && e->nbytes <= e->cap)    // within the bound: always (JMC_SLICE_MAX_BYTES)
        ((uint32_t *)e->spill)[((e->nbytes - CB_STAGE) >> 2) + threadIdx.x] = ((const uint32_t *)e->out)[threadIdx.x];
#else
    jmc_emit_plain(e, b);
#endif
}

__host__ __device__ static inline uint32_t cb_ctx_get(const jmc_enc *e, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int u = __builtin_amdgcn_readfirstlane(i), l = u & 63;
    switch (u >> 6) {
    case 0: return (uint32_t)__builtin_amdgcn_readlane((int)e->cv[0], l);
    case 1: return (uint32_t)__builtin_amdgcn_readlane((int)e->cv[1], l);
    case 2: return (uint32_t)__builtin_amdgcn_readlane((int)e->cv[2], l);
    case 3: return (uint32_t)__builtin_amdgcn_readlane((int)e->cv[3], l);
    default: return (uint32_t)__builtin_amdgcn_readlane((int)e->cv[4], l);
    }
#else
    return e->st[i];
#endif
}
__host__ __device__ static inline void cb_ctx_set(jmc_enc *e, int i, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    // the lane that holds context i takes the value (a compare and a select per register, no branch)
    const int at = __builtin_amdgcn_readfirstlane(i) - (int)threadIdx.x;
    for (int k = 0; k < 5; k++) e->cv[k] = at == 64 * k ? v : e->cv[k];
#else
    e->st[i] = (uint8_t)v;
#endif
}
__host__ __device__ static inline uint32_t cb_lps_get(const jmc_enc *e, int s, uint32_t q) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((uint32_t)__builtin_amdgcn_readlane((int)e->tl, __builtin_amdgcn_readfirstlane(s)) >> (8 * q)) & 0xffu;
#else
    return e->lps[s * 4 + q];
#endif
}
__host__ __device__ static inline int cb_tlps_get(const jmc_enc *e, int s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readlane((int)e->tt, __builtin_amdgcn_readfirstlane(s));
#else
    return e->tlps[s];
#endif
}

struct CbPic {
    const jmh_mb_result *res;
    int mbw, mbh, t8mode, cip, nmb, nslices;
    const jmh_cabac_slice_desc *sl;
};

__device__ __forceinline__ jmw_pic cb_pic(const CbPic &p) {
    jmw_pic q;
    q.res = p.res; q.mbw = p.mbw; q.mbh = p.mbh; q.t8mode = p.t8mode; q.cip = p.cip;
    return q;
}
__device__ __forceinline__ jmw_slice cb_slice(const jmh_cabac_slice_desc &d) {
    jmw_slice s;
    s.first_mb = d.first_mb; s.end_mb = d.first_mb + d.n_mb; s.slice_p = d.slice_type == JMH_P_SLICE;
    return s;
}
__device__ __forceinline__ uint64_t cb_align4(uint64_t v) { return (v + 3) & ~(uint64_t)3; }

__global__ __launch_bounds__(64 * CB_WAVES) void k_cabac_count(CbPic p, uint16_t *unit_bins, uint32_t *mb_bins, int32_t *mb_slice) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * CB_WAVES + (threadIdx.x >> 6);
    if (a >= p.nmb) return;                                      // whole wave
    int lo = 0, hi = p.nslices - 1;                              // the slice holding a (descriptors tile the picture)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.sl[mid].first_mb <= a) lo = mid; else hi = mid - 1;
    }
    const jmw_slice sl = cb_slice(p.sl[lo]);
    const jmw_pic pic = cb_pic(p);
    jmc_sink s;
    s.rec = nullptr; s.n = 0;
    if (lane < JMW_UNITS) jmc_unit(&s, &pic, &sl, a, lane);
    if (lane < 32) unit_bins[(size_t)a * 32 + lane] = (uint16_t)s.n;   // a unit holds at most 2942 bins
    uint32_t sum = s.n;
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) { mb_bins[a] = sum; mb_slice[a] = lo; }
}

// exclusive scan of v over the 1024 threads of the workgroup (Hillis-Steele in LDS); *total: the sum
__device__ uint64_t cb_block_scan(uint64_t v, uint64_t *buf, uint64_t *total) {
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

// totals[0]: the picture's bins, totals[1]: the scratch bytes that hold every slice's bound.
// ovf (may be null): set when either exceeds its capacity, decided before the enqueue; the later
// passes of that picture then write nothing (coded pictures)
__global__ __launch_bounds__(1024) void k_cabac_scan(CbPic p, const uint32_t *mb_bins, uint64_t *mb_off, uint64_t *sl_soff, uint64_t *totals,
                                                     uint64_t rec_cap, uint64_t scratch_cap, uint32_t *ovf) {
    __shared__ uint64_t buf[2048];
    const int t = threadIdx.x;
    uint64_t total;
    {   // macroblock bins -> mb_off[a] = bins of the picture's macroblocks before a; mb_off[nmb] = all
        const int per = (p.nmb + 1023) / 1024, b0 = min(t * per, p.nmb), b1 = min(b0 + per, p.nmb);
        uint64_t s = 0;
        for (int a = b0; a < b1; a++) s += mb_bins[a];
        uint64_t e = cb_block_scan(s, buf, &total);
        for (int a = b0; a < b1; a++) { mb_off[a] = e; e += mb_bins[a]; }
        if (t == 0) {
            mb_off[p.nmb] = total; totals[0] = total;
            if (ovf && total > rec_cap) *ovf = 1u;
        }
    }
    __syncthreads();
    {   // slices: the bound of their bytes (whole dwords: the coder stores dwords), scratch offsets
        const int per = (p.nslices + 1023) / 1024, b0 = min(t * per, p.nslices), b1 = min(b0 + per, p.nslices);
        uint64_t s = 0;
        for (int i = b0; i < b1; i++) {
            const jmh_cabac_slice_desc d = p.sl[i];
            s += cb_align4(JMC_SLICE_MAX_BYTES(mb_off[d.first_mb + d.n_mb] - mb_off[d.first_mb]));
        }
        uint64_t e = cb_block_scan(s, buf, &total);
        for (int i = b0; i < b1; i++) {
            const jmh_cabac_slice_desc d = p.sl[i];
            sl_soff[i] = e;
            e += cb_align4(JMC_SLICE_MAX_BYTES(mb_off[d.first_mb + d.n_mb] - mb_off[d.first_mb]));
        }
        if (t == 0) {
            sl_soff[p.nslices] = total; totals[1] = total;
            if (ovf && total > scratch_cap) *ovf = 1u;
        }
    }
}

__global__ __launch_bounds__(64 * CB_WAVES) void k_cabac_bins(CbPic p, const uint16_t *unit_bins, const int32_t *mb_slice,
                                                              const uint64_t *mb_off, uint16_t *rec, uint64_t rec_cap, const uint32_t *ovf) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * CB_WAVES + (threadIdx.x >> 6);
    if (a >= p.nmb || (ovf && *ovf)) return;                     // whole wave; whole grid: a count exceeds its capacity
    const jmw_slice sl = cb_slice(p.sl[mb_slice[a]]);
    const jmw_pic pic = cb_pic(p);
    const uint32_t ub = lane < 32 ? unit_bins[(size_t)a * 32 + lane] : 0u;
    uint32_t incl = ub;                                          // inclusive wave prefix sum of the unit bins
    for (int o = 1; o < 32; o <<= 1) {
        const uint32_t x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    const uint64_t at = mb_off[a] + incl - ub;
    if (lane >= JMW_UNITS || !ub || at + ub > rec_cap) return;   // the last: cannot happen, the buffer holds the counted bins
    jmc_sink s;
    s.rec = rec + at; s.n = 0;
    jmc_unit(&s, &pic, &sl, a, lane);
}

__global__ __launch_bounds__(64) void k_cabac_code(CbPic p, const uint64_t *mb_off, const uint64_t *sl_soff, const uint16_t *rec,
                                                   uint8_t *scratch, int64_t *sl_bytes, const uint32_t *ovf) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[CB_STAGE];
    const int lane = threadIdx.x, si = blockIdx.x;
    if (ovf && *ovf) return;                                     // whole grid
    const jmh_cabac_slice_desc d = p.sl[si];
    jmc_enc e;
    for (int k = 0; k < 5; k++) e.cv[k] = 64 * k + lane < JMR_NCTX ? jmr_init_one(64 * k + lane, d.slice_type == JMH_I_SLICE, d.slice_qp) : 0u;
    e.tl = jmr_lps[lane][0] | jmr_lps[lane][1] << 8 | jmr_lps[lane][2] << 16 | (uint32_t)jmr_lps[lane][3] << 24;
    e.tt = jmr_trans_lps[lane];
    e.st = nullptr; e.lps = nullptr; e.tlps = nullptr; e.out = stage;
    e.cap = (uint32_t)(sl_soff[si + 1] - sl_soff[si]);
    e.spill = scratch + sl_soff[si];
    jmc_enc_start(&e);
    const uint64_t r0 = mb_off[d.first_mb], nb = mb_off[d.first_mb + d.n_mb] - r0;
    // 64 records per fetch, one per lane; the next 64 are in flight while these are coded
    uint32_t nxt = (uint64_t)lane < nb ? rec[r0 + lane] : 0u;
    for (uint64_t base = 0; base < nb; base += 64) {
        const int cnt = nb - base < 64 ? (int)(nb - base) : 64;
        const uint32_t cur = nxt;
        nxt = base + 64 + lane < nb ? rec[r0 + base + 64 + lane] : 0u;
        for (int i = 0; i < cnt; i++) jmc_enc_rec(&e, (uint32_t)__builtin_amdgcn_readlane((int)cur, i));
    }
    const uint32_t nbytes = jmc_enc_finish(&e);
    const uint32_t rem = nbytes & (CB_STAGE - 1), done = nbytes - rem;
    if (4u * lane < rem && done + 4u * lane + 4u <= e.cap)
        ((uint32_t *)e.spill)[(done >> 2) + lane] = ((const uint32_t *)stage)[lane];
    if (lane == 0) sl_bytes[si] = nbytes <= e.cap ? (int64_t)nbytes : -1;   // -1: cannot happen; the host reports it
}

__global__ __launch_bounds__(1024) void k_cabac_where(CbPic p, const uint64_t *mb_off, const int64_t *sl_bytes, jmh_cabac_slice_bytes *where,
                                                      int64_t *total_bytes, uint64_t out_cap, uint32_t *ovf) {
    __shared__ uint64_t buf[2048];
    const int t = threadIdx.x;
    if (ovf && *ovf) return;                                     // every thread, before the first barrier (written below, behind the last)
    const int per = (p.nslices + 1023) / 1024, b0 = min(t * per, p.nslices), b1 = min(b0 + per, p.nslices);
    uint64_t s = 0, total;
    int bad = 0;
    for (int i = b0; i < b1; i++) { bad |= sl_bytes[i] < 0; s += (uint64_t)(sl_bytes[i] < 0 ? 0 : sl_bytes[i]); }
    uint64_t e = cb_block_scan(s, buf, &total);
    for (int i = b0; i < b1; i++) {
        const jmh_cabac_slice_desc d = p.sl[i];
        where[i].offset = (int64_t)e;
        where[i].nbytes = sl_bytes[i];
        where[i].nbins = (int64_t)(mb_off[d.first_mb + d.n_mb] - mb_off[d.first_mb]);
        e += (uint64_t)(sl_bytes[i] < 0 ? 0 : sl_bytes[i]);
    }
    const int anybad = __syncthreads_or(bad);
    if (t == 0) {
        *total_bytes = anybad ? -1 : (int64_t)total;
        if (ovf && total > out_cap) *ovf = 1u;                   // the picture's output region is too small: pack writes nothing
    }
}

__global__ __launch_bounds__(256) void k_cabac_pack(const jmh_cabac_slice_bytes *where, const uint64_t *sl_soff, const uint8_t *scratch,
                                                    uint8_t *out, uint64_t out_cap, const uint32_t *ovf) {
    if (ovf && *ovf) return;                                     // whole grid
    const jmh_cabac_slice_bytes w = where[blockIdx.x];
    const uint8_t *src = scratch + sl_soff[blockIdx.x];
    for (int64_t k = (int64_t)blockIdx.y * 256 + threadIdx.x; k < w.nbytes; k += 256 * CB_PACK_Y)
        if ((uint64_t)(w.offset + k) < out_cap) out[w.offset + k] = src[k];
}

// ---- host side ----------------------------------------------------------------------------------
struct jmh_cabac_state {
    hipStream_t st = nullptr;
    int nmb = 0;
    jmh_mb_result *d_res = nullptr;        // unit seam: the caller's results
    jmh_cabac_slice_desc *d_sl = nullptr;
    jmh_cabac_slice_bytes *d_where = nullptr;
    jmh_cabac_slice_bytes *h_where = nullptr;   // pinned: where[nmb], then the total and the two counts
    uint16_t *d_unit = nullptr;
    uint32_t *d_bins = nullptr;
    int32_t *d_slice = nullptr;
    uint64_t *d_off = nullptr, *d_soff = nullptr, *d_totals = nullptr;
    int64_t *d_slbytes = nullptr, *d_total = nullptr;
    uint16_t *d_rec = nullptr;
    size_t rec_cap = 0;                    // records
    uint8_t *d_scratch = nullptr, *d_out = nullptr;
    size_t scratch_cap = 0, out_cap = 0;   // bytes
    std::vector<void *> retired;           // outgrown buffers: freed with the state (hipFree would wait for the device)
    jmh_split_state *split = nullptr;      // the split coder's buffers (jmh_cabac_split.hip), created on first use
    jmh_cabac_split_info last = {};        // what the last synchronous call did
};

#define CBCHK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "jmhip: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return JMH_E_HIP;                                                     \
        }                                                                         \
    } while (0)

void jmh_cabac_split_last(const jmh_cabac_state *s, jmh_cabac_split_info *out) {
    *out = s ? s->last : jmh_cabac_split_info{};
}

void jmh_cabac_free(jmh_cabac_state *s) {
    if (!s) return;
    if (s->st) (void)hipStreamSynchronize(s->st);
    void *bufs[] = {s->d_res, s->d_sl, s->d_where, s->d_unit, s->d_bins, s->d_slice, s->d_off, s->d_soff, s->d_totals, s->d_slbytes,
                    s->d_total, s->d_rec, s->d_scratch, s->d_out};
    for (void *p : bufs) if (p) (void)hipFree(p);
    for (void *p : s->retired) (void)hipFree(p);
    if (s->h_where) (void)hipHostFree(s->h_where);
    jmh_split_free(s->split);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

static int cb_setup(jmh_cabac_state *s, int nmb) {
    if (!s->st) CBCHK(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
    if (s->nmb) return JMH_OK;
#define CBALLOC(p, bytes) do { if (hipMalloc((void **)&(p), (bytes)) != hipSuccess) return JMH_E_OOM; } while (0)
    CBALLOC(s->d_unit, (size_t)nmb * 32 * sizeof(uint16_t));
    CBALLOC(s->d_bins, (size_t)nmb * sizeof(uint32_t));
    CBALLOC(s->d_slice, (size_t)nmb * sizeof(int32_t));
    CBALLOC(s->d_off, ((size_t)nmb + 1) * sizeof(uint64_t));
    CBALLOC(s->d_soff, ((size_t)nmb + 1) * sizeof(uint64_t));    // at most nmb slices
    CBALLOC(s->d_totals, 2 * sizeof(uint64_t));
    CBALLOC(s->d_slbytes, (size_t)nmb * sizeof(int64_t));
    CBALLOC(s->d_total, sizeof(int64_t));
    CBALLOC(s->d_sl, (size_t)nmb * sizeof(jmh_cabac_slice_desc));
    CBALLOC(s->d_where, (size_t)nmb * sizeof(jmh_cabac_slice_bytes));
#undef CBALLOC
    if (hipHostMalloc((void **)&s->h_where, ((size_t)nmb + 2) * sizeof(jmh_cabac_slice_bytes), hipHostMallocDefault) != hipSuccess) return JMH_E_OOM;
    s->nmb = nmb;
    return JMH_OK;
}

// a device buffer of at least `need` bytes; an outgrown one is retired, not freed
static int cb_grow(jmh_cabac_state *s, void **buf, size_t *cap_bytes, size_t need, size_t floor_bytes) {
    if (need <= *cap_bytes) return JMH_OK;
    if (*buf) s->retired.push_back(*buf);
    *buf = nullptr; *cap_bytes = 0;
    const size_t want = need + need / 2 > floor_bytes ? need + need / 2 : floor_bytes;
    if (hipMalloc(buf, want) != hipSuccess) return JMH_E_OOM;
    *cap_bytes = want;
    return JMH_OK;
}

// raster runs covering the picture
int jmh_cabac_check(int nmb, int n, const jmh_cabac_slice_desc *slices) {
    if (n <= 0 || n > nmb || !slices) return JMH_E_INVALID_ARG;
    int next = 0;
    for (int i = 0; i < n; i++) {
        const jmh_cabac_slice_desc &d = slices[i];
        if (d.first_mb != next || d.n_mb <= 0 || d.n_mb > nmb - next) return JMH_E_INVALID_ARG;
        if (d.slice_type != JMH_P_SLICE && d.slice_type != JMH_I_SLICE) return JMH_E_INVALID_ARG;
        if (d.slice_qp < 0 || d.slice_qp > 51) return JMH_E_INVALID_ARG;
        next += d.n_mb;
    }
    return next == nmb ? JMH_OK : JMH_E_INVALID_ARG;
}

// the enqueue half in three parts; between them the synchronous call reads the counts back and sizes
// its buffers, the coded pictures' enqueue queues them back to back against capacities decided before
static int cb_enqueue_count(jmh_cabac_state *s, const CbPic &p, uint64_t *d_totals, uint64_t rec_cap, uint64_t scratch_cap, uint32_t *d_ovf) {
    const int grid = (p.nmb + CB_WAVES - 1) / CB_WAVES;
    hipLaunchKernelGGL(k_cabac_count, dim3(grid), dim3(64 * CB_WAVES), 0, s->st, p, s->d_unit, s->d_bins, s->d_slice);
    CBCHK(hipGetLastError());
    hipLaunchKernelGGL(k_cabac_scan, dim3(1), dim3(1024), 0, s->st, p, s->d_bins, s->d_off, s->d_soff, d_totals, rec_cap, scratch_cap, d_ovf);
    CBCHK(hipGetLastError());
    return JMH_OK;
}
// chunk_bins > 0: the split coder's launches stand in k_cabac_code's place; nbins > 0: the picture's counted bins
static int cb_enqueue_code(jmh_cabac_state *s, const CbPic &p, jmh_cabac_slice_bytes *d_where, int64_t *d_total, uint64_t out_cap,
                           uint32_t *d_ovf, int chunk_bins, uint64_t nbins) {
    const int grid = (p.nmb + CB_WAVES - 1) / CB_WAVES;
    hipLaunchKernelGGL(k_cabac_bins, dim3(grid), dim3(64 * CB_WAVES), 0, s->st, p, s->d_unit, s->d_slice, s->d_off, s->d_rec,
                       (uint64_t)(s->rec_cap / sizeof(uint16_t)), d_ovf);
    CBCHK(hipGetLastError());
    if (chunk_bins > 0) {
        const int r = jmh_split_enqueue(&s->split, s->st, p.sl, p.nslices, s->d_off, s->d_soff, s->d_rec,
                                        (uint64_t)(s->rec_cap / sizeof(uint16_t)), s->d_scratch, s->d_slbytes, d_ovf, chunk_bins, nbins != 0);
        if (r) return r;
    } else {
        hipLaunchKernelGGL(k_cabac_code, dim3(p.nslices), dim3(64), 0, s->st, p, s->d_off, s->d_soff, s->d_rec, s->d_scratch, s->d_slbytes, d_ovf);
        CBCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cabac_where, dim3(1), dim3(1024), 0, s->st, p, s->d_off, s->d_slbytes, d_where, d_total, out_cap, d_ovf);
    CBCHK(hipGetLastError());
    return JMH_OK;
}
static int cb_enqueue_pack(jmh_cabac_state *s, int n, const jmh_cabac_slice_bytes *d_where, uint8_t *d_out, uint64_t out_cap, const uint32_t *d_ovf) {
    hipLaunchKernelGGL(k_cabac_pack, dim3(n, CB_PACK_Y), dim3(256), 0, s->st, d_where, s->d_soff, s->d_scratch, d_out, out_cap, d_ovf);
    CBCHK(hipGetLastError());
    return JMH_OK;
}

// Capacities of the coder's shared buffers for a picture of out_cap output bytes: JMH_CODED_BINS_PER_BYTE
// bins per output byte (a bypass bin costs one bit and a context-coded bin less, so a picture holds
// somewhat more than 8 bins per byte; 10 is a margin, not a measurement), and the scratch that
// holds every slice's bound for that many bins
#define JMH_CODED_BINS_PER_BYTE 10
int jmh_cabac_enqueue(jmh_cabac_state **state, const jmh_mb_result *d_res, hipEvent_t after, int mbw, int mbh, int t8mode, int cip, int n,
                      const jmh_writer_job *job, hipStream_t *stream, int chunk_bins) {
    const int nmb = mbw * mbh;
    if (!*state) *state = new jmh_cabac_state();
    jmh_cabac_state *s = *state;
    int r = cb_setup(s, nmb);
    if (r) return r;
    *stream = s->st;
    const size_t rec_need = job->out_cap * JMH_CODED_BINS_PER_BYTE * sizeof(uint16_t);
    const size_t scr_need = (size_t)JMC_SLICE_MAX_BYTES(job->out_cap * JMH_CODED_BINS_PER_BYTE) + 4 * (size_t)nmb;
    if ((r = cb_grow(s, (void **)&s->d_rec, &s->rec_cap, rec_need, 0))) return r;
    if ((r = cb_grow(s, (void **)&s->d_scratch, &s->scratch_cap, scr_need, 0))) return r;
    CBCHK(hipStreamWaitEvent(s->st, after, 0));
    CBCHK(hipMemcpyAsync(job->d_sl, job->h_sl, (size_t)n * sizeof(jmh_cabac_slice_desc), hipMemcpyHostToDevice, s->st));
    CBCHK(hipMemsetAsync(job->d_meta, 0, JMH_WRITER_META_BYTES, s->st));
    CbPic p;
    p.res = d_res; p.mbw = mbw; p.mbh = mbh; p.t8mode = t8mode; p.cip = cip; p.nmb = nmb; p.nslices = n;
    p.sl = (const jmh_cabac_slice_desc *)job->d_sl;
    uint32_t *ovf = (uint32_t *)(job->d_meta + 1);
    if ((r = cb_enqueue_count(s, p, job->d_meta + 5, (uint64_t)(s->rec_cap / sizeof(uint16_t)), (uint64_t)s->scratch_cap, ovf))) return r;
    if ((r = cb_enqueue_code(s, p, (jmh_cabac_slice_bytes *)job->d_where, (int64_t *)job->d_meta, (uint64_t)job->out_cap, ovf, chunk_bins, 0))) return r;
    return cb_enqueue_pack(s, n, (const jmh_cabac_slice_bytes *)job->d_where, job->d_out, (uint64_t)job->out_cap, ovf);
}

int jmh_cabac_run(jmh_cabac_state **state, const jmh_mb_result *d_res, const jmh_mb_result *h_res, hipEvent_t after, int mbw, int mbh,
                  int t8mode, int cip, int n, const jmh_cabac_slice_desc *slices, uint8_t *out, size_t cap, jmh_cabac_slice_bytes *where,
                  int chunk_bins) {
    const int nmb = mbw * mbh;
    if (*state) (*state)->last = jmh_cabac_split_info{};
    if (!where || (!d_res && !h_res)) return JMH_E_INVALID_ARG;
    int r = jmh_cabac_check(nmb, n, slices);
    if (r) return r;
    if (!*state) *state = new jmh_cabac_state();
    jmh_cabac_state *s = *state;
    if ((r = cb_setup(s, nmb))) return r;
    if (h_res) {
        if (!s->d_res && hipMalloc((void **)&s->d_res, (size_t)nmb * sizeof(jmh_mb_result)) != hipSuccess) return JMH_E_OOM;
        CBCHK(hipMemcpyAsync(s->d_res, h_res, (size_t)nmb * sizeof(jmh_mb_result), hipMemcpyHostToDevice, s->st));
        d_res = s->d_res;
    } else if (after) CBCHK(hipStreamWaitEvent(s->st, after, 0));
    CBCHK(hipMemcpyAsync(s->d_sl, slices, (size_t)n * sizeof(jmh_cabac_slice_desc), hipMemcpyHostToDevice, s->st));
    CbPic p;
    p.res = d_res; p.mbw = mbw; p.mbh = mbh; p.t8mode = t8mode; p.cip = cip; p.nmb = nmb; p.nslices = n; p.sl = s->d_sl;
    uint64_t *h_totals = (uint64_t *)(s->h_where + nmb + 1);     // two counts behind where[] and the total
    if ((r = cb_enqueue_count(s, p, s->d_totals, 0, 0, nullptr))) return r;
    CBCHK(hipMemcpyAsync(h_totals, s->d_totals, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s->st));
    CBCHK(hipStreamSynchronize(s->st));      // the writer's own stream only
    const uint64_t nbins = h_totals[0], nscratch = h_totals[1];
    if (nbins == 0 || nbins > (uint64_t)nmb * JMC_MB_MAX_BINS) return JMH_E_STATE;   // the documented bound
    if ((r = cb_grow(s, (void **)&s->d_rec, &s->rec_cap, (size_t)nbins * sizeof(uint16_t), (size_t)nmb * 256))) return r;
    if ((r = cb_grow(s, (void **)&s->d_scratch, &s->scratch_cap, (size_t)nscratch, (size_t)nmb * 128))) return r;
    if ((r = cb_enqueue_code(s, p, s->d_where, s->d_total, 0, nullptr, chunk_bins, nbins))) return r;
    CBCHK(hipMemcpyAsync(s->h_where, s->d_where, (size_t)n * sizeof(jmh_cabac_slice_bytes), hipMemcpyDeviceToHost, s->st));
    CBCHK(hipMemcpyAsync(s->h_where + nmb, s->d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s->st));
    CBCHK(hipStreamSynchronize(s->st));
    if (chunk_bins > 0) {
        const uint64_t *t = jmh_split_totals(s->split);
        s->last.chunk_bins = chunk_bins; s->last.chunks = (int64_t)t[0]; s->last.longest_slice_chunks = (int64_t)t[2];
        s->last.scratch_bytes = (int64_t)jmh_split_bytes(s->split);
    }
    const int64_t total = s->h_where[nmb].offset;
    if (total <= 0 || (uint64_t)total > nscratch) return JMH_E_STATE;
    memcpy(where, s->h_where, (size_t)n * sizeof(jmh_cabac_slice_bytes));
    if (!out || (size_t)total > cap) return JMH_E_INVALID_ARG;    // before anything is copied: out untouched
    if ((r = cb_grow(s, (void **)&s->d_out, &s->out_cap, (size_t)total, (size_t)nmb * 64))) return r;
    if ((r = cb_enqueue_pack(s, n, s->d_where, s->d_out, (uint64_t)total, nullptr))) return r;
    CBCHK(hipMemcpyAsync(out, s->d_out, (size_t)total, hipMemcpyDeviceToHost, s->st));
    CBCHK(hipStreamSynchronize(s->st));
    return JMH_OK;
}
