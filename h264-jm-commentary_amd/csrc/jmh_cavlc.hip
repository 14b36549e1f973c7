// jmh_cavlc.hip — CAVLC slice data written on the device (include/jmhip_cavlc.h): the
// code-value half of CAVLC (jmh_cavlc_write.h, shared with the host) plus a bit-exact parallel packer,
// in three passes on a stream of the writer's own:
//
//   k_cavlc_count   one wave per macroblock; lane u < JMW_UNITS counts the bits of unit u (0: header
//                   syntax, 1..27: the residual blocks) with the counting sink; the wave finds the
//                   pending mb_skip_run (64 predecessors per ballot) and the macroblock's slice.
//                   Leaves per unit bits, per macroblock bits / run / slice.
//   k_cavlc_scan    one workgroup: exclusive scan of the macroblock bits over the picture, from it
//                   every slice's bit and byte count, and the exclusive scan of the slices' bytes
//                   (where[], total).  The scan is segmented by subtraction: a macroblock's offset
//                   inside its slice is E[a] - E[first_mb of the slice].
//   k_cavlc_write   one wave per macroblock; a wave prefix sum of the unit bits gives every lane its
//                   bit offset, the lanes OR their unit's codes into the wave's LDS stage (shifted by
//                   the macroblock's global bit offset mod 32, so that stage words are output
//                   dwords), then the stage is flushed: whole dwords by plain vector stores, the
//                   first and last dword (shared with neighbouring macroblocks / slices) by atomicOr
//                   into the zeroed output.  A slice's first macroblock also stages the header's lead
//                   bits, its last one the rbsp_stop_one_bit (the alignment zeros are the zeroed
//                   buffer).  Output words are byte-swapped: bits are MSB first within bytes.
//
// Two callers queue these passes.  The synchronous entry points (jmh_cavlc_run) read the byte count
// back between scan and write (a copy on the writer's stream, which only that stream is waited for)
// and size the output from it.  A coded picture (jmh_cavlc_enqueue) queues all three
// behind the picture's last macroblock with no host wait: the output region has a capacity decided
// before, k_cavlc_scan sets the picture's overflow word when the counted bytes exceed it, and
// k_cavlc_write then writes nothing -- a device-side predicate, no store out of bounds; the host
// sees the word at the pop.  One-macroblock-per-lane was not built: it would leave a 1080p picture at 128 waves
// of fully divergent serial work (not measured).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#define JMW_OR(p, v) atomicOr((p), (v))
#include "jmh_cavlc_write.h"
#include "jmh_cavlc.h"

#define CV_WAVES 4                                   // macroblocks (waves) per workgroup
#define CV_STAGE ((JMW_MB_MAX_BITS + 31 + 7) / 32 + 2)   // stage words: shift (31) + lead bits (7) + the macroblock

struct CvPic {
    const jmh_mb_result *res;
    int mbw, mbh, t8mode, cip, nmb, nslices;
    const jmh_slice_desc *sl;
};

__device__ __forceinline__ jmw_pic cv_pic(const CvPic &p) {
    jmw_pic q;
    q.res = p.res; q.mbw = p.mbw; q.mbh = p.mbh; q.t8mode = p.t8mode; q.cip = p.cip;
    return q;
}
__device__ __forceinline__ jmw_slice cv_slice(const jmh_slice_desc &d) {
    jmw_slice s;
    s.first_mb = d.first_mb; s.end_mb = d.first_mb + d.n_mb; s.slice_p = d.slice_type == JMH_P_SLICE;
    return s;
}

__global__ __launch_bounds__(64 * CV_WAVES) void k_cavlc_count(CvPic p, uint16_t *unit_bits, uint32_t *mb_bits, int32_t *mb_run,
                                                               int32_t *mb_slice) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * CV_WAVES + (threadIdx.x >> 6);
    if (a >= p.nmb) return;                                      // whole wave
    int lo = 0, hi = p.nslices - 1;                              // the slice holding a (descriptors tile the picture)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.sl[mid].first_mb <= a) lo = mid; else hi = mid - 1;
    }
    const jmw_slice sl = cv_slice(p.sl[lo]);
    const jmw_pic pic = cv_pic(p);
    // pending mb_skip_run: the P_Skip macroblocks of the slice right before a
    int run = 0;
    if (sl.slice_p)
        for (int b = a - 1; b >= sl.first_mb; b -= 64) {
            const int t = b - lane;
            const bool stop = t < sl.first_mb || !jmw_is_skip(p.res + t, 1);
            const unsigned long long m = __ballot(stop);
            if (m) { run += __builtin_ctzll(m); break; }
            run += 64;
        }
    jmw_sink s;
    s.w = nullptr; s.pos = 0;
    if (lane < JMW_UNITS) jmw_unit(&s, &pic, &sl, a, lane, run);
    if (lane < 32) unit_bits[(size_t)a * 32 + lane] = (uint16_t)s.pos;
    uint32_t sum = s.pos;
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) { mb_bits[a] = sum; mb_run[a] = run; mb_slice[a] = lo; }
}

// exclusive scan of v over the 1024 threads of the workgroup (Hillis-Steele in LDS); *total: the sum
__device__ uint64_t cv_block_scan(uint64_t v, uint64_t *buf, uint64_t *total) {
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

// ovf (may be null): set when the counted bytes exceed cap_bytes, the capacity decided before the
// enqueue; the write pass of that picture then writes nothing (coded pictures)
__global__ __launch_bounds__(1024) void k_cavlc_scan(CvPic p, const uint32_t *mb_bits, uint64_t *mb_off, jmh_slice_bytes *where,
                                                     int64_t *total_bytes, uint64_t cap_bytes, uint32_t *ovf) {
    __shared__ uint64_t buf[2048];
    const int t = threadIdx.x;
    uint64_t total;
    {   // macroblock bits -> mb_off[a] = bits of the picture's macroblocks before a; mb_off[nmb] = all
        const int per = (p.nmb + 1023) / 1024, b0 = min(t * per, p.nmb), b1 = min(b0 + per, p.nmb);
        uint64_t s = 0;
        for (int a = b0; a < b1; a++) s += mb_bits[a];
        uint64_t e = cv_block_scan(s, buf, &total);
        for (int a = b0; a < b1; a++) { mb_off[a] = e; e += mb_bits[a]; }
        if (t == 0) mb_off[p.nmb] = total;
    }
    __syncthreads();
    {   // slices: bits, bytes (the stop bit makes it nbits / 8 + 1), byte offsets
        const int per = (p.nslices + 1023) / 1024, b0 = min(t * per, p.nslices), b1 = min(b0 + per, p.nslices);
        uint64_t s = 0;
        for (int i = b0; i < b1; i++) {
            const jmh_slice_desc d = p.sl[i];
            const int64_t nbits = d.lead_nbits + (int64_t)(mb_off[d.first_mb + d.n_mb] - mb_off[d.first_mb]);
            where[i].nbits = nbits;
            where[i].nbytes = nbits / 8 + 1;
            s += (uint64_t)(nbits / 8 + 1);
        }
        uint64_t e = cv_block_scan(s, buf, &total);
        for (int i = b0; i < b1; i++) { where[i].offset = (int64_t)e; e += (uint64_t)where[i].nbytes; }
        if (t == 0) {
            *total_bytes = (int64_t)total;
            if (ovf && total > cap_bytes) *ovf = 1u;
        }
    }
}

__global__ __launch_bounds__(64 * CV_WAVES) void k_cavlc_write(CvPic p, const uint16_t *unit_bits, const uint32_t *mb_bits,
                                                               const int32_t *mb_run, const int32_t *mb_slice, const uint64_t *mb_off,
                                                               const jmh_slice_bytes *where, uint32_t *out, uint64_t out_words,
                                                               const uint32_t *ovf) {
    __shared__ uint32_t stage_all[CV_WAVES][CV_STAGE];
    if (ovf && *ovf) return;                                     // the whole grid: the counted bytes exceed the capacity
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = blockIdx.x * CV_WAVES + wave;
    const bool act = a < p.nmb;                                  // wave-uniform; every wave reaches the barriers
    uint32_t *stage = stage_all[wave];
    uint64_t base = 0;
    int nwords = 0;
    if (act) {
        const int si = mb_slice[a];
        const jmh_slice_desc d = p.sl[si];
        const jmw_slice sl = cv_slice(d);
        const bool first = a == sl.first_mb, last = a == sl.end_mb - 1;
        // the macroblock's first bit in the output, and the first bit this wave stages
        const uint64_t g = 8ull * (uint64_t)where[si].offset + (uint64_t)d.lead_nbits + (mb_off[a] - mb_off[sl.first_mb]);
        const uint64_t g0 = first ? g - (uint64_t)d.lead_nbits : g;
        const uint32_t sh = (uint32_t)(g0 & 31), lead = first ? (uint32_t)d.lead_nbits : 0u;
        const uint32_t nb = mb_bits[a], tot = sh + lead + nb + (last ? 1u : 0u);
        base = g0 >> 5;
        nwords = (int)((tot + 31) >> 5);
        if (nwords > CV_STAGE) nwords = 0;                       // cannot happen (JMW_MB_MAX_BITS); never write past the stage
        for (int k = lane; k < nwords; k += 64) stage[k] = 0;
    }
    __syncthreads();
    if (act && nwords) {
        const int si = mb_slice[a];
        const jmh_slice_desc d = p.sl[si];
        const jmw_slice sl = cv_slice(d);
        const jmw_pic pic = cv_pic(p);
        const bool first = a == sl.first_mb, last = a == sl.end_mb - 1;
        const uint64_t g = 8ull * (uint64_t)where[si].offset + (uint64_t)d.lead_nbits + (mb_off[a] - mb_off[sl.first_mb]);
        const uint32_t lead = first ? (uint32_t)d.lead_nbits : 0u;
        const uint32_t sh = (uint32_t)((g - lead) & 31);
        const uint32_t ub = lane < 32 ? unit_bits[(size_t)a * 32 + lane] : 0u;
        uint32_t incl = ub;                                      // inclusive wave prefix sum of the unit bits
        for (int o = 1; o < 32; o <<= 1) {
            const uint32_t x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        jmw_sink s;
        s.w = stage;
        if (lane == 0 && first) { s.pos = sh; jmw_put(&s, d.lead_bits, (int)lead); }
        s.pos = sh + lead + incl - ub;
        if (lane < JMW_UNITS && ub) jmw_unit(&s, &pic, &sl, a, lane, mb_run[a]);
        if (lane == 63 && last) { s.pos = sh + lead + mb_bits[a]; jmw_put(&s, 1, 1); }   // rbsp_stop_one_bit
    }
    __syncthreads();
    if (act)
        for (int k = lane; k < nwords; k += 64) {
            const uint32_t v = stage[k];
            if (base + k >= out_words) continue;                 // cannot happen: the buffer holds the counted bytes
            const uint32_t w = __builtin_bswap32(v);
            if (k == 0 || k == nwords - 1) { if (v) atomicOr(&out[base + k], w); }
            else out[base + k] = w;
        }
}

// ---- host side ----------------------------------------------------------------------------------
struct jmh_cavlc_state {
    hipStream_t st = nullptr;
    int nmb = 0, ncap = 0;
    jmh_mb_result *d_res = nullptr;        // unit seam: the caller's results
    jmh_slice_desc *d_sl = nullptr;
    jmh_slice_bytes *d_where = nullptr;
    jmh_slice_bytes *h_where = nullptr;    // pinned: where[ncap] then the total
    uint16_t *d_unit = nullptr;
    uint32_t *d_bits = nullptr;
    int32_t *d_run = nullptr, *d_slice = nullptr;
    uint64_t *d_off = nullptr;
    int64_t *d_total = nullptr;
    uint32_t *d_out = nullptr;
    size_t out_cap = 0;                    // bytes
    std::vector<void *> retired;           // outgrown output buffers: freed with the state (hipFree would wait for the device)
};

#define CVCHK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "jmhip: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return JMH_E_HIP;                                                     \
        }                                                                         \
    } while (0)

void jmh_cavlc_free(jmh_cavlc_state *s) {
    if (!s) return;
    if (s->st) (void)hipStreamSynchronize(s->st);
    void *bufs[] = {s->d_res, s->d_sl, s->d_where, s->d_unit, s->d_bits, s->d_run, s->d_slice, s->d_off, s->d_total, s->d_out};
    for (void *p : bufs) if (p) (void)hipFree(p);
    for (void *p : s->retired) (void)hipFree(p);
    if (s->h_where) (void)hipHostFree(s->h_where);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

static int cv_setup(jmh_cavlc_state *s, int nmb, int n) {
    // default priority: the highest one made the call slower (1.82 vs 1.70 ms at 1080p)
    if (!s->st) CVCHK(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
#define CVALLOC(p, bytes) do { if (hipMalloc((void **)&(p), (bytes)) != hipSuccess) return JMH_E_OOM; } while (0)
    if (!s->nmb) {
        CVALLOC(s->d_unit, (size_t)nmb * 32 * sizeof(uint16_t));
        CVALLOC(s->d_bits, (size_t)nmb * sizeof(uint32_t));
        CVALLOC(s->d_run, (size_t)nmb * sizeof(int32_t));
        CVALLOC(s->d_slice, (size_t)nmb * sizeof(int32_t));
        CVALLOC(s->d_off, ((size_t)nmb + 1) * sizeof(uint64_t));
        CVALLOC(s->d_total, sizeof(int64_t));
        s->nmb = nmb;
    }
    if (n > s->ncap) {                       // at most nmb slices: sized once
        if (s->d_sl) { (void)hipStreamSynchronize(s->st); (void)hipFree(s->d_sl); (void)hipFree(s->d_where); (void)hipHostFree(s->h_where); }
        s->d_sl = nullptr; s->d_where = nullptr; s->h_where = nullptr; s->ncap = 0;
        CVALLOC(s->d_sl, (size_t)nmb * sizeof(jmh_slice_desc));
        CVALLOC(s->d_where, (size_t)nmb * sizeof(jmh_slice_bytes));
        if (hipHostMalloc((void **)&s->h_where, ((size_t)nmb + 1) * sizeof(jmh_slice_bytes), hipHostMallocDefault) != hipSuccess) return JMH_E_OOM;
        s->ncap = nmb;
    }
#undef CVALLOC
    return JMH_OK;
}

// raster runs covering the picture
int jmh_cavlc_check(int nmb, int n, const jmh_slice_desc *slices) {
    if (n <= 0 || n > nmb || !slices) return JMH_E_INVALID_ARG;
    int next = 0;
    for (int i = 0; i < n; i++) {
        const jmh_slice_desc &d = slices[i];
        if (d.first_mb != next || d.n_mb <= 0 || d.n_mb > nmb - next) return JMH_E_INVALID_ARG;
        if (d.slice_type != JMH_P_SLICE && d.slice_type != JMH_I_SLICE) return JMH_E_INVALID_ARG;
        if (d.lead_nbits < 0 || d.lead_nbits > 7) return JMH_E_INVALID_ARG;
        next += d.n_mb;
    }
    return next == nmb ? JMH_OK : JMH_E_INVALID_ARG;
}

// the enqueue half, first part: count and scan.  where / total / ovf are the picture's own (device)
static int cv_enqueue_count(jmh_cavlc_state *s, const CvPic &p, jmh_slice_bytes *d_where, int64_t *d_total, uint64_t cap_bytes, uint32_t *d_ovf) {
    const int grid = (p.nmb + CV_WAVES - 1) / CV_WAVES;
    hipLaunchKernelGGL(k_cavlc_count, dim3(grid), dim3(64 * CV_WAVES), 0, s->st, p, s->d_unit, s->d_bits, s->d_run, s->d_slice);
    CVCHK(hipGetLastError());
    hipLaunchKernelGGL(k_cavlc_scan, dim3(1), dim3(1024), 0, s->st, p, s->d_bits, s->d_off, d_where, d_total, cap_bytes, d_ovf);
    CVCHK(hipGetLastError());
    return JMH_OK;
}
// ... second part: the write pass into d_out (zero_bytes of it zeroed first: whole dwords)
static int cv_enqueue_write(jmh_cavlc_state *s, const CvPic &p, const jmh_slice_bytes *d_where, uint32_t *d_out, size_t zero_bytes,
                            const uint32_t *d_ovf) {
    const int grid = (p.nmb + CV_WAVES - 1) / CV_WAVES;
    CVCHK(hipMemsetAsync(d_out, 0, zero_bytes, s->st));
    hipLaunchKernelGGL(k_cavlc_write, dim3(grid), dim3(64 * CV_WAVES), 0, s->st, p, s->d_unit, s->d_bits, s->d_run, s->d_slice, s->d_off,
                       d_where, d_out, (uint64_t)(zero_bytes / 4), d_ovf);
    CVCHK(hipGetLastError());
    return JMH_OK;
}

int jmh_cavlc_enqueue(jmh_cavlc_state **state, const jmh_mb_result *d_res, hipEvent_t after, int mbw, int mbh, int t8mode, int cip, int n,
                      const jmh_writer_job *job, hipStream_t *stream) {
    const int nmb = mbw * mbh;
    if (!*state) *state = new jmh_cavlc_state();
    jmh_cavlc_state *s = *state;
    int r = cv_setup(s, nmb, n);
    if (r) return r;
    *stream = s->st;
    CVCHK(hipStreamWaitEvent(s->st, after, 0));
    CVCHK(hipMemcpyAsync(job->d_sl, job->h_sl, (size_t)n * sizeof(jmh_slice_desc), hipMemcpyHostToDevice, s->st));
    CVCHK(hipMemsetAsync(job->d_meta, 0, JMH_WRITER_META_BYTES, s->st));
    CvPic p;
    p.res = d_res; p.mbw = mbw; p.mbh = mbh; p.t8mode = t8mode; p.cip = cip; p.nmb = nmb; p.nslices = n; p.sl = (const jmh_slice_desc *)job->d_sl;
    uint32_t *ovf = (uint32_t *)(job->d_meta + 1);
    if ((r = cv_enqueue_count(s, p, (jmh_slice_bytes *)job->d_where, (int64_t *)job->d_meta, (uint64_t)job->out_cap, ovf))) return r;
    return cv_enqueue_write(s, p, (const jmh_slice_bytes *)job->d_where, (uint32_t *)job->d_out, job->out_cap, ovf);
}

int jmh_cavlc_run(jmh_cavlc_state **state, const jmh_mb_result *d_res, const jmh_mb_result *h_res, hipEvent_t after, int mbw, int mbh,
                  int t8mode, int cip, int n, const jmh_slice_desc *slices, uint8_t *out, size_t cap, jmh_slice_bytes *where) {
    const int nmb = mbw * mbh;
    if (!where || (!d_res && !h_res)) return JMH_E_INVALID_ARG;
    int r = jmh_cavlc_check(nmb, n, slices);
    if (r) return r;
    if (!*state) *state = new jmh_cavlc_state();
    jmh_cavlc_state *s = *state;
    if ((r = cv_setup(s, nmb, n))) return r;
    if (h_res) {
        if (!s->d_res && hipMalloc((void **)&s->d_res, (size_t)nmb * sizeof(jmh_mb_result)) != hipSuccess) return JMH_E_OOM;
        CVCHK(hipMemcpyAsync(s->d_res, h_res, (size_t)nmb * sizeof(jmh_mb_result), hipMemcpyHostToDevice, s->st));
        d_res = s->d_res;
    } else if (after) CVCHK(hipStreamWaitEvent(s->st, after, 0));
    CVCHK(hipMemcpyAsync(s->d_sl, slices, (size_t)n * sizeof(jmh_slice_desc), hipMemcpyHostToDevice, s->st));
    CvPic p;
    p.res = d_res; p.mbw = mbw; p.mbh = mbh; p.t8mode = t8mode; p.cip = cip; p.nmb = nmb; p.nslices = n; p.sl = s->d_sl;
    // the synchronous call sizes its buffer from the count: the host is the collect half between the two enqueues
    if ((r = cv_enqueue_count(s, p, s->d_where, s->d_total, 0, nullptr))) return r;
    CVCHK(hipMemcpyAsync(s->h_where, s->d_where, (size_t)n * sizeof(jmh_slice_bytes), hipMemcpyDeviceToHost, s->st));
    CVCHK(hipMemcpyAsync(s->h_where + n, s->d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s->st));
    CVCHK(hipStreamSynchronize(s->st));      // the writer's own stream only
    memcpy(where, s->h_where, (size_t)n * sizeof(jmh_slice_bytes));
    const int64_t total = s->h_where[n].offset;
    if (total <= 0 || total > (int64_t)nmb * (JMW_MB_MAX_BITS / 8) + 2 * (int64_t)n) return JMH_E_STATE;   // the documented bound
    if (!out || (size_t)total > cap) return JMH_E_INVALID_ARG;    // before the write pass: out untouched
    const size_t need = ((size_t)total + 3) & ~(size_t)3;
    if (need > s->out_cap) {
        if (s->d_out) s->retired.push_back(s->d_out);
        s->d_out = nullptr; s->out_cap = 0;
        const size_t want = need * 2 > (size_t)nmb * 64 ? need * 2 : (size_t)nmb * 64;
        if (hipMalloc((void **)&s->d_out, want) != hipSuccess) return JMH_E_OOM;
        s->out_cap = want;
    }
    if ((r = cv_enqueue_write(s, p, s->d_where, s->d_out, need, nullptr))) return r;
    CVCHK(hipMemcpyAsync(out, s->d_out, (size_t)total, hipMemcpyDeviceToHost, s->st));
    CVCHK(hipStreamSynchronize(s->st));
    return JMH_OK;
}
