// jmh_nal.hip — NAL units finished on the device (include/jmhip_nal.h): the kernels
// around the shared core of jmh_nal.h.  Four launches on one stream, no host wait between them:
//   k_nal_plan   one workgroup: checks every unit's ranges, gives each unit its chunks (d_cs), sums the bins
//   k_nal_count  a wave per (unit, chunk): the chunk's record, from ballots of its tiles; four tiles
//                are loaded at once, a dword per lane, and handed to the lanes with a shuffle
//   k_nal_scan   one workgroup: every chunk's carry, size and offset, every unit's offset and size,
//                the zero words, the total, the overflow word
//   k_nal_write  a wave per (unit, chunk): the same predicate under the chunk's carry, scattered byte
//                stores; a unit's first chunk writes its start code and header byte, the last chunk
//                of all the zero words
// The chunk grid is launched at its upper bound (sizes are known on the device only); a wave past
// the planned chunks returns at once.  Nothing is read or written once the overflow word is set.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "../../include/jmhip.h"
#include "jmh_nal.h"

#define NAL_WAVES 4                   // waves of a count / write workgroup
#define NAL_SERIAL 256                // threads of the plan / scan workgroup
#define NAL_MIN(a, b) ((a) < (b) ? (a) : (b))

struct NalArgs {
    int n;
    const jmh_nal_head *heads;
    const uint8_t *payload;
    int64_t payload_cap;
    const int64_t *where;
    const uint64_t *wmeta;
    int64_t bins;
    int sum_bins, bd, nmb;
    int32_t *cs;
    jmn_chunk *ch;
    int maxch;
    int64_t *uout;
    uint64_t *meta;
    uint8_t *out;
    int64_t out_cap;
};

// the unit of chunk c: the last u with cs[u] <= c
__device__ __forceinline__ int nal_unit_of(const int32_t *cs, int n, int c) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cs[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a unit's head and payload as one string
struct NalUnit { const uint8_t *head, *pay; int64_t hn, len; };
__device__ __forceinline__ NalUnit nal_unit(const NalArgs &a, int u) {
    NalUnit r;
    r.head = a.heads[u].bytes; r.hn = a.heads[u].nbytes;
    r.pay = a.payload + a.where[3 * u]; r.len = r.hn + a.where[3 * u + 1];
    return r;
}
// Four tiles' bytes, a dword per lane (bytes pos + 4 lane .. + 3, the first one lowest; 0 past the n
// bytes left).  Where all 256 lie in the payload, which is every load but a unit's first and a
// chunk's last, a lane loads the aligned dword that holds its first byte and, unless the payload
// is dword aligned there (wave-uniform), the next one, and funnels the two: only aligned dwords that
// hold a byte of the range are read (the payload region's size is a multiple of 4).  Else bytes.
#define NAL_QUAD (4 * JMN_TILE)
__device__ __forceinline__ uint32_t nal_load4(const NalUnit &U, int64_t pos, int n, int lane) {
    if (n == NAL_QUAD && pos >= U.hn) {
        const uintptr_t addr = (uintptr_t)(U.pay + (pos - U.hn)) + 4u * (uint32_t)lane;
        const uint32_t *p = (const uint32_t *)(addr & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)(addr & 3);
        const uint32_t lo = p[0];
        return sh ? __builtin_amdgcn_alignbyte(p[1], lo, sh) : lo;
    }
    uint32_t w = 0;
    for (int j = 0; j < 4; j++) {
        const int64_t i = pos + 4 * lane + j;
        if (4 * lane + j < n) w |= (uint32_t)(i < U.hn ? U.head[i] : U.pay[i - U.hn]) << (8 * j);
    }
    return w;
}
// tile t of the four: this lane's byte (0 past the tile's n bytes) and the tile's ballots
__device__ __forceinline__ uint32_t nal_tile(uint32_t w, int t, int n, int lane, uint64_t *nz, uint64_t *le3) {
    const uint32_t x = (uint32_t)__shfl((int)w, 16 * t + (lane >> 2), 64);
    const uint32_t v = lane < n ? (x >> (8 * (lane & 3))) & 0xffu : 0;
    *nz = __ballot(lane < n && v != 0);
    *le3 = __ballot(lane < n && v <= 3);
    return v;
}

__global__ __launch_bounds__(NAL_SERIAL) void k_nal_plan(NalArgs a) {
    __shared__ int64_t s_sum[NAL_SERIAL], s_bins[NAL_SERIAL];
    __shared__ int s_bad;
    const int t = threadIdx.x;
    if (t == 0) s_bad = a.wmeta && (uint32_t)a.wmeta[1] != 0;
    __syncthreads();
    const bool skip = s_bad != 0;                     // the writer wrote nothing: its where[] places no bytes
    const int per = (a.n + NAL_SERIAL - 1) / NAL_SERIAL, u0 = t * per, u1 = NAL_MIN(a.n, u0 + per);
    int64_t sum = 0, bins = 0;
    bool bad = false;
    if (!skip)
        for (int u = u0; u < u1; u++) {
            const int64_t off = a.where[3 * u], nb = a.where[3 * u + 1];
            const int32_t hn = a.heads[u].nbytes;
            if (off < 0 || nb < 0 || off > a.payload_cap || nb > a.payload_cap - off || hn < 0 || hn > JMH_NAL_HEAD_MAX) { bad = true; break; }
            sum += jmn_unit_chunks(hn + nb);
            if (a.sum_bins) bins += a.where[3 * u + 2];
        }
    if (bad) atomicOr(&s_bad, 1);
    s_sum[t] = sum; s_bins[t] = bins;
    __syncthreads();
    if (t == 0) {
        int64_t acc = 0, b = a.bins;
        for (int i = 0; i < NAL_SERIAL; i++) { const int64_t v = s_sum[i]; s_sum[i] = acc; acc += v; b += s_bins[i]; }
        const bool over = s_bad || acc > a.maxch;
        a.meta[0] = 0; a.meta[1] = over; a.meta[2] = 0; a.meta[3] = over ? 0 : (uint64_t)acc; a.meta[4] = (uint64_t)b;
        s_bad = over;
    }
    __syncthreads();
    if (s_bad) return;
    int64_t c = s_sum[t];
    for (int u = u0; u < u1; u++) {
        a.cs[u] = (int32_t)c;
        c += jmn_unit_chunks(a.heads[u].nbytes + a.where[3 * u + 1]);
    }
    if (u1 == a.n && u0 < u1) a.cs[a.n] = (int32_t)c;
}

__global__ __launch_bounds__(64 * NAL_WAVES) void k_nal_count(NalArgs a) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * NAL_WAVES + (threadIdx.x >> 6);
    if (c >= (int)a.meta[3]) return;
    const int u = nal_unit_of(a.cs, a.n, c);
    const NalUnit U = nal_unit(a, u);
    const int64_t start = (int64_t)(c - a.cs[u]) * JMN_CHUNK;
    const int len = (int)NAL_MIN((int64_t)JMN_CHUNK, U.len - start);
    jmn_count s;
    jmn_count_begin(&s);
    for (int p = 0; p < len; p += NAL_QUAD) {
        const int n4 = NAL_MIN(NAL_QUAD, len - p);
        const uint32_t w = nal_load4(U, start + p, n4, lane);
        for (int t = 0; t * JMN_TILE < n4; t++) {
            const int n = NAL_MIN(JMN_TILE, n4 - t * JMN_TILE);
            uint64_t nz, le3;
            nal_tile(w, t, n, lane, &nz, &le3);
            const uint64_t esc = __ballot(jmn_escape((uint32_t)((le3 >> lane) & 1), jmn_lane_L(nz, lane, s.carry)));
            jmn_count_tile(&s, nz, le3, esc, n);
        }
    }
    if (lane == 0) jmn_count_end(&s, &a.ch[c]);
}

__global__ __launch_bounds__(NAL_SERIAL) void k_nal_scan(NalArgs a) {
    __shared__ int64_t s_sum[NAL_SERIAL];
    __shared__ int64_t s_total;
    if ((uint32_t)a.meta[1]) return;
    const int t = threadIdx.x, nch = (int)a.meta[3];
    // every chunk's carry: the trailing zeros of the chunk before it in the unit, passed on through chunks of zeros
    for (int c = t; c < nch; c += NAL_SERIAL) {
        const int u = nal_unit_of(a.cs, a.n, c), c0 = a.cs[u];
        int32_t carry = 0;
        for (int j = c - 1; j >= c0; j--) {
            const jmn_chunk *p = &a.ch[j];
            if (p->lead != p->n) { carry += p->trail; break; }
            carry += p->n;
        }
        jmn_chunk *q = &a.ch[c];
        q->unit = u; q->first = c == c0; q->carry = carry;
        q->outn = q->n + q->cnt + jmn_lead_escapes(carry, q->lead, q->first_le3);
    }
    __syncthreads();
    // offsets: each thread a run of chunks
    const int per = (nch + NAL_SERIAL - 1) / NAL_SERIAL, c0 = NAL_MIN(nch, t * per), c1 = NAL_MIN(nch, c0 + per);
    int64_t sum = 0;
    for (int c = c0; c < c1; c++) sum += a.ch[c].outn + (a.ch[c].first ? JMN_UNIT_OVERHEAD : 0);
    s_sum[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t acc = 0;
        for (int i = 0; i < NAL_SERIAL; i++) { const int64_t v = s_sum[i]; s_sum[i] = acc; acc += v; }
        s_total = acc;
    }
    __syncthreads();
    int64_t o = s_sum[t];
    for (int c = c0; c < c1; c++) {
        if (a.ch[c].first) o += JMN_UNIT_OVERHEAD;
        a.ch[c].out = o;
        o += a.ch[c].outn;
    }
    __syncthreads();
    const int64_t z = jmn_zero_words((int64_t)a.meta[4], a.bd, a.nmb, s_total - 4 * (int64_t)a.n), total = s_total + 3 * z;
    for (int u = t; u < a.n; u += NAL_SERIAL) {
        const int64_t b = a.ch[a.cs[u]].out - JMN_UNIT_OVERHEAD;
        const int64_t e = u + 1 < a.n ? a.ch[a.cs[u + 1]].out - JMN_UNIT_OVERHEAD : total;
        a.uout[2 * u] = b; a.uout[2 * u + 1] = e - b;
    }
    if (t == 0) { a.meta[0] = (uint64_t)total; a.meta[2] = (uint64_t)z; a.meta[1] = total > a.out_cap; }
}

__global__ __launch_bounds__(64 * NAL_WAVES) void k_nal_write(NalArgs a) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * NAL_WAVES + (threadIdx.x >> 6);
    const int nch = (int)a.meta[3];
    if ((uint32_t)a.meta[1] || c >= nch) return;
    const jmn_chunk *q = &a.ch[c];
    const int u = q->unit;
    const NalUnit U = nal_unit(a, u);
    const int64_t start = (int64_t)(c - a.cs[u]) * JMN_CHUNK;
    const int len = q->n;
    int64_t o = q->out;
    if (q->first && lane < JMN_UNIT_OVERHEAD)
        a.out[o - JMN_UNIT_OVERHEAD + lane] = lane < 3 ? 0 : lane == 3 ? 1 : (uint8_t)((a.heads[u].nal_ref_idc << 5) | a.heads[u].nal_unit_type);
    int32_t carry = q->carry;
    for (int p = 0; p < len; p += NAL_QUAD) {
        const int n4 = NAL_MIN(NAL_QUAD, len - p);
        const uint32_t w4 = nal_load4(U, start + p, n4, lane);
        for (int t = 0; t * JMN_TILE < n4; t++) {
            const int n = NAL_MIN(JMN_TILE, n4 - t * JMN_TILE);
            uint64_t nz, le3;
            const uint32_t v = nal_tile(w4, t, n, lane, &nz, &le3);
            const bool e = jmn_escape((uint32_t)((le3 >> lane) & 1), jmn_lane_L(nz, lane, carry));
            const uint64_t esc = __ballot(e);
            if (lane < n) {
                const int64_t w = o + jmn_lane_out(esc, lane);
                if (e) a.out[w - 1] = 3;
                a.out[w] = (uint8_t)v;
            }
            o += n + __builtin_popcountll(esc);
            carry = jmn_tile_carry(nz, n, carry);
        }
    }
    if (c == nch - 1)
        for (int64_t i = lane, nz3 = 3 * (int64_t)a.meta[2]; i < nz3; i += 64) a.out[o + i] = i % 3 == 2 ? 3 : 0;
}

int jmh_nal_enqueue(hipStream_t st, const jmh_nal_job *j) {
    if (!j || j->n <= 0 || j->maxch <= 0) return JMH_E_INVALID_ARG;
    NalArgs a;
    a.n = j->n; a.heads = j->d_heads; a.payload = j->d_payload; a.payload_cap = j->payload_cap; a.where = j->d_where; a.wmeta = j->d_wmeta;
    a.bins = j->bins; a.sum_bins = j->sum_bins; a.bd = j->bd; a.nmb = j->nmb; a.cs = j->d_cs; a.ch = j->d_ch; a.maxch = j->maxch;
    a.uout = j->d_uout; a.meta = j->d_meta; a.out = j->d_out; a.out_cap = j->out_cap;
    const dim3 grid((j->maxch + NAL_WAVES - 1) / NAL_WAVES), block(64 * NAL_WAVES);
    hipLaunchKernelGGL(k_nal_plan, dim3(1), dim3(NAL_SERIAL), 0, st, a);
    hipLaunchKernelGGL(k_nal_count, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_nal_scan, dim3(1), dim3(NAL_SERIAL), 0, st, a);
    hipLaunchKernelGGL(k_nal_write, grid, block, 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fprintf(stderr, "jmhip: the NAL kernels' launch failed: %s\n", hipGetErrorString(e));
        return JMH_E_HIP;
    }
    return JMH_OK;
}
