// jmh_nal.h — the shared core of the device NAL stage (include/jmhip_nal.h): one
// text that the kernels of jmh_nal.hip and the host harness (tests/harness/nal_core_check.c) both
// compile.  C99 and HIP.
//
// host/bitstream.c › jm_write_nal puts a 03 before byte v when zeros >= 2 && v <= 3 and then sets
// zeros to 0.  The same output follows from a rule on the input alone: a 03 goes before input byte
// i iff rbsp[i] <= 3 and L >= 2 and L is even, L being the zero bytes immediately before i in the
// input (in a run of zeros the serial counter is reset at every second one, which is where L is
// even).  So a unit is cut into chunks of JMN_CHUNK input bytes, one wave each, which the wave
// walks in tiles of JMN_TILE bytes, a byte per lane:
//   nz, le3   the tile's ballots: byte != 0, byte <= 3 (lanes past the tile's bytes: 0)
//   L         of a lane: from nz below the lane, or lane + carry when all of that is zero
//   carry     L at the tile's start: the trailing zeros of what came before in the unit
// Only the escapes up to and including a chunk's first non-zero byte depend on the carry into the
// chunk.  The count pass therefore counts the others and records (lead, first_le3, trail); the scan
// finds each chunk's carry from the chunks before it in the unit and adds the escapes of the lead
// in closed form (jmn_lead_escapes).
#ifndef JMH_NAL_H
#define JMH_NAL_H
#include <stdint.h>

#if defined(__HIPCC__)
#define JMN_FN __host__ __device__ static __forceinline__
#else
#define JMN_FN static inline
#endif

#define JMN_TILE 64                   // input bytes of one wave step
#define JMN_TILES_PER_CHUNK 64
#define JMN_CHUNK (JMN_TILE * JMN_TILES_PER_CHUNK)   // input bytes of one wave
#define JMN_UNIT_OVERHEAD 5           // 00 00 00 01 and the NAL header byte

typedef struct jmn_chunk {
    // count pass
    int32_t n;                        // input bytes (0: the only chunk of an empty unit)
    int32_t lead;                     // leading zero bytes; n: the chunk is all zeros
    int32_t first_le3;                // the byte behind them exists and is 1..3
    int32_t trail;                    // trailing zero bytes (n when all zeros)
    int32_t cnt;                      // escapes behind the first non-zero byte: any carry gives these
    // scan
    int32_t unit, first;              // its unit; 1: the unit's first chunk (writes the start code)
    int32_t carry;                    // L at its first byte
    int32_t outn;                     // its output bytes, a first chunk's JMN_UNIT_OVERHEAD not among them
    int32_t pad;
    int64_t out;                      // where its first output byte goes
} jmn_chunk;

// the escape predicate on a byte and the zeros before it
JMN_FN int jmn_escape(uint32_t v_le3, int32_t L) { return v_le3 && L >= 2 && !(L & 1); }

// L of a lane of a tile
JMN_FN int32_t jmn_lane_L(uint64_t nz, int lane, int32_t carry) {
    const uint64_t below = nz & ((1ull << lane) - 1);
    return below ? lane - 64 + (int32_t)__builtin_clzll(below) : lane + carry;
}
// L behind a tile of n bytes
JMN_FN int32_t jmn_tile_carry(uint64_t nz, int n, int32_t carry) { return nz ? n - 64 + (int32_t)__builtin_clzll(nz) : carry + n; }
// where a lane's byte goes behind the tile's first output byte (its own 03, if any, one before that)
JMN_FN int jmn_lane_out(uint64_t esc, int lane) { return lane + __builtin_popcountll(esc & ((2ull << lane) - 1)); }

// The count pass's state over a chunk's tiles (wave-uniform); carry starts at 0: what it gives the
// lanes up to the first non-zero byte is masked out of esc here and found by the scan
typedef struct jmn_count { int32_t carry, seen, lead, first_le3, cnt, n; } jmn_count;
JMN_FN void jmn_count_begin(jmn_count *s) { s->carry = 0; s->seen = 0; s->lead = 0; s->first_le3 = 0; s->cnt = 0; s->n = 0; }
// esc: the tile's escape ballot under s->carry
JMN_FN void jmn_count_tile(jmn_count *s, uint64_t nz, uint64_t le3, uint64_t esc, int n) {
    if (!s->seen) {
        if (!nz) { esc = 0; s->lead += n; }
        else {
            const int f = __builtin_ctzll(nz);
            s->lead += f; s->first_le3 = (int32_t)((le3 >> f) & 1); s->seen = 1;
            esc &= ~((2ull << f) - 1);
        }
    }
    s->cnt += __builtin_popcountll(esc);
    s->carry = jmn_tile_carry(nz, n, s->carry);
    s->n += n;
}
JMN_FN void jmn_count_end(const jmn_count *s, jmn_chunk *c) {
    c->n = s->n; c->lead = s->lead; c->first_le3 = s->first_le3; c->trail = s->seen ? s->carry : s->n; c->cnt = s->cnt;
}

// the escapes among a chunk's leading zeros and the byte behind them, for L = carry at its first
// byte: the even m >= 2 in [carry, carry + lead + first_le3)
JMN_FN int32_t jmn_lead_escapes(int32_t carry, int32_t lead, int32_t first_le3) {
    const int32_t a = carry > 2 ? carry : 2, b = carry + lead + first_le3;
    return b > a ? (b + 1) / 2 - (a + 1) / 2 : 0;
}
// L behind a chunk
JMN_FN int32_t jmn_chunk_carry(const jmn_chunk *c, int32_t carry) { return c->lead == c->n ? carry + c->n : c->trail; }
// chunks of a unit of len input bytes (an empty unit keeps one: its start code needs a writer)
JMN_FN int64_t jmn_unit_chunks(int64_t len) { return len > 0 ? (len + JMN_CHUNK - 1) / JMN_CHUNK : 1; }

// cabac_zero_words (7.4.2.10), the rule of host/encoder.c › encode_picture_slices: bytes are the
// access unit's bytes less 4 per NAL unit, bd the bit depth (at least 8), nmb the picture's macroblocks
JMN_FN int64_t jmn_zero_words(int64_t bins, int bd, int64_t nmb, int64_t bytes) {
    if (bins <= 0) return 0;
    const int64_t excess = 3 * bins - 36 * (int64_t)(bd > 8 ? bd : 8) * nmb - 32 * bytes;
    return excess > 0 ? (excess + 95) / 96 : 0;
}

#if defined(__HIPCC__)
// ---- host entry of the kernels (jmh_nal.hip), called by the C ABI ----
#include <hip/hip_runtime.h>
#include "../../include/jmhip.h"
#define JMN_META_WORDS 8              // [0] the access unit's bytes  [1] overflow word  [2] zero words  [3] chunks  [4] bins
struct jmh_nal_job {
    int n;                            // units
    const jmh_nal_head *d_heads;      // device [n]
    const uint8_t *d_payload;         // device: the payloads' buffer
    int64_t payload_cap;              //   its bytes: a range outside sets the overflow word
    const int64_t *d_where;           // device [n][3]: offset, nbytes of unit i's payload, a count of bins
    const uint64_t *d_wmeta;          // the slice writer's meta words (null: none): its overflow word set, nothing is read
    int64_t bins;                     // the picture's bins, to which sum_bins adds d_where[i][2]
    int sum_bins, bd, nmb;
    int32_t *d_cs;                    // device [n + 1]: each unit's first chunk
    jmn_chunk *d_ch;                  // device [maxch]
    int maxch;
    int64_t *d_uout;                  // device [n][2]: offset, nbytes of unit i in out
    uint64_t *d_meta;                 // device [JMN_META_WORDS]
    uint8_t *d_out;                   // device: the access unit
    int64_t out_cap;
};
// chunks that n units of total_len input bytes can have at most
static inline int64_t jmh_nal_max_chunks(int n, int64_t total_len) { return n + total_len / JMN_CHUNK + 1; }
// the four launches on st, no host wait between them
int jmh_nal_enqueue(hipStream_t st, const jmh_nal_job *job);
#endif

#endif // JMH_NAL_H
