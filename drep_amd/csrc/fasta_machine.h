// fasta_machine.h -- the byte machine of the device FASTA ingest
// (ingest_device.hip) and the algebra of its summaries, as inline functions
// the kernels call and a host program can call too: kseq's reader restricted
// to FASTA, one byte at a time, from any of four entry states at once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace drephip {

constexpr uint32_t kTextTile = 8192;          // text bytes per tile
constexpr uint32_t kTextWG = 256;             // lanes per tile workgroup
constexpr uint32_t kLaneBytes = kTextTile / kTextWG;   // 32: two 16-byte loads per lane
static_assert(kLaneBytes == 32, "a lane holds its bytes in eight dwords");

enum : uint32_t { ST_HUNT = 0, ST_HDR = 1, ST_SEQ = 2, ST_START = 3 };

// One entry state's summary in a dword: bits 0-1 exit state, bit 2 '+' seen,
// bits 3-16 sequence bytes (<= kTextTile), bits 17-31 records (<= kTextTile/2).
constexpr uint32_t kPlusBit = 4u;
constexpr uint32_t kSeqOne = 1u << 3, kRecOne = 1u << 17;
constexpr uint32_t kCountMask = ~7u;
struct Sum { uint32_t e[4]; };

__host__ __device__ __forceinline__ uint32_t sum_sel(const Sum &b, uint32_t s) {
    return s == 0 ? b.e[0] : s == 1 ? b.e[1] : s == 2 ? b.e[2] : b.e[3];
}
// a, then b
__host__ __device__ __forceinline__ Sum compose(const Sum &a, const Sum &b) {
    Sum r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t x = a.e[i], y = sum_sel(b, x & 3u);
        r.e[i] = (y & 3u) | ((x | y) & kPlusBit) | ((x & kCountMask) + (y & kCountMask));
    }
    return r;
}
__host__ __device__ __forceinline__ Sum sum_identity() { return Sum{{0u, 1u, 2u, 3u}}; }

// What one byte is to the machine, whatever state it meets.
struct ByteClass {
    bool nl, hdr, plus;
    uint32_t seq_add;      // kSeqOne unless the byte is a line-final '\r'
    uint32_t rec_add;      // kRecOne unless the byte is the file's last
};
__host__ __device__ __forceinline__ ByteClass classify(uint32_t c, uint32_t next, bool has_next) {
    ByteClass b;
    b.nl = c == '\n';
    b.hdr = c == '>' || c == '@';
    b.plus = c == '+';
    b.seq_add = (c == '\r' && (!has_next || next == '\n')) ? 0u : kSeqOne;
    b.rec_add = has_next ? kRecOne : 0u;
    return b;
}
// One byte from packed state x (state in bits 0-1, counts above).
__host__ __device__ __forceinline__ uint32_t step(uint32_t x, const ByteClass &b) {
    const uint32_t s = x & 3u;
    uint32_t ns = s;
    if (b.nl) {
        ns = s == ST_HUNT ? ST_HUNT : ST_START;
    } else if (s == ST_START) {
        ns = (b.hdr || b.plus) ? ST_HDR : ST_SEQ;
        if (b.plus) x |= kPlusBit;
    } else if (s == ST_HUNT) {
        ns = b.hdr ? ST_HDR : ST_HUNT;
    }
    if (b.hdr && (s == ST_HUNT || s == ST_START)) x += b.rec_add;
    if (ns == ST_SEQ) x += b.seq_add;          // SEQ is only entered or kept on a base
    return (x & ~3u) | ns;
}

// A lane's bytes: [p, p + nb) of the text, nb <= 32, p 16-byte aligned; whole
// 16-byte pieces by one vector load, the file's ragged end byte by byte.
struct LaneText {
    uint32_t w[8];
    uint32_t nb;
    uint32_t peek;          // the byte after the lane's last one
    bool has_peek;          // false: the lane ends the file
};
__host__ __device__ __forceinline__ LaneText load_lane(const uint8_t *text, uint64_t p, uint64_t fend) {
    LaneText t;
    t.nb = p >= fend ? 0u : (uint32_t)(fend - p < kLaneBytes ? fend - p : kLaneBytes);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        const uint32_t have = t.nb > 16u * h ? t.nb - 16u * h : 0u;
        if (have >= 16u) {
            const uint4 q = *(const uint4 *)(text + p + 16u * h);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if ((uint32_t)(4 * j + b) < have) v[j] |= (uint32_t)text[p + 16u * h + 4 * j + b] << (8 * b);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) t.w[4 * h + j] = v[j];
    }
    t.has_peek = p + t.nb < fend;
    t.peek = t.has_peek ? (uint32_t)text[p + t.nb] : 0u;
    return t;
}
__host__ __device__ __forceinline__ uint32_t lane_byte(const LaneText &t, int i) { return (t.w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }
__host__ __device__ __forceinline__ ByteClass lane_class(const LaneText &t, int i) {
    const bool last = (uint32_t)i + 1u == t.nb;          // always so for i = 31
    const uint32_t in_lane = i + 1 < (int)kLaneBytes ? lane_byte(t, i + 1 < (int)kLaneBytes ? i + 1 : i) : 0u;
    return classify(lane_byte(t, i), last ? t.peek : in_lane, last ? t.has_peek : true);
}

// the lane's summary for the four entry states
__host__ __device__ __forceinline__ Sum lane_summary(const LaneText &t) {
    Sum s = sum_identity();
#pragma unroll
    for (int i = 0; i < (int)kLaneBytes; i++) {
        if ((uint32_t)i < t.nb) {
            const ByteClass b = lane_class(t, i);
#pragma unroll
            for (int e = 0; e < 4; e++) s.e[e] = step(s.e[e], b);
        }
    }
    return s;
}

// The lane's bases when it is entered with packed state x (the entry state and
// the tile's counts up to the lane): emit(q, r, byte) for each, q sequence
// bytes and r records started before it in the tile.
template <class F>
__host__ __device__ __forceinline__ void lane_bases(const LaneText &t, uint32_t x, F &&emit) {
#pragma unroll
    for (int i = 0; i < (int)kLaneBytes; i++) {
        if ((uint32_t)i < t.nb) {
            const uint32_t y = step(x, lane_class(t, i));
            if (((y ^ x) & (kRecOne - 1) & kCountMask) != 0) emit((x >> 3) & 0x3FFFu, y >> 17, lane_byte(t, i));
            x = y;
        }
    }
}

// the file of tile / chunk t: the last f < n with first[f] <= t (empty files
// share their successor's first tile and are passed over)
__host__ __device__ __forceinline__ uint32_t find_file(const uint32_t *first, uint32_t n, uint32_t t) {
    uint32_t lo = 0, hi = n;            // first[lo] <= t < first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// The host's lists for one pack call: tile_first[f] = text tiles of the files
// before f, chunk_first[f] = sketch tiles (of tile_bases bases) of the regions
// before f, n + 1 entries each.  false: more than 2^32 - 1 of either.
inline bool build_firsts(const uint64_t *text_beg, const uint64_t *text_end, const uint64_t *cap, uint32_t n,
                         uint64_t tile_bases, std::vector<uint32_t> &tile_first, std::vector<uint32_t> &chunk_first) {
    tile_first.assign((size_t)n + 1, 0);
    chunk_first.assign((size_t)n + 1, 0);
    uint64_t nt = 0, nc = 0;
    for (uint32_t f = 0; f < n; f++) {
        tile_first[f] = (uint32_t)nt;
        chunk_first[f] = (uint32_t)nc;
        nt += (text_end[f] - text_beg[f] + kTextTile - 1) / kTextTile;
        nc += cap[f] / tile_bases;
        if (nt >= (1ull << 32) || nc >= (1ull << 32)) return false;
    }
    tile_first[n] = (uint32_t)nt;
    chunk_first[n] = (uint32_t)nc;
    return true;
}

}  // namespace drephip
