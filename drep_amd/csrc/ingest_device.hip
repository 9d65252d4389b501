// ingest_device.hip -- FASTA text in HBM -> the packed layout (2-bit codes +
// validity bitmap, include/drephip.h), bit-exact with read_fasta + pack_records
// (ingest.cpp) for every file that never enters kseq's FASTQ states.
//
// The text of a file is cut into tiles of kTextTile bytes (tiles never span
// files).  kseq's reader, restricted to FASTA, is a four-state byte machine:
//   HUNT   no header yet: skip to the first '>' or '@' (anywhere in a line)
//   HDR    inside a header line (or a FASTQ '+' line, which flags the file)
//   SEQ    inside a sequence line: every byte but '\n' is a base, minus one
//          line-final '\r'
//   START  first byte of a line inside a record: '\n' stays, '>'/'@' starts a
//          record, '+' flags the file for the host path, anything else is the
//          first base of a sequence line
// A '>'/'@' that is the file's last byte starts no record (kseq_read's -1).
// A stretch of text is summarised, for each of the four states it may be
// entered in, by (exit state, sequence bytes, records started, '+' seen);
// summaries compose associatively (Sum, compose), which is all the passes use:
//   k_fasta_tile_summary  one workgroup per tile: each lane walks its 32 bytes
//                         for the four entry states, the lanes' summaries are
//                         composed in order into the tile's
//   k_fasta_tile_scan     one workgroup per call composes the tile summaries in
//                         file order (every file enters in HUNT): each tile's
//                         true entry state and its sequence-byte / record
//                         prefix, and the per-file totals, span and status
//   k_fasta_tile_pack     per tile: the lanes' summaries scanned again give each
//                         lane its entry state and prefix, so every base knows
//                         its position; codes and validity bits are assembled
//                         in an LDS window of the tile's output range, interior
//                         words stored plainly, the first and last word (shared
//                         with the neighbouring tiles) OR-ed atomically into
//                         the zeroed region
//   k_valid_kmers         per genome, positions ending a run of >= k valid
//                         bases, from the bitmap words (run_k_mask's count)
// No workgroup waits on another: ordering comes from kernel boundaries only.
#include "ctx.h"
#include "fasta_machine.h"
#include "../../include/drephip.h"

#include <algorithm>
#include <vector>

namespace drephip {

constexpr uint32_t kScanWG = 512;             // lanes of the one scan workgroup

uint32_t text_tile_bytes() { return kTextTile; }

__device__ __forceinline__ Sum sum_shfl_up(const Sum &v, int d) {
    Sum o;
#pragma unroll
    for (int i = 0; i < 4; i++) o.e[i] = __shfl_up(v.e[i], d, 64);
    return o;
}
// Workgroup scan of the lanes' summaries in lane order: *excl = everything
// before this lane, *total = the whole workgroup.  wave_tot: kTextWG/64 slots.
__device__ __forceinline__ void block_scan(const Sum &mine, Sum *wave_tot, Sum *excl, Sum *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Sum inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Sum o = sum_shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc = compose(o, inc);
    }
    Sum ex = sum_shfl_up(inc, 1);
    if (lane == 0) ex = sum_identity();
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    Sum pre = sum_identity(), tot = sum_identity();
    for (uint32_t w = 0; w < kTextWG / 64; w++) {
        const Sum t = wave_tot[w];
        if (w < wave) pre = compose(pre, t);
        tot = compose(tot, t);
    }
    *excl = compose(pre, ex);
    *total = tot;
}

struct TileEntry {
    uint64_t seq;          // sequence bytes of the file before the tile
    uint32_t rec;          // records started before it
    uint32_t state;
};

// ------------------------------------------------------------ pass 1
__global__ __launch_bounds__(kTextWG) void k_fasta_tile_summary(const uint8_t *__restrict__ text,
                                                                 const uint64_t *__restrict__ text_beg, const uint64_t *__restrict__ text_end,
                                                                 const uint32_t *__restrict__ tile_first, uint32_t n,
                                                                 uint32_t t0, uint32_t ntiles, uint4 *__restrict__ sums) {
    __shared__ Sum wave_tot[kTextWG / 64];
    const uint32_t t = t0 + blockIdx.x;
    if (t >= ntiles) return;
    const uint32_t f = find_file(tile_first, n, t);
    const uint64_t p = text_beg[f] + (uint64_t)(t - tile_first[f]) * kTextTile + (uint64_t)threadIdx.x * kLaneBytes;
    const LaneText lt = load_lane(text, p, text_end[f]);
    Sum ex, tot;
    block_scan(lane_summary(lt), wave_tot, &ex, &tot);
    if (threadIdx.x == 0) sums[t] = make_uint4(tot.e[0], tot.e[1], tot.e[2], tot.e[3]);
}

// ------------------------------------------------------------ pass 2
struct Run {               // a walk's state from one entry state
    uint64_t seq;
    uint32_t rec;
    uint32_t sp;           // state | '+' bit
};
__device__ __forceinline__ void run_apply(Run &r, const uint4 &s) {
    const uint32_t st = r.sp & 3u;
    const uint32_t y = st == 0 ? s.x : st == 1 ? s.y : st == 2 ? s.z : s.w;
    r.sp = (y & 3u) | ((r.sp | y) & kPlusBit);
    r.seq += (y >> 3) & 0x3FFFu;
    r.rec += y >> 17;
}

__global__ __launch_bounds__(kScanWG) void k_fasta_tile_scan(const uint4 *__restrict__ sums,
                                                             const uint32_t *__restrict__ tile_first, uint32_t n,
                                                             uint32_t ntiles, const uint64_t *__restrict__ cap,
                                                             uint64_t tile_bases, TileEntry *__restrict__ entries,
                                                             uint64_t *__restrict__ length, uint64_t *__restrict__ padded,
                                                             uint32_t *__restrict__ nrec, uint32_t *__restrict__ status) {
    __shared__ Run chunk_res[kScanWG][4];
    __shared__ uint32_t chunk_reset[kScanWG];
    __shared__ Run chunk_in[kScanWG];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + kScanWG - 1) / kScanWG;
    const uint32_t c0 = (uint64_t)tid * per < ntiles ? tid * per : ntiles;
    const uint32_t c1 = (uint64_t)c0 + per < ntiles ? c0 + per : ntiles;
    auto finish = [&](uint32_t f, uint64_t seq, uint32_t rec, bool plus) {
        const uint64_t span = seq + (rec ? rec - 1 : 0);
        const uint64_t P = (span + 1 + tile_bases - 1) / tile_bases * tile_bases;
        length[f] = seq;
        nrec[f] = rec;
        padded[f] = P;
        status[f] = plus ? 1u : P > cap[f] ? 2u : 0u;
    };
    // files without a tile (empty)
    for (uint32_t f = tid; f < n; f += kScanWG)
        if (tile_first[f] == tile_first[f + 1]) finish(f, 0, 0, false);
    // A: this lane's run of tiles from each of the four entry states; a file
    // start inside it makes the outcome independent of the entry
    Run r[4];
#pragma unroll
    for (int e = 0; e < 4; e++) r[e] = Run{0, 0, (uint32_t)e};
    uint32_t reset = 0;
    uint32_t f = c0 < c1 ? find_file(tile_first, n, c0) : 0;
    const uint32_t f_start = f;
    for (uint32_t t = c0; t < c1; t++) {
        while (t >= tile_first[f + 1]) f++;
        if (t == tile_first[f]) {
#pragma unroll
            for (int e = 0; e < 4; e++) r[e] = Run{0, 0, ST_HUNT};
            reset = 1;
        }
        const uint4 s = sums[t];
#pragma unroll
        for (int e = 0; e < 4; e++) run_apply(r[e], s);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) chunk_res[tid][e] = r[e];
    chunk_reset[tid] = reset;
    __syncthreads();
    // B: the chunks in order (tile 0 starts a file, so the first entry is moot)
    if (tid == 0) {
        Run cur = Run{0, 0, ST_HUNT};
        for (uint32_t l = 0; l < kScanWG; l++) {
            chunk_in[l] = cur;
            const Run o = chunk_res[l][cur.sp & 3u];
            if (chunk_reset[l]) cur = o;
            else cur = Run{cur.seq + o.seq, cur.rec + o.rec, (o.sp & 3u) | ((cur.sp | o.sp) & kPlusBit)};
        }
    }
    __syncthreads();
    // C: the same walk from the true entry
    Run cur = chunk_in[tid];
    f = f_start;
    for (uint32_t t = c0; t < c1; t++) {
        while (t >= tile_first[f + 1]) f++;
        if (t == tile_first[f]) cur = Run{0, 0, ST_HUNT};
        entries[t] = TileEntry{cur.seq, cur.rec, cur.sp & 3u};
        run_apply(cur, sums[t]);
        if (t + 1 == tile_first[f + 1]) finish(f, cur.seq, cur.rec, (cur.sp & kPlusBit) != 0);
    }
}

// ------------------------------------------------------------ pass 3
// A tile's bases land in at most 31 (alignment) + kTextTile + kTextTile/2
// (separators: a record costs two text bytes) positions from its window base.
constexpr uint32_t kWinBases = 32 + kTextTile + kTextTile / 2 + 32;
constexpr uint32_t kWinValid = kWinBases / 32, kWinCodes = kWinBases / 16;

__global__ __launch_bounds__(kTextWG) void k_fasta_tile_pack(const uint8_t *__restrict__ text,
                                                              const uint64_t *__restrict__ text_beg, const uint64_t *__restrict__ text_end,
                                                              const uint32_t *__restrict__ tile_first, uint32_t n,
                                                              uint32_t t0, uint32_t ntiles,
                                                              const TileEntry *__restrict__ entries,
                                                              const uint64_t *__restrict__ base_off,
                                                              const uint32_t *__restrict__ status,
                                                              uint32_t *__restrict__ codes, uint32_t *__restrict__ valid) {
    __shared__ Sum wave_tot[kTextWG / 64];
    __shared__ uint32_t s_codes[kWinCodes], s_valid[kWinValid];
    __shared__ uint32_t s_min, s_max;
    const uint32_t t = t0 + blockIdx.x;
    if (t >= ntiles) return;
    const uint32_t f = find_file(tile_first, n, t);
    if (status[f] != 0) return;                 // host path, or the region is too small: nothing is written
    for (uint32_t i = threadIdx.x; i < kWinCodes; i += kTextWG) s_codes[i] = 0;
    for (uint32_t i = threadIdx.x; i < kWinValid; i += kTextWG) s_valid[i] = 0;
    if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_max = 0; }
    const uint64_t p = text_beg[f] + (uint64_t)(t - tile_first[f]) * kTextTile + (uint64_t)threadIdx.x * kLaneBytes;
    const LaneText lt = load_lane(text, p, text_end[f]);
    Sum ex, tot;
    block_scan(lane_summary(lt), wave_tot, &ex, &tot);      // its barrier also covers the LDS clears
    const TileEntry te = entries[t];
    // position of a base = base_off + sequence bytes before it + records started before it - 1
    const uint64_t first_pos = base_off[f] + te.seq + (te.rec ? te.rec : 1u) - 1;
    const uint64_t win0 = first_pos & ~31ull;
    // local index of a base with q sequence bytes and r records before it in the tile: rel + q + r
    const int32_t rel = (int32_t)(int64_t)(base_off[f] + te.seq + te.rec - 1 - win0);
    const uint32_t x = ex.e[te.state];          // state, and the counts of the tile up to this lane
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    lane_bases(lt, x, [&](uint32_t q, uint32_t r, uint32_t c) {
        const int32_t loc = rel + (int32_t)q + (int32_t)r;
        if (loc < 0 || (uint32_t)loc >= kWinBases) return;      // cannot happen (kWinBases)
        lo = min(lo, (uint32_t)loc);
        hi = max(hi, (uint32_t)loc);
        const uint32_t u = c & 0xDFu;
        if (u == 'A' || u == 'C' || u == 'G' || u == 'T') {
            const uint32_t code = ((c >> 1) ^ (c >> 2)) & 3u;
            if (code) atomicOr(&s_codes[loc >> 4], code << (2 * (loc & 15)));
            atomicOr(&s_valid[loc >> 5], 1u << (loc & 31));
        }
    });
    if (lo != 0xFFFFFFFFu) { atomicMin(&s_min, lo); atomicMax(&s_max, hi); }
    __syncthreads();
    const uint32_t mn = s_min, mx = s_max;
    if (mn == 0xFFFFFFFFu) return;              // no base in this tile
    // words strictly inside the tile's range are its own; the two end words may
    // hold a neighbouring tile's bases too
    {
        const uint32_t w0 = mn >> 5, w1 = mx >> 5;
        uint32_t *g = valid + (win0 >> 5);
        for (uint32_t w = w0 + threadIdx.x; w <= w1; w += kTextWG) {
            const uint32_t v = s_valid[w];
            if (w == w0 || w == w1) { if (v) atomicOr(g + w, v); }
            else g[w] = v;
        }
    }
    {
        const uint32_t w0 = mn >> 4, w1 = mx >> 4;
        uint32_t *g = codes + (win0 >> 4);
        for (uint32_t w = w0 + threadIdx.x; w <= w1; w += kTextWG) {
            const uint32_t v = s_codes[w];
            if (w == w0 || w == w1) { if (v) atomicOr(g + w, v); }
            else g[w] = v;
        }
    }
}

// ------------------------------------------------------------ pass 4
// Mask of positions (bits) ending a run of >= k set bits in v (ingest.cpp).
__device__ __forceinline__ uint64_t run_k_mask_dev(uint64_t v, int k) {
    uint64_t a[6];
    a[0] = v;
#pragma unroll
    for (int i = 1; i < 6; i++) a[i] = a[i - 1] & (a[i - 1] << (1 << (i - 1)));
    uint64_t m = ~0ull;
    int off = 0;
#pragma unroll
    for (int i = 5; i >= 0; i--)
        if (k & (1 << i)) { m &= a[i] << off; off += 1 << i; }
    return m;
}

constexpr uint32_t kKmerWG = 256, kKmerWords = 4;     // one workgroup: 1024 bitmap words = one sketch tile
__global__ __launch_bounds__(kKmerWG) void k_valid_kmers(const uint32_t *__restrict__ valid,
                                                          const uint32_t *__restrict__ chunk_first, uint32_t n,
                                                          uint32_t c0, uint32_t nchunks,
                                                          const uint64_t *__restrict__ base_off,
                                                          const uint64_t *__restrict__ padded,
                                                          const uint32_t *__restrict__ status, int k,
                                                          unsigned long long *__restrict__ nk) {
    __shared__ uint32_t part[kKmerWG / 64];
    const uint32_t c = c0 + blockIdx.x;
    if (c >= nchunks) return;
    const uint32_t f = find_file(chunk_first, n, c);
    const uint64_t rel = (uint64_t)(c - chunk_first[f]) * (kKmerWG * kKmerWords * 32ull);
    if (status[f] != 0 || rel >= padded[f]) return;
    const uint64_t gw0 = base_off[f] >> 5;                  // the genome's first bitmap word
    const uint64_t w = gw0 + (rel >> 5) + (uint64_t)threadIdx.x * kKmerWords;
    uint32_t cnt = 0;
    if (((w - gw0) << 5) < padded[f]) {                     // padded is a multiple of this lane's 128 bases
        uint64_t prev = w == gw0 ? 0u : valid[w - 1];
#pragma unroll
        for (uint32_t j = 0; j < kKmerWords; j++) {
            const uint64_t cur = valid[w + j];
            cnt += __popcll(run_k_mask_dev(prev | (cur << 32), k) >> 32);
            prev = cur;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (uint32_t i = 0; i < kKmerWG / 64; i++) s += part[i];
        if (s) atomicAdd(&nk[f], (unsigned long long)s);
    }
}

// ------------------------------------------------------------ host driver
int fasta_pack_device_impl(drephip_ctx *ctx, const uint8_t *d_text, const uint64_t *text_beg,
                           const uint64_t *text_end, uint32_t n,
                           const uint64_t *base_off, const uint64_t *cap, uint32_t *d_codes, uint32_t *d_valid,
                           uint64_t *length_out, uint64_t *padded_out, uint32_t *n_records_out, uint64_t *n_kmers_out,
                           uint8_t *status_out, hipStream_t st) {
    if (n == 0) return DREPHIP_OK;
    static_assert(kKmerWG * kKmerWords * 32ull == kTile, "a k-mer count chunk is one sketch tile");
    // tiles per file, k-mer count chunks per region
    std::vector<uint32_t> tile_first, chunk_first;
    if (!build_firsts(text_beg, text_end, cap, n, kTile, tile_first, chunk_first)) {
        set_error("too much text for one call"); return DREPHIP_ERR_UNSUPPORTED;
    }
    const uint32_t ntiles = tile_first[n], nchunks = chunk_first[n];
    // device metadata: four uint64 arrays, then the two uint32 ones
    const size_t n64 = 4 * (size_t)n;
    std::vector<uint64_t> meta(n64 + (2 * (size_t)(n + 1) + 1) / 2);
    std::copy(text_beg, text_beg + n, meta.begin());
    std::copy(text_end, text_end + n, meta.begin() + n);
    std::copy(base_off, base_off + n, meta.begin() + 2 * (size_t)n);
    std::copy(cap, cap + n, meta.begin() + 3 * (size_t)n);
    uint32_t *m32 = (uint32_t *)(meta.data() + n64);
    std::copy(tile_first.begin(), tile_first.end(), m32);
    std::copy(chunk_first.begin(), chunk_first.end(), m32 + (n + 1));
    uint64_t *d_meta, *d_res;
    uint4 *d_sums;
    TileEntry *d_ent;
    int rc;
    if ((rc = scratch(ctx, "fp_meta", meta.size() * 8, (void **)&d_meta))) return rc;
    if ((rc = scratch(ctx, "fp_res", (size_t)n * 32, (void **)&d_res))) return rc;
    if ((rc = scratch(ctx, "fp_sums", (size_t)ntiles * sizeof(uint4), (void **)&d_sums))) return rc;
    if ((rc = scratch(ctx, "fp_entries", (size_t)ntiles * sizeof(TileEntry), (void **)&d_ent))) return rc;
    const uint64_t *d_beg = d_meta, *d_end = d_meta + n, *d_base = d_end + n, *d_cap = d_base + n;
    const uint32_t *d_tile_first = (const uint32_t *)(d_meta + n64), *d_chunk_first = d_tile_first + (n + 1);
    uint64_t *d_len = d_res, *d_pad = d_res + n, *d_nk = d_res + 2 * (size_t)n;
    uint32_t *d_nrec = (uint32_t *)(d_res + 3 * (size_t)n), *d_status = d_nrec + n;
    HIPC(hipMemcpyAsync(d_meta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, st));
    HIPC(hipMemsetAsync(d_res, 0, (size_t)n * 32, st));
    // zero the regions (adjacent ones in one call)
    for (uint32_t f = 0; f < n;) {
        uint64_t b0 = base_off[f], b1 = b0 + cap[f];
        uint32_t g = f + 1;
        while (g < n && base_off[g] == b1) { b1 += cap[g]; g++; }
        if (b1 > b0) {
            HIPC(hipMemsetAsync(d_codes + b0 / 16, 0, (b1 - b0) / 16 * 4, st));
            HIPC(hipMemsetAsync(d_valid + b0 / 32, 0, (b1 - b0) / 32 * 4, st));
        }
        f = g;
    }
    const uint32_t mb = (uint32_t)max_blocks(kTextWG);
    for (uint32_t t0 = 0; t0 < ntiles; t0 += mb)
        k_fasta_tile_summary<<<std::min(mb, ntiles - t0), kTextWG, 0, st>>>(d_text, d_beg, d_end, d_tile_first, n, t0,
                                                                            ntiles, d_sums);
    k_fasta_tile_scan<<<1, kScanWG, 0, st>>>(d_sums, d_tile_first, n, ntiles, d_cap, kTile, d_ent, d_len, d_pad, d_nrec,
                                             d_status);
    for (uint32_t t0 = 0; t0 < ntiles; t0 += mb)
        k_fasta_tile_pack<<<std::min(mb, ntiles - t0), kTextWG, 0, st>>>(d_text, d_beg, d_end, d_tile_first, n, t0, ntiles,
                                                                         d_ent, d_base, d_status, d_codes, d_valid);
    for (uint32_t c0 = 0; c0 < nchunks; c0 += mb)
        k_valid_kmers<<<std::min(mb, nchunks - c0), kKmerWG, 0, st>>>(d_valid, d_chunk_first, n, c0, nchunks, d_base,
                                                                      d_pad, d_status, ctx->k,
                                                                      (unsigned long long *)d_nk);
    HIPC(hipGetLastError());
    std::vector<uint64_t> res((size_t)n * 4);
    HIPC(hipMemcpyAsync(res.data(), d_res, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    const uint32_t *h_nrec = (const uint32_t *)(res.data() + 3 * (size_t)n), *h_status = h_nrec + n;
    for (uint32_t f = 0; f < n; f++) {
        if (length_out) length_out[f] = res[f];
        if (padded_out) padded_out[f] = res[n + f];
        if (n_kmers_out) n_kmers_out[f] = res[2 * (size_t)n + f];
        if (n_records_out) n_records_out[f] = h_nrec[f];
        if (status_out) status_out[f] = (uint8_t)h_status[f];
    }
    return DREPHIP_OK;
}

}  // namespace drephip
