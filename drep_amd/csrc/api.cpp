// api.cpp -- the extern "C" surface of libdrephip.so (include/drephip.h).
// Host glue only: argument checks, device scratch, host<->device staging.
// All sketch/dist arithmetic runs in the HIP kernels of sketch.hip and
// allpairs.hip; the FASTA ingest is ingest_pipeline.cpp.
#include "ctx.h"
#include "api_checks.h"
#include "canon.h"
#include "ingest_pipeline.h"
#include "prefilter.h"
#include "../../include/drephip.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#define DREPHIP_EXPORT extern "C" __attribute__((visibility("default")))

namespace drephip {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

int scratch(drephip_ctx *ctx, const char *name, size_t bytes, void **out) {
    DevBuf &b = ctx->bufs[name];
    if (bytes == 0) bytes = 8;
    if (b.bytes < bytes) {
        const size_t want = std::max(bytes, b.bytes + b.bytes / 4);
        if (b.ptr) {
            HIPC(hipStreamSynchronize(ctx->stream));
            HIPC(hipDeviceSynchronize());
            HIPC(hipFree(b.ptr));
            b.ptr = nullptr; b.bytes = 0;
        }
        ctx->alloc_gen++;                      // invalidates contents cached in scratch
        hipError_t e = hipMalloc(&b.ptr, want);
        if (e != hipSuccess) {
            set_error(std::string("hipMalloc(") + std::to_string(want) + ") for " + name + ": " +
                      hipGetErrorString(e));
            b.ptr = nullptr;
            return DREPHIP_ERR_NOMEM;
        }
        b.bytes = want;
    }
    *out = b.ptr;
    return DREPHIP_OK;
}

int pinned_host(drephip_ctx *ctx, const char *name, size_t bytes, void **out) {
    DevBuf &b = ctx->pinned[name];
    if (bytes == 0) bytes = 8;
    if (b.bytes < bytes) {
        if (b.ptr) {
            HIPC(hipStreamSynchronize(ctx->stream));
            HIPC(hipHostFree(b.ptr));
            b.ptr = nullptr; b.bytes = 0;
        }
        const size_t want = std::max(bytes, (size_t)4096);
        hipError_t e = hipHostMalloc(&b.ptr, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            set_error(std::string("hipHostMalloc for ") + name + ": " + hipGetErrorString(e));
            b.ptr = nullptr;
            return DREPHIP_ERR_NOMEM;
        }
        b.bytes = want;
    }
    *out = b.ptr;
    return DREPHIP_OK;
}

void timing_begin(drephip_ctx *ctx) {
    for (int i = 0; i < 6; i++) { ctx->kms[i] = 0; ctx->kn[i] = 0; }
    ctx->spans.clear();
    ctx->ev_used = 0;
}

static hipEvent_t next_event(drephip_ctx *ctx) {
    if (ctx->ev_used == ctx->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        ctx->ev_pool.push_back(e);
    }
    return ctx->ev_pool[ctx->ev_used++];
}

void timing_mark(drephip_ctx *ctx, int which, hipStream_t st, bool start) {
    if (!((ctx->timing >> which) & 1u)) return;
    hipEvent_t e = next_event(ctx);
    if (!e) return;
    (void)hipEventRecord(e, st);
    if (start) ctx->spans.push_back({which, e, nullptr});
    else if (!ctx->spans.empty()) ctx->spans.back().b = e;
}

void timing_collect(drephip_ctx *ctx) {
    if (!ctx->timing) return;
    for (auto &sp : ctx->spans) {
        if (!sp.a || !sp.b) continue;
        float ms = 0;
        if (hipEventSynchronize(sp.b) == hipSuccess && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            ctx->kms[sp.which] += ms;
            ctx->kn[sp.which] += 1;
        }
    }
    ctx->spans.clear();
    ctx->ev_used = 0;
}

}  // namespace drephip

using namespace drephip;

// Device-pointer entry points run on the caller's stream.  0 is the HIP null
// stream (also torch's default stream handle), exactly as in the HIP API, so
// work is ordered after whatever the caller queued there.
static hipStream_t pick_stream(drephip_ctx *, void *stream) { return (hipStream_t)stream; }
static void pend_release(drephip_ctx *ctx);

// The call frame's tail ("The C API's call frame"): `impl` runs
// between timing_begin and timing_collect.  A call that fails leaves its
// events uncollected; nomem_ok: DREPHIP_ERR_NOMEM (a record form whose buffer
// is too small) counts as a run that finished, and is returned.
template <class Impl>
static int timed(drephip_ctx *ctx, bool nomem_ok, Impl &&impl) {
    timing_begin(ctx);
    const int rc = impl();
    if (rc && !(nomem_ok && rc == DREPHIP_ERR_NOMEM)) return rc;
    timing_collect(ctx);
    return rc;
}

// A deferred sketch (drephip_sketch_device_async) owns the sketch scratch and
// its status check until drephip_sketch_wait: any other sketch call is refused
// rather than dropping that check or reusing scratch its kernels still read.
int drephip::refuse_if_pending(drephip_ctx *ctx) {
    if (!ctx->pend.active) return DREPHIP_OK;
    set_error("a deferred sketch (drephip_sketch_device_async) is pending: call drephip_sketch_wait first");
    return DREPHIP_ERR_ARG;
}

DREPHIP_EXPORT int drephip_version(void) { return 500; }

#ifndef DREPHIP_SRC_DIGEST
#define DREPHIP_SRC_DIGEST "unknown"
#endif
#ifndef DREPHIP_BUILD_FLAGS
#define DREPHIP_BUILD_FLAGS ""
#endif
DREPHIP_EXPORT const char *drephip_build_id(void) {
    return "src=" DREPHIP_SRC_DIGEST ";arch=gfx950;extra=" DREPHIP_BUILD_FLAGS;
}

DREPHIP_EXPORT const char *drephip_last_error(void) { return g_err.c_str(); }

DREPHIP_EXPORT int drephip_device_count(int *n) {
    if (!n) { set_error("null pointer"); return DREPHIP_ERR_ARG; }
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; set_error(hipGetErrorString(e)); return DREPHIP_ERR_HIP; }
    *n = c;
    return DREPHIP_OK;
}

DREPHIP_EXPORT uint32_t drephip_max_sketch(void) { return kMaxSketch; }
DREPHIP_EXPORT uint64_t drephip_tile_bases(void) { return kTile; }

DREPHIP_EXPORT uint64_t drephip_padded_bases(const uint64_t *rec_len, uint32_t n_rec) {
    return padded_span(genome_span(rec_len, n_rec));
}

DREPHIP_EXPORT int drephip_create(int device, int k, uint32_t s, uint32_t seed, drephip_ctx **out) {
    if (!out) { set_error("null out"); return DREPHIP_ERR_ARG; }
    *out = nullptr;
    if (k < 1 || k > 32) { set_error("k must be in 1..32"); return DREPHIP_ERR_ARG; }
    if (s < 1 || s > kMaxSketch) {
        set_error("sketch size must be in 1.." + std::to_string(kMaxSketch));
        return DREPHIP_ERR_UNSUPPORTED;
    }
    int n = 0;
    HIPC(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { set_error("no such HIP device"); return DREPHIP_ERR_ARG; }
    HIPC(hipSetDevice(device));
    drephip_ctx *c = new (std::nothrow) drephip_ctx();
    if (!c) { set_error("out of host memory"); return DREPHIP_ERR_NOMEM; }
    c->device = device; c->k = k; c->s = s; c->seed = seed;
    if (const char *lp = std::getenv("DREPHIP_LINK_PATH"))      // default linkage path (tests, A/B runs)
        c->link_path = !strcmp(lp, "dense") ? DREPHIP_LINK_PATH_DENSE : !strcmp(lp, "sparse") ? DREPHIP_LINK_PATH_SPARSE
                                                                                                : DREPHIP_LINK_PATH_AUTO;
    if (const char *ip = std::getenv("DREPHIP_INGEST"))         // default ingest path of drephip_sketch_files
        c->ingest_path = !strcmp(ip, "device") ? DREPHIP_INGEST_DEVICE : DREPHIP_INGEST_HOST;
    if (const char *rb = std::getenv("DREPHIP_RECT_BAND"))      // default band mode of the rectangle (tests, A/B runs)
        c->rect_band = !strcmp(rb, "off") ? DREPHIP_RECT_BAND_OFF : !strcmp(rb, "force") ? DREPHIP_RECT_BAND_FORCE
                                                                                          : DREPHIP_RECT_BAND_AUTO;
    if (const char *rcap = std::getenv("DREPHIP_RECT_BAND_CAP")) {
        const long v = std::atol(rcap);
        if (v >= 1 && v <= 1024) c->rect_band_cap = (uint32_t)v;
    }
    if (const char *rs = std::getenv("DREPHIP_RECT_SCREEN"))    // default mode of the rectangle's two-set screen
        (void)drephip_rect_screen_mode_of(rs, &c->rect_screen_mode);
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; set_error(hipGetErrorString(e)); return DREPHIP_ERR_HIP; }
    *out = c;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_destroy(drephip_ctx *ctx) {
    if (!ctx) return DREPHIP_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    // deferred calls may still be writing the pinned readback buffers
    if (ctx->pend.active && ctx->pend.done) (void)hipEventSynchronize(ctx->pend.done);
    if (ctx->apend.active && ctx->apend.ev) (void)hipEventSynchronize(ctx->apend.ev);
    for (auto &kv : ctx->bufs) if (kv.second.ptr) (void)hipFree(kv.second.ptr);
    for (auto &kv : ctx->pinned) if (kv.second.ptr) (void)hipHostFree(kv.second.ptr);
    pend_release(ctx);
    for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->pend.done) (void)hipEventDestroy(ctx->pend.done);
    if (ctx->apend.ev) (void)hipEventDestroy(ctx->apend.ev);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_set_timing(drephip_ctx *ctx, int kernels) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    ctx->timing = (uint32_t)kernels & 0x3Fu;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_set_allpairs_path(drephip_ctx *ctx, int path, uint32_t band_cap) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (path < DREPHIP_AP_AUTO || path > DREPHIP_AP_MERGE) { set_error("unknown all-pairs path"); return DREPHIP_ERR_ARG; }
    if (band_cap < 1 || band_cap > 1024) { set_error("band_cap must be in 1..1024"); return DREPHIP_ERR_ARG; }
    ctx->ap_path = path;
    ctx->band_cap = band_cap;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_set_rect_band(drephip_ctx *ctx, int mode, uint32_t band_cap) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (mode < DREPHIP_RECT_BAND_AUTO || mode > DREPHIP_RECT_BAND_FORCE) { set_error("unknown rectangle band mode"); return DREPHIP_ERR_ARG; }
    if (band_cap < 1 || band_cap > 1024) { set_error("band_cap must be in 1..1024"); return DREPHIP_ERR_ARG; }
    ctx->rect_band = mode;
    ctx->rect_band_cap = band_cap;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_rect_screen_mode_of(const char *text, int *mode) {
    if (!text || !mode) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    *mode = !strcmp(text, "off") ? DREPHIP_RECT_SCREEN_OFF : !strcmp(text, "force") ? DREPHIP_RECT_SCREEN_FORCE
                                                                                    : DREPHIP_RECT_SCREEN_AUTO;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_set_rect_screen(drephip_ctx *ctx, int mode) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (mode < DREPHIP_RECT_SCREEN_AUTO || mode > DREPHIP_RECT_SCREEN_FORCE) { set_error("unknown rectangle screen mode"); return DREPHIP_ERR_ARG; }
    ctx->rect_screen_mode = mode;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_rect_screen_stats(drephip_ctx *ctx, int *used, uint32_t *blocks, uint64_t *query_entries,
                                                  uint64_t *distinct, uint64_t *checks, uint64_t *marked,
                                                  uint32_t *dense_blocks) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    const RectScreenStats &r = ctx->rect_screen;
    if (used) *used = r.used;
    if (blocks) *blocks = r.blocks;
    if (query_entries) *query_entries = r.query_entries;
    if (distinct) *distinct = r.distinct;
    if (checks) *checks = r.checks;
    if (marked) *marked = r.marked;
    if (dense_blocks) *dense_blocks = r.dense_blocks;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_rect_screen_ms(drephip_ctx *ctx, double ms[5]) {
    if (!ctx || !ms) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    for (int i = 0; i < 5; i++) ms[i] = ctx->rect_screen.phase_ms[i];
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_rect_info(drephip_ctx *ctx, int *kernel, int *fallback) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (kernel) *kernel = ctx->rect_kernel;
    if (fallback) *fallback = ctx->rect_fallback;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_set_allpairs_screen(drephip_ctx *ctx, int mode) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (mode < DREPHIP_SCREEN_AUTO || mode > DREPHIP_SCREEN_OFF) { set_error("unknown screen mode"); return DREPHIP_ERR_ARG; }
    ctx->screen = mode;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_screen_stats(drephip_ctx *ctx, int *used, uint64_t *entries, uint64_t *runs,
                                             uint64_t *checks, uint64_t *marked, uint64_t *simple) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    const ScreenResult &r = ctx->last_screen;
    if (used) *used = r.use ? 1 : 0;
    if (entries) *entries = r.entries;
    if (runs) *runs = r.runs;
    if (checks) *checks = r.checks;
    if (marked) *marked = r.marked;
    if (simple) *simple = r.simple;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_kernel_ms(drephip_ctx *ctx, int which, double *ms, int *launches) {
    if (!ctx || which < 0 || which > 5 || !ms) { set_error("bad argument"); return DREPHIP_ERR_ARG; }
    *ms = ctx->kms[which];
    if (launches) *launches = ctx->kn[which];
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_fasta_info(const char *path, int k, uint64_t *length, uint64_t *padded,
                                      uint32_t *n_records, uint64_t *n_kmers) {
    if (!path) { set_error("null path"); return DREPHIP_ERR_ARG; }
    Genome g;
    if (read_fasta(path, g)) return DREPHIP_ERR_IO;
    const uint32_t nr = (uint32_t)g.rec_len.size();
    if (length) *length = g.length;
    if (padded) *padded = padded_span(genome_span(g.rec_len.data(), nr));
    if (n_records) *n_records = nr;
    if (n_kmers) {
        uint64_t nk = 0, off = 0;
        for (uint32_t r = 0; r < nr; r++) {
            uint64_t run = 0;
            for (uint64_t i = 0; i < g.rec_len[r]; i++) {
                const uint8_t c = g.seq[off + i] & 0xDF;
                const bool ok = c == 'A' || c == 'C' || c == 'G' || c == 'T';
                run = ok ? run + 1 : 0;
                nk += run >= (uint64_t)k;
            }
            off += g.rec_len[r];
        }
        *n_kmers = nk;
    }
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_fasta_pack(const char *path, int k, uint32_t *codes, uint32_t *valid,
                                      uint64_t base_off, uint64_t cap_bases, uint64_t *length,
                                      uint64_t *n_kmers) {
    if (!path || !codes || !valid) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    if (base_off % kTile) { set_error("base_off must be a tile multiple"); return DREPHIP_ERR_ARG; }
    Genome g;
    if (read_fasta(path, g)) return DREPHIP_ERR_IO;
    const uint32_t nr = (uint32_t)g.rec_len.size();
    const uint64_t P = padded_span(genome_span(g.rec_len.data(), nr));
    if (base_off + P > cap_bases) { set_error("packed buffer too small"); return DREPHIP_ERR_ARG; }
    const uint64_t nk = pack_records(g.seq.data(), g.rec_len.data(), nr, k, codes, valid, base_off);
    if (length) *length = g.length;
    if (n_kmers) *n_kmers = nk;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_sketch(drephip_ctx *ctx, const uint8_t *seq, const uint64_t *rec_off,
                                  uint32_t n_rec, const uint64_t *genome_rec_off, uint32_t n_genomes,
                                  uint64_t *hashes_out, uint32_t *nhash_out, uint64_t *length_out) {
    GUARD_CTX(ctx);
    if (n_genomes == 0) return DREPHIP_OK;
    if (!rec_off || !genome_rec_off || !hashes_out || !nhash_out || (!seq && n_rec && rec_off[n_rec] > 0)) {
        set_error("null argument"); return DREPHIP_ERR_ARG;
    }
    if (genome_rec_off[0] != 0 || genome_rec_off[n_genomes] != n_rec) {
        set_error("genome_rec_off must start at 0 and end at n_rec"); return DREPHIP_ERR_ARG;
    }
    std::vector<uint64_t> off(n_genomes), pad(n_genomes), nk(n_genomes), reclen(n_rec);
    for (uint32_t r = 0; r < n_rec; r++) {
        if (rec_off[r + 1] < rec_off[r]) { set_error("rec_off must be non-decreasing"); return DREPHIP_ERR_ARG; }
        reclen[r] = rec_off[r + 1] - rec_off[r];
    }
    uint64_t cur = kTile;
    for (uint32_t g = 0; g < n_genomes; g++) {
        const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1];
        if (r1 < r0) { set_error("genome_rec_off must be non-decreasing"); return DREPHIP_ERR_ARG; }
        off[g] = cur;
        pad[g] = padded_span(genome_span(reclen.data() + r0, (uint32_t)(r1 - r0)));
        cur += pad[g];
        uint64_t L = 0;
        for (uint64_t r = r0; r < r1; r++) L += reclen[r];
        if (length_out) length_out[g] = L;
    }
    std::vector<uint32_t> codes(cur / 16, 0), valid(cur / 32, 0);
    worker_pool(n_genomes, 0, [&](uint32_t, uint32_t g) {
        const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1];
        nk[g] = pack_records(seq + (r1 > r0 ? rec_off[r0] : 0), reclen.data() + r0, (uint32_t)(r1 - r0),
                             ctx->k, codes.data(), valid.data(), off[g]);
    });
    return sketch_packed_host(ctx, codes.data(), codes.size(), valid.data(), valid.size(), off, pad, nk, hashes_out,
                              nhash_out);
}

DREPHIP_EXPORT int drephip_sketch_files(drephip_ctx *ctx, const char *const *paths, uint32_t n_genomes,
                                        int threads, uint64_t *hashes_out, uint32_t *nhash_out,
                                        uint64_t *length_out) {
    GUARD_CTX(ctx);
    ctx->ingest = IngestStats();
    ctx->ingest_paths = IngestPaths();
    if (n_genomes == 0) return DREPHIP_OK;
    if (!paths || !hashes_out || !nhash_out) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc;
    if ((rc = refuse_if_pending(ctx))) return rc;
    return sketch_files_impl(ctx, paths, n_genomes, threads, hashes_out, nhash_out, length_out);
}

DREPHIP_EXPORT int drephip_last_ingest_stats(drephip_ctx *ctx, double *produce_s, double *gpu_s, double *wall_s,
                                             uint32_t *batches) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (produce_s) *produce_s = ctx->ingest.produce_s;
    if (gpu_s) *gpu_s = ctx->ingest.gpu_s;
    if (wall_s) *wall_s = ctx->ingest.wall_s;
    if (batches) *batches = ctx->ingest.batches;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_ingest_phases(drephip_ctx *ctx, double *read_thread_s, double *pack_thread_s,
                                              uint32_t *overflow) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (read_thread_s) *read_thread_s = ctx->ingest.read_thread_s;
    if (pack_thread_s) *pack_thread_s = ctx->ingest.pack_thread_s;
    if (overflow) *overflow = ctx->ingest.overflow;
    return DREPHIP_OK;
}

DREPHIP_EXPORT uint32_t drephip_text_tile_bytes(void) { return text_tile_bytes(); }

DREPHIP_EXPORT int drephip_fasta_pack_device(drephip_ctx *ctx, const uint8_t *d_text, const uint64_t *h_text_off,
                                             uint32_t n_files, const uint64_t *h_base_off, const uint64_t *h_cap_bases,
                                             uint32_t *d_codes, uint32_t *d_valid, uint64_t *length_out,
                                             uint64_t *padded_out, uint32_t *n_records_out, uint64_t *n_kmers_out,
                                             uint8_t *status_out, void *stream) {
    GUARD_CTX(ctx);
    if (n_files == 0) return DREPHIP_OK;
    if (!d_text || !h_text_off || !h_base_off || !h_cap_bases || !d_codes || !d_valid) {
        set_error("null argument"); return DREPHIP_ERR_ARG;
    }
    if ((uintptr_t)d_text % 16 || h_text_off[0] % 16) {
        set_error("d_text and text_off[0] must be 16-byte aligned"); return DREPHIP_ERR_ARG;
    }
    // file f: from the 16-byte boundary at or after text_off[f] to text_off[f + 1]
    std::vector<uint64_t> beg(n_files), end(n_files);
    for (uint32_t f = 0; f < n_files; f++) {
        if (h_text_off[f + 1] < h_text_off[f]) { set_error("text_off must be non-decreasing"); return DREPHIP_ERR_ARG; }
        if (h_base_off[f] % kTile || h_cap_bases[f] % kTile) {
            set_error("base_off and cap_bases must be tile multiples"); return DREPHIP_ERR_ARG;
        }
        beg[f] = round_up(h_text_off[f], 16);
        end[f] = std::max(beg[f], h_text_off[f + 1]);
    }
    return fasta_pack_device_impl(ctx, d_text, beg.data(), end.data(), n_files, h_base_off, h_cap_bases, d_codes, d_valid,
                                  length_out, padded_out, n_records_out, n_kmers_out, status_out,
                                  pick_stream(ctx, stream));
}

DREPHIP_EXPORT int drephip_set_ingest_path(drephip_ctx *ctx, int path) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (path != DREPHIP_INGEST_HOST && path != DREPHIP_INGEST_DEVICE) { set_error("unknown ingest path"); return DREPHIP_ERR_ARG; }
    ctx->ingest_path = path;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_get_ingest_path(drephip_ctx *ctx, int *path) {
    if (!ctx || !path) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    *path = ctx->ingest_path;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_ingest_paths(drephip_ctx *ctx, uint32_t *device_files, uint32_t *host_files,
                                             uint64_t *text_bytes) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (device_files) *device_files = ctx->ingest_paths.device_files;
    if (host_files) *host_files = ctx->ingest_paths.host_files;
    if (text_bytes) *text_bytes = ctx->ingest_paths.text_bytes;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_sketch_device(drephip_ctx *ctx, const uint32_t *d_codes, const uint32_t *d_valid,
                                         const uint64_t *h_base_off, const uint64_t *h_padded,
                                         const uint64_t *h_nkmers, uint32_t n_genomes, uint64_t *d_hashes,
                                         uint32_t *d_nhash, void *stream) {
    GUARD_CTX(ctx);
    if (n_genomes == 0) return DREPHIP_OK;
    if (!d_codes || !d_valid || !h_base_off || !h_padded || !h_nkmers || !d_hashes || !d_nhash) {
        set_error("null argument"); return DREPHIP_ERR_ARG;
    }
    int rc;
    if ((rc = refuse_if_pending(ctx))) return rc;
    return timed(ctx, false, [&] {
        return sketch_device_impl(ctx, d_codes, d_valid, h_base_off, h_padded, h_nkmers, n_genomes, d_hashes, d_nhash,
                                  pick_stream(ctx, stream));
    });
}

// Drop a deferred sketch's bookkeeping: its timing events go back to the pool.
static void pend_release(drephip_ctx *ctx) {
    auto &p = ctx->pend;
    for (hipEvent_t e : p.events) ctx->ev_pool.push_back(e);
    p.events.clear();
    p.spans.clear();
    p.active = false;
}

DREPHIP_EXPORT int drephip_sketch_device_async(drephip_ctx *ctx, const uint32_t *d_codes, const uint32_t *d_valid,
                                               const uint64_t *h_base_off, const uint64_t *h_padded,
                                               const uint64_t *h_nkmers, uint32_t n_genomes, uint64_t *d_hashes,
                                               uint32_t *d_nhash, void *stream) {
    GUARD_CTX(ctx);
    int rc;
    if ((rc = refuse_if_pending(ctx))) return rc;
    if (n_genomes == 0) return DREPHIP_OK;
    if (!d_codes || !d_valid || !h_base_off || !h_padded || !h_nkmers || !d_hashes || !d_nhash) {
        set_error("null argument"); return DREPHIP_ERR_ARG;
    }
    hipStream_t st = pick_stream(ctx, stream);
    timing_begin(ctx);
    rc = sketch_device_impl(ctx, d_codes, d_valid, h_base_off, h_padded, h_nkmers, n_genomes, d_hashes,
                            d_nhash, st, true);
    if (rc) { ctx->pend.active = false; return rc; }
    // the queued kernels' events leave the pool until drephip_sketch_wait reads them
    auto &p = ctx->pend;
    p.spans.swap(ctx->spans);
    p.events.assign(ctx->ev_pool.begin(), ctx->ev_pool.begin() + ctx->ev_used);
    ctx->ev_pool.erase(ctx->ev_pool.begin(), ctx->ev_pool.begin() + ctx->ev_used);
    ctx->ev_used = 0;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_sketch_wait(drephip_ctx *ctx, int *redone) {
    GUARD_CTX(ctx);
    if (redone) *redone = 0;
    auto &p = ctx->pend;
    if (!p.active) return DREPHIP_OK;
    HIPC(hipEventSynchronize(p.done));                 // the status copy (not what was queued after it)
    double kms[2] = {0, 0};
    int kn[2] = {0, 0};
    for (auto &sp : p.spans) {
        float ms = 0;
        if (sp.a && sp.b && sp.which < 2 && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            kms[sp.which] += ms;
            kn[sp.which] += 1;
        }
    }
    bool ok = true;
    for (uint32_t g = 0; g < p.n; g++) ok &= p.h_status[g] == 0;   // ST_OK
    pend_release(ctx);
    if (ok) {
        for (int w = 0; w < 2; w++) { ctx->kms[w] = kms[w]; ctx->kn[w] = kn[w]; }
        return DREPHIP_OK;
    }
    // a genome needs another threshold round: rerun the whole call synchronously
    // (finalize left every set empty, so this starts from a clean state)
    const auto off = p.off, pad = p.pad, nk = p.nk;
    int rc = timed(ctx, false, [&] {
        return sketch_device_impl(ctx, p.d_codes, p.d_valid, off.data(), pad.data(), nk.data(), p.n, p.d_hashes,
                                  p.d_nhash, p.st);
    });
    if (rc) return rc;
    if (redone) *redone = 1;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_synth_device(drephip_ctx *ctx, uint64_t seed, uint32_t g0, uint32_t n,
                                        uint32_t family_size, uint64_t L, uint32_t *d_codes, uint32_t *d_valid,
                                        void *stream) {
    GUARD_CTX(ctx);
    if (!d_codes || !d_valid) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    return synth_device_impl(ctx, seed, g0, n, family_size, L, d_codes, d_valid, pick_stream(ctx, stream));
}

DREPHIP_EXPORT int drephip_allpairs_device(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                           uint32_t N, uint32_t row0, uint32_t row1, uint16_t *d_common,
                                           uint16_t *d_denom, void *stream) {
    GUARD_CTX(ctx);
    if (!d_hashes || !d_nhash || !d_common) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    return timed(ctx, false, [&] {
        return allpairs_device_impl(ctx, d_hashes, d_nhash, N, row0, row1, d_common, d_denom, pick_stream(ctx, stream), false);
    });
}

DREPHIP_EXPORT int drephip_allpairs_device_async(drephip_ctx *ctx, const uint64_t *d_hashes,
                                                 const uint32_t *d_nhash, uint32_t N, uint32_t row0,
                                                 uint32_t row1, uint16_t *d_common, uint16_t *d_denom,
                                                 void *stream) {
    GUARD_CTX(ctx);
    if (!d_hashes || !d_nhash || !d_common) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc = allpairs_wait_impl(ctx);                  // an earlier call's check comes first
    if (rc) return rc;
    timing_begin(ctx);
    rc = allpairs_device_impl(ctx, d_hashes, d_nhash, N, row0, row1, d_common, d_denom,
                              pick_stream(ctx, stream), false, true);
    if (rc) { ctx->apend.active = false; return rc; }
    if (!ctx->apend.active) timing_collect(ctx);      // the call completed synchronously
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_allpairs_wait(drephip_ctx *ctx) {
    GUARD_CTX(ctx);
    return allpairs_wait_impl(ctx);
}

// ------------------------------------------------------------ sharded screen
DREPHIP_EXPORT int drephip_screen_geometry(drephip_ctx *ctx, uint32_t *rows_per_tile) {
    if (!ctx || !rows_per_tile) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    uint32_t R;
    int path;
    int rc = allpairs_geometry(ctx, &R, &path);
    if (rc) return rc;
    *rows_per_tile = R;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_screen_part(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                       uint32_t N, uint32_t part, uint32_t nparts, uint64_t *checks,
                                       uint32_t *n_cells, uint32_t *n_records, void *stream) {
    GUARD_CTX(ctx);
    if (!d_hashes || !d_nhash || !checks || !n_cells || !n_records) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    if (nparts == 0 || part >= nparts) { set_error("part must be below nparts"); return DREPHIP_ERR_ARG; }
    if (N < 2) { set_error("the screen needs N >= 2"); return DREPHIP_ERR_ARG; }
    if (ctx->apend.active) {
        int rc = allpairs_wait_impl(ctx);
        if (rc) return rc;
    }
    uint32_t R;
    int path;
    int rc = allpairs_geometry(ctx, &R, &path);
    if (rc) return rc;
    return timed(ctx, false, [&] {
        return screen_part_impl(ctx, d_hashes, d_nhash, N, R, part, nparts, pick_stream(ctx, stream), checks, n_cells,
                                n_records);
    });
}

DREPHIP_EXPORT int drephip_screen_part_copy(drephip_ctx *ctx, uint32_t *d_cells, uint32_t *d_records, void *stream) {
    GUARD_CTX(ctx);
    const PartResult &p = ctx->part;
    if (!p.valid) { set_error("no screen part to copy (drephip_screen_part first)"); return DREPHIP_ERR_ARG; }
    if ((p.ncells && !d_cells) || (p.nrec && !d_records)) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    hipStream_t st = pick_stream(ctx, stream);
    if (p.ncells) HIPC(hipMemcpyAsync(d_cells, p.cells, (uint64_t)p.ncells * 16, hipMemcpyDeviceToDevice, st));
    if (p.nrec) HIPC(hipMemcpyAsync(d_records, p.rec, (uint64_t)p.nrec * 16, hipMemcpyDeviceToDevice, st));
    HIPC(hipStreamSynchronize(st));
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_screen_worth(drephip_ctx *ctx, uint32_t N, uint64_t checks, int *applies, int *use) {
    if (!ctx || !use) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    const bool ap = screen_applies(ctx, N);
    if (applies) *applies = ap ? 1 : 0;
    *use = ap && (screen_mode(ctx) == DREPHIP_SCREEN_ON || screen_worth(N, ctx->s, checks)) ? 1 : 0;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_allpairs_device_marked(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                                  uint32_t N, uint32_t row0, uint32_t row1, uint16_t *d_common,
                                                  uint16_t *d_denom, const uint32_t *d_cells, uint64_t n_cells,
                                                  const uint32_t *d_records, uint64_t n_records, void *stream) {
    GUARD_CTX(ctx);
    if (!d_hashes || !d_nhash || !d_common || (n_cells && !d_cells) || (n_records && !d_records)) {
        set_error("null argument");
        return DREPHIP_ERR_ARG;
    }
    if ((uint64_t)N * ctx->s >= (1ull << 32)) { set_error("the screen needs N x s < 2^32"); return DREPHIP_ERR_UNSUPPORTED; }
    if (ctx->ap_path == DREPHIP_AP_MERGE) { set_error("marks need the table or band path"); return DREPHIP_ERR_ARG; }
    const ExtMarks marks{(const uint4 *)d_cells, n_cells, (const uint4 *)d_records, n_records};
    return timed(ctx, false, [&] {
        return allpairs_device_impl(ctx, d_hashes, d_nhash, N, row0, row1, d_common, d_denom, pick_stream(ctx, stream),
                                    false, false, &marks);
    });
}

DREPHIP_EXPORT int drephip_allpairs_merge_device(drephip_ctx *ctx, const uint64_t *d_hashes,
                                                 const uint32_t *d_nhash, uint32_t N, uint32_t row0,
                                                 uint32_t row1, uint16_t *d_common, uint16_t *d_denom,
                                                 void *stream) {
    GUARD_CTX(ctx);
    if (!d_hashes || !d_nhash || !d_common) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    return timed(ctx, false, [&] {
        return allpairs_device_impl(ctx, d_hashes, d_nhash, N, row0, row1, d_common, d_denom, pick_stream(ctx, stream), true);
    });
}

// What the triangle's host forms share once their pointers are known not to
// be null, the counterpart of rect_host_stage: row1 clipped, an empty call
// told apart (*empty: the form returns at once), the matrix checked and staged
// onto the context's device (*d_h, *d_n).  The sparse forms (ordered) check
// the rows, and a _sig form its lengths, before the empty test: an empty call
// with a bad matrix is refused there, and returns 0 in the dense forms.
static int tri_host_stage(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, const uint64_t *length,
                          uint32_t N, uint32_t row0, uint32_t *row1, bool ordered, uint64_t **d_h, uint32_t **d_n,
                          bool *empty) {
    *empty = !tri_clip(N, row0, row1);
    int rc;
    if ((ordered || !*empty) && (rc = check_rows(hashes, nhash, N, ctx->s, ordered))) return rc;
    if (length && (rc = check_lengths(length, nhash, N))) return rc;
    if (*empty) return DREPHIP_OK;
    if ((rc = scratch(ctx, "ap_in_h", (uint64_t)N * ctx->s * 8, (void **)d_h))) return rc;
    if ((rc = scratch(ctx, "ap_in_n", N * 4ull, (void **)d_n))) return rc;
    HIPC(hipMemcpyAsync(*d_h, hashes, (uint64_t)N * ctx->s * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(*d_n, nhash, N * 4ull, hipMemcpyHostToDevice, ctx->stream));
    return DREPHIP_OK;
}

// Host-buffer all-pairs over rows [row0, row1): stage the sketch matrix, run
// the kernels on the context's stream, copy the condensed segment back.
static int allpairs_host_rows(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                              uint32_t row0, uint32_t row1, uint16_t *common_out, uint16_t *denom_out) {
    if (!hashes || !nhash || !common_out) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    hipStream_t st = ctx->stream;
    uint64_t *d_h;
    uint32_t *d_n;
    uint16_t *d_c, *d_d = nullptr;
    bool empty;
    int rc;
    if ((rc = tri_host_stage(ctx, hashes, nhash, nullptr, N, row0, &row1, false, &d_h, &d_n, &empty)) || empty) return rc;
    const uint64_t npairs = tri_pairs(N, row0, row1);
    if ((rc = scratch(ctx, "ap_out_c", npairs * 2, (void **)&d_c))) return rc;
    if (denom_out && (rc = scratch(ctx, "ap_out_d", npairs * 2, (void **)&d_d))) return rc;
    if ((rc = timed(ctx, false, [&] { return allpairs_device_impl(ctx, d_h, d_n, N, row0, row1, d_c, d_d, st, false); })))
        return rc;
    HIPC(hipMemcpyAsync(common_out, d_c, npairs * 2, hipMemcpyDeviceToHost, st));
    if (denom_out) HIPC(hipMemcpyAsync(denom_out, d_d, npairs * 2, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_allpairs(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                                    uint16_t *common_out, uint16_t *denom_out) {
    GUARD_CTX(ctx);
    return allpairs_host_rows(ctx, hashes, nhash, N, 0, N, common_out, denom_out);
}

DREPHIP_EXPORT int drephip_allpairs_rows(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                                         uint32_t row0, uint32_t row1, uint16_t *common_out, uint16_t *denom_out) {
    GUARD_CTX(ctx);
    return allpairs_host_rows(ctx, hashes, nhash, N, row0, row1, common_out, denom_out);
}

// ------------------------------------------------------------ sparse all-pairs
DREPHIP_EXPORT int drephip_allpairs_sparse_device(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                                  uint32_t N, uint32_t row0, uint32_t row1, uint32_t *d_pairs,
                                                  uint64_t cap, uint64_t *n_pairs, void *stream) {
    GUARD_CTX(ctx);
    if (!d_hashes || !d_nhash || !n_pairs || (cap && !d_pairs)) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    return timed(ctx, true, [&] {
        return allpairs_sparse_impl(ctx, d_hashes, d_nhash, N, row0, row1, (uint4 *)d_pairs, cap, n_pairs,
                                    pick_stream(ctx, stream));
    });
}

DREPHIP_EXPORT int drephip_allpairs_sparse_device_marked(drephip_ctx *ctx, const uint64_t *d_hashes,
                                                         const uint32_t *d_nhash, uint32_t N, uint32_t row0,
                                                         uint32_t row1, const uint32_t *d_cells, uint64_t n_cells,
                                                         const uint32_t *d_records, uint64_t n_records,
                                                         uint32_t *d_pairs, uint64_t cap, uint64_t *n_pairs,
                                                         void *stream) {
    GUARD_CTX(ctx);
    if (!d_hashes || !d_nhash || !n_pairs || (cap && !d_pairs) || (n_cells && !d_cells) || (n_records && !d_records)) {
        set_error("null argument");
        return DREPHIP_ERR_ARG;
    }
    *n_pairs = 0;
    if ((uint64_t)N * ctx->s >= (1ull << 32)) { set_error("the screen needs N x s < 2^32"); return DREPHIP_ERR_UNSUPPORTED; }
    if (ctx->ap_path == DREPHIP_AP_MERGE) { set_error("marks need the table or band path"); return DREPHIP_ERR_ARG; }
    const ExtMarks marks{(const uint4 *)d_cells, n_cells, (const uint4 *)d_records, n_records};
    return timed(ctx, true, [&] {
        return allpairs_sparse_impl(ctx, d_hashes, d_nhash, N, row0, row1, (uint4 *)d_pairs, cap, n_pairs,
                                    pick_stream(ctx, stream), &marks);
    });
}

// The record protocol's last step on the host forms: the first
// min(n, cap) records, and their p-values where there are any, copied out and
// the stream waited for; rc -- 0, or DREPHIP_ERR_NOMEM when n > cap -- passes through.
static int records_out(int rc, const void *d_rec, const double *d_p, uint64_t n, uint64_t cap, uint32_t *pairs,
                       double *pval, hipStream_t st) {
    const uint64_t have = std::min(n, cap);
    if (have) HIPC(hipMemcpyAsync(pairs, d_rec, have * 16, hipMemcpyDeviceToHost, st));
    if (have && pval) HIPC(hipMemcpyAsync(pval, d_p, have * 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return rc;
}

DREPHIP_EXPORT int drephip_allpairs_sparse(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                                           uint32_t row0, uint32_t row1, uint32_t *pairs, uint64_t cap,
                                           uint64_t *n_pairs) {
    GUARD_CTX(ctx);
    if (!hashes || !nhash || !n_pairs || (cap && !pairs)) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    *n_pairs = 0;
    hipStream_t st = ctx->stream;
    uint64_t *d_h;
    uint32_t *d_n, *d_p = nullptr;
    bool empty;
    int rc;
    if ((rc = tri_host_stage(ctx, hashes, nhash, nullptr, N, row0, &row1, true, &d_h, &d_n, &empty)) || empty) return rc;
    if (cap && (rc = scratch(ctx, "sp_out", cap * 16, (void **)&d_p))) return rc;
    rc = timed(ctx, true, [&] { return allpairs_sparse_impl(ctx, d_h, d_n, N, row0, row1, (uint4 *)d_p, cap, n_pairs, st); });
    if (rc && rc != DREPHIP_ERR_NOMEM) return rc;
    return records_out(rc, d_p, nullptr, *n_pairs, cap, pairs, nullptr, st);
}

// ------------------------------------------------- query against reference
// `mash dist <reference.msh> <query.msh>`: the Q x N rectangle (allpairs.hip,
// rect_device_impl / rect_sparse_impl)
static bool rect_null(const RectSets &in) {
    return (in.Q && (!in.qh || !in.qn)) || (in.N && (!in.rh || !in.rn));
}

// the body of the two dense device forms
static int rect_dense_device(drephip_ctx *ctx, const RectSets &in, uint32_t q0, uint32_t q1, uint16_t *d_common,
                             uint16_t *d_denom, void *stream, bool force_merge) {
    GUARD_CTX(ctx);
    if (rect_null(in) || (in.Q && in.N && q0 < q1 && !d_common)) {
        set_error("null argument");
        return DREPHIP_ERR_ARG;
    }
    return timed(ctx, false, [&] {
        return rect_device_impl(ctx, in, q0, q1, d_common, d_denom, pick_stream(ctx, stream), force_merge);
    });
}

DREPHIP_EXPORT int drephip_dist_rect_device(drephip_ctx *ctx, const uint64_t *d_qhashes, const uint32_t *d_qnhash,
                                            uint32_t Q, const uint64_t *d_rhashes, const uint32_t *d_rnhash, uint32_t N,
                                            uint32_t q0, uint32_t q1, uint16_t *d_common, uint16_t *d_denom,
                                            void *stream) {
    return rect_dense_device(ctx, {d_qhashes, d_qnhash, Q, d_rhashes, d_rnhash, N}, q0, q1, d_common, d_denom, stream, false);
}

DREPHIP_EXPORT int drephip_dist_rect_merge_device(drephip_ctx *ctx, const uint64_t *d_qhashes, const uint32_t *d_qnhash,
                                                  uint32_t Q, const uint64_t *d_rhashes, const uint32_t *d_rnhash,
                                                  uint32_t N, uint32_t q0, uint32_t q1, uint16_t *d_common,
                                                  uint16_t *d_denom, void *stream) {
    return rect_dense_device(ctx, {d_qhashes, d_qnhash, Q, d_rhashes, d_rnhash, N}, q0, q1, d_common, d_denom, stream, true);
}

// What the three host forms share once their inputs are known not to be null
// (each form tests that itself: the tests that go with it differ): q1 clipped,
// an empty call told apart (*empty: the form returns at once), the form's
// outputs tested (out_null), both matrices checked and staged onto the
// context's device (*dev).
static int rect_host_stage(drephip_ctx *ctx, const RectSets &in, uint32_t q0, uint32_t *q1, bool out_null, RectSets *dev,
                           bool *empty) {
    if (*q1 > in.Q) *q1 = in.Q;
    *empty = in.Q == 0 || in.N == 0 || q0 >= *q1;
    if (*empty) return DREPHIP_OK;
    if (out_null) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc;
    if ((rc = check_rows(in.qh, in.qn, in.Q, ctx->s, true)) || (rc = check_rows(in.rh, in.rn, in.N, ctx->s, true))) return rc;
    const uint64_t qbytes = (uint64_t)in.Q * ctx->s * 8, rbytes = (uint64_t)in.N * ctx->s * 8;
    hipStream_t st = ctx->stream;
    uint64_t *d_qh, *d_rh;
    uint32_t *d_qn, *d_rn;
    if ((rc = scratch(ctx, "rect_in_qh", qbytes, (void **)&d_qh))) return rc;
    if ((rc = scratch(ctx, "rect_in_qn", in.Q * 4ull, (void **)&d_qn))) return rc;
    if ((rc = scratch(ctx, "rect_in_rh", rbytes, (void **)&d_rh))) return rc;
    if ((rc = scratch(ctx, "rect_in_rn", in.N * 4ull, (void **)&d_rn))) return rc;
    HIPC(hipMemcpyAsync(d_qh, in.qh, qbytes, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_qn, in.qn, in.Q * 4ull, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_rh, in.rh, rbytes, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_rn, in.rn, in.N * 4ull, hipMemcpyHostToDevice, st));
    *dev = RectSets{d_qh, d_qn, in.Q, d_rh, d_rn, in.N};
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_dist_rect(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash, uint32_t Q,
                                     const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N, uint32_t q0,
                                     uint32_t q1, uint16_t *common_out, uint16_t *denom_out) {
    GUARD_CTX(ctx);
    const RectSets in{qhashes, qnhash, Q, rhashes, rnhash, N};
    if (rect_null(in)) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    RectSets dev;
    bool empty;
    int rc;
    if ((rc = rect_host_stage(ctx, in, q0, &q1, !common_out, &dev, &empty)) || empty) return rc;
    hipStream_t st = ctx->stream;
    uint16_t *d_c, *d_d = nullptr;
    const uint64_t cells = (uint64_t)(q1 - q0) * N;
    if ((rc = scratch(ctx, "rect_out_c", cells * 2, (void **)&d_c))) return rc;
    if (denom_out && (rc = scratch(ctx, "rect_out_d", cells * 2, (void **)&d_d))) return rc;
    if ((rc = timed(ctx, false, [&] { return rect_device_impl(ctx, dev, q0, q1, d_c, d_d, st, false); }))) return rc;
    HIPC(hipMemcpyAsync(common_out, d_c, cells * 2, hipMemcpyDeviceToHost, st));
    if (denom_out) HIPC(hipMemcpyAsync(denom_out, d_d, cells * 2, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_dist_rect_sparse_device(drephip_ctx *ctx, const uint64_t *d_qhashes,
                                                   const uint32_t *d_qnhash, uint32_t Q, const uint64_t *d_rhashes,
                                                   const uint32_t *d_rnhash, uint32_t N, uint32_t q0, uint32_t q1,
                                                   uint32_t *d_pairs, uint64_t cap, uint64_t *n_pairs, void *stream) {
    GUARD_CTX(ctx);
    const RectSets in{d_qhashes, d_qnhash, Q, d_rhashes, d_rnhash, N};
    if (rect_null(in) || !n_pairs || (cap && !d_pairs)) {
        set_error("null argument");
        return DREPHIP_ERR_ARG;
    }
    return timed(ctx, true, [&] {
        return rect_sparse_impl(ctx, in, q0, q1, (uint4 *)d_pairs, cap, n_pairs, pick_stream(ctx, stream));
    });
}

DREPHIP_EXPORT int drephip_dist_rect_sparse(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash,
                                            uint32_t Q, const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N,
                                            uint32_t q0, uint32_t q1, uint32_t *pairs, uint64_t cap,
                                            uint64_t *n_pairs) {
    GUARD_CTX(ctx);
    const RectSets in{qhashes, qnhash, Q, rhashes, rnhash, N};
    if (rect_null(in) || !n_pairs || (cap && !pairs)) {
        set_error("null argument");
        return DREPHIP_ERR_ARG;
    }
    *n_pairs = 0;
    RectSets dev;
    bool empty;
    int rc;
    if ((rc = rect_host_stage(ctx, in, q0, &q1, false, &dev, &empty)) || empty) return rc;
    hipStream_t st = ctx->stream;
    uint32_t *d_p = nullptr;
    if (cap && (rc = scratch(ctx, "rect_sp_out", cap * 16, (void **)&d_p))) return rc;
    rc = timed(ctx, true, [&] { return rect_sparse_impl(ctx, dev, q0, q1, (uint4 *)d_p, cap, n_pairs, st); });
    if (rc && rc != DREPHIP_ERR_NOMEM) return rc;
    return records_out(rc, d_p, nullptr, *n_pairs, cap, pairs, nullptr, st);
}

// ------------------------------------------------------------ significance
// The record calls with Mash's p-value and its -v / -d filters applied on the
// device, before the copy (pvalue.hip).
static int sig_args(drephip_ctx *ctx, double max_p, bool null_arg) {
    if (null_arg) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    if (!(max_p >= 0.0 && max_p <= 1.0)) { set_error("max_p must lie in [0, 1]"); return DREPHIP_ERR_ARG; }
    (void)ctx;
    return DREPHIP_OK;
}

// The record protocol's first half in the two _sig forms: the records counted
// (`list` with no buffer), room for exactly that many taken ("sig_rec"), the
// records listed into it and the two counts compared.  list(d_rec, cap, &n) is
// the form's sparse impl on its staged inputs.
template <class List>
static int sig_list(drephip_ctx *ctx, List &&list, uint4 **d_rec, uint64_t *listed) {
    uint64_t again = 0;
    *d_rec = nullptr;
    timing_begin(ctx);
    int rc = list(nullptr, 0, listed);
    if (rc && rc != DREPHIP_ERR_NOMEM) return rc;
    if (*listed) {
        if ((rc = scratch(ctx, "sig_rec", *listed * 16, (void **)d_rec))) return rc;
        timing_begin(ctx);
        if ((rc = list(*d_rec, *listed, &again))) return rc;
        if (again != *listed) { set_error("the record count changed between two runs"); return DREPHIP_ERR_INTERNAL; }
    }
    timing_collect(ctx);
    return DREPHIP_OK;
}

// What the two _sig forms share once the `listed` records are in d_rec: the
// lengths and cmin staged, the p-values, the stable filter, and the survivors
// (at most cap) copied out with their p-values.
static int sig_finish(drephip_ctx *ctx, const uint4 *d_rec, uint64_t listed, const uint64_t *len_a, uint32_t n_a,
                      const uint64_t *len_b, uint32_t n_b, double max_p, const uint32_t *cmin, uint32_t *pairs,
                      uint64_t cap, double *pval, uint64_t *n_pairs, hipStream_t st) {
    *n_pairs = 0;
    if (listed == 0) return DREPHIP_OK;
    uint64_t *d_la, *d_lb;
    uint32_t *d_cmin = nullptr;
    double *d_p, *d_pout;
    uint4 *d_out;
    int rc;
    if ((rc = scratch(ctx, "sig_len_a", n_a * 8ull, (void **)&d_la))) return rc;
    HIPC(hipMemcpyAsync(d_la, len_a, n_a * 8ull, hipMemcpyHostToDevice, st));
    d_lb = d_la;
    if (len_b != len_a || n_b != n_a) {
        if ((rc = scratch(ctx, "sig_len_b", n_b * 8ull, (void **)&d_lb))) return rc;
        HIPC(hipMemcpyAsync(d_lb, len_b, n_b * 8ull, hipMemcpyHostToDevice, st));
    }
    if (cmin) {
        if ((rc = scratch(ctx, "sig_cmin", (ctx->s + 1) * 4ull, (void **)&d_cmin))) return rc;
        HIPC(hipMemcpyAsync(d_cmin, cmin, (ctx->s + 1) * 4ull, hipMemcpyHostToDevice, st));
    }
    if ((rc = scratch(ctx, "sig_p", listed * 8, (void **)&d_p))) return rc;
    if ((rc = scratch(ctx, "sig_out", listed * 16, (void **)&d_out))) return rc;
    if ((rc = scratch(ctx, "sig_pout", listed * 8, (void **)&d_pout))) return rc;
    if ((rc = pvalue_records_impl(ctx, d_rec, listed, d_la, n_a, d_lb, n_b, d_p, st))) return rc;
    uint64_t kept = 0;
    if ((rc = records_filter_impl(ctx, d_rec, d_p, listed, max_p, d_cmin, d_out, d_pout, &kept, st))) return rc;
    *n_pairs = kept;
    if ((rc = records_out(DREPHIP_OK, d_out, d_pout, kept, cap, pairs, pval, st))) return rc;
    if (kept > cap) { set_error("more records than cap"); return DREPHIP_ERR_NOMEM; }
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_allpairs_sparse_sig(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash,
                                               uint32_t N, uint32_t row0, uint32_t row1, const uint64_t *length,
                                               double max_p, const uint32_t *cmin, uint32_t *pairs, uint64_t cap,
                                               double *pval, uint64_t *n_pairs, uint64_t *n_listed) {
    GUARD_CTX(ctx);
    int rc;
    if ((rc = sig_args(ctx, max_p, !hashes || !nhash || !length || !n_pairs || (cap && !pairs)))) return rc;
    *n_pairs = 0;
    if (n_listed) *n_listed = 0;
    hipStream_t st = ctx->stream;
    uint64_t *d_h;
    uint32_t *d_n;
    bool empty;
    if ((rc = tri_host_stage(ctx, hashes, nhash, length, N, row0, &row1, true, &d_h, &d_n, &empty)) || empty) return rc;
    uint4 *d_rec;
    uint64_t listed = 0;
    rc = sig_list(ctx, [&](uint4 *d, uint64_t room, uint64_t *n) {
        return allpairs_sparse_impl(ctx, d_h, d_n, N, row0, row1, d, room, n, st); }, &d_rec, &listed);
    if (rc) return rc;
    if (n_listed) *n_listed = listed;
    return sig_finish(ctx, d_rec, listed, length, N, length, N, max_p, cmin, pairs, cap, pval, n_pairs, st);
}

DREPHIP_EXPORT int drephip_dist_rect_sparse_sig(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash,
                                                uint32_t Q, const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N,
                                                uint32_t q0, uint32_t q1, const uint64_t *qlength,
                                                const uint64_t *rlength, double max_p, const uint32_t *cmin,
                                                uint32_t *pairs, uint64_t cap, double *pval, uint64_t *n_pairs,
                                                uint64_t *n_listed) {
    GUARD_CTX(ctx);
    const RectSets in{qhashes, qnhash, Q, rhashes, rnhash, N};
    int rc;
    if ((rc = sig_args(ctx, max_p, rect_null(in) || (Q && !qlength) || (N && !rlength) || !n_pairs || (cap && !pairs))))
        return rc;
    *n_pairs = 0;
    if (n_listed) *n_listed = 0;
    RectSets dev;
    bool empty;
    if ((rc = rect_host_stage(ctx, in, q0, &q1, false, &dev, &empty)) || empty) return rc;
    if ((rc = check_lengths(qlength, qnhash, Q)) || (rc = check_lengths(rlength, rnhash, N))) return rc;
    hipStream_t st = ctx->stream;
    uint4 *d_rec;
    uint64_t listed = 0;
    rc = sig_list(ctx, [&](uint4 *d, uint64_t room, uint64_t *n) { return rect_sparse_impl(ctx, dev, q0, q1, d, room, n, st); },
                  &d_rec, &listed);
    if (rc) return rc;
    if (n_listed) *n_listed = listed;
    return sig_finish(ctx, d_rec, listed, qlength, Q, rlength, N, max_p, cmin, pairs, cap, pval, n_pairs, st);
}

static int rect_top_args(uint32_t top) {
    if (top < 1 || top > 64) { set_error("top must be in 1..64"); return DREPHIP_ERR_ARG; }
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_dist_rect_top_device(drephip_ctx *ctx, const uint64_t *d_qhashes, const uint32_t *d_qnhash,
                                                uint32_t Q, const uint64_t *d_rhashes, const uint32_t *d_rnhash,
                                                uint32_t N, uint32_t q0, uint32_t q1, uint32_t top, uint32_t *d_hits,
                                                uint32_t *d_count, void *stream) {
    GUARD_CTX(ctx);
    const RectSets in{d_qhashes, d_qnhash, Q, d_rhashes, d_rnhash, N};
    if (rect_null(in) || (Q && N && q0 < q1 && (!d_hits || !d_count))) {
        set_error("null argument");
        return DREPHIP_ERR_ARG;
    }
    int rc;
    if ((rc = rect_top_args(top))) return rc;
    return timed(ctx, false, [&] { return rect_top_impl(ctx, in, q0, q1, top, d_hits, d_count, pick_stream(ctx, stream)); });
}

DREPHIP_EXPORT int drephip_dist_rect_top(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash, uint32_t Q,
                                         const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N, uint32_t q0,
                                         uint32_t q1, uint32_t top, uint32_t *hits, uint32_t *count) {
    GUARD_CTX(ctx);
    const RectSets in{qhashes, qnhash, Q, rhashes, rnhash, N};
    if (rect_null(in)) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    RectSets dev;
    bool empty;
    int rc;
    if ((rc = rect_top_args(top))) return rc;
    if ((rc = rect_host_stage(ctx, in, q0, &q1, !hits || !count, &dev, &empty)) || empty) return rc;
    hipStream_t st = ctx->stream;
    uint32_t *d_h, *d_n;
    const uint64_t rows = q1 - q0;
    if ((rc = scratch(ctx, "rect_top_hits", rows * top * 16, (void **)&d_h))) return rc;
    if ((rc = scratch(ctx, "rect_top_count", rows * 4, (void **)&d_n))) return rc;
    if ((rc = timed(ctx, false, [&] { return rect_top_impl(ctx, dev, q0, q1, top, d_h, d_n, st); }))) return rc;
    HIPC(hipMemcpyAsync(hits, d_h, rows * top * 16, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(count, d_n, rows * 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_sparse_stats(drephip_ctx *ctx, uint32_t *blocks, uint64_t *direct, uint64_t *fallback,
                                             uint64_t *scratch_bytes) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (blocks) *blocks = ctx->sparse.blocks;
    if (direct) *direct = ctx->sparse.direct;
    if (fallback) *fallback = ctx->sparse.fallback;
    if (scratch_bytes) *scratch_bytes = ctx->sparse.scratch_bytes;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_distance_lut(int k, uint32_t denom, double *lut) {
    if (!lut || k < 1 || denom == 0) { set_error("bad argument"); return DREPHIP_ERR_ARG; }
    for (uint32_t c = 0; c <= denom; c++) {
        double d;
        if (c == denom) d = 0.0;
        else if (c == 0) d = 1.0;
        else {
            const double j = (double)c / (double)denom;
            d = -std::log(2.0 * j / (1.0 + j)) / (double)k;
            if (d > 1.0) d = 1.0;
        }
        lut[c] = d;
    }
    return DREPHIP_OK;
}

// The sketch kernel's prefilter on the host (prefilter.h: the inline functions
// k_sketch_hash21 calls), for tests/test_sketch_prefilter.py
DREPHIP_EXPORT int drephip_prefilter_eval(const uint64_t *q1, const uint64_t *q2, uint64_t n, uint64_t T,
                                          uint8_t *pass, uint8_t *exact) {
    if (n && (!q1 || !q2 || !pass || !exact)) { set_error("bad argument"); return DREPHIP_ERR_ARG; }
    const uint32_t Tp = prefilter_bound(T);
    for (uint64_t i = 0; i < n; i++) {
        pass[i] = prefilter_hi(q1[i], q2[i]) <= Tp;
        exact[i] = murmur_fin(q1[i], q2[i]) <= T;
    }
    return DREPHIP_OK;
}

// The sketch kernel's canonical-strand cut on the host (canon.h: the inline
// functions k_sketch_hash21 calls), for tests/test_sketch_canon.py and
// tests/test_sketch_tail.py.  The cut yields the tail table's index; the
// natural tail index comes back through the map the table was stored by
DREPHIP_EXPORT int drephip_canon_eval(const uint32_t *words, uint64_t n, uint32_t r, uint32_t *hi, uint32_t *tail) {
    if (r > 15 || (n && (!words || !hi || !tail))) { set_error("bad argument"); return DREPHIP_ERR_ARG; }
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t *f = words + 3 * i;           // F[m-2], F[m-1], F[m]
        uint32_t toff;
        canon_cut(~f[1], ~f[2], rev_fields16(f[0]), rev_fields16(f[1]), rev_fields16(f[2]), (int)r, hi[i], toff);
        tail[i] = tail_index_of_head(toff >> 3);
    }
    return DREPHIP_OK;
}

// Sparse linkage limits.  The automatic choice takes the sparse path only
// where it beats the dense GPU chain: a step there scans one row of the top's
// component on the host (~1 us per 1000 members) against ~6 us per GPU step,
// so the largest component may hold 4096 members (DREPHIP_LINK_SPARSE_MAXCOMP)
// and the matrices 2^28 cells (2 GB; DREPHIP_LINK_SPARSE_CELLS); the pair list
// is first counted on the device and not read back beyond 32 pairs per genome
// (+2^20).  Mash data at s = 1000 has a few random shared hashes per 1000
// unrelated pairs (two 5 Mbp genomes share ~6 random 21-mers), so beyond a few
// thousand genomes everything is one component and the dense path runs.  An
// explicit sparse request (drephip_set_linkage_path / drephip_linkage_sparse)
// allows 2^31 cells and any component size.
constexpr uint64_t kSparseMaxCells = 1ull << 31;      // 16 GB
constexpr uint64_t kSparseMaxPairs = 1ull << 26;      // device pair list: 768 MB

static uint64_t sparse_cells(const drephip_ctx *ctx) {
    return ctx->link_path == DREPHIP_LINK_PATH_SPARSE ? kSparseMaxCells : env_u64("DREPHIP_LINK_SPARSE_CELLS", 1ull << 28);
}
static uint32_t sparse_maxcomp(const drephip_ctx *ctx) {
    return ctx->link_path == DREPHIP_LINK_PATH_SPARSE ? 0xFFFFFFFFu
                                                      : (uint32_t)env_u64("DREPHIP_LINK_SPARSE_MAXCOMP", 4096);
}
static uint64_t sparse_pair_cap(const drephip_ctx *ctx, uint32_t n) {
    const uint64_t all = (uint64_t)n * (n - 1) / 2;
    const uint64_t cap = ctx->link_path == DREPHIP_LINK_PATH_SPARSE ? kSparseMaxPairs
                                                                    : std::min<uint64_t>(kSparseMaxPairs, 32ull * n + (1ull << 20));
    return std::min(all, cap);
}

static int linkage_size_ok(uint32_t n) {
    if (n <= 200000) return DREPHIP_OK;
    set_error("linkage supports n <= 200000 (n x n f64 matrix in HBM)");
    return DREPHIP_ERR_UNSUPPORTED;
}

// The bracket of a linkage call that runs: figures and timing reset, the wall
// clock started (returned); link_end collects both.
static double link_begin(drephip_ctx *ctx) {
    timing_begin(ctx);
    ctx->link = LinkStats{};
    return host_now_s();
}
static int link_end(drephip_ctx *ctx, double t0) {
    timing_collect(ctx);
    ctx->link.wall_s = host_now_s() - t0;
    return DREPHIP_OK;
}

// a sparse run (linkage_sparse_impl into ctx->link.sp) that produced Z
static void link_sparse_done(drephip_ctx *ctx, double matrix_s) {
    ctx->link.sparse = 1;
    ctx->link.matrix_s = matrix_s;
    ctx->link.chain_s = ctx->link.sp.setup_s + ctx->link.sp.chain_s;
    ctx->link.finish_s = ctx->link.sp.finish_s;
}

DREPHIP_EXPORT int drephip_set_linkage_path(drephip_ctx *ctx, int path) {
    GUARD_CTX(ctx);
    if (path < DREPHIP_LINK_PATH_AUTO || path > DREPHIP_LINK_PATH_SPARSE) { set_error("bad linkage path"); return DREPHIP_ERR_ARG; }
    ctx->link_path = path;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_linkage_sparse(uint32_t n, uint64_t npairs, const uint32_t *i, const uint32_t *j,
                                          const double *v, int method, double *Z) {
    if (n < 2) return DREPHIP_OK;
    if (!Z || (npairs && (!i || !j || !v))) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    // components too large for their matrices: the sparse-row chain
    return linkage_sparse_impl(n, npairs, i, j, v, method, kSparseMaxCells, 0xFFFFFFFFu, Z, nullptr, 1);
}

// the sparse path from a host condensed vector: the pairs below 1.0 when no
// value exceeds 1.0; returns 1 when it produced Z, 0 when the dense path must run
static int linkage_condensed_sparse(drephip_ctx *ctx, const double *y, uint32_t n, int method, double *Z, int *rc) {
    *rc = DREPHIP_OK;
    if (ctx->link_path == DREPHIP_LINK_PATH_DENSE) return 0;
    if (method == DREPHIP_LINK_WARD) {                 // no sparse form: dense, or refused when sparse is forced
        if (ctx->link_path == DREPHIP_LINK_PATH_SPARSE) { set_error(kLinkWardSparse); *rc = DREPHIP_ERR_UNSUPPORTED; }
        return 0;
    }
    const double t0 = host_now_s();
    // the pairs below 1.0, scanned by host threads over row ranges of equal
    // pair counts; any value above 1.0 (or NaN) means no sparse form, more
    // pairs than the cap means the dense path
    const uint64_t np_all = (uint64_t)n * (n - 1) / 2, cap = sparse_pair_cap(ctx, n);
    const unsigned T = host_threads();
    std::vector<uint32_t> rb(T + 1, n - 1);
    rb[0] = 0;
    for (unsigned k = 1; k < T; k++) {             // first row whose pairs start at or after k/T of all
        const uint64_t target = np_all * k / T;
        uint32_t lo = rb[k - 1], hi = n - 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if ((uint64_t)mid * n - (uint64_t)mid * (mid + 1) / 2 < target) lo = mid + 1; else hi = mid;
        }
        rb[k] = lo;
    }
    std::vector<std::vector<uint32_t>> qi(T), qj(T);
    std::vector<std::vector<double>> qv(T);
    std::atomic<int> above(0);
    std::atomic<uint64_t> found(0);
    {
        std::vector<std::thread> pool;
        for (unsigned k = 0; k < T; k++)
            pool.emplace_back([&, k] {
                uint64_t t = (uint64_t)rb[k] * n - (uint64_t)rb[k] * (rb[k] + 1) / 2;
                for (uint32_t a = rb[k]; a < rb[k + 1] && !above.load(std::memory_order_relaxed); a++) {
                    uint64_t local = 0;
                    for (uint32_t b = a + 1; b < n; b++, t++) {
                        const double d = y[t];
                        // above 1.0, NaN or negative: no sparse form (scipy takes negative
                        // values; the dense path does too)
                        if (!(d <= 1.0) || d < 0.0) { above = 1; return; }
                        if (d < 1.0) { qi[k].push_back(a); qj[k].push_back(b); qv[k].push_back(d); local++; }
                    }
                    if (found.fetch_add(local) + local > cap) return;     // dense path; stop early
                }
            });
        for (auto &th : pool) th.join();
    }
    if (above) {
        if (ctx->link_path == DREPHIP_LINK_PATH_SPARSE) { set_error("sparse linkage: a distance above 1.0, below 0 or NaN"); *rc = DREPHIP_ERR_ARG; }
        return 0;
    }
    if (found.load() > cap) {
        if (ctx->link_path == DREPHIP_LINK_PATH_SPARSE) { set_error("sparse linkage: more pairs below 1.0 than the pair list holds"); *rc = DREPHIP_ERR_UNSUPPORTED; }
        return 0;
    }
    std::vector<uint32_t> pi, pj;
    std::vector<double> pv;
    pi.reserve(found.load()); pj.reserve(found.load()); pv.reserve(found.load());
    for (unsigned k = 0; k < T; k++) {
        pi.insert(pi.end(), qi[k].begin(), qi[k].end());
        pj.insert(pj.end(), qj[k].begin(), qj[k].end());
        pv.insert(pv.end(), qv[k].begin(), qv[k].end());
    }
    const double t1 = host_now_s();
    const int r = linkage_sparse_impl(n, pi.size(), pi.data(), pj.data(), pv.data(), method, sparse_cells(ctx),
                                      sparse_maxcomp(ctx), Z, &ctx->link.sp,
                                      ctx->link_path == DREPHIP_LINK_PATH_SPARSE ? 1 : 0);
    if (r == DREPHIP_ERR_UNSUPPORTED && ctx->link_path != DREPHIP_LINK_PATH_SPARSE) return 0;
    if (r) { *rc = r; return 0; }
    link_sparse_done(ctx, t1 - t0);
    return 1;
}

DREPHIP_EXPORT int drephip_linkage(drephip_ctx *ctx, const double *y, uint32_t n, int method, double *Z) {
    GUARD_CTX(ctx);
    if (n < 2) return DREPHIP_OK;
    if (!y || !Z) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc;
    if ((rc = linkage_size_ok(n))) return rc;
    if (!link_method_dense(method)) { set_error(kLinkMethodRefusal); return DREPHIP_ERR_UNSUPPORTED; }
    const double t0 = link_begin(ctx);
    if (!linkage_condensed_sparse(ctx, y, n, method, Z, &rc)) {
        if (rc) return rc;
        double *d_D;
        rc = dist_from_condensed_impl(ctx, y, n, &d_D, ctx->stream, method == DREPHIP_LINK_WARD);
        if (rc) return rc;
        rc = linkage_device_impl(ctx, d_D, n, method, Z, ctx->stream);
        if (rc) return rc;
    }
    return link_end(ctx, t0);
}

DREPHIP_EXPORT int drephip_linkage_square(drephip_ctx *ctx, const float *M, uint32_t n, int method, double *Z) {
    GUARD_CTX(ctx);
    if (n < 2) return DREPHIP_OK;
    if (!M || !Z) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc;
    if ((rc = linkage_size_ok(n))) return rc;
    if (!link_method_dense(method)) { set_error(kLinkMethodRefusal); return DREPHIP_ERR_UNSUPPORTED; }
    const double t0 = link_begin(ctx);
    double *d_D;
    uint32_t flags = 0;
    if ((rc = dist_from_square_impl(ctx, M, n, &d_D, &flags, ctx->stream))) return rc;
    // scipy's order: squareform's symmetry check, its diagonal check, then linkage's finiteness check
    if (flags & 1) { set_error("Distance matrix 'X' must be symmetric."); return DREPHIP_ERR_ARG; }
    if (flags & 2) { set_error("Distance matrix 'X' diagonal must be zero."); return DREPHIP_ERR_ARG; }
    if (flags & 4) { set_error("The condensed distance matrix must contain only finite values."); return DREPHIP_ERR_ARG; }
    if ((flags & 8) && method == DREPHIP_LINK_WARD) { set_error(kLinkWardNegative); return DREPHIP_ERR_UNSUPPORTED; }
    if ((rc = linkage_device_impl(ctx, d_D, n, method, Z, ctx->stream))) return rc;
    return link_end(ctx, t0);
}

DREPHIP_EXPORT int drephip_linkage_counts_device(drephip_ctx *ctx, const uint16_t *d_common, const uint16_t *d_denom,
                                                 uint32_t n, const uint32_t *perm, const double *lut,
                                                 uint32_t lut_len, const int32_t *lut_off, int method, double *Z,
                                                 void *stream) {
    GUARD_CTX(ctx);
    if (n < 2) return DREPHIP_OK;
    if (!d_common || !perm || !lut || !lut_off || !Z) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc;
    if ((rc = linkage_size_ok(n)) || (rc = check_lut(lut_off, lut_len, ctx->s, d_denom != nullptr)) || (rc = check_perm(perm, n)))
        return rc;
    // the counts are read after everything the caller queued on `stream`
    // (e.g. the all-pairs call that wrote them, deferred or not)
    if ((rc = allpairs_wait_impl(ctx))) return rc;
    HIPC(hipStreamSynchronize(pick_stream(ctx, stream)));
    const double t0 = link_begin(ctx);
    bool done = false;
    if (method == DREPHIP_LINK_WARD && ctx->link_path == DREPHIP_LINK_PATH_SPARSE) {
        set_error(kLinkWardSparse);
        return DREPHIP_ERR_UNSUPPORTED;
    }
    if (ctx->link_path != DREPHIP_LINK_PATH_DENSE && method != DREPHIP_LINK_WARD) {
        // sparse path: the pairs below 1.0 (nonzero counts) extracted on the GPU,
        // scipy's algorithm replayed on them on the host (linkage_sparse.cpp)
        const bool forced = ctx->link_path == DREPHIP_LINK_PATH_SPARSE;
        const uint64_t cap = sparse_pair_cap(ctx, n);
        uint32_t *ij = nullptr, *lidx = nullptr, flags = 0;
        uint64_t np = 0;
        rc = sparse_pairs_impl(ctx, d_common, d_denom, n, perm, lut, lut_len, lut_off, cap, &ij, &lidx, &np, &flags,
                               ctx->stream);
        if (rc) return rc;
        ctx->link.sp.pairs = np;
        if (flags & 1) {
            set_error("a pair's denominator has no distance table (lut_off < 0) or its count exceeds it");
            return DREPHIP_ERR_ARG;
        }
        const double t1 = host_now_s() - t0;
        if (!(flags & 2) && np <= cap) {
            std::vector<uint32_t> pi(np), pj(np);
            std::vector<double> pv(np);
            for (uint64_t t = 0; t < np; t++) { pi[t] = ij[2 * t]; pj[t] = ij[2 * t + 1]; pv[t] = lut[lidx[t]]; }
            rc = linkage_sparse_impl(n, np, pi.data(), pj.data(), pv.data(), method, sparse_cells(ctx),
                                     sparse_maxcomp(ctx), Z, &ctx->link.sp, forced ? 1 : 0);
            if (rc == DREPHIP_OK) {
                done = true;
                link_sparse_done(ctx, t1);
            } else if (rc != DREPHIP_ERR_UNSUPPORTED || forced) {
                return rc;
            }
        } else if (forced) {
            set_error(flags & 2 ? "sparse linkage: the distance table holds a value above 1.0 (or 0 shared hashes is not 1.0)"
                                : "sparse linkage: more pairs below 1.0 than the pair list holds");
            return DREPHIP_ERR_UNSUPPORTED;
        }
    }
    if (!done) {
        double *d_D;
        rc = dist_matrix_impl(ctx, d_common, d_denom, n, perm, lut, lut_len, lut_off, &d_D, ctx->stream,
                              method == DREPHIP_LINK_WARD);
        if (rc) return rc;
        rc = linkage_device_impl(ctx, d_D, n, method, Z, ctx->stream);
        if (rc) return rc;
    }
    return link_end(ctx, t0);
}

DREPHIP_EXPORT int drephip_linkage_reserve(drephip_ctx *ctx, uint32_t n) {
    GUARD_CTX(ctx);
    if (int rc = linkage_size_ok(n)) return rc;
    if (n < 2) return DREPHIP_OK;
    void *p;
    return scratch(ctx, "lk_D", (uint64_t)n * n * 8, &p);
}

DREPHIP_EXPORT int drephip_last_linkage_info(drephip_ctx *ctx, int *sparse, uint64_t *pairs, uint32_t *components,
                                             uint32_t *largest) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (!sparse || !pairs || !components || !largest) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    *sparse = ctx->link.sparse;
    *pairs = ctx->link.sp.pairs;
    *components = ctx->link.sp.components;
    *largest = ctx->link.sp.largest;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_linkage_launches(drephip_ctx *ctx, uint64_t *launches) {
    if (!ctx || !launches) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    *launches = ctx->link.launches;
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_last_linkage_stats(drephip_ctx *ctx, double *alloc_s, double *matrix_s, double *chain_s,
                                              double *finish_s, double *wall_s) {
    if (!ctx) { set_error("null context"); return DREPHIP_ERR_ARG; }
    if (!alloc_s || !matrix_s || !chain_s || !finish_s || !wall_s) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    *alloc_s = ctx->link.alloc_s;
    *matrix_s = ctx->link.matrix_s;
    *chain_s = ctx->link.chain_s;
    *finish_s = ctx->link.finish_s;
    *wall_s = ctx->link.wall_s;
    return DREPHIP_OK;
}
