// ingest_pipeline.cpp -- drephip_sketch_files: FASTA files read, packed and
// sketched in batches, on the host path (worker threads parse and pack) or the
// device path (raw text to the GPU, ingest_device.hip packs).  The two paths
// are the stages below; the batch plan, the worker pool and the producer /
// consumer driver they share are in ingest_pipeline.h.
#include "ctx.h"
#include "ingest_pipeline.h"
#include "../../include/drephip.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cstring>

namespace drephip {

// The end of every batch: sketch the genomes staged in device memory and bring
// the sketches to the host.
static int sketch_batch_to_host(drephip_ctx *ctx, const uint32_t *d_codes, const uint32_t *d_valid,
                                const std::vector<uint64_t> &off, const std::vector<uint64_t> &pad,
                                const std::vector<uint64_t> &nk, uint64_t *hashes_out, uint32_t *nhash_out) {
    const uint32_t n = (uint32_t)off.size();
    hipStream_t st = ctx->stream;
    uint64_t *d_hashes;
    uint32_t *d_nhash;
    int rc;
    if ((rc = scratch(ctx, "out_hashes", (uint64_t)n * ctx->s * 8, (void **)&d_hashes))) return rc;
    if ((rc = scratch(ctx, "out_nhash", n * 4ull, (void **)&d_nhash))) return rc;
    timing_begin(ctx);
    rc = sketch_device_impl(ctx, d_codes, d_valid, off.data(), pad.data(), nk.data(), n, d_hashes, d_nhash, st);
    if (rc) return rc;
    timing_collect(ctx);
    HIPC(hipMemcpyAsync(hashes_out, d_hashes, (uint64_t)n * ctx->s * 8, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(nhash_out, d_nhash, n * 4ull, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return DREPHIP_OK;
}

int sketch_packed_host(drephip_ctx *ctx, const uint32_t *codes, uint64_t n_codes, const uint32_t *valid,
                       uint64_t n_valid, const std::vector<uint64_t> &off, const std::vector<uint64_t> &pad,
                       const std::vector<uint64_t> &nk, uint64_t *hashes_out, uint32_t *nhash_out) {
    uint32_t *d_codes, *d_valid;
    int rc;
    if ((rc = refuse_if_pending(ctx))) return rc;
    if ((rc = scratch(ctx, "in_codes", n_codes * 4, (void **)&d_codes))) return rc;
    if ((rc = scratch(ctx, "in_valid", n_valid * 4, (void **)&d_valid))) return rc;
    HIPC(hipMemcpyAsync(d_codes, codes, n_codes * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(d_valid, valid, n_valid * 4, hipMemcpyHostToDevice, ctx->stream));
    return sketch_batch_to_host(ctx, d_codes, d_valid, off, pad, nk, hashes_out, nhash_out);
}

static uint64_t ingest_batch_bases() {
    if (const uint64_t v = env_u64("DREPHIP_INGEST_BATCH_BASES", 0)) return v;     // tests: force many batches
    return 1ull << 30;                  // ~1 Gbase of sequence per batch
}

// A pool worker's reused read buffer (no fresh pages per file) and its clocks.
struct Worker {
    Genome g;
    double read_s = 0, pack_s = 0;
};
// The outcome of a pooled pass over a batch's files: the first failing file's,
// in file order.
struct PassErrors {
    std::vector<int> rc;
    std::vector<std::string> msg;
    explicit PassErrors(uint32_t n) : rc(n, 0), msg(n) {}
    void set(uint32_t i, int r, const std::string &m) { rc[i] = r; msg[i] = m; }
    int first(std::string *m) const {
        for (size_t i = 0; i < rc.size(); i++)
            if (rc[i]) { *m = msg[i]; return rc[i]; }
        return 0;
    }
};

struct Packed {
    uint64_t pad = 0, nk = 0, length = 0;
};
struct PackRoom {
    uint32_t *codes = nullptr, *valid = nullptr;    // null: no room, leave the genome unpacked in the worker
    uint64_t off = 0;
};
// One file through the host reader and, while its sequence is cache-hot, the
// packer, both on the worker's clocks.  room(padded span) gives the zeroed
// place to pack it at.
template <class Room>
static int read_and_pack(const char *path, int k, Worker &w, Packed &p, Room room) {
    const auto r0 = IngestClock::now();
    const int rr = read_fasta(path, w.g);
    const auto r1 = IngestClock::now();
    w.read_s += std::chrono::duration<double>(r1 - r0).count();
    if (rr) return DREPHIP_ERR_IO;
    const uint32_t nr = (uint32_t)w.g.rec_len.size();
    p.pad = padded_span(genome_span(w.g.rec_len.data(), nr));
    p.length = w.g.length;
    const PackRoom at = room(p.pad);
    if (!at.codes) return DREPHIP_OK;
    p.nk = pack_records(w.g.seq.data(), w.g.rec_len.data(), nr, k, at.codes, at.valid, at.off);
    w.pack_s += seconds_since(r1);
    return DREPHIP_OK;
}

// ------------------------------------------------------------- host ingest
// One batch of FASTA files read and packed into pinned host memory.
struct IngestBatch : PipelineBatch {
    std::vector<uint64_t> off, pad, nk, length;
    uint64_t bases = 0;                 // padded positions of the batch (codes/valid span)
    uint32_t overflow = 0;
};

// Grow a pinned slot keeping its first `keep_c` / `keep_v` words.
static int grow_pinned(PinnedSlot &slot, size_t cb, size_t vb, size_t keep_c, size_t keep_v) {
    PinnedSlot n;
    if (n.reserve(cb, vb)) return -1;
    memcpy(n.codes, slot.codes, keep_c * 4);
    memcpy(n.valid, slot.valid, keep_v * 4);
    std::swap(slot.codes, n.codes); std::swap(slot.codes_bytes, n.codes_bytes);
    std::swap(slot.valid, n.valid); std::swap(slot.valid_bytes, n.valid_bytes);
    return 0;                          // n frees the old buffers
}

// The host path's producer: ONE pass over the planned files on `threads`
// workers: a worker reads + parses a file and packs it straight into its
// region of the pinned batch (a genome whose real span outgrew its estimate is
// kept and packed after the pass, at the end of the batch).  Regions are zeroed
// by their worker; the slack between a genome's padded span and its region
// stays zero and no tile covers it.
static void produce_batch(const char *const *paths, uint32_t n_genomes, int threads, int k, uint64_t target,
                          PinnedSlot &slot, IngestBatch &B, int device) {
    (void)hipSetDevice(device);         // the pinned batch belongs with the context's device
    const BatchPlan plan = plan_batch(paths, B.g0, n_genomes, target);
    const uint32_t n = B.n = (uint32_t)plan.files.size();
    B.off.resize(n); B.pad.resize(n); B.nk.resize(n); B.length.resize(n);
    for (uint32_t i = 0; i < n; i++) B.off[i] = plan.files[i].off;
    const uint64_t cur = plan.bases;
    if (slot.reserve(cur / 16 * 4, cur / 32 * 4)) {
        B.err = DREPHIP_ERR_NOMEM; B.msg = "hipHostMalloc of the pinned ingest batch failed"; return;
    }
    memset(slot.codes, 0, kTile / 16 * 4);
    memset(slot.valid, 0, kTile / 32 * 4);
    PassErrors errs(n);
    std::vector<Genome> overflow(n);                 // genomes whose span outgrew the estimate (rare)
    std::vector<char> over(n, 0);
    std::vector<Worker> work(pool_size(n, threads));
    worker_pool(n, threads, [&](uint32_t w, uint32_t i) {
        const PlanFile &f = plan.files[i];
        Packed p;
        const int rc = read_and_pack(paths[B.g0 + i], k, work[w], p, [&](uint64_t P) {
            if (P > f.reserved) return PackRoom();
            memset(slot.codes + f.off / 16, 0, f.reserved / 16 * 4);
            memset(slot.valid + f.off / 32, 0, f.reserved / 32 * 4);
            return PackRoom{slot.codes, slot.valid, f.off};
        });
        if (rc) { errs.set(i, rc, drephip_last_error()); return; }
        B.pad[i] = p.pad; B.nk[i] = p.nk; B.length[i] = p.length;
        if (p.pad > f.reserved) { std::swap(overflow[i], work[w].g); over[i] = 1; }
    });
    if ((B.err = errs.first(&B.msg))) return;
    for (const Worker &w : work) { B.read_thread_s += w.read_s; B.pack_thread_s += w.pack_s; }
    uint64_t end = cur;
    for (uint32_t i = 0; i < n; i++) if (over[i]) { end += B.pad[i]; B.overflow++; }
    if (end > cur) {
        if (grow_pinned(slot, end / 16 * 4, end / 32 * 4, cur / 16, cur / 32)) {
            B.err = DREPHIP_ERR_NOMEM; B.msg = "hipHostMalloc of the pinned ingest batch failed"; return;
        }
        uint64_t at = cur;
        for (uint32_t i = 0; i < n; i++) {
            if (!over[i]) continue;
            const Genome &g = overflow[i];
            B.off[i] = at;
            memset(slot.codes + at / 16, 0, B.pad[i] / 16 * 4);
            memset(slot.valid + at / 32, 0, B.pad[i] / 32 * 4);
            B.nk[i] = pack_records(g.seq.data(), g.rec_len.data(), (uint32_t)g.rec_len.size(), k, slot.codes,
                                   slot.valid, at);
            at += B.pad[i];
        }
    }
    B.bases = end;
}

// ----------------------------------------------------------- device ingest
// One file read and packed by the host code into buffers of its own (the
// device path's gzip and FASTQ files), at base 0.
struct HostPacked : Packed {
    std::vector<uint32_t> codes, valid;
};
static int host_pack_file(const char *path, int k, Worker &w, HostPacked &hp) {
    return read_and_pack(path, k, w, hp, [&](uint64_t P) {
        hp.codes.assign(P / 16, 0);
        hp.valid.assign(P / 32, 0);
        return PackRoom{hp.codes.data(), hp.valid.data(), 0};
    });
}

// One batch of the device path: the plain files' bytes in a pinned text
// buffer (16-byte aligned starts), the gzip files packed by the host code.
struct TextBatch : PipelineBatch {
    BatchPlan plan;                             // each file's region, and a plain file's bytes in the text buffer
    std::vector<char> host;                     // 1: packed by the host code (hp)
    std::vector<HostPacked> hp;
    uint64_t text_bytes = 0;
};

// The device path's producer: on `threads` workers, each planned plain file's
// bytes go into the pinned text buffer with one pread, unparsed, and each gzip
// file through the host reader and packer.  A plain file whose size is no
// longer the probed one takes the host reader too, which reads it whole.
static void produce_text_batch(const char *const *paths, uint32_t n_genomes, int threads, int k, uint64_t target,
                               PinnedText &slot, TextBatch &B, int device) {
    (void)hipSetDevice(device);
    B.plan = plan_batch(paths, B.g0, n_genomes, target);
    std::vector<PlanFile> &files = B.plan.files;
    const uint32_t n = B.n = (uint32_t)files.size();
    if (B.plan.unopened >= 0) {
        B.err = DREPHIP_ERR_IO; B.msg = std::string("cannot open ") + paths[B.g0 + B.plan.unopened]; return;
    }
    for (const PlanFile &f : files) B.host.push_back(f.gz ? 1 : 0);
    B.hp.resize(n);
    if (slot.reserve(std::max<uint64_t>(B.plan.text_span, 16))) {
        B.err = DREPHIP_ERR_NOMEM; B.msg = "hipHostMalloc of the pinned text batch failed"; return;
    }
    PassErrors errs(n);
    std::vector<Worker> work(pool_size(n, threads));
    worker_pool(n, threads, [&](uint32_t w, uint32_t i) {
        const char *path = paths[B.g0 + i];
        PlanFile &f = files[i];
        if (!B.host[i]) {
            const auto r0 = IngestClock::now();
            const int fd = open(path, O_RDONLY);
            if (fd < 0) { errs.set(i, DREPHIP_ERR_IO, std::string("cannot open ") + path); return; }
            const uint64_t want = f.text_end - f.text_beg;
            struct stat sb;
            bool same = fstat(fd, &sb) == 0 && (uint64_t)sb.st_size == want;
            uint64_t got = 0;
            bool bad = false;
            while (same && got < want) {           // one pread, repeated only when it comes back short
                const ssize_t r = pread(fd, slot.ptr + f.text_beg + got, want - got, (off_t)got);
                if (r < 0) { bad = true; break; }
                if (r == 0) { same = false; break; }
                got += (uint64_t)r;
            }
            close(fd);
            if (bad) { errs.set(i, DREPHIP_ERR_IO, std::string("read error in ") + path); return; }
            work[w].read_s += seconds_since(r0);
            if (same) return;
            B.host[i] = 1;                         // the file changed since the probe
            f.text_end = f.text_beg;
        }
        const int rc = host_pack_file(path, k, work[w], B.hp[i]);
        if (rc) errs.set(i, rc, drephip_last_error());
    });
    if ((B.err = errs.first(&B.msg))) return;
    for (const Worker &w : work) { B.read_thread_s += w.read_s; B.pack_thread_s += w.pack_s; }
    for (const PlanFile &f : files) B.text_bytes += f.text_end - f.text_beg;
}

// The device path's consumer: text to the device, pack kernels, the host
// reader for the files the kernels hand back, then the device-resident sketch.
// A host-packed file (gzip, FASTQ, or a defensive status 2) is copied over its
// region, which is zeroed whole first: the slack behind a genome's padded span
// is read by the sketch of the genome that follows and must not keep what an
// earlier batch left in the scratch.  One whose span outgrew its region goes to
// the end of the batch (its old region zeroed all the same).
static int consume_text_batch(drephip_ctx *ctx, const char *const *paths, int threads, TextBatch &B,
                              const PinnedText &slot, uint64_t *hashes_out, uint32_t *nhash_out,
                              uint64_t *length_out) {
    const uint32_t n = B.n;
    const std::vector<PlanFile> &files = B.plan.files;
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> pad(n, 0), nk(n, 0), length(n, 0), off(n);
    uint32_t moved = 0, device_files = 0, host_files = 0;
    uint64_t end = B.plan.bases;
    for (uint32_t i = 0; i < n; i++) {
        off[i] = files[i].off;
        if (B.host[i] && B.hp[i].pad > files[i].reserved) { off[i] = end; end += B.hp[i].pad; moved++; }
    }
    uint8_t *d_text;
    uint32_t *d_codes, *d_valid;
    int rc;
    if ((rc = scratch(ctx, "in_text", std::max<uint64_t>(B.plan.text_span, 16), (void **)&d_text))) return rc;
    if ((rc = scratch(ctx, "in_codes", end / 16 * 4, (void **)&d_codes))) return rc;
    if ((rc = scratch(ctx, "in_valid", end / 32 * 4, (void **)&d_valid))) return rc;
    if (B.plan.text_span) HIPC(hipMemcpyAsync(d_text, slot.ptr, B.plan.text_span, hipMemcpyHostToDevice, st));
    HIPC(hipMemsetAsync(d_codes, 0, kTile / 16 * 4, st));
    HIPC(hipMemsetAsync(d_valid, 0, kTile / 32 * 4, st));
    for (uint32_t i = 0; i < n; i++) {                   // the host-packed files' regions (the pack call zeroes the others)
        if (!B.host[i]) continue;
        HIPC(hipMemsetAsync(d_codes + files[i].off / 16, 0, files[i].reserved / 16 * 4, st));
        HIPC(hipMemsetAsync(d_valid + files[i].off / 32, 0, files[i].reserved / 32 * 4, st));
    }
    std::vector<uint32_t> dev;                           // the plain files
    for (uint32_t i = 0; i < n; i++) if (!B.host[i]) dev.push_back(i);
    std::vector<uint32_t> back;                          // handed back to the host reader
    if (!dev.empty()) {
        const uint32_t m = (uint32_t)dev.size();
        std::vector<uint64_t> tb(m), te(m), bo(m), cp(m), ln(m), pd(m), kk(m);
        std::vector<uint32_t> nr(m);
        std::vector<uint8_t> stt(m);
        for (uint32_t j = 0; j < m; j++) {
            const PlanFile &f = files[dev[j]];
            tb[j] = f.text_beg; te[j] = f.text_end; bo[j] = f.off; cp[j] = f.reserved;
        }
        rc = fasta_pack_device_impl(ctx, d_text, tb.data(), te.data(), m, bo.data(), cp.data(), d_codes, d_valid, ln.data(),
                                    pd.data(), nr.data(), kk.data(), stt.data(), st);
        if (rc) return rc;
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t i = dev[j];
            if (stt[j] == 0) { length[i] = ln[j]; pad[i] = pd[j]; nk[i] = kk[j]; device_files++; }
            else back.push_back(i);
        }
    }
    if (!back.empty()) {
        const uint32_t m = (uint32_t)back.size();
        PassErrors errs(m);
        std::vector<Worker> work(pool_size(m, threads));
        worker_pool(m, threads, [&](uint32_t w, uint32_t j) {
            const int e = host_pack_file(paths[B.g0 + back[j]], ctx->k, work[w], B.hp[back[j]]);
            if (e) errs.set(j, e, drephip_last_error());
        });
        std::string msg;
        if ((rc = errs.first(&msg))) { set_error(msg); return rc; }
        for (const Worker &w : work) { ctx->ingest.read_thread_s += w.read_s; ctx->ingest.pack_thread_s += w.pack_s; }
        bool again = false;
        for (uint32_t i : back) {
            B.host[i] = 1;
            again |= B.hp[i].pad > files[i].reserved;
        }
        // A handed-back file that outgrew its region needs room behind the batch, as
        // a gzip file does: start over with it among the host-packed files (the
        // buffers may move).  A plain file's span never exceeds its size's, so
        // this is a defence only.
        if (again) return consume_text_batch(ctx, paths, threads, B, slot, hashes_out, nhash_out, length_out);
    }
    for (uint32_t i = 0; i < n; i++) {
        if (!B.host[i]) continue;
        const HostPacked &hp = B.hp[i];
        HIPC(hipMemcpyAsync(d_codes + off[i] / 16, hp.codes.data(), hp.pad / 16 * 4, hipMemcpyHostToDevice, st));
        HIPC(hipMemcpyAsync(d_valid + off[i] / 32, hp.valid.data(), hp.pad / 32 * 4, hipMemcpyHostToDevice, st));
        length[i] = hp.length; pad[i] = hp.pad; nk[i] = hp.nk;
        host_files++;
    }
    if (length_out) std::copy(length.begin(), length.end(), length_out + B.g0);
    rc = sketch_batch_to_host(ctx, d_codes, d_valid, off, pad, nk, hashes_out + (uint64_t)B.g0 * ctx->s, nhash_out + B.g0);
    if (rc) return rc;
    ctx->ingest_paths.text_bytes += B.text_bytes;
    ctx->ingest_paths.device_files += device_files;
    ctx->ingest_paths.host_files += host_files;
    ctx->ingest.overflow += moved;
    return DREPHIP_OK;
}

int sketch_files_impl(drephip_ctx *ctx, const char *const *paths, uint32_t n_genomes, int threads,
                      uint64_t *hashes_out, uint32_t *nhash_out, uint64_t *length_out) {
    const uint64_t target = ingest_batch_bases();
    const int k = ctx->k;
    if (ctx->ingest_path == DREPHIP_INGEST_DEVICE)
        return run_pipeline<TextBatch>(
            n_genomes, ctx->ingest,
            [&](uint32_t, uint32_t, uint32_t slot, TextBatch &B) {
                produce_text_batch(paths, n_genomes, threads, k, target, ctx->ingest_text[slot], B, ctx->device);
            },
            [&](TextBatch &B, uint32_t slot) {
                return consume_text_batch(ctx, paths, threads, B, ctx->ingest_text[slot], hashes_out, nhash_out,
                                          length_out);
            });
    ctx->ingest_paths.host_files = n_genomes;
    PinnedSlot *slots = ctx->ingest_slots;          // kept across calls: pinned allocation is slow
    return run_pipeline<IngestBatch>(
        n_genomes, ctx->ingest,
        [&](uint32_t, uint32_t, uint32_t slot, IngestBatch &B) {
            produce_batch(paths, n_genomes, threads, k, target, slots[slot], B, ctx->device);
        },
        [&](IngestBatch &B, uint32_t slot) {
            if (length_out) std::copy(B.length.begin(), B.length.end(), length_out + B.g0);
            ctx->ingest.overflow += B.overflow;
            return sketch_packed_host(ctx, slots[slot].codes, B.bases / 16, slots[slot].valid, B.bases / 32, B.off, B.pad,
                                      B.nk, hashes_out + (uint64_t)B.g0 * ctx->s, nhash_out + B.g0);
        });
}

}  // namespace drephip
