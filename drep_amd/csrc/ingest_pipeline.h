// ingest_pipeline.h -- the host machinery of drephip_sketch_files that both
// ingest paths share: the look at a file, the choice of a batch's files and
// regions, the worker pool and the double-buffered producer / consumer.
// Plain C++ threads and stdio: it calls no HIP runtime function, so
// tools/ingest_pipeline_check.cpp runs it without a GPU (and under the thread
// sanitizer).  The stages themselves are in ingest_pipeline.cpp.
#pragma once

#include "common.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

namespace drephip {

using IngestClock = std::chrono::steady_clock;
inline double seconds_since(IngestClock::time_point t0) {
    return std::chrono::duration<double>(IngestClock::now() - t0).count();
}

// ------------------------------------------------------------------- probe
// One look at a file: its size, whether it is gzip, and an upper bound on its
// bases (every base is one byte of the uncompressed text): the size of a plain
// file; for a gzip file its trailer's ISIZE (the uncompressed size mod 2^32 of
// the LAST member -- exact for the usual single-member file; a multi-member
// (bgzf) file shows an ISIZE below its compressed size and gets the generic
// guess of 4x).  A wrong guess costs an overflow repack, never a wrong result.
struct FileProbe {
    uint64_t size = 0, est = 0;
    bool gz = false;
};
// false: it cannot be opened (*p stays all zero)
inline bool probe_file(const char *path, FileProbe *p) {
    *p = FileProbe();
    FILE *fp = fopen(path, "rb");
    if (!fp) return false;
    uint8_t magic[2] = {0, 0};
    const size_t got = fread(magic, 1, 2, fp);
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    p->size = p->est = sz > 0 ? (uint64_t)sz : 0;
    p->gz = got == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    uint8_t t[4];
    if (p->gz && sz >= 18 && fseek(fp, -4, SEEK_END) == 0 && fread(t, 1, 4, fp) == 4) {
        const uint64_t isize = (uint64_t)t[0] | (uint64_t)t[1] << 8 | (uint64_t)t[2] << 16 | (uint64_t)t[3] << 24;
        p->est = isize >= p->size ? isize : 4 * p->size;
    }
    fclose(fp);
    return true;
}

// -------------------------------------------------------------------- plan
// One batch: files [g0, ...) taken until their estimated bases reach `target`
// (at least one), each given a tile-aligned region of its estimate's padded
// span, the first at kTile.  A plain file also gets room for its bytes in the
// batch's text, at a 16-byte aligned start (the device path's; the host path
// ignores it).  A file that cannot be opened counts as empty here; `unopened`
// is the first such file of the batch, for the path that stops at it (the other
// leaves the error to its reader).
struct PlanFile : FileProbe {
    uint64_t off = 0, reserved = 0;          // region (bases)
    uint64_t text_beg = 0, text_end = 0;     // its bytes in the batch's text (gzip: none)
};
struct BatchPlan {
    std::vector<PlanFile> files;
    uint64_t bases = kTile;                  // end of the last region
    uint64_t text_span = 0;                  // bytes of text, alignment gaps included
    int unopened = -1;
};
inline BatchPlan plan_batch(const char *const *paths, uint32_t g0, uint32_t n_genomes, uint64_t target) {
    BatchPlan plan;
    uint64_t est_total = 0;
    for (uint32_t g = g0; g < n_genomes && (g == g0 || est_total < target); g++) {
        PlanFile f;
        if (!probe_file(paths[g], &f) && plan.unopened < 0) plan.unopened = (int)(g - g0);
        f.off = plan.bases;
        f.reserved = padded_span(f.est);
        plan.bases += f.reserved;
        f.text_beg = plan.text_span;
        f.text_end = f.gz ? f.text_beg : f.text_beg + f.size;
        plan.text_span = round_up(f.text_end, 16);
        est_total += f.est;
        plan.files.push_back(f);
    }
    return plan;
}

// -------------------------------------------------------------------- pool
// fn(worker, item) for every item in [0, n), items handed out dynamically to
// pool_size(n, threads) workers; the calling thread is worker 0.  threads <= 0:
// as many as the machine has hardware threads.
inline uint32_t pool_size(uint32_t n, int threads) {
    const int64_t nt = threads > 0 ? threads : (int64_t)std::thread::hardware_concurrency();
    return (uint32_t)std::max<int64_t>(1, std::min<int64_t>(nt, n));
}
template <class F>
void worker_pool(uint32_t n, int threads, F fn) {
    std::atomic<uint32_t> next(0);
    auto run = [&](uint32_t w) {
        for (uint32_t i = next++; i < n; i = next++) fn(w, i);
    };
    const uint32_t nt = pool_size(n, threads);
    std::vector<std::thread> pool;
    for (uint32_t w = 1; w < nt; w++) pool.emplace_back(run, w);
    run(0);
    for (auto &th : pool) th.join();
}

// ---------------------------------------------------------------- pipeline
// What the driver needs of a batch; the stages' batch types add their own.
struct PipelineBatch {
    uint32_t g0 = 0, n = 0;            // genomes [g0, g0 + n): g0 set by the driver, n by produce (>= 1)
    int err = 0;                       // produce failed: the call's return code and error text
    std::string msg;
    double seconds = 0;                // produce's wall time (the driver's clock)
    double read_thread_s = 0, pack_thread_s = 0;
};

// Ingest pipeline: one producer thread runs produce(i, first genome, slot,
// batch) for batch i + 1 (into the other of two slots) while the calling thread
// runs consume(batch, slot) -> return code for batch i -- the GPU work hides
// behind the host ingest, which is the slower side by an order of magnitude.
// The producer lives for the whole call (a thread per batch paid the HIP
// runtime's per-thread setup and teardown, ~30 ms, on every batch).  Batches
// are consumed once each, in order; slot i & 1 is the producer's from the
// moment batch i - 2 is released until it hands batch i over.  The first error
// of either side ends the call after the producer is joined.  `st` takes the
// figures both paths keep alike (ctx.h, IngestStats).
template <class Batch, class Stats, class Produce, class Consume>
int run_pipeline(uint32_t n_genomes, Stats &st, Produce produce, Consume consume) {
    if (n_genomes == 0) return 0;
    const auto t0 = IngestClock::now();
    Batch B[2];
    std::mutex mu;
    std::condition_variable cv;
    uint32_t produced = 0, consumed = 0;            // batches handed over / released
    bool stop = false;
    std::thread producer([&] {
        uint32_t g = 0;
        for (uint32_t i = 0; g < n_genomes; i++) {
            {   // slot i & 1 is free once batch i - 2 has been consumed
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || consumed + 2 > i; });
                if (stop) return;
            }
            Batch &b = B[i & 1];
            b = Batch();
            b.g0 = g;
            const auto p0 = IngestClock::now();
            produce(i, g, i & 1, b);
            b.seconds = seconds_since(p0);
            const bool last = b.err || g + b.n >= n_genomes;
            g += b.n;
            {
                std::lock_guard<std::mutex> lk(mu);
                produced = i + 1;
            }
            cv.notify_all();
            if (last) return;
        }
    });
    int rc = 0;
    for (uint32_t b = 0;; b++) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return produced > b; });
        }
        Batch &cur = B[b & 1];
        if (cur.err) { set_error(cur.msg); rc = cur.err; break; }
        const bool more = cur.g0 + cur.n < n_genomes;
        const auto c0 = IngestClock::now();
        rc = consume(cur, b & 1);
        st.gpu_s += seconds_since(c0);
        st.produce_s += cur.seconds;
        st.read_thread_s += cur.read_thread_s;
        st.pack_thread_s += cur.pack_thread_s;
        st.batches++;
        {
            std::lock_guard<std::mutex> lk(mu);
            consumed = b + 1;
        }
        cv.notify_all();
        if (rc || !more) break;
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;                                // a producer waiting for a slot ends
    }
    cv.notify_all();
    producer.join();
    st.wall_s = seconds_since(t0);
    return rc;
}

}  // namespace drephip
