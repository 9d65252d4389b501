// ingest_pipeline_check.cpp -- host check of drep_amd/csrc/ingest_pipeline.h,
// the machinery both paths of drephip_sketch_files share: the producer /
// consumer driver under fake stages that record what they see (order, slot
// ownership, errors on either side with the other parked or mid-batch), the
// batch plan on files written to a temporary directory, and the worker pool.
// No GPU.  Build (a sanitizer build is the point of it: address + undefined
// behaviour, and again with -fsanitize=thread):
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined \
//         -I drep_amd/csrc tools/ingest_pipeline_check.cpp -o tools/bin/ingest_pipeline_check -lz
// Exit status 0: every case agreed.
#include "ingest_pipeline.h"

#include <unistd.h>
#include <zlib.h>
#include <cstdlib>
#include <cstring>
#include <string>

namespace drephip {
static std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
}  // namespace drephip
using namespace drephip;

static int g_cases = 0, g_bad = 0;
static void check(bool ok, const char *what, long a = 0, long b = 0, long c = 0) {
    g_cases++;
    if (ok) return;
    g_bad++;
    fprintf(stderr, "FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
}

// ------------------------------------------------------------------ driver
struct FakeBatch : PipelineBatch {
    uint32_t index = 0;
    std::vector<uint32_t> payload;     // written by produce, read by consume: a race on it is a sanitizer report
};
struct FakeStats {
    double gpu_s = 0, produce_s = 0, read_thread_s = 0, pack_thread_s = 0, wall_s = 0;
    uint32_t batches = 0;
};
constexpr int kProducerError = -3, kConsumerError = -7;

// n_batches batches of two genomes (the last of one); producer_us / consumer_us:
// how long a stage holds its slot; perr / cerr: the batch at which that side fails.
static void drive(uint32_t n_batches, int perr, int cerr, int producer_us, int consumer_us) {
    const uint32_t n_genomes = 2 * n_batches - 1;
    std::atomic<int> owner[2];         // 0 nobody, 1 the producer, 2 the consumer
    owner[0] = owner[1] = 0;
    std::atomic<uint32_t> released(0); // batches the consumer is done with
    std::atomic<int> violations(0);
    std::vector<uint32_t> produced, consumed;   // each written by its own thread, read after the call
    FakeStats st;
    g_err.clear();
    const int rc = run_pipeline<FakeBatch>(
        n_genomes, st,
        [&](uint32_t i, uint32_t g, uint32_t slot, FakeBatch &b) {
            if (slot != (i & 1) || b.g0 != g || g != 2 * i) violations++;
            if (i >= 2 && released.load() + 2 <= i) violations++;      // batch i - 2 not released yet
            if (owner[slot].exchange(1) != 0) violations++;
            produced.push_back(i);
            b.index = i;
            b.payload.assign(64, i);
            usleep(producer_us);
            for (uint32_t v : b.payload) violations += v != i;
            b.n = std::min(2u, n_genomes - g);
            b.read_thread_s = 1;
            b.pack_thread_s = 2;
            if ((int)i == perr) { b.err = kProducerError; b.msg = "fake producer error " + std::to_string(i); }
            if (owner[slot].exchange(0) != 1) violations++;
        },
        [&](FakeBatch &b, uint32_t slot) {
            if (owner[slot].exchange(2) != 0) violations++;
            if (slot != (b.index & 1) || b.g0 != 2 * b.index) violations++;
            consumed.push_back(b.index);
            usleep(consumer_us);
            for (uint32_t v : b.payload) violations += v != b.index;
            if (owner[slot].exchange(0) != 2) violations++;
            released = b.index + 1;
            if ((int)b.index == cerr) { set_error("fake consumer error"); return kConsumerError; }
            return 0;
        });
    // (a producer thread left running would have ended the program in std::thread's destructor)
    const long tag = n_batches * 100 + (perr >= 0 ? 10 + perr : cerr >= 0 ? 20 + cerr : 0);
    check(violations == 0, "slot ownership / hand-off", tag, violations);
    bool order = true;
    for (size_t j = 0; j < consumed.size(); j++) order &= consumed[j] == j;
    for (size_t j = 0; j < produced.size(); j++) order &= produced[j] == j;
    check(order, "batches in order, once each", tag);
    check(st.batches == consumed.size() && st.read_thread_s == consumed.size() && st.pack_thread_s == 2.0 * consumed.size() &&
              st.wall_s > 0,
          "driver statistics", tag, st.batches);
    if (perr >= 0) {
        check(rc == kProducerError && g_err == "fake producer error " + std::to_string(perr), "producer error comes back", tag, rc);
        check(consumed.size() == (size_t)perr && produced.size() == (size_t)perr + 1, "producer error: batches before it consumed",
              tag, consumed.size(), produced.size());
    } else if (cerr >= 0) {
        check(rc == kConsumerError && g_err == "fake consumer error", "consumer error comes back", tag, rc);
        check(consumed.size() == (size_t)cerr + 1 && produced.size() <= (size_t)cerr + 3 && produced.size() >= consumed.size(),
              "consumer error: nothing past batch j + 2 produced", tag, consumed.size(), produced.size());
    } else {
        check(rc == 0 && consumed.size() == n_batches && produced.size() == n_batches, "every batch consumed", tag, rc,
              consumed.size());
    }
}

static void check_driver() {
    for (uint32_t n : {1u, 2u, 3u, 7u})
        for (int slow = 0; slow < 3; slow++)       // neither side, the producer, the consumer the slower one
            drive(n, -1, -1, slow == 1 ? 1500 : 100, slow == 2 ? 1500 : 100);
    for (int at : {0, 1, 3})
        for (int slow = 0; slow < 2; slow++) {
            drive(7, at, -1, slow ? 1500 : 50, slow ? 50 : 1500);
            // the consumer fails with a fast producer parked for a slot, and with a slow one mid-batch
            drive(7, -1, at, slow ? 3000 : 50, slow ? 300 : 3000);
        }
    FakeStats st;                                  // no genomes: neither stage runs
    check(run_pipeline<FakeBatch>(0, st, [](uint32_t, uint32_t, uint32_t, FakeBatch &) { abort(); },
                                  [](FakeBatch &, uint32_t) { abort(); return 0; }) == 0 && st.batches == 0, "empty call");
}

// -------------------------------------------------------------------- plan
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
static std::string acgt(size_t n) {
    std::string s(n, 'A');
    for (auto &c : s) c = "ACGT"[rnd() & 3];
    return s;
}
static void write_file(const std::string &path, const std::string &bytes) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp || fwrite(bytes.data(), 1, bytes.size(), fp) != bytes.size()) { perror(path.c_str()); exit(2); }
    fclose(fp);
}
static void gzip_member(const std::string &path, const std::string &bytes, const char *mode) {
    gzFile gz = gzopen(path.c_str(), mode);        // "ab" appends a member of its own
    if (!gz || gzwrite(gz, bytes.data(), (unsigned)bytes.size()) != (int)bytes.size()) { perror(path.c_str()); exit(2); }
    gzclose(gz);
}
static uint64_t file_size(const std::string &path) {
    FILE *fp = fopen(path.c_str(), "rb");
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fclose(fp);
    return (uint64_t)sz;
}

static void check_plan() {
    const char *tmp = getenv("TMPDIR");
    std::string dir = std::string(tmp && *tmp ? tmp : "/tmp") + "/ingest_pipeline_check.XXXXXX";
    if (!mkdtemp(&dir[0])) { perror("mkdtemp"); exit(2); }
    const std::string names[6] = {"plain.fa", "one.fa.gz", "two.fa.gz", "tiny.gz", "empty.fa", "missing.fa"};
    std::string path[6];
    for (int i = 0; i < 6; i++) path[i] = dir + "/" + names[i];
    const uint64_t kPlain = 70001, kOne = 50000;
    write_file(path[0], ">p\n" + acgt(kPlain - 4) + "\n");
    gzip_member(path[1], ">g\n" + acgt(kOne - 4) + "\n", "wb");
    gzip_member(path[2], ">g\n" + acgt(40000) + "\n", "wb");           // two members: the trailer's ISIZE is the
    gzip_member(path[2], acgt(100) + "\n", "ab");                      // second's 101, below the file's size
    write_file(path[3], std::string("\x1f\x8b", 2) + "12345678");      // the magic and no room for a trailer
    write_file(path[4], "");
    const uint64_t two_size = file_size(path[2]);
    check(file_size(path[1]) < kOne && two_size > 101 + 18, "the gzip files are what the cases need", file_size(path[1]), two_size);
    const char *paths[6];
    for (int i = 0; i < 6; i++) paths[i] = path[i].c_str();

    const uint64_t want_est[6] = {kPlain, kOne, 4 * two_size, 10, 0, 0};
    const uint64_t want_size[6] = {kPlain, file_size(path[1]), two_size, 10, 0, 0};
    const bool want_gz[6] = {false, true, true, true, false, false};
    for (int i = 0; i < 6; i++) {
        FileProbe p;
        const bool ok = probe_file(paths[i], &p);
        check(ok == (i != 5) && p.est == want_est[i] && p.size == want_size[i] && p.gz == want_gz[i], "probe", i, p.est, p.size);
    }
    // every file in one batch: regions and text
    const BatchPlan all = plan_batch(paths, 0, 6, ~0ull);
    check(all.files.size() == 6 && all.unopened == 5, "plan takes every file below the target", all.files.size(), all.unopened);
    uint64_t at = kTile, text = 0;
    for (size_t i = 0; i < all.files.size(); i++) {
        const PlanFile &f = all.files[i];
        check(f.est == want_est[i] && f.size == want_size[i] && f.gz == want_gz[i], "plan carries the probe", i);
        check(f.off == at && f.reserved == padded_span(want_est[i]) && f.reserved % kTile == 0 && f.reserved > f.est,
              "regions: tile multiples, contiguous from kTile", i, f.off, f.reserved);
        check(f.text_beg % 16 == 0 && f.text_beg >= text && f.text_end - f.text_beg == (f.gz ? 0 : f.size),
              "text: aligned starts, plain files only", i, f.text_beg, f.text_end);
        at += f.reserved;
        text = f.text_end;
    }
    check(all.bases == at && all.text_span == round_up(kPlain, 16) && all.text_span % 16 == 0, "plan totals", all.bases, all.text_span);
    check(all.files[0].reserved == 3 * kTile && all.files[4].reserved == kTile, "an empty file still has a tile");
    // take until the target is reached, at least one file
    struct { uint32_t g0; uint64_t target; size_t want; } take[] = {
        {0, 1, 1}, {1, 1, 1}, {3, 1, 1}, {4, 1, 2},                    // (the empty file adds no bases: the next one joins it)
        {5, 1, 1}, {0, kPlain, 1}, {0, kPlain + 1, 2}, {0, kPlain + kOne, 2}, {0, kPlain + kOne + 1, 3}, {2, ~0ull, 4},
    };
    for (auto &t : take) {
        const BatchPlan p = plan_batch(paths, t.g0, 6, t.target);
        check(p.files.size() == t.want && p.files[0].off == kTile && p.files[0].text_beg == 0, "take until target", t.g0,
              (long)t.target, p.files.size());
        check(p.unopened == (t.g0 + t.want == 6 ? (int)(5 - t.g0) : -1), "the unopened file is named from the batch's start", t.g0);
    }
    for (int i = 0; i < 5; i++) unlink(paths[i]);
    rmdir(dir.c_str());
}

// -------------------------------------------------------------------- pool
static void check_pool() {
    const std::thread::id me = std::this_thread::get_id();
    struct { uint32_t n; int threads; } cases[] = {{1000, 4}, {3, 16}, {50, 1}, {0, 4}, {1, 0}, {200, 0}};
    for (auto &c : cases) {
        const uint32_t nt = pool_size(c.n, c.threads);
        check(nt >= 1 && (c.threads <= 0 || nt == std::max(1u, std::min<uint32_t>(c.threads, c.n))), "pool size", c.n, c.threads, nt);
        std::vector<std::atomic<int>> seen(c.n);
        for (auto &s : seen) s = 0;
        std::atomic<int> wrong(0);
        std::vector<std::vector<uint32_t>> mine(nt);   // per worker, unshared: a worker index used twice is a race report
        worker_pool(c.n, c.threads, [&](uint32_t w, uint32_t i) {
            if (w >= nt || i >= c.n || (w == 0) != (std::this_thread::get_id() == me)) { wrong++; return; }
            seen[i]++;
            mine[w].push_back(i);
        });
        size_t total = 0;
        for (auto &m : mine) total += m.size();
        bool once = total == c.n;
        for (auto &s : seen) once &= s == 1;
        check(once && wrong == 0, "every item once, worker 0 on the calling thread", c.n, c.threads, wrong);
    }
}

int main() {
    check_driver();
    check_plan();
    check_pool();
    printf("ingest_pipeline_check: %d cases, %d disagree\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
