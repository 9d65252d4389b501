// fasta_machine_check.cpp -- host check of the device FASTA ingest's byte
// machine (drep_amd/csrc/fasta_machine.h): the tile / lane decomposition the
// kernels of ingest_device.hip use, replayed on the CPU through the same
// inline functions, against a line-by-line restatement of kseq's FASTA rules.
// No GPU.  Build (a sanitizer build is the point of it):
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined \
//         -I drep_amd/csrc tools/fasta_machine_check.cpp -o tools/bin/fasta_machine_check
// Exit status 0: every case agreed.
#include "fasta_machine.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

using namespace drephip;

struct Parsed {
    std::vector<std::pair<uint64_t, uint8_t>> bases;   // (position from the region start, byte)
    uint64_t length = 0, records = 0;
    bool plus = false;
};

// kseq's rules for FASTA, by lines: skip to the first '>' / '@'; the rest of
// that line is the header; then every line by its first byte.
static Parsed reference(const std::vector<uint8_t> &t) {
    Parsed p;
    const size_t n = t.size();
    size_t i = 0;
    while (i < n && t[i] != '>' && t[i] != '@') i++;
    if (i >= n || i + 1 == n) return p;               // no header, or it is the last byte
    p.records = 1;
    while (i < n && t[i] != '\n') i++;
    i++;
    while (i < n) {
        size_t e = i;
        while (e < n && t[e] != '\n') e++;             // line [i, e)
        const uint8_t c = t[i];
        if (e == i) {
        } else if (c == '>' || c == '@') {
            if (i + 1 < n) p.records++;
        } else if (c == '+') {
            p.plus = true;
            return p;
        } else {
            size_t le = e;
            if (t[le - 1] == '\r') le--;
            for (size_t j = i; j < le; j++) p.bases.push_back({p.length++ + p.records - 1, t[j]});
        }
        i = e + 1;
    }
    return p;
}

// The kernels' decomposition: lanes of kLaneBytes, tiles of kTextTile.
static Parsed tiled(const std::vector<uint8_t> &t) {
    Parsed p;
    const uint64_t n = t.size();
    const uint8_t *text = t.data();
    uint32_t state = ST_HUNT;
    uint64_t seq = 0, rec = 0;
    for (uint64_t t0 = 0; t0 < n; t0 += kTextTile) {
        std::vector<LaneText> lanes(kTextWG);
        std::vector<Sum> excl(kTextWG);
        Sum run = sum_identity();
        for (uint32_t l = 0; l < kTextWG; l++) {
            lanes[l] = load_lane(text, t0 + (uint64_t)l * kLaneBytes, n);
            excl[l] = run;
            run = compose(run, lane_summary(lanes[l]));
        }
        for (uint32_t l = 0; l < kTextWG; l++)
            lane_bases(lanes[l], excl[l].e[state], [&](uint32_t q, uint32_t r, uint32_t c) {
                p.bases.push_back({seq + q + rec + r - 1, (uint8_t)c});
            });
        const uint32_t y = run.e[state];
        state = y & 3u;
        p.plus |= (y & kPlusBit) != 0;
        seq += (y >> 3) & 0x3FFFu;
        rec += y >> 17;
    }
    p.length = seq;
    p.records = rec;
    return p;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static int compare(const std::vector<uint8_t> &t, const char *what, int id) {
    // the vector is sized exactly: a read past the file's end is a sanitizer report
    const Parsed a = reference(t), b = tiled(t);
    if (a.plus != b.plus) { fprintf(stderr, "%s %d: '+' flag %d vs %d\n", what, id, a.plus, b.plus); return 1; }
    if (a.plus) return 0;
    if (a.length != b.length || a.records != b.records || a.bases != b.bases) {
        fprintf(stderr, "%s %d (%zu bytes): length %llu vs %llu, records %llu vs %llu, bases %s\n", what, id, t.size(),
                (unsigned long long)a.length, (unsigned long long)b.length, (unsigned long long)a.records,
                (unsigned long long)b.records, a.bases == b.bases ? "equal" : "differ");
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0, cases = 0;
    const char *fixed[] = {"", ">", "@", ">a", ">\n", "x>y\nAC\n", "junk >h\nACGT\nacgtN\n>two\nGGGG\n", ">f\nACGT\n>",
                           ">f\nACGT\n>g", ">a\n>b\n>c\n", ">a\r\nACG\r\n\r\nTTA\r\n\n", ">a\nAC\r\r\nGT\r", ">a\n\r\nAC",
                           "no header at all\nACGT\n", ">a\nAC\n+\nII\n", "+\n>a\nAC\n", ">a\n\n\nAC\n\n", ">a\nAC>GT@\n"};
    for (const char *f : fixed) {
        const std::string s(f);
        bad += compare(std::vector<uint8_t>(s.begin(), s.end()), "fixed", cases++);
    }
    // random text over an alphabet rich in the bytes the machine cares about,
    // sizes around the lane, the 16-byte piece and the tile
    const char alpha_dense[] = "\n\n>@\r\rACGTacgtN+ x";
    const char alpha_seq[] = "ACGTACGTACGTacgtNRY\r";
    const uint32_t sizes[] = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, kTextTile - 1, kTextTile, kTextTile + 1,
                              2 * kTextTile, 3 * kTextTile + 5};
    for (int round = 0; round < 40; round++)
        for (uint32_t sz : sizes) {
            std::vector<uint8_t> t(sz);
            const bool dense = round & 1;
            const uint32_t line = 1 + rnd() % (round % 4 == 2 ? 3 * kTextTile : 90);
            for (uint32_t i = 0; i < sz; i++) {
                if (dense) t[i] = alpha_dense[rnd() % (sizeof(alpha_dense) - 1)];
                else if (i % line == line - 1) t[i] = '\n';
                else if (i % line == 0 && rnd() % 5 == 0) t[i] = ">@\n\rA"[rnd() % 5];
                else t[i] = alpha_seq[rnd() % (sizeof(alpha_seq) - 1)];
            }
            if (!dense && sz > 4 && round % 3) { t[0] = '>'; t[1] = 'h'; t[2] = '\n'; }
            // the '+' rule is checked on a few rounds; elsewhere it would end most dense cases early
            if (dense && round % 8 != 1) for (auto &c : t) if (c == '+') c = 'A';
            bad += compare(t, "random", cases++);
        }
    // every byte of interest at every offset around a tile boundary
    const char edge[] = "\n\r>@A";
    for (int d = -2; d <= 2; d++)
        for (char c1 : std::string(edge, 5))
            for (char c2 : std::string(edge, 5)) {
                std::vector<uint8_t> t(2 * kTextTile, 'A');
                t[0] = '>'; t[1] = '\n';
                for (uint32_t i = 70; i < t.size(); i += 71) t[i] = '\n';
                t[kTextTile + d - 1] = (uint8_t)c1;
                t[kTextTile + d] = (uint8_t)c2;
                bad += compare(t, "edge", cases++);
                t.resize(kTextTile + d + 1);           // and the same pair ending the file
                bad += compare(t, "edge-eof", cases++);
            }
    // the pack call's tile and chunk lists and the kernels' search in them, with
    // empty files and empty regions anywhere (also first, last and in a row)
    for (int round = 0; round < 200; round++) {
        const uint32_t n = 1 + rnd() % 12;
        std::vector<uint64_t> beg(n), end(n), cap(n);
        uint64_t at = 0;
        for (uint32_t f = 0; f < n; f++) {
            const uint32_t kind = rnd() % 4;
            const uint64_t sz = kind == 0 ? 0 : kind == 1 ? rnd() % 40 : rnd() % (3 * kTextTile + 2);
            beg[f] = at; end[f] = at + sz;
            at = (at + sz + 15) / 16 * 16;
            cap[f] = (uint64_t)(rnd() % 4) * 32768;
        }
        std::vector<uint32_t> tf, cf;
        int wrong = !build_firsts(beg.data(), end.data(), cap.data(), n, 32768, tf, cf);
        uint32_t t = 0, c = 0;
        for (uint32_t f = 0; f < n && !wrong; f++) {
            for (uint64_t o = 0; o < end[f] - beg[f]; o += kTextTile, t++)
                wrong |= find_file(tf.data(), n, t) != f || t - tf[f] != o / kTextTile;
            for (uint64_t o = 0; o < cap[f]; o += 32768, c++) wrong |= find_file(cf.data(), n, c) != f;
        }
        wrong |= t != tf[n] || c != cf[n];
        if (wrong) fprintf(stderr, "lists %d: tile or chunk lists disagree\n", round);
        bad += wrong;
        cases++;
    }
    printf("fasta_machine_check: %d cases, %d disagree\n", cases, bad);
    return bad ? 1 : 0;
}
