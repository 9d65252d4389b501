// api_checks_check.cpp -- host check of drep_amd/csrc/api_checks.h, the pure
// argument checks of the C API: the row check (ordered and not), the length
// check, the permutation and distance-table checks, and the triangle's row
// range with its pair count, each against a restatement that shares nothing
// with it.  Every array is a heap block of exactly the size the check may
// read, so a read past it is a sanitizer report.  No GPU.  Build:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined \
//         -I drep_amd/csrc tools/api_checks_check.cpp -o tools/bin/api_checks_check
// Prints "N checks, 0 disagree"; exit status 0: every case agreed.
#include "api_checks.h"

#include <cstdio>
#include <cstring>

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
// rc and the message: want == nullptr means DREPHIP_OK
static void expect(int rc, const char *want, const char *what, long a = 0, long b = 0, long c = 0) {
    check(want ? rc == DREPHIP_ERR_ARG && g_err == want : rc == DREPHIP_OK, what, a, b, c);
}

constexpr uint32_t S = 8;
constexpr uint64_t PAD = ~0ull;
static const char *kBig = "nhash[i] > s", *kOrder = "sketch rows must be ascending and distinct",
                  *kPad = "sketch rows must be UINT64_MAX past nhash[i]";

// n rows of nh hashes each: 10, 20, ... then the padding
static std::vector<uint64_t> matrix(uint32_t n, uint32_t nh) {
    std::vector<uint64_t> h((size_t)n * S, PAD);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = 0; j < nh; j++) h[(size_t)i * S + j] = 10 * (j + 1) + i;
    return h;
}

static void check_the_row_check() {
    for (uint32_t n : {0u, 1u, 2u, 3u})
        for (uint32_t nh = 0; nh <= S; nh++) {
            const std::vector<uint64_t> good = matrix(n, nh);
            const std::vector<uint32_t> cnt(n, nh);
            for (bool ordered : {false, true})
                expect(check_rows(good.data(), cnt.data(), n, S, ordered), nullptr, "a good matrix", n, nh, ordered);
            // a violation at the first and the last position of a row, in the first and the last row
            for (uint32_t row : {0u, n ? n - 1 : 0u}) {
                if (row >= n) continue;
                for (bool ordered : {false, true}) {
                    std::vector<uint32_t> big = cnt;
                    big[row] = S + 1;
                    expect(check_rows(good.data(), big.data(), n, S, ordered), kBig, "nhash above s", n, nh, row);
                    if (nh >= 2)
                        for (uint32_t j : {1u, nh - 1}) {
                            std::vector<uint64_t> swap = good, dup = good;
                            std::swap(swap[(size_t)row * S + j - 1], swap[(size_t)row * S + j]);
                            dup[(size_t)row * S + j] = dup[(size_t)row * S + j - 1];
                            expect(check_rows(swap.data(), cnt.data(), n, S, ordered), ordered ? kOrder : nullptr,
                                   "an unordered row", n, nh, j);
                            expect(check_rows(dup.data(), cnt.data(), n, S, ordered), ordered ? kOrder : nullptr,
                                   "a repeated hash", n, nh, j);
                        }
                    if (nh < S)
                        for (uint32_t j : {nh, S - 1}) {
                            std::vector<uint64_t> pad = good;
                            pad[(size_t)row * S + j] = 5;
                            expect(check_rows(pad.data(), cnt.data(), n, S, ordered), kPad, "a hash in the padding", n, nh, j);
                        }
                }
                // the order of the messages within a row: nhash, then order, then padding
                if (nh >= 2 && nh < S) {
                    std::vector<uint64_t> both = good;
                    std::swap(both[(size_t)row * S], both[(size_t)row * S + 1]);
                    both[(size_t)row * S + S - 1] = 5;
                    expect(check_rows(both.data(), cnt.data(), n, S, true), kOrder, "order before padding", n, nh, row);
                    expect(check_rows(both.data(), cnt.data(), n, S, false), kPad, "padding alone when unordered", n, nh, row);
                }
            }
            std::vector<uint64_t> len(n, 1000);
            expect(check_lengths(len.data(), cnt.data(), n), nullptr, "lengths given", n, nh);
            for (uint32_t row : {0u, n ? n - 1 : 0u}) {
                if (row >= n) continue;
                std::vector<uint64_t> zero = len;
                zero[row] = 0;
                expect(check_lengths(zero.data(), cnt.data(), n), nh ? "a genome with a non-empty sketch has length 0" : nullptr,
                       "a length of 0", n, nh, row);
            }
        }
}

static void check_the_range() {
    for (uint32_t N = 0; N <= 6; N++)
        for (uint32_t row0 = 0; row0 <= N + 2; row0++)
            for (uint32_t row1 = 0; row1 <= N + 2; row1++) {
                uint64_t pairs = 0;                      // brute force: the pairs (i, j), i in [row0, row1), i < j < N
                for (uint32_t i = row0; i < row1 && i < N; i++)
                    for (uint32_t j = i + 1; j < N; j++) pairs++;
                uint32_t r1 = row1;
                const bool any = tri_clip(N, row0, &r1);
                check(r1 == (row1 < N ? row1 : N), "row1 clipped to N", N, row0, row1);
                check(any == (pairs > 0), "an empty range is one with no pair", N, row0, row1);
                if (any) check(tri_pairs(N, row0, r1) == pairs, "pair count", N, row0, row1);
            }
}

static void check_perm_and_lut() {
    for (uint32_t n : {0u, 1u, 2u, 5u}) {
        std::vector<uint32_t> p(n);
        for (uint32_t i = 0; i < n; i++) p[i] = (i * 3 + 1) % (n == 5 ? 5 : n ? n : 1);      // a permutation (3 and 5 coprime)
        if (n == 2) { p[0] = 1; p[1] = 0; }
        expect(check_perm(p.data(), n), nullptr, "a permutation", n);
        for (uint32_t at : {0u, n ? n - 1 : 0u}) {
            if (at >= n) continue;
            std::vector<uint32_t> out = p, rep = p;
            out[at] = n;                                 // out of range (and so another entry missing)
            expect(check_perm(out.data(), n), "perm is not a permutation of 0..n-1", "an entry out of range", n, at);
            out[at] = 0xFFFFFFFFu;
            expect(check_perm(out.data(), n), "perm is not a permutation of 0..n-1", "an entry far out of range", n, at);
            if (n >= 2) {
                rep[at] = p[(at + 1) % n];               // a repeat
                expect(check_perm(rep.data(), n), "perm is not a permutation of 0..n-1", "a repeated entry", n, at);
            }
        }
    }
    // tables for the denominators S - 1 and S, packed one after the other
    std::vector<int32_t> off(S + 1, -1);
    off[S - 1] = 0;
    off[S] = S;
    const uint32_t len = S + S + 1;
    for (bool denom : {false, true}) {
        expect(check_lut(off.data(), len, S, denom), nullptr, "tables that fit", denom);
        expect(check_lut(off.data(), len - 1, S, denom), "lut_off/lut_len mismatch", "the last table one entry short", denom);
        std::vector<int32_t> first = off;
        first[0] = len;                                  // denominator 0 needs one entry
        expect(check_lut(first.data(), len, S, denom), "lut_off/lut_len mismatch", "the first table past the end", denom);
        first[0] = len - 1;
        expect(check_lut(first.data(), len, S, denom), nullptr, "the first table in the last entry", denom);
        first[0] = 0x7FFFFFFF;                           // no 32-bit overflow in the test
        expect(check_lut(first.data(), 0xFFFFFFFFu, S, denom), nullptr, "the largest offset", denom);
    }
    std::vector<int32_t> none(S + 1, -1);
    expect(check_lut(none.data(), 0, S, true), nullptr, "no table, denominators given");
    expect(check_lut(none.data(), 0, S, false), "d_denom is NULL (every denominator is s) but lut_off[s] < 0",
           "no table for s, no denominators");
}

int main() {
    check_the_row_check();
    check_the_range();
    check_perm_and_lut();
    printf("api_checks_check: %d checks, %d disagree\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
