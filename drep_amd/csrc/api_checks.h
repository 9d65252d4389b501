// api_checks.h -- the pure argument checks of the C API (api.cpp): what a host
// sketch matrix, a length array, a permutation and a distance-table layout
// must satisfy, and the triangle's row range.  No HIP call and no context in
// here, so tools/api_checks_check.cpp drives every one of them on the host.
#pragma once

#include "../../include/drephip.h"

#include <stdint.h>
#include <string>
#include <vector>

namespace drephip {

void set_error(const std::string &msg);

// A host sketch matrix as the kernels need it: nhash <= s and UINT64_MAX past
// nhash (they read whole rows); ordered: each row ascending and distinct as
// well.  The dense triangle host forms pass ordered = false (include/drephip.h).
inline int check_rows(const uint64_t *hashes, const uint32_t *nhash, uint32_t n, uint32_t s, bool ordered) {
    for (uint32_t i = 0; i < n; i++) {
        if (nhash[i] > s) { set_error("nhash[i] > s"); return DREPHIP_ERR_ARG; }
        const uint64_t *row = hashes + (uint64_t)i * s;
        for (uint32_t j = 1; ordered && j < nhash[i]; j++)
            if (row[j - 1] >= row[j]) { set_error("sketch rows must be ascending and distinct"); return DREPHIP_ERR_ARG; }
        for (uint32_t j = nhash[i]; j < s; j++)
            if (row[j] != ~0ull) { set_error("sketch rows must be UINT64_MAX past nhash[i]"); return DREPHIP_ERR_ARG; }
    }
    return DREPHIP_OK;
}

// a genome that holds a hash has a length (of at least k)
inline int check_lengths(const uint64_t *length, const uint32_t *nhash, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (nhash[i] && !length[i]) { set_error("a genome with a non-empty sketch has length 0"); return DREPHIP_ERR_ARG; }
    return DREPHIP_OK;
}

inline int check_perm(const uint32_t *perm, uint32_t n) {
    std::vector<char> seen(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (perm[i] >= n || seen[perm[i]]) { set_error("perm is not a permutation of 0..n-1"); return DREPHIP_ERR_ARG; }
        seen[perm[i]] = 1;
    }
    return DREPHIP_OK;
}

// The distance tables of drephip_linkage_counts_device: denominator d's d + 1
// entries start at lut_off[d] (< 0: none) and end inside lut_len; without a
// denominator array every denominator is s, whose table must exist.
inline int check_lut(const int32_t *lut_off, uint32_t lut_len, uint32_t s, bool have_denom) {
    for (uint32_t d = 0; d <= s; d++)
        if (lut_off[d] >= 0 && (uint64_t)lut_off[d] + d + 1 > lut_len) { set_error("lut_off/lut_len mismatch"); return DREPHIP_ERR_ARG; }
    if (!have_denom && lut_off[s] < 0) {
        set_error("d_denom is NULL (every denominator is s) but lut_off[s] < 0");
        return DREPHIP_ERR_ARG;
    }
    return DREPHIP_OK;
}

// Rows [row0, row1) of the N-genome triangle (row i: the pairs (i, j), j > i):
// row1 clipped to N; false when the range holds no pair.
inline bool tri_clip(uint32_t N, uint32_t row0, uint32_t *row1) {
    if (*row1 > N) *row1 = N;
    return !(N < 2 || row0 >= *row1 || row0 >= N - 1);
}
// the pairs of those rows: the length of their condensed segment
inline uint64_t tri_pairs(uint32_t N, uint32_t row0, uint32_t row1) {
    auto start = [&](uint64_t i) { return i * N - i * (i + 1) / 2; };
    return start(row1 < N - 1 ? row1 : N - 1) - start(row0);
}

}  // namespace drephip
