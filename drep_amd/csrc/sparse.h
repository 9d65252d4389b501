// sparse.h -- the pair list of the sparse all-pairs call
// (drephip_allpairs_sparse_device): the kernels that would store a count at
// its condensed offset append a record {i, j, common, denom} (i < j, genome
// indices as given to the call) for every pair with common > 0 instead.
#pragma once

#include "ctx.h"

namespace drephip {

// Where the records go: rec[0 .. cap), *count = records so far.  A kernel
// reserves slots with one atomic add for many records (a wave's, below) and
// stores only the records whose slot lies below cap; past cap it keeps
// counting, so the caller learns the size it needs.
struct SparseOut {
    uint4 *rec = nullptr;
    unsigned long long *count = nullptr;
    uint64_t cap = 0;
};

#if defined(__HIPCC__)
// One record from every lane that calls this (any subset of a wave, inside
// divergent code too): the calling lanes' records take consecutive slots
// reserved by ONE atomic add of the wave's first calling lane -- a counter
// bump per record serialises on the counter (linkage.hip, k_sparse_pairs).
// One 16-byte store per record.
__device__ __forceinline__ void sparse_append(const SparseOut &o, uint32_t i, uint32_t j, uint32_t common,
                                              uint32_t denom) {
    const uint64_t act = __ballot(1);                                  // the calling lanes
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
    const int leader = __ffsll((long long)act) - 1;
    unsigned long long base = 0;
    if (below == 0) base = atomicAdd(o.count, (unsigned long long)__popcll(act));
    const uint32_t blo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, leader);
    const uint32_t bhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(base >> 32), leader);
    const uint64_t idx = (((uint64_t)bhi << 32) | blo) + below;
    if (idx < o.cap) o.rec[idx] = make_uint4(i, j, common, denom);
}
#endif

}  // namespace drephip
