// canon.h -- the sketch hash kernel's canonical-strand choice on the 2-bit code
// stream.  Host and device: the kernel (sketch.hip) and the host evaluator
// behind drephip_canon_eval (api.cpp, tests/test_sketch_canon.py) call the
// same inline functions.
//
// Streams (code word j holds bases 16j..16j+15, base i at bits 2i):
//   NF[j] = ~F[j]: a little-endian cut holding bases q-15..q has base q in the
//     top bits, i.e. it is the reverse complement read MSB-first;
//   R[j] = F[j] with its 16 fields reversed (rev_fields16): a big-endian cut of
//     R starting at base q-20 is the forward k-mer MSB-first.
// For the window end q = 16m + r the kernel holds NF[m-1..m] and R[m-2..m].
//
// What Murmur needs of the canonical 21-mer is its first 16 bases as one word
// (bases 0-3 in the top byte: four table indices) and bases 16-20 as a 10-bit
// index into the tail table.  memcmp order of the ASCII k-mers is unsigned
// order of the MSB-first codes (A<C<G<T = 0<1<2<3).
//
// The high words decide.  Base 10 of the forward k-mer is the code c at
// position q-10; base 10 of the reverse complement is the complement of the
// base at q-20+10, the same position: 3 - c.  c != 3 - c (2c is even), and
// base 10 lies in the high word (bases 0-15), so fhi != chi for every window,
// whatever the codes: the 64-bit comparison of the two top-aligned k-mers is
// the 32-bit comparison of their high words, forward <= reverse  <=>  fhi < chi
// (k odd: a k-mer never equals its reverse complement).  The canonical high
// word is min(fhi, chi): no compare, no strand bit.
//
// Tail.  The canonical strand's bases 16-20 stand in the high word of the
// strand that lost.  Let f[0..20] be the forward k-mer and r[i] = 3 - f[20-i]
// its reverse complement.  The top five bases of chi are r[0..4] =
// 3-f[20], 3-f[19], .., 3-f[16]: the forward tail f[16..20], reversed and
// complemented.  The top five bases of fhi are f[0..4], and the reverse tail
// is r[16+j] = 3 - f[4-j]: again the tail, reversed and complemented, by the
// same map.  Whichever strand wins, the other's high word is max(fhi, chi)
// (fhi != chi), so with u = the top 10 bits of max(fhi, chi) the canonical
// tail is t[16+j] = 3 - u_field[4-j], as a number (base 16 on top)
//     y = rev5(~u & 0x3FF)          (rev5: the five 2-bit fields reversed)
// = tail_index_of_head(u).  Complement and field reversal commute and each is
// its own inverse, so u -> y is an involution, hence a bijection of 0..1023.
// The kernel's tail table is stored permuted -- the entry of tail y at index
// tail_index_of_head(y), so index u holds the entry of tail y(u) -- and the
// tail offset is u << 3 = (max(fhi, chi) >> 19) & 0x1FF8: one v_max_u32, one
// shift, one AND, the same at every residue, reading no further code word.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace drephip {

// low word of (hi:lo) >> s, 0 <= s <= 31: one v_alignbit_b32
__host__ __device__ __forceinline__ uint32_t alignbit32(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u));
#endif
}

__host__ __device__ __forceinline__ uint32_t rev_fields16(uint32_t x) {     // reverse the 16 2-bit fields
    const uint32_t y = __builtin_bitreverse32(x);
    return ((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1);
}

constexpr uint32_t kTailOffMask = 0x1FF8u;      // 10-bit tail index << 3

// The canonical tail (bases 16-20, base 16 on top) from u = bases 0-4 of the
// other strand (base 0 on top), and back: rev5(~u & 0x3FF), an involution.
// The tail table's index map (sketch.hip build_tables) and the host
// evaluator's (api.cpp drephip_canon_eval).
__host__ __device__ __forceinline__ uint32_t tail_index_of_head(uint32_t u) {
    return rev_fields16(~u & 0x3FFu) >> 22;      // fields 0-4 land in fields 15-11
}

// Canonical k-mer of window end q = 16m + r, 0 <= r <= 15 (a constant in the
// kernel's unrolled body), from nf1, nf2 = NF[m-1..m] and r0..r2 = R[m-2..m]:
// hi = its bases 0-15 MSB-first, toff = 8 * (bases 0-4 of the other strand as
// a 10-bit number, base 0 on top) -- the byte offset of the canonical tail's
// entry in the permuted tail table; its bases 16-20 are
// tail_index_of_head(toff >> 3).
__host__ __device__ __forceinline__ void canon_cut(uint32_t nf1, uint32_t nf2, uint32_t r0, uint32_t r1,
                                                   uint32_t r2, int r, uint32_t &hi, uint32_t &toff) {
    // reverse strand: bases q..q-15 complemented
    const uint32_t chi = r == 15 ? nf2 : alignbit32(nf2, nf1, 2 * (r + 1));
    // forward strand: bases q-20..q-5; q-20 is field r+12 of word m-2 or field r-4 of word m-1
    const uint32_t fhi = r < 4 ? alignbit32(r0, r1, 32 - 2 * (r + 12)) : r == 4 ? r1 : alignbit32(r1, r2, 32 - 2 * (r - 4));
    hi = fhi < chi ? fhi : chi;
    toff = ((fhi < chi ? chi : fhi) >> 19) & kTailOffMask;
}

}  // namespace drephip
