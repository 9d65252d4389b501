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
// For the window end q = 16m + r the kernel holds NF[m-2..m] and R[m-2..m].
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
// word is min(fhi, chi) -- no dependency on the compare, so the four block
// table reads issue straight from it -- and only the tail waits for the strand
// bit.
//
// Tail.  The forward strand's bases 16-20 are bases q-4..q of R, the reverse
// strand's are the complements of bases q-16..q-20, bases q-20..q-16 of NF read
// MSB-first: a 10-bit field of one code word for r >= 4 and of two for r < 4
// (both strands straddle at the same residues).  The field is moved to bits
// 3..12 -- the byte offset of an 8-byte table entry -- by one shift or one
// v_alignbit_b32, with junk above and below; one select on the strand bit and
// one AND with 0x1FF8 finish it.
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

// x's 10-bit field at bits at..at+9, moved to bits 3..12 (junk around it)
__host__ __device__ __forceinline__ uint32_t field_to_3(uint32_t x, int at) {
    return at >= 3 ? x >> (at - 3) : x << (3 - at);
}

// Canonical k-mer of window end q = 16m + r, 0 <= r <= 15 (a constant in the
// kernel's unrolled body), from nf0..nf2 = NF[m-2..m] and r0..r2 = R[m-2..m]:
// hi = its bases 0-15 MSB-first, toff = 8 * (its bases 16-20 as a 10-bit
// number, base 16 on top).
__host__ __device__ __forceinline__ void canon_cut(uint32_t nf0, uint32_t nf1, uint32_t nf2, uint32_t r0,
                                                   uint32_t r1, uint32_t r2, int r, uint32_t &hi, uint32_t &toff) {
    // reverse strand: bases q..q-15 complemented
    const uint32_t chi = r == 15 ? nf2 : alignbit32(nf2, nf1, 2 * (r + 1));
    // forward strand: bases q-20..q-5; q-20 is field r+12 of word m-2 or field r-4 of word m-1
    const uint32_t fhi = r < 4 ? alignbit32(r0, r1, 32 - 2 * (r + 12)) : r == 4 ? r1 : alignbit32(r1, r2, 32 - 2 * (r - 4));
    uint32_t ft, ct;
    if (r < 4) {
        // forward: bits 30-2r..39-2r of r1:r2; reverse: bits 24+2r..33+2r of nf1:nf0
        ft = alignbit32(r1, r2, 27 - 2 * r);
        ct = alignbit32(nf1, nf0, 21 + 2 * r);
    } else {
        ft = field_to_3(r2, 30 - 2 * r);         // base q at bits 30-2r of R[m]
        ct = field_to_3(nf1, 2 * (r - 4));       // base q-20 at field r-4 of NF[m-1]
    }
    hi = fhi < chi ? fhi : chi;
    toff = (fhi < chi ? ft : ct) & kTailOffMask;
}

}  // namespace drephip
