// prefilter.h -- the end of MurmurHash3's fmix64 pair as the sketch hash kernel
// splits it, and the reject-early test in front of it.  Host and device: the
// kernel (sketch.hip) and the host evaluator behind drephip_prefilter_eval
// (api.cpp, tests/test_sketch_prefilter.py) call the same inline functions.
//
// The kernel carries a k-mer's two Murmur lanes as the fmix64 states before
// their last multiply, q1 and q2.  With p = q C2 (mod 2^64) and
// fin(p) = p ^ (p >> 33),
//     h1 = fin(p1) + fin(p2)                                  (murmur_fin)
// and a k-mer is admitted iff h1 <= T.  The prefilter is a cheaper necessary
// condition on (q1, q2), so the exact test runs only on its rare survivors.
//
// Identity.  Multiplication by C2 is linear mod 2^64:
//     P = p1 + p2 = (q1 + q2) C2,
// one 64-bit add and one high-word product instead of two high words.
//
// Bound.  fin leaves the high word unchanged, so
//     hi(h1) = hi(p1) + hi(p2) + cf,  cf = carry of lo(fin p1) + lo(fin p2),
//     hi(P)  = hi(p1) + hi(p2) + cp,  cp = carry of lo(p1) + lo(p2),
// both carries 0 or 1: hi(P) - hi(h1) is -1, 0 or +1 (mod 2^32).  With
// v = hi(P) + 1 (mod 2^32), v - hi(h1) is 0, 1 or 2, and while
// hi(T) <= 0xFFFFFFFD nothing wraps:
//     h1 <= T   implies   hi(h1) <= hi(T)   implies   v <= hi(T) + 2 = Tp.
// For hi(T) >= 0xFFFFFFFE the bound is 0xFFFFFFFF: every k-mer goes to the
// exact test (T = kMaxThr, the short-genome path).  The +1 keeps the case
// hi(h1) = 0 with difference -1 (hi(P) = 0xFFFFFFFF) inside the window; the
// window passes hi(T) + 3 values of hi(h1)'s ~2^32, against hi(T) + 1 exact.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace drephip {

constexpr uint64_t kFmixC1 = 0xff51afd7ed558ccdULL;
constexpr uint64_t kFmixC2 = 0xc4ceb9fe1a85ec53ULL;

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// fmix64 up to its last multiply: q = ((k ^ k >> 33) C1) ^ (... >> 33); the
// state before fmix64's final xorshift is then q C2 (fmix_mul)
__host__ __device__ __forceinline__ uint64_t fmix64_q(uint64_t k) {
    k ^= k >> 33;
    // x C1 = lo x lo C1 + ((lo x hi C1 + hi x lo C1) << 32) with the cross terms
    // chained through the multiply-adds: v_mul_lo_u32 + 2 v_mad_u64_u32, where
    // the compiler's own 64-bit multiply is v_mul_hi_u32, 2 v_mul_lo_u32, a
    // v_mad_u64_u32 and a v_add3_u32
    const uint32_t lo = (uint32_t)k, hi = (uint32_t)(k >> 32);
    const uint32_t t = hi * (uint32_t)kFmixC1;
    const uint32_t cross = (uint32_t)((uint64_t)lo * (uint32_t)(kFmixC1 >> 32) + t);
    k = (uint64_t)lo * (uint32_t)kFmixC1 + ((uint64_t)cross << 32);
    k ^= k >> 33;
    return k;
}
__host__ __device__ __forceinline__ uint64_t fmix_mul(uint64_t q) { return q * kFmixC2; }
__host__ __device__ __forceinline__ uint64_t murmur_fin(uint64_t q1, uint64_t q2) {
    const uint64_t p1 = fmix_mul(q1), p2 = fmix_mul(q2);
    return (p1 ^ (p1 >> 33)) + (p2 ^ (p2 >> 33));
}

// Tp: the prefilter bound of threshold T (once per workgroup)
__host__ __device__ __forceinline__ uint32_t prefilter_bound(uint64_t T) {
    return __builtin_elementwise_add_sat((uint32_t)(T >> 32), 2u);    // hi(T) + 2, or all ones from 0xFFFFFFFE on
}
// v = hi((q1 + q2) C2) + 1 (mod 2^32), from
// hi(Q C2) = hi(lo Q lo C2) + lo Q hi C2 + hi Q lo C2 (mod 2^32).
// On the device: v_lshl_add_u64 (the compiler's own 64-bit add; as an asm
// statement it drew an s_nop in front of the multiply that reads it),
// v_mul_hi_u32, v_mul_lo_u32, v_mad_u64_u32 (the second product added to the
// first) and one v_add3_u32 that also carries the +1
__host__ __device__ __forceinline__ uint32_t prefilter_hi(uint64_t q1, uint64_t q2) {
    const uint64_t Q = q1 + q2;
    const uint32_t a = (uint32_t)Q, b = (uint32_t)(Q >> 32);
    return mulhi32(a, (uint32_t)kFmixC2) + a * (uint32_t)(kFmixC2 >> 32) + b * (uint32_t)kFmixC2 + 1u;
}

}  // namespace drephip
