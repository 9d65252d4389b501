// pvalue.h -- the p-value column of `mash dist` (drep/d_cluster.py:569-573),
// host and device: the kernels (pvalue.hip) and the host evaluator behind
// drephip_pvalue_eval call the same inline functions, and the file that holds
// both is compiled with -ffp-contract=off, so the two agree bit for bit and
// the numerics are tested on the CPU (tests/test_pvalue_host.py).
//
// Definition (Mash's, as drep_amd/d_cluster.py:mash_pvalue states it):
//     kspace = 4^k
//     px = 1/(1 + kspace/len_a),  py = 1/(1 + kspace/len_b)
//     r  = px py / (px + py - px py)
//     M  = kspace (px + py) / (1 + r)
//     n  = floor(min(M, s))
//     p  = 1 if common == 0, 0 if common > n, else P(X >= common), X ~ Binomial(n, r)
// r and n are formed with these IEEE operations in this order (numpy's).
//
// The tail uses IEEE + - x / and comparisons only; exponents are handled as
// integers on the bit pattern (no libm / OCML call), so every operation is
// correctly rounded on both sides.  A scaled value is (m, e): m in [0.5, 1),
// value m 2^e.
//     T_c = prod_{j=1..c} ((n-c+j)/j r) x (1-r)^(n-c)     first term, scaled;
//           the power by binary exponentiation, then one first-order factor
//           1 + (n-c) d/q for the rounding d of q = fl(1-r)
//     T_{i+1} = T_i (n-i)/(i+1) r/(1-r)                    summed relative to T_c
// until a term falls below 2^-60 of the sum.  common below the mean n r takes
// the complement instead, 1 - (T_{c-1} + T_{c-2} + ...), summed downwards the
// same way: every sum runs over falling terms, so none needs rescaling.  The
// factors of the product fall with j, so once one is below 1 and the scaled
// exponent is below -1100 the result is below 2^-1022 (the tail then falls
// too: at most n + 1 terms no larger than T_c): the loop is left and the
// record costs no more.  Results below 2^-1022 are 0.0 (no subnormals,
// whatever the denormal mode); results above 1 are 1.0.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace drephip {

__host__ __device__ __forceinline__ uint64_t pv_bits(double x) { return __builtin_bit_cast(uint64_t, x); }
__host__ __device__ __forceinline__ double pv_from_bits(uint64_t b) { return __builtin_bit_cast(double, b); }
// 2^e, -1022 <= e <= 1023
__host__ __device__ __forceinline__ double pv_exp2i(int e) { return pv_from_bits((uint64_t)(e + 1023) << 52); }
// frexp of a positive normal x: m in [0.5, 1), x = m 2^(*e); 0 stays 0
__host__ __device__ __forceinline__ double pv_split(double x, int *e) {
    const uint64_t b = pv_bits(x);
    const int be = (int)((b >> 52) & 0x7ff);
    if (be == 0) { *e = 0; return 0.0; }
    *e = be - 1022;
    return pv_from_bits((b & ~(0x7ffull << 52)) | (1022ull << 52));
}

// r and n of a pair of genome lengths (k-mer size k, sketch size s)
__host__ __device__ __forceinline__ void pvalue_rn(int k, uint32_t s, uint64_t len_a, uint64_t len_b, double *r_out,
                                                   uint32_t *n_out) {
    const double kspace = pv_exp2i(2 * k);
    const double px = 1.0 / (1.0 + kspace / (double)len_a);
    const double py = 1.0 / (1.0 + kspace / (double)len_b);
    const double pxy = px * py;
    const double r = pxy / (px + py - pxy);
    const double M = kspace * (px + py) / (1.0 + r);
    const double sd = (double)s;
    const double nf = M < sd ? M : sd;                  // (a NaN from a zero length: s)
    *r_out = r;
    *n_out = nf >= 0.0 ? (uint32_t)nf : 0u;             // floor of a value in [0, s]
}

// q^N as a scaled value, q in (0, 1]
__host__ __device__ __forceinline__ double pv_pow(double q, uint32_t N, int *e_out) {
    double rm = 0.5, bm;
    int re = 1, be, d;
    bm = pv_split(q, &be);
    while (N) {
        if (N & 1u) { rm = pv_split(rm * bm, &d); re += be + d; }
        N >>= 1;
        if (N) { bm = pv_split(bm * bm, &d); be = 2 * be + d; }
    }
    *e_out = re;
    return rm;
}

// T_c = C(n, c) r^c q^(n-c) as a scaled value, q = fl(1 - r); false when the
// factors have fallen below 1 with the product below 2^-1100 (T_c and every
// later term are below it then)
__host__ __device__ __forceinline__ bool pv_term(uint32_t c, uint32_t n, double r, double q, double *m_out, int *e_out) {
    const double nc = (double)(n - c);
    double m = 0.5;
    int e = 1, d;
    for (uint32_t j = 1; j <= c; j++) {
        const double jd = (double)j;
        const double f = (nc + jd) / jd * r;
        m = pv_split(m * f, &d);
        e += d;
        if (e < -1100 && f < 1.0) return false;
    }
    int pe;
    const double pm = pv_pow(q, n - c, &pe);
    m = pv_split(m * pm, &d);
    e += pe + d;
    const double dq = (1.0 - q) - r;                     // 1 - r = q + dq
    m = pv_split(m * (1.0 + nc * (dq / q)), &d);
    *m_out = m;
    *e_out = e + d;
    return true;
}

// P(X >= c), X ~ Binomial(n, r).  At or above the mean: the upper tail from
// T_c upwards.  Below it: 1 - P(X <= c - 1), the lower tail from T_{c-1}
// downwards -- both sums run over falling terms away from the mean, so the
// value falls with c beyond its rounding (which a sum across the mean, next to
// 1, would not).
__host__ __device__ __forceinline__ double pvalue_tail(uint32_t c, uint32_t n, double r) {
    if (c == 0) return 1.0;
    if (c > n) return 0.0;
    const double q = 1.0 - r;
    if (!(q > 0.0)) return 1.0;                          // r = 1 (or a NaN): every trial hits
    if (!(r > 0.0)) return 0.0;                          // no trial ever hits
    const bool lower = (double)c < (double)n * r;
    double m, S = 1.0, t = 1.0;
    int e, d;
    if (lower) {
        if (!pv_term(c - 1, n, r, q, &m, &e)) return 1.0;
        const double qr = q / r;
        for (uint32_t i = c - 1; i >= 1; i--) {          // T_{i-1} = T_i i/(n-i+1) q/r, ratios below 1
            t = t * ((double)i / (double)(n - i + 1) * qr);
            S = S + t;
            if (t < S * 0x1p-60) break;
        }
        m = pv_split(m * S, &d);
        e += d;
        if (e < -1021) return 1.0;
        if (e > 0) return 0.0;
        return 1.0 - m * pv_exp2i(e);
    }
    if (!pv_term(c, n, r, q, &m, &e)) return 0.0;
    const double rq = r / q;
    for (uint32_t i = c; i < n; i++) {                   // T_{i+1} = T_i (n-i)/(i+1) r/q, ratios below 1
        t = t * ((double)(n - i) / (double)(i + 1) * rq);
        S = S + t;
        if (t < S * 0x1p-60) break;
    }
    m = pv_split(m * S, &d);
    e += d;
    if (e < -1021) return 0.0;
    if (e > 0) return 1.0;
    return m * pv_exp2i(e);
}

__host__ __device__ __forceinline__ double pvalue_of(int k, uint32_t s, uint32_t common, uint64_t len_a, uint64_t len_b) {
    if (common == 0) return 1.0;
    double r;
    uint32_t n;
    pvalue_rn(k, s, len_a, len_b, &r, &n);
    return pvalue_tail(common, n, r);
}

}  // namespace drephip
