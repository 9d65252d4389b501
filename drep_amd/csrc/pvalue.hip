// pvalue.hip -- the p-value column and the -v / -d record filters of
// `mash dist` (drep/d_cluster.py:569-573) on the device, and the host
// evaluator of the same arithmetic (pvalue.h).  Compiled with
// -ffp-contract=off (Makefile): the kernels and drephip_pvalue_eval agree bit
// for bit.
//
//   k_pvalue_records  one lane per record {a, b, common, denom}: p of
//                     (common, len_a[a], len_b[b]) at the context's k and s
//   k_pvalue_hits     one lane per best-hit slot {r, common, denom, 0}
//   k_filter_flags / k_filter_scatter
//                     the stable record filter: a flag per record (p <= max_p
//                     and common >= cmin[denom]), an exclusive sum of the
//                     flags (hipcub), the survivors written at their ranks
//
// The loops of pvalue_tail differ in length inside a wave (common runs from 1
// to several hundred among neighbouring records); the long ones are nearly
// all zeros and leave through pvalue_tail's early exit after the few dozen
// factors it takes to pass 2^-1100, so a wave waits for its longest non-zero
// record only.
#include "ctx.h"
#include "pvalue.h"
#include "../../include/drephip.h"

#include <hipcub/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#define DREPHIP_EXPORT extern "C" __attribute__((visibility("default")))

namespace drephip {

constexpr uint32_t kPvWG = 256;

__global__ __launch_bounds__(kPvWG) void k_pvalue_records(const uint4 *__restrict__ rec, uint64_t n,
                                                          const uint64_t *__restrict__ len_a, uint32_t n_a,
                                                          const uint64_t *__restrict__ len_b, uint32_t n_b, int k,
                                                          uint32_t s, double *__restrict__ pval) {
    const uint64_t t = (uint64_t)blockIdx.x * kPvWG + threadIdx.x;
    if (t >= n) return;
    const uint4 q = rec[t];
    // an index outside its length array (the host form rejects it): NaN, nothing read
    double p = std::numeric_limits<double>::quiet_NaN();
    if (q.x < n_a && q.y < n_b) p = pvalue_of(k, s, q.z, len_a[q.x], len_b[q.y]);
    pval[t] = p;
}

__global__ __launch_bounds__(kPvWG) void k_pvalue_hits(const uint4 *__restrict__ hits,
                                                       const uint32_t *__restrict__ count, uint32_t rows, uint32_t top,
                                                       const uint64_t *__restrict__ qlen,
                                                       const uint64_t *__restrict__ rlen, uint32_t N, int k, uint32_t s,
                                                       double *__restrict__ pval) {
    const uint64_t t = (uint64_t)blockIdx.x * kPvWG + threadIdx.x;
    if (t >= (uint64_t)rows * top) return;
    const uint32_t row = (uint32_t)(t / top), slot = (uint32_t)(t % top);
    double p = 1.0;
    if (slot < count[row]) {
        const uint4 h = hits[t];
        p = h.x < N ? pvalue_of(k, s, h.y, qlen[row], rlen[h.x]) : std::numeric_limits<double>::quiet_NaN();
    }
    pval[t] = p;
}

// flag[t] = record t survives: p <= max_p (no test without pval) and
// common >= cmin[denom] (no test without cmin; a denominator above s fails)
__global__ __launch_bounds__(kPvWG) void k_filter_flags(const uint4 *__restrict__ rec, const double *__restrict__ pval,
                                                        uint32_t n, double max_p, const uint32_t *__restrict__ cmin,
                                                        uint32_t s, uint32_t *__restrict__ flag) {
    const uint32_t t = blockIdx.x * kPvWG + threadIdx.x;
    if (t >= n) return;
    bool keep = true;
    if (pval) keep = pval[t] <= max_p;
    if (cmin) {
        const uint4 q = rec[t];
        keep = keep && q.w <= s && q.z >= cmin[q.w];
    }
    flag[t] = keep ? 1u : 0u;
}

__global__ __launch_bounds__(kPvWG) void k_filter_scatter(const uint4 *__restrict__ rec, const double *__restrict__ pval,
                                                          uint32_t n, const uint32_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ pos, uint4 *__restrict__ out,
                                                          double *__restrict__ pval_out,
                                                          uint32_t *__restrict__ kept) {
    const uint32_t t = blockIdx.x * kPvWG + threadIdx.x;
    if (t >= n) return;
    const uint32_t f = flag[t], at = pos[t];
    if (f) {
        out[at] = rec[t];
        if (pval_out) pval_out[at] = pval[t];
    }
    if (t == n - 1) *kept = at + f;
}

static inline uint32_t pv_grid(uint64_t n) { return (uint32_t)((n + kPvWG - 1) / kPvWG); }

// queued on st, no wait
int pvalue_records_impl(drephip_ctx *ctx, const uint4 *d_rec, uint64_t n, const uint64_t *d_len_a, uint32_t n_a,
                        const uint64_t *d_len_b, uint32_t n_b, double *d_pval, hipStream_t st) {
    if (n == 0) return DREPHIP_OK;
    if (n > (uint64_t)0x7fffffffu * kPvWG) { set_error("too many records for one call"); return DREPHIP_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(k_pvalue_records, dim3(pv_grid(n)), dim3(kPvWG), 0, st, d_rec, n, d_len_a, n_a, d_len_b, n_b,
                       ctx->k, ctx->s, d_pval);
    HIPC(hipGetLastError());
    return DREPHIP_OK;
}

int pvalue_hits_impl(drephip_ctx *ctx, const uint32_t *d_hits, const uint32_t *d_count, uint32_t rows, uint32_t top,
                     const uint64_t *d_qlen, const uint64_t *d_rlen, uint32_t N, double *d_pval, hipStream_t st) {
    const uint64_t n = (uint64_t)rows * top;
    if (n == 0) return DREPHIP_OK;
    hipLaunchKernelGGL(k_pvalue_hits, dim3(pv_grid(n)), dim3(kPvWG), 0, st, (const uint4 *)d_hits, d_count, rows, top,
                       d_qlen, d_rlen, N, ctx->k, ctx->s, d_pval);
    HIPC(hipGetLastError());
    return DREPHIP_OK;
}

// The stable filter, in chunks of at most 2^26 records (the flags and ranks
// are 32-bit; DREPHIP_FILTER_CHUNK sets fewer, for tests).  Waits for each
// chunk's count.
int records_filter_impl(drephip_ctx *ctx, const uint4 *d_rec, const double *d_pval, uint64_t n, double max_p,
                        const uint32_t *d_cmin, uint4 *d_out, double *d_pval_out, uint64_t *n_out, hipStream_t st) {
    *n_out = 0;
    if (n == 0) return DREPHIP_OK;
    uint64_t chunk = 1ull << 26;
    const uint64_t v = env_u64("DREPHIP_FILTER_CHUNK", 0);
    if (v >= 1 && v < chunk) chunk = v;
    chunk = std::min(chunk, n);
    uint32_t *d_flag, *d_pos, *d_kept, *h_kept;
    void *tmp;
    size_t tb = 0;
    int rc;
    if ((rc = scratch(ctx, "filt_flag", chunk * 4, (void **)&d_flag))) return rc;
    if ((rc = scratch(ctx, "filt_pos", chunk * 4, (void **)&d_pos))) return rc;
    if ((rc = scratch(ctx, "filt_kept", 4, (void **)&d_kept))) return rc;
    if ((rc = pinned_host(ctx, "filt_kept", 4, (void **)&h_kept))) return rc;
    HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_flag, d_pos, (int)chunk, st));
    if ((rc = scratch(ctx, "filt_tmp", std::max<size_t>(tb, 16), &tmp))) return rc;
    uint64_t kept = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - c0);
        hipLaunchKernelGGL(k_filter_flags, dim3(pv_grid(m)), dim3(kPvWG), 0, st, d_rec + c0, d_pval ? d_pval + c0 : nullptr,
                           m, max_p, d_cmin, ctx->s, d_flag);
        HIPC(hipGetLastError());
        HIPC(hipcub::DeviceScan::ExclusiveSum(tmp, tb, d_flag, d_pos, (int)m, st));
        hipLaunchKernelGGL(k_filter_scatter, dim3(pv_grid(m)), dim3(kPvWG), 0, st, d_rec + c0,
                           d_pval ? d_pval + c0 : nullptr, m, d_flag, d_pos, d_out + kept,
                           d_pval && d_pval_out ? d_pval_out + kept : nullptr, d_kept);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(h_kept, d_kept, 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        kept += *h_kept;
    }
    *n_out = kept;
    return DREPHIP_OK;
}

}  // namespace drephip

using namespace drephip;

DREPHIP_EXPORT int drephip_pvalue_eval(int k, uint32_t s, const uint32_t *common, const uint64_t *len_a,
                                       const uint64_t *len_b, uint64_t n, double *pval, double *r_out,
                                       uint32_t *n_out) {
    if (k < 1 || k > 32 || s < 1) { set_error("bad k or s"); return DREPHIP_ERR_ARG; }
    if (n && (!common || !len_a || !len_b || !pval)) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    for (uint64_t i = 0; i < n; i++)
        if (common[i] && (!len_a[i] || !len_b[i])) {
            set_error("a genome of length 0 shares no hash");
            return DREPHIP_ERR_ARG;
        }
    for (uint64_t i = 0; i < n; i++) {
        double r;
        uint32_t nn;
        pvalue_rn(k, s, len_a[i], len_b[i], &r, &nn);
        pval[i] = pvalue_tail(common[i], nn, r);
        if (r_out) r_out[i] = r;
        if (n_out) n_out[i] = nn;
    }
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_pvalue_records_device(drephip_ctx *ctx, const uint32_t *d_records, uint64_t n,
                                                 const uint64_t *d_len_a, uint32_t n_a, const uint64_t *d_len_b,
                                                 uint32_t n_b, double *d_pval, void *stream) {
    GUARD_CTX(ctx);
    if (n == 0) return DREPHIP_OK;
    if (!d_records || !d_len_a || !d_len_b || !d_pval) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc;
    if ((rc = pvalue_records_impl(ctx, (const uint4 *)d_records, n, d_len_a, n_a, d_len_b, n_b, d_pval,
                                  (hipStream_t)stream)))
        return rc;
    HIPC(hipStreamSynchronize((hipStream_t)stream));
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_pvalue_records(drephip_ctx *ctx, const uint32_t *records, uint64_t n, const uint64_t *len_a,
                                          uint32_t n_a, const uint64_t *len_b, uint32_t n_b, double *pval) {
    GUARD_CTX(ctx);
    if (n == 0) return DREPHIP_OK;
    if (!records || !len_a || !len_b || !pval) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    for (uint64_t t = 0; t < n; t++) {
        const uint32_t *q = records + 4 * t;
        if (q[0] >= n_a || q[1] >= n_b) { set_error("a record names a genome outside its length array"); return DREPHIP_ERR_ARG; }
        if (q[2] > q[3] || q[3] > ctx->s) { set_error("a record needs common <= denom <= s"); return DREPHIP_ERR_ARG; }
        if (q[2] && (!len_a[q[0]] || !len_b[q[1]])) { set_error("a genome of length 0 shares no hash"); return DREPHIP_ERR_ARG; }
    }
    hipStream_t st = ctx->stream;
    uint4 *d_rec;
    uint64_t *d_la, *d_lb;
    double *d_p;
    int rc;
    if ((rc = scratch(ctx, "pv_rec", n * 16, (void **)&d_rec))) return rc;
    if ((rc = scratch(ctx, "pv_len_a", n_a * 8ull, (void **)&d_la))) return rc;
    if ((rc = scratch(ctx, "pv_len_b", n_b * 8ull, (void **)&d_lb))) return rc;
    if ((rc = scratch(ctx, "pv_out", n * 8, (void **)&d_p))) return rc;
    HIPC(hipMemcpyAsync(d_rec, records, n * 16, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_la, len_a, n_a * 8ull, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_lb, len_b, n_b * 8ull, hipMemcpyHostToDevice, st));
    if ((rc = pvalue_records_impl(ctx, d_rec, n, d_la, n_a, d_lb, n_b, d_p, st))) return rc;
    HIPC(hipMemcpyAsync(pval, d_p, n * 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_pvalue_hits_device(drephip_ctx *ctx, const uint32_t *d_hits, const uint32_t *d_count,
                                              uint32_t rows, uint32_t top, const uint64_t *d_qlen,
                                              const uint64_t *d_rlen, uint32_t N, double *d_pval, void *stream) {
    GUARD_CTX(ctx);
    if (rows == 0 || top == 0) return DREPHIP_OK;
    if (!d_hits || !d_count || !d_qlen || !d_rlen || !d_pval) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    int rc;
    if ((rc = pvalue_hits_impl(ctx, d_hits, d_count, rows, top, d_qlen, d_rlen, N, d_pval, (hipStream_t)stream)))
        return rc;
    HIPC(hipStreamSynchronize((hipStream_t)stream));
    return DREPHIP_OK;
}

DREPHIP_EXPORT int drephip_records_filter_device(drephip_ctx *ctx, const uint32_t *d_records, const double *d_pval,
                                                 uint64_t n, double max_p, const uint32_t *d_cmin, uint32_t *d_out,
                                                 double *d_pval_out, uint64_t *n_out, void *stream) {
    GUARD_CTX(ctx);
    if (!n_out) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    *n_out = 0;
    if (!(max_p >= 0.0 && max_p <= 1.0)) { set_error("max_p must lie in [0, 1]"); return DREPHIP_ERR_ARG; }
    if (n == 0) return DREPHIP_OK;
    if (!d_records || !d_out) { set_error("null argument"); return DREPHIP_ERR_ARG; }
    if (d_out == d_records || (d_pval && d_pval_out == d_pval)) {
        set_error("the filter's outputs must not alias its inputs");
        return DREPHIP_ERR_ARG;
    }
    return records_filter_impl(ctx, (const uint4 *)d_records, d_pval, n, max_p, d_cmin, (uint4 *)d_out, d_pval_out,
                               n_out, (hipStream_t)stream);
}
