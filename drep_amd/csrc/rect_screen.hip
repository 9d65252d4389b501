// rect_screen.hip -- the two-set shared-hash screen of the query-against-
// reference rectangle ("Screened rectangle").
//
// The triangle's screen (screen.hip) groups every entry of one set and marks
// every pair of a run.  Here the two sets are joined instead: only the block's
// query entries are sorted, and the reference matrix is streamed past them, so
// a hash that many references and no query hold costs one failed lookup per
// reference entry, and query-query or reference-reference pairs are never
// looked at.  Per block of query rows [b0, b1):
//
//   1. keys    (hash64, (q - b0) s + k) of the block's valid entries (k < nhash)
//   2. sort    one radix sort on the 64-bit hash (stable: a run lists its
//              queries in ascending order)
//   3. heads   the distinct values U[] ascending and the run bounds ustart[]
//   4. count   (AUTO only) every valid reference entry looked up in U, the hit
//              runs' lengths summed into `checks`: the marking's bit tests.
//              Every reference is taken, no sample.  The block is screened
//              when checks * ratio <= rows * N * s (the triangle's ratio).
//   5. mark    the same walk; a hit sets bit r of the tile row of every query
//              of the run in the bitmap [row tiles from b0][ceil(N / 32)]
//   6. lists   screen_lists (screen.hip): per-tile column lists + LIST items
//
// The screen keeps a superset of the cells with common > 0 (two sketches with
// no equal valid hash share nothing); the LIST kernels recompute the kept cells
// and rect_screen_fill writes the others as 0 / min(s, nq + nr).
#include "common.h"
#include "ctx.h"
#include "../../include/drephip.h"

#include <hipcub/device/device_radix_sort.hpp>
#include <hipcub/device/device_scan.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace drephip {

constexpr int kRsWG = 256;
constexpr uint64_t kRsBitmapBytes = 256ull << 20;   // the block's bitmap stays within this
constexpr uint64_t kRsMaxEntries = 1ull << 26;      // query entries sorted per block (their scratch: ~40 B each)

// the block's entry offsets are the exclusive scan of its rows' counts; the
// total goes behind them
__global__ void k_rs_total(const uint32_t *__restrict__ nh, uint32_t *__restrict__ eoff, uint32_t n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) eoff[n] = eoff[n - 1] + nh[n - 1];
}

// one workgroup per query row g of the block: its valid entries at eoff[g] + k
__global__ __launch_bounds__(kRsWG) void k_rs_keys(const uint64_t *__restrict__ H, const uint32_t *__restrict__ nh,
                                                   const uint32_t *__restrict__ eoff, uint32_t s,
                                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t g = blockIdx.x;
    const uint32_t n = min(nh[g], s);
    const uint32_t o = eoff[g];
    const uint64_t *A = H + (uint64_t)g * s;
    for (uint32_t k = threadIdx.x; k < n; k += kRsWG) {
        keys[o + k] = A[k];
        vals[o + k] = g * s + k;
    }
}

__global__ __launch_bounds__(kRsWG) void k_rs_flags(const uint64_t *__restrict__ keys, uint32_t M,
                                                    uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * kRsWG + threadIdx.x;
    if (i < M) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// pos = the exclusive scan of flag: run u starts at its head i, U[u] = its value
__global__ __launch_bounds__(kRsWG) void k_rs_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ flag,
                                                    const uint32_t *__restrict__ pos, uint32_t M,
                                                    uint64_t *__restrict__ U, uint32_t *__restrict__ ustart,
                                                    uint32_t *__restrict__ nu) {
    const uint32_t i = blockIdx.x * kRsWG + threadIdx.x;
    if (i >= M) return;
    if (flag[i]) { U[pos[i]] = keys[i]; ustart[pos[i]] = i; }
    if (i == M - 1) {
        const uint32_t n = pos[i] + flag[i];
        *nu = n;
        ustart[n] = M;
    }
}

// first index in [a, b) with U[index] >= x (b when none)
__device__ __forceinline__ uint32_t rs_lower(const uint64_t *__restrict__ U, uint32_t a, uint32_t b, uint64_t x) {
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (U[m] < x) a = m + 1; else b = m;
    }
    return a;
}

// The join: one wave per reference genome (waves strided over the references),
// lanes on consecutive entries, each looked up in U by a binary search narrowed
// to the row's own [first, last] value range.  MARK = false: the hit runs'
// lengths summed into *checks.  MARK = true: bit r of the tile row of every
// query of a hit run, tested before the atomic so hubs and families do not
// hammer one word (a stale read only costs an atomic).  R = 1 << rshift.
template <bool MARK>
__global__ __launch_bounds__(kRsWG) void k_rs_join(const uint64_t *__restrict__ rh, const uint32_t *__restrict__ rn,
                                                   uint32_t s, uint32_t N, const uint64_t *__restrict__ U,
                                                   const uint32_t *__restrict__ ustart, uint32_t nu,
                                                   const uint32_t *__restrict__ vals, uint32_t rshift, uint32_t NW,
                                                   uint32_t *__restrict__ bm, unsigned long long *__restrict__ checks) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwaves = gridDim.x * (kRsWG / 64);
    unsigned long long mine = 0;
    for (uint32_t r = blockIdx.x * (kRsWG / 64) + (threadIdx.x >> 6); r < N; r += nwaves) {
        const uint32_t n = min(rn[r], s);
        if (n == 0) continue;
        const uint64_t *A = rh + (uint64_t)r * s;
        const uint32_t lo = rs_lower(U, 0, nu, A[0]);
        if (lo >= nu) continue;
        const uint64_t last = A[n - 1];
        // one past the last U <= last
        uint32_t hi = rs_lower(U, lo, nu, last);
        if (hi < nu && U[hi] == last) hi++;
        if (lo >= hi) continue;
        const uint32_t bit = 1u << (r & 31u);
        for (uint32_t k = lane; k < n; k += 64) {
            const uint64_t x = A[k];
            const uint32_t a = rs_lower(U, lo, hi, x);
            if (a >= hi || U[a] != x) continue;
            const uint32_t j0 = ustart[a], j1 = ustart[a + 1];
            if constexpr (!MARK) {
                mine += j1 - j0;
            } else {
                uint32_t tlast = 0xFFFFFFFFu;
                for (uint32_t j = j0; j < j1; j++) {
                    const uint32_t t = (vals[j] / s) >> rshift;
                    if (t == tlast) continue;            // the run's queries ascend: a tile's come together
                    tlast = t;
                    uint32_t *w = bm + (uint64_t)t * NW + (r >> 5);
                    if (!(*(volatile uint32_t *)w & bit)) atomicOr(w, bit);
                }
            }
        }
    }
    if constexpr (!MARK) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        if (lane == 0 && mine) atomicAdd(checks, mine);
    }
}

// denominators of the cells with no shared hash: min(s, nq + nr); one workgroup
// per query row of the block (strided over the grid)
__global__ __launch_bounds__(kRsWG) void k_rs_denoms(const uint32_t *__restrict__ qn, const uint32_t *__restrict__ rn,
                                                     uint32_t s, uint32_t N, uint32_t b0, uint32_t nrows,
                                                     uint16_t *__restrict__ denom) {
    for (uint32_t g = blockIdx.x; g < nrows; g += gridDim.x) {
        const uint32_t nq = qn[b0 + g];
        uint16_t *out = denom + (uint64_t)g * N;
        for (uint32_t r = threadIdx.x; r < N; r += kRsWG) {
            const uint32_t u = nq + rn[r];
            out[r] = (uint16_t)(u < s ? u : s);
        }
    }
}

// Phase times of the screen (sort, count pass, marking, lists, fill) into
// ctx->rect_screen.phase_ms while the screen's timing bit (4) is set: an event
// per phase boundary, waited for at the next one.
struct RsPhases {
    drephip_ctx *ctx;
    hipStream_t st;
    hipEvent_t prev = nullptr;
    RsPhases(drephip_ctx *c, hipStream_t s) : ctx(c), st(s) {
        if (ctx->timing & (1u << 4)) {
            if (hipEventCreate(&prev) != hipSuccess) prev = nullptr;
            else (void)hipEventRecord(prev, st);
        }
    }
    void end(int phase) {
        if (!prev) return;
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, st);
        (void)hipEventSynchronize(e);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, prev, e);
        ctx->rect_screen.phase_ms[phase] += ms;
        (void)hipEventDestroy(prev);
        prev = e;
    }
    ~RsPhases() { if (prev) (void)hipEventDestroy(prev); }
};

// Query rows per screened block: the bitmap within kRsBitmapBytes, the entry
// values (row of the block * s + k) within 32 bits and the sort within
// kRsMaxEntries, at least one row tile; DREPHIP_RECT_SCREEN_BLOCK_ROWS only
// lowers it.
uint32_t rect_screen_block_rows(drephip_ctx *ctx, uint32_t N, uint32_t R) {
    const uint64_t NW = ((uint64_t)N + 31) / 32;
    uint64_t rows = std::max<uint64_t>(1, kRsBitmapBytes / (NW * 4)) * R;
    rows = std::min<uint64_t>(rows, std::max<uint64_t>(1, kRsMaxEntries / ctx->s));
    rows = std::min<uint64_t>(rows, 0xFFFFFFFFull / ctx->s);
    rows = std::min<uint64_t>(rows, 0x7FFFFFFFu);
    if (const char *e = getenv("DREPHIP_RECT_SCREEN_BLOCK_ROWS"))
        if (atoll(e) > 0) rows = std::min<uint64_t>(rows, (uint64_t)atoll(e));
    return (uint32_t)std::max<uint64_t>(rows, 1);
}

// the verdict: the marking's bit tests against the block's probes, with the
// triangle's ratio (screen_worth; DREPHIP_SCREEN_RATIO)
static bool rect_screen_worth(uint32_t rows, uint32_t N, uint32_t s, uint64_t checks) {
    const char *re = getenv("DREPHIP_SCREEN_RATIO");
    const double ratio = re ? atof(re) : 16.0;
    return (double)checks * ratio <= (double)rows * (double)N * (double)s;
}

int rect_screen_block(drephip_ctx *ctx, const RectSets &in, uint32_t b0, uint32_t b1, uint32_t R, uint32_t C, bool force,
                      hipStream_t st, ScreenResult *res) {
    const uint64_t *d_qh = in.qh, *d_rh = in.rh;
    const uint32_t *d_qn = in.qn, *d_rn = in.rn, N = in.N;
    *res = ScreenResult{};
    RectScreenStats &S = ctx->rect_screen;
    const uint32_t s = ctx->s, nrows = b1 - b0;
    if ((uint64_t)nrows * s >= (1ull << 32)) return DREPHIP_OK;      // (the caller's blocks never are: rect_screen_block_rows)
    uint32_t rshift = 0;
    while ((1u << rshift) < R) rshift++;
    const uint32_t ntiles = (nrows + R - 1) / R, NW = (N + 31) / 32;
    int rc;
    timing_mark(ctx, 4, st, true);
    RsPhases ph(ctx, st);
    ScreenProf prof;
    prof.mark("start", st);
    S.blocks++;
    uint32_t *d_eoff, *h_tot;
    if ((rc = scratch(ctx, "rs_eoff", (nrows + 1) * 4ull, (void **)&d_eoff))) return rc;
    if ((rc = pinned_host(ctx, "rs_tot", 64, (void **)&h_tot))) return rc;
    {
        size_t tb = 0;
        HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_qn + b0, d_eoff, nrows, st));
        void *tmp;
        if ((rc = scratch(ctx, "rs_scan_tmp", std::max<size_t>(tb, 16), &tmp))) return rc;
        HIPC(hipcub::DeviceScan::ExclusiveSum(tmp, tb, d_qn + b0, d_eoff, nrows, st));
    }
    hipLaunchKernelGGL(k_rs_total, dim3(1), dim3(64), 0, st, d_qn + b0, d_eoff, nrows);
    HIPC(hipMemcpyAsync(h_tot, d_eoff + nrows, 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    const uint32_t M = h_tot[0];
    S.query_entries += M;
    uint32_t *d_bm;
    unsigned long long *d_zero;
    if ((rc = scratch(ctx, "rs_bm", (uint64_t)ntiles * NW * 4, (void **)&d_bm))) return rc;
    if ((rc = scratch(ctx, "rs_zero", 16, (void **)&d_zero))) return rc;
    HIPC(hipMemsetAsync(d_zero, 0, 16, st));                         // [0]: no pairs written by this screen; [1]: checks
    HIPC(hipMemsetAsync(d_bm, 0, (uint64_t)ntiles * NW * 4, st));
    if (M > 0) {
        uint64_t *k_in, *k_out, *d_U;
        uint32_t *v_in, *v_out, *d_flag, *d_pos, *d_ustart, *d_nu;
        if ((rc = scratch(ctx, "rs_kin", M * 8ull, (void **)&k_in))) return rc;
        if ((rc = scratch(ctx, "rs_kout", M * 8ull, (void **)&k_out))) return rc;
        if ((rc = scratch(ctx, "rs_vin", M * 4ull, (void **)&v_in))) return rc;
        if ((rc = scratch(ctx, "rs_vout", M * 4ull, (void **)&v_out))) return rc;
        if ((rc = scratch(ctx, "rs_pos", M * 4ull, (void **)&d_pos))) return rc;
        if ((rc = scratch(ctx, "rs_ustart", (M + 1) * 4ull, (void **)&d_ustart))) return rc;
        if ((rc = scratch(ctx, "rs_nu", 4, (void **)&d_nu))) return rc;
        hipLaunchKernelGGL(k_rs_keys, dim3(nrows), dim3(kRsWG), 0, st, d_qh + (uint64_t)b0 * s, d_qn + b0, d_eoff, s, k_in,
                           v_in);
        {
            size_t tb = 0;
            HIPC(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k_in, k_out, v_in, v_out, M, 0, 64, st));
            void *tmp;
            if ((rc = scratch(ctx, "rs_sort_tmp", std::max<size_t>(tb, 16), &tmp))) return rc;
            HIPC(hipcub::DeviceRadixSort::SortPairs(tmp, tb, k_in, k_out, v_in, v_out, M, 0, 64, st));
        }
        d_flag = v_in;                                               // free after the sort, as is k_in (U)
        d_U = k_in;
        const uint32_t gm = (M + kRsWG - 1) / kRsWG;
        hipLaunchKernelGGL(k_rs_flags, dim3(gm), dim3(kRsWG), 0, st, k_out, M, d_flag);
        {
            size_t tb = 0;
            HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_flag, d_pos, M, st));
            void *tmp;
            if ((rc = scratch(ctx, "rs_scan_tmp2", std::max<size_t>(tb, 16), &tmp))) return rc;
            HIPC(hipcub::DeviceScan::ExclusiveSum(tmp, tb, d_flag, d_pos, M, st));
        }
        hipLaunchKernelGGL(k_rs_heads, dim3(gm), dim3(kRsWG), 0, st, k_out, d_flag, d_pos, M, d_U, d_ustart, d_nu);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(h_tot, d_nu, 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        const uint32_t nu = h_tot[0];
        S.distinct += nu;
        prof.mark("sort+heads", st);
        ph.end(0);
        // waves for the join: a wave per reference, at most a few per SIMD of the chip
        const uint32_t gj = (uint32_t)std::min<uint64_t>(((uint64_t)N + kRsWG / 64 - 1) / (kRsWG / 64), 256 * 16);
        if (!force) {
            hipLaunchKernelGGL(k_rs_join<false>, dim3(gj), dim3(kRsWG), 0, st, d_rh, d_rn, s, N, d_U, d_ustart, nu, v_out,
                               rshift, NW, d_bm, d_zero + 1);
            HIPC(hipGetLastError());
            unsigned long long *h_chk = (unsigned long long *)(h_tot + 2);
            HIPC(hipMemcpyAsync(h_chk, d_zero + 1, 8, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            const uint64_t checks = *h_chk;
            S.checks += checks;
            prof.mark("count", st);
            ph.end(1);
            if (!rect_screen_worth(nrows, N, s, checks)) {
                S.dense_blocks++;
                timing_mark(ctx, 4, st, false);
                return DREPHIP_OK;                                   // res->use stays false: every item runs
            }
        }
        hipLaunchKernelGGL(k_rs_join<true>, dim3(gj), dim3(kRsWG), 0, st, d_rh, d_rn, s, N, d_U, d_ustart, nu, v_out,
                           rshift, NW, d_bm, (unsigned long long *)nullptr);
        HIPC(hipGetLastError());
        prof.mark("mark", st);
        ph.end(2);
    }
    rc = screen_lists(ctx, d_bm, ntiles, NW, C, b0, R, d_zero, st, prof, res);
    ph.end(3);
    timing_mark(ctx, 4, st, false);
    if (rc) return rc;
    if (res->use) {
        S.used = 1;
        S.marked += res->marked;
    }
    return DREPHIP_OK;
}

// The block's cells as no-shared-hash cells: common 0 and, when wanted, denom
// min(s, nq + nr); the LIST kernels then overwrite the listed cells.  d_common /
// d_denom: the block's first row.
int rect_screen_fill(drephip_ctx *ctx, const RectSets &in, uint32_t b0, uint32_t b1, uint16_t *d_common,
                     uint16_t *d_denom, hipStream_t st) {
    RsPhases ph(ctx, st);
    HIPC(hipMemsetAsync(d_common, 0, (uint64_t)(b1 - b0) * in.N * 2, st));
    if (d_denom) {
        hipLaunchKernelGGL(k_rs_denoms, dim3(std::min<uint32_t>(b1 - b0, 65535u)), dim3(kRsWG), 0, st, in.qn, in.rn, ctx->s,
                           in.N, b0, b1 - b0, d_denom);
        HIPC(hipGetLastError());
    }
    ph.end(4);
    return DREPHIP_OK;
}

}  // namespace drephip
