#!/usr/bin/env python3
"""The query-against-reference rectangle (drephip_dist_rect_device) against the
only route the library had for the same numbers: drephip_allpairs_device with
the screen off over rows [0, Q) of the stacked [queries; references] matrix.
Writes profiles/rect_dist.json, keyed on drephip_build_id.

  python tools/rect_bench.py                      # Q = 1000, N = 100000, s = 1000

Synthetic genome families as tools/sparse_scale.py makes them (seed 0xD2E9,
families of 100), sketched on the device; the queries are every
(N + Q) / Q-th genome of the set, so each has relatives among the references.
After one warm-up of each route, `--repeats` interleaved repeats: the RECT
kernel (drephip_last_kernel_ms which 2; which 3, its table build, recorded
beside it), the triangle route's kernel on a stacked matrix that already
exists, and the stacking copy itself (torch.cat of the two matrices, timed
with events).  Every run is recorded.  The bar: the rectangle's median kernel
time per pair is no worse than the triangle route's median, beyond the
triangle route's own min-max spread in this run.  The rectangle's cells are
also compared with the triangle route's once.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--q", type=int, default=1000)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--s", type=int, default=1000)
    ap.add_argument("--L", type=int, default=5_000_000)
    ap.add_argument("--fam", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=10000, help="genomes sketched per chunk")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_dist.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from drep_amd import _lib

    Q, N, s, L, seed = a.q, a.n, a.s, a.L, 0xD2E9
    M = Q + N
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx = _lib.Context(device=0, k=21, s=s, seed=42)
    ctx.set_rect_screen(ctx.RECT_SCREEN_OFF)                  # this record is of the unscreened kernels
    res = {"build_id": _lib.lib().drephip_build_id().decode(), "device": torch.cuda.get_device_name(0),
           "queries": Q, "references": N, "sketch": s, "genome_bp": L, "family_size": a.fam, "seed": seed,
           "repeats": a.repeats}

    tile, P = _lib.tile_bases(), _lib.padded_bases([L])
    CH = min(M, a.chunk)
    codes = torch.zeros((tile + CH * P) // 16, dtype=torch.int32, device=dev)
    valid = torch.zeros((tile + CH * P) // 32, dtype=torch.int32, device=dev)
    hh = torch.full((M, s), -1, dtype=torch.int64, device=dev)
    nn = torch.zeros(M, dtype=torch.int32, device=dev)
    for g0 in range(0, M, CH):
        n = min(CH, M - g0)
        ctx.synth_device(seed, g0, n, a.fam, L, codes.data_ptr(), valid.data_ptr(), stream)
        ctx.sketch_device(codes.data_ptr(), valid.data_ptr(), np.array([tile + i * P for i in range(n)], np.uint64),
                          np.full(n, P, np.uint64), np.full(n, L - 20, np.uint64), n, hh[g0].data_ptr(),
                          nn[g0:].data_ptr(), stream)
    torch.cuda.synchronize()
    del codes, valid
    qsel = torch.zeros(M, dtype=torch.bool, device=dev)
    qsel[torch.arange(Q, device=dev) * (M // Q)] = True
    d_qh, d_qn = hh[qsel].contiguous(), nn[qsel].contiguous()
    d_rh, d_rn = hh[~qsel].contiguous(), nn[~qsel].contiguous()
    del hh, nn
    torch.cuda.empty_cache()

    rect_c = torch.zeros((Q, N), dtype=torch.int16, device=dev)
    rect_d = torch.zeros((Q, N), dtype=torch.int16, device=dev)
    tri_pairs = Q * M - Q * (Q + 1) // 2                      # rows [0, Q) of the stacked triangle
    tri_c = torch.zeros(tri_pairs, dtype=torch.int16, device=dev)
    tri_d = torch.zeros(tri_pairs, dtype=torch.int16, device=dev)
    ctx.set_allpairs_screen(2)                                # DREPHIP_SCREEN_OFF
    ctx.set_timing(True, kernels=(2, 3))

    def rect():
        ctx.dist_rect_device(d_qh.data_ptr(), d_qn.data_ptr(), Q, d_rh.data_ptr(), d_rn.data_ptr(), N, 0, Q,
                             rect_c.data_ptr(), rect_d.data_ptr(), stream)
        return ctx.kernel_ms(2)[0], ctx.kernel_ms(3)[0]

    def stack():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sh, sn = torch.cat([d_qh, d_rh]), torch.cat([d_qn, d_rn])
        e1.record()
        torch.cuda.synchronize()
        return sh, sn, e0.elapsed_time(e1)

    def tri(sh, sn):
        ctx.allpairs_device(sh.data_ptr(), sn.data_ptr(), M, 0, Q, tri_c.data_ptr(), tri_d.data_ptr(), stream)
        return ctx.kernel_ms(2)[0], ctx.kernel_ms(3)[0]

    rect()                                                    # warm-up of both routes
    sh, sn, _ = stack()
    tri(sh, sn)
    torch.cuda.synchronize()
    # the same numbers: row q of the triangle segment is its Q - 1 - q query columns, then the N references
    ok = True
    for q in (0, 1, Q // 2, Q - 1):
        a0 = q * M - q * (q + 1) // 2 + (Q - 1 - q)
        ok = ok and bool(torch.equal(tri_c[a0:a0 + N], rect_c[q])) and bool(torch.equal(tri_d[a0:a0 + N], rect_d[q]))
    res["rows_equal_triangle_route"] = ok
    del sh, sn

    runs = []
    for _ in range(a.repeats):
        r_ms, r_build = rect()
        sh, sn, copy_ms = stack()
        t_ms, t_build = tri(sh, sn)
        del sh, sn
        runs.append({"rect_kernel_ms": r_ms, "rect_build_ms": r_build, "triangle_kernel_ms": t_ms,
                     "triangle_build_ms": t_build, "stack_copy_ms": copy_ms})
    rect_pairs = Q * N
    r = [x["rect_kernel_ms"] / rect_pairs * 1e6 for x in runs]       # ns per pair
    t = [x["triangle_kernel_ms"] / tri_pairs * 1e6 for x in runs]
    tc = [(x["triangle_kernel_ms"] + x["stack_copy_ms"]) / tri_pairs * 1e6 for x in runs]
    spread = max(t) - min(t)
    res.update(runs=runs, rect_pairs=rect_pairs, triangle_pairs=tri_pairs,
               rect_ns_per_pair_median=statistics.median(r), triangle_ns_per_pair_median=statistics.median(t),
               triangle_with_copy_ns_per_pair_median=statistics.median(tc), triangle_ns_per_pair_spread=spread,
               bar="rect median <= triangle median + triangle (max - min)",
               bar_met=bool(statistics.median(r) <= statistics.median(t) + spread))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
