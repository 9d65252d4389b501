#!/usr/bin/env python3
"""The query-against-reference rectangle above the whole-row tables
(drephip_dist_rect_device at s > 2048): the RECT flavour of the band kernel
against the two routes a caller had before it.  Writes profiles/rect_band.json,
keyed on drephip_build_id.

  python tools/rect_band_bench.py                 # Q = 1000, N = 10000, s = 10000

Synthetic genome families as tools/rect_bench.py makes them (seed 0xD2E9,
families of 100, 5 Mbp), sketched on the device; the queries are every
(N + Q) / Q-th genome of the set, so each has relatives among the references.
Routes:
  (a) the band rectangle (DREPHIP_RECT_BAND_AUTO);
  (b) the same call under DREPHIP_RECT_BAND_OFF: k_rect_merge, the route before
      the band kernel;
  (c) drephip_allpairs_device, DREPHIP_AP_AUTO, screen off, rows [0, Q) of the
      stacked [queries; references] matrix: the triangle's band kernel, the
      only band-speed route a caller had.
One warm-up of each route, then `--repeats` interleaved repeats, every run
recorded (drephip_last_kernel_ms which 2).  Bars, against the routes measured
in the same run:
  (i)  (a)'s median ns per pair <= (c)'s median + (c)'s own max - min spread;
  (ii) (a)'s slowest run is faster than (b)'s fastest.
Recorded without a bar: the (b) / (a) ratio, whether (a) and (b) are equal
cell for cell, whether rows 0, 1, Q / 2 and Q - 1 of (a) equal (c)'s, and the
wall time of drephip_dist_rect_top_device(top = 10) on routes (a) and (b).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--q", type=int, default=1000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--s", type=int, default=10000)
    ap.add_argument("--L", type=int, default=5_000_000)
    ap.add_argument("--fam", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=5500, help="genomes sketched per chunk")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_band.json"))
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
           "repeats": a.repeats, "top": a.top}

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
    sh, sn = torch.cat([d_qh, d_rh]), torch.cat([d_qn, d_rn])     # route (c)'s stacked matrix
    torch.cuda.synchronize()

    band_c = torch.zeros((Q, N), dtype=torch.int16, device=dev)
    band_d = torch.zeros((Q, N), dtype=torch.int16, device=dev)
    merge_c = torch.zeros((Q, N), dtype=torch.int16, device=dev)
    merge_d = torch.zeros((Q, N), dtype=torch.int16, device=dev)
    tri_pairs = Q * M - Q * (Q + 1) // 2                      # rows [0, Q) of the stacked triangle
    tri_c = torch.zeros(tri_pairs, dtype=torch.int16, device=dev)
    tri_d = torch.zeros(tri_pairs, dtype=torch.int16, device=dev)
    hits = torch.zeros((Q, a.top, 4), dtype=torch.int32, device=dev)
    count = torch.zeros(Q, dtype=torch.int32, device=dev)
    ctx.set_allpairs_screen(2)                                # DREPHIP_SCREEN_OFF
    ctx.set_timing(True, kernels=(2, 3))
    want = {ctx.RECT_BAND_AUTO: (ctx.AP_BAND, 0), ctx.RECT_BAND_OFF: (ctx.AP_MERGE, 0)}

    def rect(mode, c, d):
        ctx.set_rect_band(mode)
        ctx.dist_rect_device(d_qh.data_ptr(), d_qn.data_ptr(), Q, d_rh.data_ptr(), d_rn.data_ptr(), N, 0, Q,
                             c.data_ptr(), d.data_ptr(), stream)
        assert ctx.last_rect_info() == want[mode], ctx.last_rect_info()
        return ctx.kernel_ms(2)[0]

    def tri():
        ctx.allpairs_device(sh.data_ptr(), sn.data_ptr(), M, 0, Q, tri_c.data_ptr(), tri_d.data_ptr(), stream)
        return ctx.kernel_ms(2)[0]

    def top(mode):
        ctx.set_rect_band(mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.dist_rect_top_device(d_qh.data_ptr(), d_qn.data_ptr(), Q, d_rh.data_ptr(), d_rn.data_ptr(), N, 0, Q, a.top,
                                 hits.data_ptr(), count.data_ptr(), stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rect(ctx.RECT_BAND_AUTO, band_c, band_d)                  # warm-up of the three routes
    rect(ctx.RECT_BAND_OFF, merge_c, merge_d)
    tri()
    torch.cuda.synchronize()
    res["band_equals_merge"] = bool(torch.equal(band_c, merge_c)) and bool(torch.equal(band_d, merge_d))
    # row q of the triangle segment is its Q - 1 - q query columns, then the N references
    ok = True
    for q in (0, 1, Q // 2, Q - 1):
        a0 = q * M - q * (q + 1) // 2 + (Q - 1 - q)
        ok = ok and bool(torch.equal(tri_c[a0:a0 + N], band_c[q])) and bool(torch.equal(tri_d[a0:a0 + N], band_d[q]))
    res["rows_equal_triangle_route"] = ok
    res["nonzero_cells"] = int((band_c != 0).sum().item())

    runs = []
    for _ in range(a.repeats):
        runs.append({"band_kernel_ms": rect(ctx.RECT_BAND_AUTO, band_c, band_d),
                     "merge_kernel_ms": rect(ctx.RECT_BAND_OFF, merge_c, merge_d),
                     "triangle_kernel_ms": tri()})
    top(ctx.RECT_BAND_AUTO)                                   # warm-up (scratch rectangle)
    res["top_wall_ms"] = {"band": [top(ctx.RECT_BAND_AUTO) for _ in range(3)],
                          "merge": [top(ctx.RECT_BAND_OFF) for _ in range(3)]}
    rect_pairs = Q * N
    ba = [x["band_kernel_ms"] / rect_pairs * 1e6 for x in runs]       # ns per pair
    me = [x["merge_kernel_ms"] / rect_pairs * 1e6 for x in runs]
    tr = [x["triangle_kernel_ms"] / tri_pairs * 1e6 for x in runs]
    spread = max(tr) - min(tr)
    res.update(runs=runs, rect_pairs=rect_pairs, triangle_pairs=tri_pairs,
               band_ns_per_pair_median=statistics.median(ba), merge_ns_per_pair_median=statistics.median(me),
               triangle_ns_per_pair_median=statistics.median(tr), triangle_ns_per_pair_spread=spread,
               band_pairs_per_s_median=1e9 / statistics.median(ba),
               merge_over_band=statistics.median(me) / statistics.median(ba),
               bar_i="band median <= triangle median + triangle (max - min)",
               bar_i_met=bool(statistics.median(ba) <= statistics.median(tr) + spread),
               bar_ii="band slowest < merge fastest", bar_ii_met=bool(max(ba) < min(me)),
               not_measured=["Q >> 10^3", "several GPUs", "s = 32767"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    return 0 if ok and res["band_equals_merge"] else 1


if __name__ == "__main__":
    sys.exit(main())
