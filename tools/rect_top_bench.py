#!/usr/bin/env python3
"""Best hits per query (drephip_dist_rect_top_device) against the route a caller
had before it: drephip_dist_rect_sparse_device, the records copied to the host,
and a numpy selection there.  Writes profiles/rect_top.json, keyed on
drephip_build_id.

  python tools/rect_top_bench.py                  # Q = 1000, N = 100000, s = 1000, top 1 and 10

Synthetic genome families as tools/rect_bench.py makes them (seed 0xD2E9,
families of 100), sketched on the device; the queries are every
(N + Q) / Q-th genome of the set, so each has relatives among the references.
Per `top`: one warm-up of each route, then `--repeats` interleaved repeats.
Route (a): the call, then its hits and counts copied to the host.  Route (b):
the record call into a device buffer sized by the warm-up, the records copied
to the host, then per query the `top` largest of the kernel's own 64-bit key
(floor(common (2^32 - 1) / denom) << 32 | ~r) by one numpy sort.  Every run is
recorded: both routes' whole wall time (host clock, ending after the copy or
the selection), route (a)'s counts kernel (drephip_last_kernel_ms which 2) and
selection kernel (which 5), the bytes each route brought to the host.  Both
routes must give the same hits.  The bar: route (a)'s median wall time is no
worse than route (b)'s median plus (b)'s own max - min spread.  The selection
kernel's share of the counts kernel's time is reported, not gated.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def select_on_host(rec, Q, top):
    """(ref int64 [Q, top] with -1 past count, common, denom, count) from the
    records {q, r, common, denom} (uint32 [n, 4], any order)."""
    import numpy as np
    q, r = rec[:, 0].astype(np.int64), rec[:, 1]
    c, d = rec[:, 2].astype(np.uint64), rec[:, 3].astype(np.uint64)
    key = ((c * np.uint64(0xFFFFFFFF) // d) << np.uint64(32)) | (~r).astype(np.uint64)
    order = np.lexsort((~key, q))                              # query ascending, key descending
    q, rec = q[order], rec[order]
    first = np.searchsorted(q, np.arange(Q))
    rank = np.arange(len(q)) - first[q]
    keep = rank < top
    ref = np.full((Q, top), -1, np.int64)
    common = np.zeros((Q, top), np.uint16)
    denom = np.zeros((Q, top), np.uint16)
    ref[q[keep], rank[keep]] = rec[keep, 1]
    common[q[keep], rank[keep]] = rec[keep, 2]
    denom[q[keep], rank[keep]] = rec[keep, 3]
    count = np.minimum(np.bincount(q, minlength=Q), top).astype(np.uint32)
    return ref, common, denom, count


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--q", type=int, default=1000)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--s", type=int, default=1000)
    ap.add_argument("--L", type=int, default=5_000_000)
    ap.add_argument("--fam", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=10000, help="genomes sketched per chunk")
    ap.add_argument("--tops", default="1,10")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_top.json"))
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
        print("sketched %d / %d" % (g0 + n, M), file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    del codes, valid
    qsel = torch.zeros(M, dtype=torch.bool, device=dev)
    qsel[torch.arange(Q, device=dev) * (M // Q)] = True
    d_qh, d_qn = hh[qsel].contiguous(), nn[qsel].contiguous()
    d_rh, d_rn = hh[~qsel].contiguous(), nn[~qsel].contiguous()
    del hh, nn
    torch.cuda.empty_cache()
    args = (d_qh.data_ptr(), d_qn.data_ptr(), Q, d_rh.data_ptr(), d_rn.data_ptr(), N, 0, Q)
    ctx.set_timing(True, kernels=(2, 5))

    # the record list's size, for route (b)'s buffer and the non-zero share
    rc, n_rec = ctx.dist_rect_sparse_device(*args, None, 0, stream)
    d_rec = torch.zeros((n_rec + 1024, 4), dtype=torch.int32, device=dev)
    res.update(records=n_rec, nonzero_share=n_rec / (Q * N))
    ok = True
    res["tops"] = {}
    for top in (int(t) for t in a.tops.split(",")):
        d_hits = torch.zeros((Q, top, 4), dtype=torch.int32, device=dev)
        d_count = torch.zeros(Q, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def route_a():
            t0 = time.perf_counter()
            ctx.dist_rect_top_device(*args, top, d_hits.data_ptr(), d_count.data_ptr(), stream)
            counts_ms, select_ms = ctx.kernel_ms(2)[0], ctx.kernel_ms(5)[0]
            hits = d_hits.cpu().numpy().view(np.uint32)
            count = d_count.cpu().numpy().view(np.uint32)
            wall = time.perf_counter() - t0
            ref = hits[:, :, 0].astype(np.int64)
            ref[ref == 0xFFFFFFFF] = -1
            return (ref, hits[:, :, 1].astype(np.uint16), hits[:, :, 2].astype(np.uint16), count), \
                {"a_wall_ms": wall * 1e3, "a_counts_kernel_ms": counts_ms, "a_select_kernel_ms": select_ms,
                 "a_bytes_to_host": hits.nbytes + count.nbytes}

        def route_b():
            t0 = time.perf_counter()
            rc, n = ctx.dist_rect_sparse_device(*args, d_rec.data_ptr(), len(d_rec), stream)
            assert rc == 0 and n == n_rec
            rec = d_rec[:n].cpu().numpy().view(np.uint32)
            got = select_on_host(rec, Q, top)
            wall = time.perf_counter() - t0
            return got, {"b_wall_ms": wall * 1e3, "b_counts_kernel_ms": ctx.kernel_ms(2)[0], "b_bytes_to_host": rec.nbytes}

        ga, _ = route_a()                                     # warm-up of both routes, and the same hits
        gb, _ = route_b()
        same = all(np.array_equal(x, y) for x, y in zip(ga, gb))
        ok = ok and same
        runs = []
        for _ in range(a.repeats):
            ga, ra = route_a()
            gb, rb = route_b()
            same = same and all(np.array_equal(x, y) for x, y in zip(ga, gb))
            runs.append({**ra, **rb})
        ok = ok and same
        wa, wb = [x["a_wall_ms"] for x in runs], [x["b_wall_ms"] for x in runs]
        spread = max(wb) - min(wb)
        share = [x["a_select_kernel_ms"] / x["a_counts_kernel_ms"] for x in runs]
        res["tops"][str(top)] = {
            "runs": runs, "routes_give_the_same_hits": bool(same), "hits_listed": int(ga[3].sum()),
            "a_wall_ms_median": statistics.median(wa), "b_wall_ms_median": statistics.median(wb),
            "b_wall_ms_spread": spread, "select_share_of_counts_kernel_median": statistics.median(share),
            "bar": "a median wall <= b median wall + b (max - min)",
            "bar_met": bool(statistics.median(wa) <= statistics.median(wb) + spread)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: ({t: {x: y for x, y in v[t].items() if x != "runs"} for t in v} if k == "tops" else v)
                      for k, v in res.items()}))
    assert ok, "the two routes disagree"
    return 0


if __name__ == "__main__":
    sys.exit(main())
