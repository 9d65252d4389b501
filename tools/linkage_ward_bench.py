"""Ward next to average on the dense GPU chain, on the configs[2] counts (n
synthetic 5 Mbp genomes at s = 1000, families of 100, generated, sketched and
compared on the device as tests/test_scale.py does):

  python tools/linkage_ward_bench.py [--n 10000] [--runs 3] [--scipy] [--out profiles/linkage_ward.json]

Per method: chain_s (scratch, graph capture and the steps), wall_s of the
whole call, launches per merge -- the median of --runs calls in this one
process -- and, with --scipy, the host time of scipy's linkage on the same
input and whether Z equals it.  Prints one JSON line; --out merges it into a
JSON file under the key "n=<n>".

The library is the one drep_amd._lib loads ($DREPHIP_LIB for another build:
--methods average then works with builds older than ward).  --counts-cache
keeps the counts in a .npy between processes (same-box A/B runs)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_counts(ctx, N, s, L, fam, seed, dev, stream, chunk=10000):
    import torch
    from drep_amd import _lib
    tile = _lib.tile_bases()
    P = _lib.padded_bases([L])
    CH = min(N, chunk)
    codes = torch.zeros((tile + CH * P) // 16, dtype=torch.int32, device=dev)
    valid = torch.zeros((tile + CH * P) // 32, dtype=torch.int32, device=dev)
    hh = torch.full((N, s), -1, dtype=torch.int64, device=dev)
    nn = torch.zeros(N, dtype=torch.int32, device=dev)
    for g0 in range(0, N, CH):
        n = min(CH, N - g0)
        ctx.synth_device(seed, g0, n, fam, L, codes.data_ptr(), valid.data_ptr(), stream)
        ctx.sketch_device(codes.data_ptr(), valid.data_ptr(), np.array([tile + i * P for i in range(n)], np.uint64),
                          np.full(n, P, np.uint64), np.full(n, L - 20, np.uint64), n,
                          hh[g0].data_ptr(), nn[g0:].data_ptr(), stream)
    del codes, valid
    d_common = torch.zeros(N * (N - 1) // 2, dtype=torch.int16, device=dev)
    ctx.allpairs_device(hh.data_ptr(), nn.data_ptr(), N, 0, N, d_common.data_ptr(), None, stream)
    torch.cuda.synchronize()
    return d_common


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--methods", default="average,ward")
    ap.add_argument("--genome-bp", type=int, default=5_000_000)
    ap.add_argument("--scipy", action="store_true", help="time scipy's linkage on the host and compare Z")
    ap.add_argument("--counts-cache", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from drep_amd import _lib
    from drep_amd.d_cluster import linkage_tables
    N, s = a.n, 1000
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"n": N, "sketch": s, "genome_bp": a.genome_bp, "family_size": 100, "runs": a.runs,
           "build": _lib.build_id(), "lib": os.path.relpath(_lib.LIB_PATH, ROOT)}
    with _lib.Context(device=0, k=21, s=s, seed=42) as ctx:
        if a.counts_cache and os.path.exists(a.counts_cache):
            d_common = torch.from_numpy(np.load(a.counts_cache)).to(dev)
        else:
            d_common = device_counts(ctx, N, s, a.genome_bp, 100, 0xD2E9, dev, stream)
            if a.counts_cache:
                np.save(a.counts_cache, d_common.cpu().numpy())
    lut, lut_off = linkage_tables(np.array([s]), s)
    perm = np.arange(N, dtype=np.uint32)
    y = None
    with _lib.Context(device=0, k=21, s=s, seed=42) as ctx:
        ctx.linkage_reserve(N)
        ctx.set_linkage_path(ctx.LINK_DENSE)
        for method in a.methods.split(","):
            runs = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                Z = ctx.linkage_counts_device(d_common.data_ptr(), None, N, perm, lut, lut_off, method, stream)
                wall = time.perf_counter() - t0
                st = ctx.linkage_stats()
                runs.append({"chain_s": st["chain_s"], "matrix_s": st["matrix_s"], "finish_s": st["finish_s"],
                             "wall_s": wall, "launches_per_merge": ctx.linkage_launches() / (N - 1)})
            r = {"runs": runs, "chain_s": float(np.median([x["chain_s"] for x in runs])),
                 "wall_s": float(np.median([x["wall_s"] for x in runs])),
                 "launches_per_merge": runs[-1]["launches_per_merge"]}
            if a.scipy:
                import scipy.cluster.hierarchy as sch
                if y is None:
                    y = lut[d_common.cpu().numpy().view(np.uint16)]
                t0 = time.perf_counter()
                Zs = sch.linkage(y, method=method)
                r["scipy_host_s"] = time.perf_counter() - t0
                r["Z_equals_scipy"] = bool(np.array_equal(Z, Zs))
            res[method] = r
    print(json.dumps(res))
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["n=%d" % N] = res
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
