#!/usr/bin/env python3
"""Scale records of the sparse all-pairs call (drephip_allpairs_sparse_device):
profiles/sparse_<N>.json, keyed on drephip_build_id.

  python tools/sparse_scale.py 100000            # against the dense route, same build and box
  python tools/sparse_scale.py 1000000 --L 200000 --cluster

Each N runs in a child process of its own under `timeout` (--limit seconds);
the child rewrites its record after every stage, so a run that does not fit or
finish leaves the stages it completed and "stopped_after".  Synthetic genome
families as tests/test_scale.py generates them (seed 0xD2E9, families of 100),
sketched on the device in chunks.

N <= 2x10^5 (--dense, default there): the sparse call is timed against
drephip_allpairs_device plus the pair extraction drephip_linkage_counts_device
performs on the condensed result (k_sparse_pairs; its linkage_stats matrix_s),
and the two pair lists are compared.  Larger N: no dense result can exist, so
10^6 randomly drawn listed pairs and 10^6 randomly drawn unlisted pairs are
merged again by the C oracle (Mash's literal merge); --cluster also times
cluster_mash_sparse on the list.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(a):
    import numpy as np
    import torch
    import oracle
    from drep_amd import _lib, d_cluster

    N, s, L, fam, seed = a.n, a.s, a.L, a.fam, 0xD2E9
    out_path = os.path.join(ROOT, "profiles", "sparse_%d.json" % N)
    res = {"build_id": _lib.lib().drephip_build_id().decode(), "genomes": N, "genome_bp": L, "sketch": s,
           "family_size": fam, "seed": seed, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}

    def stage(name, **kv):
        res.update(kv)
        res["stopped_after"] = name
        json.dump(res, open(out_path, "w"), indent=1)
        print("%.1f %s %s" % (time.time(), name, json.dumps(kv)[:300]), flush=True)

    def hbm_used():
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx = _lib.Context(device=0, k=21, s=s, seed=42)
    tile, P = _lib.tile_bases(), _lib.padded_bases([L])
    CH = min(N, a.chunk)
    codes = torch.zeros((tile + CH * P) // 16, dtype=torch.int32, device=dev)
    valid = torch.zeros((tile + CH * P) // 32, dtype=torch.int32, device=dev)
    hh = torch.full((N, s), -1, dtype=torch.int64, device=dev)
    nn = torch.zeros(N, dtype=torch.int32, device=dev)
    t0 = time.perf_counter()
    for g0 in range(0, N, CH):
        n = min(CH, N - g0)
        ctx.synth_device(seed, g0, n, fam, L, codes.data_ptr(), valid.data_ptr(), stream)
        ctx.sketch_device(codes.data_ptr(), valid.data_ptr(), np.array([tile + i * P for i in range(n)], np.uint64),
                          np.full(n, P, np.uint64), np.full(n, L - 20, np.uint64), n, hh[g0].data_ptr(),
                          nn[g0:].data_ptr(), stream)
    torch.cuda.synchronize()
    del codes, valid
    torch.cuda.empty_cache()
    stage("sketch", synth_and_sketch_s=time.perf_counter() - t0, hbm_after_sketch=hbm_used())

    def sparse_call(buf, cap):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc, n = ctx.allpairs_sparse_device(hh.data_ptr(), nn.data_ptr(), N, 0, N, buf.data_ptr() if cap else None, cap,
                                           stream)
        torch.cuda.synchronize()
        return rc, n, time.perf_counter() - t

    # warm-up (scratch allocation) and the size: a count-only call
    rc, npairs, t_count = sparse_call(None, 0)
    stage("count", pairs=npairs, count_only_first_call_s=t_count, sparse_stats_count=ctx.sparse_stats())
    buf = torch.empty((max(npairs, 1), 4), dtype=torch.int32, device=dev)
    ctx.set_timing(True, kernels=[2, 4])
    times = []
    for _ in range(a.repeats + 1):                       # the first (buffer just allocated) is not kept
        rc, n, t = sparse_call(buf, npairs)
        assert rc == 0 and n == npairs
        times.append(t)
    st = ctx.sparse_stats()
    stage("sparse", sparse_allpairs_s=times[1:], sparse_allpairs_median_s=float(np.median(times[1:])),
          sparse_stats=st, row_blocks=st["blocks"], peak_scratch_bytes=st["scratch_bytes"],
          screen=ctx.screen_stats(), screen_ms=ctx.kernel_ms(4)[0], list_kernel_ms=ctx.kernel_ms(2)[0],
          hbm_after_sparse=hbm_used())
    ctx.set_timing(False)
    rec = buf.cpu().numpy().view(np.uint32)
    order = np.lexsort((rec[:, 1], rec[:, 0]))
    rec = rec[order]
    key = rec[:, 0].astype(np.int64) * N + rec[:, 1]
    assert (np.diff(key) > 0).all(), "a pair is listed twice"
    del buf
    torch.cuda.empty_cache()

    if a.dense:
        total = N * (N - 1) // 2
        d_common = torch.zeros(total, dtype=torch.int16, device=dev)
        dctx = _lib.Context(device=0, k=21, s=s, seed=42)           # its own scratch: the build's dense route
        dctx.set_linkage_path(dctx.LINK_SPARSE)
        lut, lut_off = d_cluster.linkage_tables(np.array([s]), s)
        perm = np.arange(N, dtype=np.uint32)
        td, tx = [], []
        for _ in range(a.repeats + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            dctx.allpairs_device(hh.data_ptr(), nn.data_ptr(), N, 0, N, d_common.data_ptr(), None, stream)
            torch.cuda.synchronize()
            td.append(time.perf_counter() - t)
            dctx.linkage_counts_device(d_common.data_ptr(), None, N, perm, lut, lut_off, "single")
            tx.append(dctx.linkage_stats()["matrix_s"])
        info = dctx.linkage_info()
        step = 1 << 30                                   # (torch.nonzero indexes a tensor of < 2^31 elements)
        nz = np.concatenate([torch.nonzero(d_common[a0:a0 + step])[:, 0].cpu().numpy() + a0
                             for a0 in range(0, total, step)])
        cc = np.concatenate([d_common[a0:a0 + step][d_common[a0:a0 + step] != 0].cpu().numpy()
                             for a0 in range(0, total, step)]).view(np.uint16)
        di, dj = d_cluster._condensed_ij(nz, N)
        equal = bool(len(nz) == len(rec) and np.array_equal(di, rec[:, 0]) and np.array_equal(dj, rec[:, 1]) and
                     np.array_equal(cc, rec[:, 2]) and (rec[:, 3] == s).all())
        dense_s = [x + y for x, y in zip(td[1:], tx[1:])]
        stage("dense", dense_allpairs_s=td[1:], dense_extraction_s=tx[1:], dense_route_s=dense_s,
              dense_route_median_s=float(np.median(dense_s)), dense_linkage_info=info, lists_equal=equal,
              dense_pairs=int(len(nz)), hbm_after_dense=hbm_used())
        assert equal
    else:
        H = hh.cpu().numpy().view(np.uint64)
        NH = nn.cpu().numpy().view(np.uint32)
        rng = np.random.default_rng(N)
        m = min(a.sample, len(rec))
        pick = rng.choice(len(rec), m, replace=False)
        oc, od = oracle.dist_pairs_list(H, NH, s, rec[pick, 0], rec[pick, 1], threads=16)
        bad_listed = int(((oc != rec[pick, 2]) | (od != rec[pick, 3])).sum())
        ui = rng.integers(0, N, 3 * a.sample).astype(np.int64)
        uj = rng.integers(0, N, 3 * a.sample).astype(np.int64)
        lo, hi = np.minimum(ui, uj), np.maximum(ui, uj)
        k = lo != hi
        lo, hi = lo[k], hi[k]
        listed = np.isin(lo * N + hi, key)
        lo, hi = lo[~listed][:a.sample], hi[~listed][:a.sample]
        oc, _ = oracle.dist_pairs_list(H, NH, s, lo.astype(np.uint32), hi.astype(np.uint32), threads=16)
        stage("sampled", sampled_listed=int(m), sampled_listed_mismatches=bad_listed, sampled_unlisted=int(len(lo)),
              sampled_unlisted_mismatches=int((oc != 0).sum()), checker="oracle.dist_pairs_list (Mash's literal merge)")
        assert bad_listed == 0 and int((oc != 0).sum()) == 0

    if a.cluster:
        names = ["g%07d" % g for g in range(N)]
        sm = d_cluster.SparseMash(names, names, rec[:, 0], rec[:, 1], rec[:, 2].astype(np.uint16),
                                  rec[:, 3].astype(np.uint16), nn.cpu().numpy().view(np.uint32),
                                  np.full(N, L, np.uint64), s)
        t = time.perf_counter()
        Cdb, _ = d_cluster.cluster_mash_sparse(sm, clusterAlg=a.alg, P_ani=0.9)
        stage("cluster", cluster_mash_sparse_s=time.perf_counter() - t, cluster_alg=a.alg,
              clusters=int(Cdb["primary_cluster"].nunique()))
    stage("done", hbm_peak_seen=hbm_used())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", type=int, nargs="+", help="genome counts, one child process each")
    ap.add_argument("--s", type=int, default=1000)
    ap.add_argument("--L", type=int, default=None, help="genome length (default 5000000 up to 2x10^5 genomes, else 200000)")
    ap.add_argument("--fam", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=10000, help="genomes sketched per chunk")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--alg", default="single")
    ap.add_argument("--dense", action="store_true", default=None, help="compare with the dense route (default: N <= 200000)")
    ap.add_argument("--cluster", action="store_true", help="time cluster_mash_sparse on the list")
    ap.add_argument("--limit", type=int, default=540, help="seconds each child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        a.n = a.n[0]
        a.L = a.L or (5_000_000 if a.n <= 200_000 else 200_000)
        a.dense = a.n <= 200_000 if a.dense is None else a.dense
        worker(a)
        return 0
    for n in a.n:
        cmd =["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), str(n), "--worker",
               "--s", str(a.s), "--fam", str(a.fam), "--chunk", str(a.chunk), "--repeats", str(a.repeats),
               "--sample", str(a.sample), "--alg", a.alg, "--limit", str(a.limit)] + \
              (["--L", str(a.L)] if a.L else []) + (["--dense"] if a.dense else []) + (["--cluster"] if a.cluster else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:                                      # a fault, an abort or the time limit: nothing more is started
            print("N = %d stopped with exit status %d; see profiles/sparse_%d.json (stopped_after)" % (n, rc, n))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
