#!/usr/bin/env python3
"""Mash p-values on the GPU, measured: profiles/pvalue.json, keyed on
drephip_build_id.

  python tools/pvalue_bench.py                 # 10^5 synthetic genomes, s = 1000
  python tools/pvalue_bench.py --n 20000       # a smaller set
  python tools/pvalue_bench.py --no-gpu        # the accuracy section only

Accuracy (no GPU): the worst relative error of drephip_pvalue_eval -- the
kernels' arithmetic, bit for bit -- and of scipy's binom.sf (d_cluster.mash_pvalue)
over the normal-range rows of tests/golden/pvalue_grid.json.

Timing (one GPU): the record list of the sparse all-pairs call over synthetic
genome families (as tools/sparse_scale.py makes them), then
  - k_pvalue_records over the whole list (drephip_pvalue_records_device),
  - the stable filter at max_p (drephip_records_filter_device),
  - the copy of the survivors against the copy of the whole list,
  - drephip_allpairs_sparse_sig as a whole from host matrices, against
    drephip_allpairs_sparse plus the copy it makes,
  - d_cluster.mash_pvalue (scipy, one process) on the same records.
Wall-clock medians of --repeats blocking calls after one warm-up call.  No pass
mark goes with these numbers.
"""
import argparse
import json
import os
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "pvalue.json")


def accuracy():
    import numpy as np
    from drep_amd import _lib, d_cluster
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "pvalue_grid.json")))
    tiny = Fraction(1, 2 ** 1022)
    worst = {"pvalue_eval": Fraction(0), "scipy": Fraction(0)}
    text = {"pvalue_eval": 0, "scipy": 0}
    rows = 0
    for q in g["rows"]:
        ex = Fraction(q["exact"])
        if ex < tiny:
            continue
        rows += 1
        c, la, lb = np.array([q["common"]]), np.array([q["len_a"]]), np.array([q["len_b"]])
        got = {"pvalue_eval": float(_lib.pvalue_eval(c, la, lb, q["s"], g["k"])[0]),
               "scipy": float(d_cluster.mash_pvalue(c, la, lb, q["s"], g["k"])[0])}
        for k, v in got.items():
            worst[k] = max(worst[k], abs(Fraction(v) - ex) / ex)
            text[k] += "%g" % v != "%g" % float(ex)
    return {"grid_rows_normal_range": rows, "grid_rows": len(g["rows"]),
            "worst_relative_error": {k: float(v) for k, v in worst.items()},
            "g_text_mismatches": text, "bound_asserted_by_tests": 1e-11}


def timing(a):
    import numpy as np
    import torch
    from drep_amd import _lib, d_cluster

    N, s, L, fam, seed = a.n, a.s, a.L, a.fam, 0xD2E9
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx = _lib.Context(device=0, k=21, s=s, seed=42)
    tile, P = _lib.tile_bases(), _lib.padded_bases([L])
    CH = min(N, a.chunk)
    codes = torch.zeros((tile + CH * P) // 16, dtype=torch.int32, device=dev)
    valid = torch.zeros((tile + CH * P) // 32, dtype=torch.int32, device=dev)
    hh = torch.full((N, s), -1, dtype=torch.int64, device=dev)
    nn = torch.zeros(N, dtype=torch.int32, device=dev)
    for g0 in range(0, N, CH):
        n = min(CH, N - g0)
        ctx.synth_device(seed, g0, n, fam, L, codes.data_ptr(), valid.data_ptr(), stream)
        ctx.sketch_device(codes.data_ptr(), valid.data_ptr(), np.array([tile + i * P for i in range(n)], np.uint64),
                          np.full(n, P, np.uint64), np.full(n, L - 20, np.uint64), n, hh[g0].data_ptr(),
                          nn[g0:].data_ptr(), stream)
    torch.cuda.synchronize()
    del codes, valid
    torch.cuda.empty_cache()
    print("sketched %d genomes" % N, flush=True)

    def timed(fn, repeats=a.repeats):
        fn()                                             # warm-up: scratch allocation
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts)), ts, r

    _, npairs = ctx.allpairs_sparse_device(hh.data_ptr(), nn.data_ptr(), N, 0, N, None, 0, stream)
    rec = torch.empty((max(npairs, 1), 4), dtype=torch.int32, device=dev)
    t_list, _, _ = timed(lambda: ctx.allpairs_sparse_device(hh.data_ptr(), nn.data_ptr(), N, 0, N, rec.data_ptr(),
                                                            npairs, stream))
    # synthetic genomes all have length L; real sets differ, so lengths are drawn around it
    rng = np.random.default_rng(seed)
    length = (L * np.exp(rng.uniform(-0.7, 0.7, N))).astype(np.uint64)
    d_len = torch.tensor(length.view(np.int64), device=dev)
    pv = torch.empty(max(npairs, 1), dtype=torch.float64, device=dev)
    t_p, ts_p, _ = timed(lambda: ctx.pvalue_records_device(rec.data_ptr(), npairs, d_len.data_ptr(), N,
                                                           d_len.data_ptr(), N, pv.data_ptr(), stream))
    out = torch.empty_like(rec)
    pout = torch.empty_like(pv)
    t_f, ts_f, kept = timed(lambda: ctx.filter_records_device(rec.data_ptr(), pv.data_ptr(), npairs, a.max_p, None,
                                                              out.data_ptr(), pout.data_ptr(), stream))
    t_copy_all, _, _ = timed(lambda: (rec[:npairs].cpu(), pv[:npairs].cpu()))
    t_copy_kept, _, _ = timed(lambda: (out[:kept].cpu(), pout[:kept].cpu()))
    h_rec = rec[:npairs].cpu().numpy().view(np.uint32)
    h_p = pv[:npairs].cpu().numpy()
    res = {"genomes": N, "genome_bp": L, "sketch": s, "family_size": fam, "seed": seed, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "max_p": a.max_p, "records": int(npairs),
           "survivors": int(kept), "common_histogram_1_2_3_more": [int((h_rec[:, 2] == c).sum()) for c in (1, 2, 3)] +
           [int((h_rec[:, 2] > 3).sum())],
           "sparse_list_call_s": t_list, "k_pvalue_records_s": t_p, "k_pvalue_records_all_s": ts_p,
           "k_pvalue_records_ns_per_record": 1e9 * t_p / max(npairs, 1),
           "filter_s": t_f, "filter_all_s": ts_f,
           "bytes_copied_without_filter": int(npairs) * 24, "bytes_copied_with_filter": int(kept) * 24,
           "bytes_per_record_with_p": 24,
           "copy_all_records_and_p_s": t_copy_all, "copy_survivors_and_p_s": t_copy_kept}
    print(json.dumps(res)[:600], flush=True)
    # bit for bit against the host evaluator, on a sample
    pick = rng.choice(npairs, min(npairs, 200_000), replace=False) if npairs else np.zeros(0, np.int64)
    want = _lib.pvalue_eval(h_rec[pick, 2], length[h_rec[pick, 0]], length[h_rec[pick, 1]], s, 21)
    res["device_equals_host_evaluator_on_sample"] = bool(np.array_equal(want.view(np.uint64), h_p[pick].view(np.uint64)))
    # scipy on the same records, one process
    m = min(npairs, a.scipy_records)
    t = time.perf_counter()
    sp = d_cluster.mash_pvalue(h_rec[:m, 2], length[h_rec[:m, 0]], length[h_rec[:m, 1]], s)
    t_sp = time.perf_counter() - t
    ok = sp >= 2.0 ** -1022
    res.update({"scipy_records": int(m), "scipy_mash_pvalue_s": t_sp, "scipy_us_per_record": 1e6 * t_sp / max(m, 1),
                "scipy_threads": "one process, %s" % os.environ.get("OMP_NUM_THREADS", "default threads"),
                "max_relative_difference_to_scipy": float(np.max(np.abs(h_p[:m][ok] - sp[ok]) / sp[ok])) if ok.any()
                else 0.0})
    # the _sig call as a whole, from host matrices
    del rec, out, pv, pout
    torch.cuda.empty_cache()
    H = hh.cpu().numpy().view(np.uint64)
    NH = nn.cpu().numpy().view(np.uint32)
    del hh, nn
    torch.cuda.empty_cache()
    buf = np.empty((max(npairs, 1), 4), np.uint32)
    pbuf = np.empty(max(npairs, 1), np.float64)
    t_plain, _, _ = timed(lambda: ctx.allpairs_sparse_raw(H, NH, 0, N, buf), a.sig_repeats)
    t_sig, _, r = timed(lambda: ctx.allpairs_sparse_sig_raw(H, NH, length, 0, N, a.max_p, None, buf, pbuf), a.sig_repeats)
    t_sig1, _, r1 = timed(lambda: ctx.allpairs_sparse_sig_raw(H, NH, length, 0, N, 1.0, None, buf, pbuf), a.sig_repeats)
    res.update({"host_allpairs_sparse_s": t_plain, "host_allpairs_sparse_sig_s": t_sig,
                "host_allpairs_sparse_sig_unfiltered_s": t_sig1, "sig_survivors": int(r[1]), "sig_listed": int(r[2]),
                "sig_repeats": a.sig_repeats,
                "note": "the _sig call lists twice (a counting run, then the records) and stages the same matrices"})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--s", type=int, default=1000)
    ap.add_argument("--L", type=int, default=5_000_000)
    ap.add_argument("--fam", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sig-repeats", type=int, default=2)
    ap.add_argument("--max-p", type=float, default=1e-10)
    ap.add_argument("--scipy-records", type=int, default=4_000_000)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from drep_amd import _lib
    res = {"build_id": _lib.lib().drephip_build_id().decode(), "accuracy": accuracy()}
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res["accuracy"]), flush=True)
    if not a.no_gpu:
        res["timing"] = timing(a)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
