"""Whole-call wall time of four C API calls whose host side is api.cpp's call
frame, staging helpers and record protocol, for a same-box A/B of two library
builds (DREPHIP_LIB names the library; tools/build_ab.sh builds the other one):

  drephip_allpairs               N = 2000, s = 1000
  drephip_allpairs_sparse_sig    N = 10000
  drephip_dist_rect_sparse       Q = 1000 x N = 10000
  drephip_linkage_counts_device  n = 10000 (average linkage, counts on the device)

Each call is warmed once, then repeated until about a second has passed (3 to
40 times); prints one JSON line: the library's build id and per call the
median, min, max and every sample in seconds.

The A/B itself, in one GPU call:
  tools/build_ab.sh parent <parent rev>
  python tools/api_ab.py --ab drep_amd/lib_ab/parent/libdrephip.so --out profiles/api_refactor_ab.json
runs, as fresh child processes in the order parent, branch, parent, `bench.py
--gpus 1 --steps 5 --warmup 2` and this script, each under its own time limit
(the first failure ends the run), and writes the file: bench.py's step time per
leg, the four calls per leg, both build ids, the spread of the two parent legs
(smallest min to largest max) and whether each branch median lies within it.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drep_amd import _lib  # noqa: E402

S, FAM = 1000, 10


def sketches(n, seed):
    """n full sorted sketches in families of FAM drawing from a pool of 2 s hashes."""
    rng = np.random.default_rng(seed)
    H = np.empty((n, S), np.uint64)
    for g in range(n):
        if g % FAM == 0:
            pool = np.unique(rng.integers(1, 2 ** 63, size=2 * S + 64, dtype=np.uint64))[:2 * S]
        H[g] = np.sort(rng.choice(pool, S, replace=False))
    return H, np.full(n, S, np.uint32)


def timed(fn):
    fn()                                                               # warm: scratch, tables, caches
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    reps = max(3, min(40, math.ceil(1.0 / max(first, 1e-6))))
    samples = [first]
    for _ in range(reps - 1):
        t0 = time.perf_counter()
        fn()
        samples.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(samples)), "min_s": min(samples), "max_s": max(samples),
            "samples_s": [round(x, 6) for x in samples]}


def main():
    import torch
    H, NH = sketches(10000, 7)
    LEN = np.full(len(NH), 5_000_000, np.uint64)
    out = {"build_id": _lib.build_id().get("src"), "lib": os.path.relpath(_lib.LIB_PATH), "calls": {}}
    with _lib.Context(0, 21, S, 42) as ctx:
        out["calls"]["drephip_allpairs N=2000"] = timed(lambda: ctx.allpairs(H[:2000], NH[:2000], want_denom=False))
        out["calls"]["drephip_allpairs_sparse_sig N=10000"] = timed(lambda: ctx.allpairs_sparse_sig(H, NH, LEN))
        out["calls"]["drephip_dist_rect_sparse Q=1000 N=10000"] = timed(
            lambda: ctx.dist_rect_sparse(H[:1000], NH[:1000], H, NH))
        n = len(NH)
        dH = torch.from_numpy(H.view(np.int64)).cuda()
        dN = torch.from_numpy(NH.view(np.int32)).cuda()
        dC = torch.zeros(n * (n - 1) // 2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ctx.allpairs_device(dH.data_ptr(), dN.data_ptr(), n, 0, n, dC.data_ptr())
        lut = _lib.distance_lut(S)
        lut_off = np.full(S + 1, -1, np.int32)
        lut_off[S] = 0
        perm = np.arange(n, dtype=np.uint32)
        out["calls"]["drephip_linkage_counts_device n=10000"] = timed(
            lambda: ctx.linkage_counts_device(dC.data_ptr(), None, n, perm, lut, lut_off, "average"))
        out["linkage_info"] = ctx.linkage_info()
    print(json.dumps(out))


def last_json(text):
    return json.loads([l for l in text.splitlines() if l.startswith("{")][-1])


def ab(parent_lib, out_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    legs = ("parent1", "branch", "parent2")
    bench, calls = {}, {}
    for leg in legs:
        env = {k: v for k, v in os.environ.items() if k != "DREPHIP_LIB"}
        if leg != "branch":
            env["DREPHIP_LIB"] = os.path.abspath(parent_lib)
        for what, cmd, into in (("bench", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], bench),
                                ("calls", [os.path.join("tools", "api_ab.py")], calls)):
            r = subprocess.run([sys.executable] + cmd, env=env, cwd=root, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("%s of leg %s failed (%d):\n%s" % (what, leg, r.returncode, r.stderr[-2000:]))
            into[leg] = last_json(r.stdout)
        print(leg, "done", file=sys.stderr, flush=True)
    ids = {leg: calls[leg]["build_id"] for leg in legs}
    assert ids["parent1"] == ids["parent2"] != ids["branch"], ids
    keys = ("median_s", "min_s", "max_s")
    doc = {"what": "the parent commit's library (tools/build_ab.sh parent <rev>; DREPHIP_LIB) against this one in one GPU "
                   "call on one MI355X, fresh processes in the order parent, branch, parent: bench.py --gpus 1 --steps 5 "
                   "--warmup 2 (ms_per_step) and tools/api_ab.py (whole-call wall time of four calls at user sizes, "
                   "each warmed once and repeated for about a second)",
           "criterion": "each branch median lies within the spread of the two parent legs around it, smallest min to "
                        "largest max, as measured in this run",
           "library_src": {"parent": ids["parent1"], "branch": ids["branch"]},
           "bench_ms_per_step": {leg: bench[leg]["ms_per_step"] for leg in legs}, "calls": {}}
    b = doc["bench_ms_per_step"]
    doc["bench_branch_no_slower_than_a_parent_leg"] = b["branch"] <= max(b["parent1"], b["parent2"])
    for name in calls["branch"]["calls"]:
        p1, br, p2 = (calls[leg]["calls"][name] for leg in legs)
        lo, hi = min(p1["min_s"], p2["min_s"]), max(p1["max_s"], p2["max_s"])
        doc["calls"][name] = {"parent1": {k: p1[k] for k in keys}, "branch": {k: br[k] for k in keys},
                              "parent2": {k: p2[k] for k in keys}, "repeats": len(br["samples_s"]),
                              "parent_spread_s": [lo, hi],
                              "parent_medians_differ_by": abs(p1["median_s"] - p2["median_s"]) / min(p1["median_s"], p2["median_s"]),
                              "branch_median_over_mean_parent_median": br["median_s"] / ((p1["median_s"] + p2["median_s"]) / 2),
                              "branch_median_within_parent_spread": lo <= br["median_s"] <= hi,
                              "samples_s": {leg: calls[leg]["calls"][name]["samples_s"] for leg in legs}}
    doc["linkage_info"] = calls["branch"].get("linkage_info")
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"bench": b, "calls": {k: [v["parent1"]["median_s"], v["branch"]["median_s"], v["parent2"]["median_s"],
                                                 v["branch_median_within_parent_spread"]] for k, v in doc["calls"].items()}},
                     indent=1))


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--ab" and sys.argv[3] == "--out":
        ab(sys.argv[2], sys.argv[4])
    else:
        main()
