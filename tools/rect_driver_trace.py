#!/usr/bin/env python3
"""What the query-against-reference host side queues, call by call: for
refactors of it that must not add, drop or reorder a launch or a
synchronisation.

  rocprofv3 --hip-trace --kernel-trace -f csv -d DIR -o t -- python tools/rect_driver_trace.py run
  python tools/rect_driver_trace.py summarize DIR out.json
  python tools/rect_driver_trace.py compare parent.json branch.json [both.json]

`run` makes one host-form call (rows [3, 38) of 41 queries x 97 references,
s = 64, DREPHIP_RECT_BLOCK_ROWS = DREPHIP_RECT_TOP_BLOCK_ROWS = 5,
DREPHIP_RECT_SCREEN_BLOCK_ROWS = 7) of every form (dense, records, best hits)
by every kernel (table and band with the screen off and forced; merge), each in
a context of its own, with a hipRuntimeGetVersion call -- which nothing else in
the process makes -- before each and after the last.  `summarize` cuts the HIP
trace at those marks and lists per call the kernels in launch order and the
counts of hipStreamSynchronize, hipMemcpyAsync and hipMemsetAsync.  DREPHIP_LIB
selects the library, as everywhere."""
import csv
import ctypes
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NQ, NREF, S, Q0, Q1 = 41, 97, 64, 3, 38
CALLS = [(form, kernel, screen) for form in ("dense", "records", "top")
         for kernel, screen in (("table", "off"), ("table", "force"), ("band", "off"), ("band", "force"), ("merge", "off"))]
MARK, COUNTED = "hipRuntimeGetVersion", ("hipStreamSynchronize", "hipMemcpyAsync", "hipMemsetAsync")


def sets(np):
    """97 sketches in families of 8 drawn from a family's pool of 2 s hashes;
    row 11 empty, row 5 partial.  The queries are the first 41."""
    rng = np.random.default_rng(64)
    H = np.full((NREF, S), np.iinfo(np.uint64).max, dtype=np.uint64)
    NH = np.full(NREF, S, dtype=np.uint32)
    pools = [np.unique(rng.integers(1, 1 << 62, size=2 * S + 8, dtype=np.uint64))[:2 * S] for _ in range(-(-NREF // 8))]
    NH[11], NH[5] = 0, S // 2
    for g in range(NREF):
        H[g, :NH[g]] = np.sort(rng.choice(pools[g // 8], S, replace=False))[:NH[g]]
    return H, NH


def run():
    import numpy as np
    from drep_amd import _lib
    os.environ.update(DREPHIP_RECT_BLOCK_ROWS="5", DREPHIP_RECT_TOP_BLOCK_ROWS="5", DREPHIP_RECT_SCREEN_BLOCK_ROWS="7")
    H, NH = sets(np)
    _lib.lib()
    # the HIP runtime the library runs on, not a second copy
    hip = ctypes.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln))
    version = ctypes.c_int(0)
    for form, kernel, screen in CALLS:
        with _lib.Context(0, 21, S, 42) as ctx:
            if kernel == "band":
                ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
            elif kernel == "merge":
                ctx.set_allpairs_path(ctx.AP_MERGE)
            ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE if screen == "force" else ctx.RECT_SCREEN_OFF)
            hip.hipRuntimeGetVersion(ctypes.byref(version))
            if form == "dense":
                ctx.dist_rect(H[:NQ], NH[:NQ], H, NH, Q0, Q1)
            elif form == "records":
                ctx.dist_rect_sparse(H[:NQ], NH[:NQ], H, NH, Q0, Q1, cap=NQ * NREF)
            else:
                ctx.dist_rect_top(H[:NQ], NH[:NQ], H, NH, 3, Q0, Q1)
            hip.hipRuntimeGetVersion(ctypes.byref(version))
    print("build " + _lib.lib().drephip_build_id().decode())


def rows(directory, suffix):
    out = []
    for path in glob.glob(os.path.join(directory, "**", "*" + suffix), recursive=True):
        out += list(csv.DictReader(open(path)))
    return out


def summarize(directory, out):
    api = sorted(rows(directory, "hip_api_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    kernel = {r["Correlation_Id"]: r["Kernel_Name"] for r in rows(directory, "kernel_trace.csv")}
    marks = [i for i, r in enumerate(api) if r["Function"] == MARK]
    assert len(marks) == 2 * len(CALLS), "%d marks, %d calls" % (len(marks), len(CALLS))
    calls = []
    for n, (form, kernel_name, screen) in enumerate(CALLS):
        seg = api[marks[2 * n] + 1:marks[2 * n + 1]]
        rec = {"form": form, "kernel": kernel_name, "screen": screen,
               "kernels": [kernel[r["Correlation_Id"]] for r in seg if r["Correlation_Id"] in kernel]}
        rec.update({f: sum(r["Function"] == f for r in seg) for f in COUNTED})
        calls.append(rec)
    json.dump({"calls": calls}, open(out, "w"), indent=1)
    for c in calls:
        print(c["form"], c["kernel"], c["screen"], len(c["kernels"]), "kernels", {f: c[f] for f in COUNTED})


def compare(a, b, out=None):
    """Equal call by call?  `out`: both summaries in one file, the kernel
    names (long: hipCUB's templates) listed once and referred to by index."""
    A, B = json.load(open(a))["calls"], json.load(open(b))["calls"]
    bad = [(x["form"], x["kernel"], x["screen"]) for x, y in zip(A, B) if x != y]
    print("%d calls, %d differ %s" % (len(A), len(bad), bad))
    if out:
        names = sorted({k for c in A + B for k in c["kernels"]})
        index = {k: i for i, k in enumerate(names)}
        both = [{"form": x["form"], "kernel": x["kernel"], "screen": x["screen"], "equal": x == y,
                 **{side: dict({f: c[f] for f in COUNTED}, kernels=[index[k] for k in c["kernels"]])
                    for side, c in (("parent", x), ("branch", y))}} for x, y in zip(A, B)]
        json.dump({"what": __doc__.split("\n\n")[0].replace("\n", " "), "shape": "rows [3, 38) of 41 x 97, s = 64; "
                   "block rows 5 (scratch rectangle) and 7 (screen)", "calls_differing": len(bad),
                   "kernel_names": names, "calls": both}, open(out, "w"), indent=None, separators=(",", ":"))
    return 1 if bad or len(A) != len(B) else 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "run":
        run()
    elif mode == "summarize" and len(sys.argv) == 4:
        summarize(sys.argv[2], sys.argv[3])
    elif mode == "compare" and len(sys.argv) in (4, 5):
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
