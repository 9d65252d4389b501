#!/usr/bin/env python3
"""The rectangle's two-set shared-hash screen (rect_screen.hip) against the
unscreened RECT kernels on the same build, in one process.  Writes
profiles/rect_screen.json, keyed on drephip_build_id.

  python tools/rect_screen_bench.py                          # every shape below
  python tools/rect_screen_bench.py --shapes 256x100000x1000 # Q x N x s [x L [x fam]]

Synthetic genome families as tools/rect_bench.py makes them (seed 0xD2E9,
5 Mbp genomes in families of 100), sketched on the device; the queries are
every (N + Q) / Q-th genome, so each has relatives among the references.  The
dense shape is one family: 2000 queries against 10^4 of their own relatives.
Per shape: one warm-up of each route, then `--repeats` interleaved repeats of
drephip_dist_rect_device with the screen forced and with it off -- the call's
wall time, the kernel and its table build (drephip_last_kernel_ms 2 / 3) and the
screen's phases (drephip_last_rect_screen_ms) -- then one call under AUTO with
the shipped floors (does it engage, does the verdict decline).  The two routes'
rectangles are compared cell for cell.

Bars: (i) where AUTO engages and screens, the forced call's median is no worse
than the unscreened median plus the unscreened min-max spread; (ii) at
Q = 10^4 x N = 10^5 the forced call's slowest run beats the unscreened fastest.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "256x100000x1000,1000x100000x1000,10000x100000x1000,1000x10000x10000,2000x10000x1000x5000000x12000"


def sketches(ctx, torch, np, _lib, M, s, L, fam, seed, chunk, stream, dev):
    tile, P = _lib.tile_bases(), _lib.padded_bases([L])
    CH = min(M, chunk)
    codes = torch.zeros((tile + CH * P) // 16, dtype=torch.int32, device=dev)
    valid = torch.zeros((tile + CH * P) // 32, dtype=torch.int32, device=dev)
    hh = torch.full((M, s), -1, dtype=torch.int64, device=dev)
    nn = torch.zeros(M, dtype=torch.int32, device=dev)
    for g0 in range(0, M, CH):
        n = min(CH, M - g0)
        ctx.synth_device(seed, g0, n, fam, L, codes.data_ptr(), valid.data_ptr(), stream)
        ctx.sketch_device(codes.data_ptr(), valid.data_ptr(), np.array([tile + i * P for i in range(n)], np.uint64),
                          np.full(n, P, np.uint64), np.full(n, L - 20, np.uint64), n, hh[g0].data_ptr(),
                          nn[g0:].data_ptr(), stream)
    torch.cuda.synchronize()
    return hh, nn


def one_shape(Q, N, s, L, fam, a, torch, np, _lib):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    M = Q + N
    rec = {"queries": Q, "references": N, "sketch": s, "genome_bp": L, "family_size": fam}
    with _lib.Context(device=0, k=21, s=s, seed=42) as ctx:
        t0 = time.perf_counter()
        hh, nn = sketches(ctx, torch, np, _lib, M, s, L, fam, 0xD2E9, a.chunk, stream, dev)
        rec["sketch_s"] = time.perf_counter() - t0
        qsel = torch.zeros(M, dtype=torch.bool, device=dev)
        qsel[torch.arange(Q, device=dev) * (M // Q)] = True
        d_qh, d_qn = hh[qsel].contiguous(), nn[qsel].contiguous()
        d_rh, d_rn = hh[~qsel].contiguous(), nn[~qsel].contiguous()
        del hh, nn
        torch.cuda.empty_cache()
        out = {m: (torch.zeros((Q, N), dtype=torch.int16, device=dev), torch.zeros((Q, N), dtype=torch.int16, device=dev))
               for m in ("force", "off")}
        ctx.set_timing(True, kernels=(2, 3, 4))
        modes = {"force": ctx.RECT_SCREEN_FORCE, "off": ctx.RECT_SCREEN_OFF, "auto": ctx.RECT_SCREEN_AUTO}

        def call(mode):
            ctx.set_rect_screen(modes[mode])
            c, d = out["off" if mode == "off" else "force"]
            torch.cuda.synchronize()
            t = time.perf_counter()
            ctx.dist_rect_device(d_qh.data_ptr(), d_qn.data_ptr(), Q, d_rh.data_ptr(), d_rn.data_ptr(), N, 0, Q,
                                 c.data_ptr(), d.data_ptr(), stream)
            r = {"call_ms": (time.perf_counter() - t) * 1e3, "kernel_ms": ctx.kernel_ms(2)[0],
                 "build_ms": ctx.kernel_ms(3)[0]}
            if mode != "off":
                r["screen_ms"] = ctx.kernel_ms(4)[0]
                r["phases_ms"] = ctx.last_rect_screen_ms()
                r["stats"] = ctx.last_rect_screen_stats()
            return r

        call("force")
        call("off")
        rec["cells_equal"] = bool(torch.equal(out["force"][0], out["off"][0]) and
                                  torch.equal(out["force"][1], out["off"][1]))
        runs = []
        for _ in range(a.repeats):
            runs.append({"force": call("force"), "off": call("off")})
        auto = call("auto")
        rec["cells_equal"] = rec["cells_equal"] and bool(torch.equal(out["force"][0], out["off"][0]) and
                                                         torch.equal(out["force"][1], out["off"][1]))
    f = [r["force"]["call_ms"] for r in runs]
    o = [r["off"]["call_ms"] for r in runs]
    st = runs[-1]["force"]["stats"]
    rec.update(runs=runs, auto=auto, marked=st["marked"], blocks=st["blocks"], checks_auto=auto["stats"]["checks"],
               forced_call_ms={"median": statistics.median(f), "min": min(f), "max": max(f)},
               off_call_ms={"median": statistics.median(o), "min": min(o), "max": max(o)},
               forced_phases_ms_median={k: statistics.median(r["force"]["phases_ms"][k] for r in runs)
                                        for k in runs[0]["force"]["phases_ms"]},
               forced_kernel_ms_median=statistics.median(r["force"]["kernel_ms"] for r in runs),
               off_kernel_ms_median=statistics.median(r["off"]["kernel_ms"] for r in runs),
               auto_engages=bool(auto["stats"]["blocks"] > 0), auto_screens=bool(auto["stats"]["used"]),
               auto_dense_blocks=auto["stats"]["dense_blocks"])
    rec["bar_i_met"] = bool(statistics.median(f) <= statistics.median(o) + (max(o) - min(o)))
    rec["bar_ii_slowest_forced_beats_fastest_off"] = bool(max(f) < min(o))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma list of QxNxs[xL[xfam]] (L 5000000, fam 100)")
    ap.add_argument("--chunk", type=int, default=10000, help="genomes sketched per chunk")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_screen.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from drep_amd import _lib

    res = {"build_id": _lib.lib().drephip_build_id().decode(), "device": torch.cuda.get_device_name(0),
           "seed": 0xD2E9, "repeats": a.repeats, "shapes": [],
           "bar_i": "where AUTO screens: forced median <= off median + off (max - min), call wall time",
           "bar_ii": "Q = 10^4 x N = 10^5: forced max < off min",
           "not_measured": ["Q = 10^4 x N = 10^6 (200 kbp genomes)", "several GPUs"]}
    if os.path.exists(a.out):                            # shapes measured by an earlier run of the same build are kept
        old = json.load(open(a.out))
        if old.get("build_id") == res["build_id"]:
            res["shapes"] = old.get("shapes", [])
    for spec in a.shapes.split(","):
        v = [int(x) for x in spec.split("x")]
        Q, N, s = v[:3]
        L = v[3] if len(v) > 3 else 5_000_000
        fam = v[4] if len(v) > 4 else 100
        rec = one_shape(Q, N, s, L, fam, a, torch, np, _lib)
        res["shapes"] = [x for x in res["shapes"] if (x["queries"], x["references"], x["sketch"], x["family_size"]) !=
                         (Q, N, s, fam)] + [rec]
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)         # after every shape: a cut run keeps what it measured
        print(json.dumps({k: v for k, v in rec.items() if k not in ("runs", "auto")}), flush=True)
    return 0 if all(x["cells_equal"] for x in res["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
