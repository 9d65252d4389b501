"""FASTA ingest + sketch of drephip_sketch_files, and the whole drop-in
all_vs_all_MASH, on the reference's test genomes replicated into many files
(plain and gzip).  Reports the host ingest time (read + pack, producer
thread) next to the device time and the wall time of the overlapped pipeline
(the plain set twice: the first call also pins its two batch buffers).
Not part of the product.

usage: python tools/ingest_bench.py [copies_per_genome] > profiles/<round>_ingest.json
       python tools/ingest_bench.py [copies_per_genome] --ingest both > profiles/ingest_device.json
       python tools/ingest_bench.py [copies_per_genome] --ingest host|device

--ingest both: the host and the device ingest path (Context.set_ingest_path)
on the same plain files in this process, interleaved, `--runs` each after one
warm-up each; then the pack kernels alone on one batch of text already in
device memory (Context.fasta_pack_device between two HIP events).
--ingest host / device: the timed runs of that one path only (for a same-box
comparison against another library through DREPHIP_LIB).
"""
import glob
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drep_amd import _lib, d_cluster  # noqa: E402

import argparse  # noqa: E402
_ap = argparse.ArgumentParser()
_ap.add_argument("copies", nargs="?", type=int, default=125)
_ap.add_argument("--ingest", choices=["host", "device", "both"], default=None)
_ap.add_argument("--runs", type=int, default=3)
_ap.add_argument("--pack-bases", type=int, default=1 << 30, help="text bytes of the pack-kernel timing batch")
_args = _ap.parse_args()
copies = _args.copies


def ingest_legs(ctx, plain, threads, legs, runs):
    """Interleaved timed sketch_files runs per ingest path (one warm-up each)."""
    res = {leg: [] for leg in legs}
    ref = None
    has_paths = hasattr(_lib.lib(), "drephip_set_ingest_path")          # not in an older library (DREPHIP_LIB)
    for it in range(runs + 1):
        for leg in legs:
            if has_paths:
                ctx.set_ingest_path(leg)
            t0 = time.perf_counter()
            h, nh, ln = ctx.sketch_files(plain, threads=threads)
            dt = time.perf_counter() - t0
            if ref is None:
                ref = (h, nh, ln)
            same = bool((h == ref[0]).all() and (nh == ref[1]).all() and (ln == ref[2]).all())
            if it == 0:
                continue                                                   # warm-up: buffers pinned, scratch grown
            st = ctx.ingest_stats()
            paths = ctx.ingest_paths() if has_paths else {}
            bases = int(ln.sum())
            res[leg].append({"wall_s": dt, "Mbp_per_s": bases / dt / 1e6, "produce_s": st["produce_s"],
                             "gpu_s": st["gpu_s"], "read_thread_s": st["read_thread_s"],
                             "pack_thread_s": st["pack_thread_s"], "batches": st["batches"],
                             "text_bytes": paths.get("text_bytes", 0), "device_files": paths.get("device_files", 0),
                             "host_files": paths.get("host_files", len(plain)), "bases": bases,
                             "identical_to_first_run": same})
    return res


def summarise(runs, pack):
    """Ranges over the timed runs of each path, their wall-time ratio and the copy rates."""
    def rng(xs):
        return [round(min(xs), 4), round(max(xs), 4)]
    out = {}
    for leg, rs in runs.items():
        out[leg] = {k + "_range": rng([r[k] for r in rs])
                    for k in ("wall_s", "produce_s", "gpu_s", "read_thread_s", "pack_thread_s")}
        out[leg]["Gbp_per_s_range"] = rng([r["Mbp_per_s"] / 1e3 for r in rs])
    h, d = [r["wall_s"] for r in runs["host"]], [r["wall_s"] for r in runs["device"]]
    out["device_over_host_speed"] = rng([min(h) / max(d), max(h) / min(d)])
    c = pack["h2d_from_pinned"]
    out["h2d_GB_per_s"] = {"text": round(c["text_bytes"] / (sum(c["text_ms"]) / len(c["text_ms"])) / 1e6, 1),
                           "packed": round(c["packed_bytes"] / (sum(c["packed_ms"]) / len(c["packed_ms"])) / 1e6, 1)}
    return out


def pack_kernel_leg(ctx, plain, want_bytes):
    """The pack call alone on ~want_bytes of text resident in device memory."""
    import numpy as np
    import torch
    sizes, files = [], []
    total = 0
    while total < want_bytes:
        for p in plain:
            sizes.append(os.path.getsize(p))
            files.append(p)
            total += sizes[-1]
            if total >= want_bytes:
                break
    starts, off = _lib.text_layout(sizes)
    host = np.zeros(int(off[-1]) + 16, np.uint8)
    cache = {}
    for p, st in zip(files, starts):
        if p not in cache:
            cache[p] = np.fromfile(p, np.uint8)
        host[int(st):int(st) + len(cache[p])] = cache[p]
    # the copy the device path pays for: this text from pinned memory, against
    # the packed form (3 bits per base) the host path copies
    pinned = torch.from_numpy(host).pin_memory()
    text = torch.empty(len(host), dtype=torch.uint8, device="cuda")
    h2d = {"text_ms": [], "packed_ms": []}
    packed_bytes = len(host) * 3 // 8
    for it in range(4):
        for name, nbytes in (("text_ms", len(host)), ("packed_ms", packed_bytes)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            text[:nbytes].copy_(pinned[:nbytes], non_blocking=True)
            e1.record()
            e1.synchronize()
            if it:
                h2d[name].append(e0.elapsed_time(e1))
    h2d["text_bytes"], h2d["packed_bytes"] = len(host), packed_bytes
    text.copy_(pinned)
    cap = np.array([_lib.padded_bases([sz]) for sz in sizes], np.uint64)
    tile = _lib.tile_bases()
    base = tile + np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
    end = int(tile + cap.sum())
    codes = torch.empty(end // 16, dtype=torch.int32, device="cuda")
    valid = torch.empty(end // 32, dtype=torch.int32, device="cuda")
    runs = []
    for it in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = ctx.fasta_pack_device(text, off, base, cap, codes, valid, stream=0)
        e1.record()
        e1.synchronize()
        if it:
            runs.append(e0.elapsed_time(e1))
    assert not r["status"].any()
    return {"files": len(files), "text_bytes": int(sum(sizes)), "bases": int(r["length"].sum()),
            "call_ms": runs, "h2d_from_pinned": h2d, "note": "HIP events on the call's stream around drephip_fasta_pack_device: region "
                                     "zeroing, the four kernels, the per-file readback (text already resident)"}


threads = int(os.environ.get("OMP_NUM_THREADS", "16") or 16)
src = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "genomes", "*.gz")))
out = {"source": "tests/golden/genomes (4 reference FASTAs) x %d copies each" % copies, "threads": threads}
with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as td:
    plain, gz = [], []
    for i, f in enumerate(src):
        txt = gzip.open(f).read()
        for c in range(copies):
            p = os.path.join(td, "c%04d_%s" % (c, os.path.basename(f)[:-3]))
            open(p, "wb").write(txt)
            plain.append(p)
        q = os.path.join(td, "z_" + os.path.basename(f))
        shutil.copy(f, q)
        gz.extend([q] * max(1, copies // 4))
    out["files_plain"] = len(plain)
    out["fasta_bytes"] = sum(os.path.getsize(p) for p in plain)
    if _args.ingest:
        out["build_id"] = _lib.build_id()
        out["library"] = os.path.relpath(_lib.LIB_PATH, ROOT)
        legs = ["host", "device"] if _args.ingest == "both" else [_args.ingest]
        with _lib.Context(0, 21, 1000, 42) as ctx:
            out["runs"] = ingest_legs(ctx, plain, threads, legs, _args.runs)
            if _args.ingest == "both":
                out["pack_kernels"] = pack_kernel_leg(ctx, plain, _args.pack_bases)
                out["summary"] = summarise(out["runs"], out["pack_kernels"])
        print(json.dumps(out, indent=1))
        sys.exit(0)
    with _lib.Context(0, 21, 1000, 42) as ctx:
        ctx.sketch_files(plain[:2], threads=threads)                       # warm-up
        for name, files in (("plain_first_call", plain), ("plain", plain), ("gzip", gz)):
            t0 = time.perf_counter()
            h, nh, ln = ctx.sketch_files(files, threads=threads)
            dt = time.perf_counter() - t0
            st = ctx.ingest_stats()
            bases = int(ln.sum())
            out[name] = {"files": len(files), "bases": bases, "wall_s": dt, "Mbp_per_s": bases / dt / 1e6,
                         "library_wall_s": st["wall_s"],
                         "host_read_pack_s": st["produce_s"], "device_s": st["gpu_s"], "batches": st["batches"],
                         "read_parse_thread_s": st["read_thread_s"], "pack_thread_s": st["pack_thread_s"],
                         "overflow_genomes": st["overflow_genomes"],
                         "ingest_only_Mbp_per_s": bases / st["produce_s"] / 1e6,
                         "overlap_note": "wall ~ host read+pack of every batch + the last batch's device work "
                                         "(the other batches' device work runs behind the next batch's ingest)"}
    # the whole drop-in on the plain files: sketch (ingest overlapped) + all-pairs + Mdb
    Bdb = pd.DataFrame({"genome": [os.path.basename(p) for p in plain], "location": plain})
    wd = os.path.join(td, "wd")
    t0 = time.perf_counter()
    Mdb = d_cluster.all_vs_all_MASH(Bdb, wd, processors=threads)
    out["dropin_all_vs_all_MASH"] = {"genomes": len(plain), "wall_s": time.perf_counter() - t0, "mdb_rows": len(Mdb),
                                     "note": "sketch files (+ .msh writing) + HIP all-pairs + float32 Mdb build"}
print(json.dumps(out, indent=1))
