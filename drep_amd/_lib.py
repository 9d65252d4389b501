"""ctypes binding of libdrephip.so (include/drephip.h).

There is no fallback: if the HIP library is missing or cannot be loaded, every
entry point raises :class:`DrepHipError`.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C drep_amd/csrc``.

The library is linked against the HIP runtime (libamdhip64.so.7).  PyTorch-ROCm
ships its own copy; to keep exactly one HIP runtime in a process that may also
import torch (bench.py, the multi-GPU path), the torch copy is preloaded with
RTLD_GLOBAL before libdrephip.so when torch is installed, so both bind to it.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys
import threading
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DREPHIP_LIB", os.path.join(_HERE, "lib", "libdrephip.so"))

ERR = {0: "OK", -1: "invalid argument", -2: "HIP error", -3: "I/O error", -4: "out of memory",
       -5: "unsupported", -6: "internal error"}


class DrepHipError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()

u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
u16p = np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
vp = C.c_void_p

# name -> (restype, argtypes); every symbol declared in include/drephip.h
SIGNATURES = {
    "drephip_version": (C.c_int, []),
    "drephip_build_id": (C.c_char_p, []),
    "drephip_last_error": (C.c_char_p, []),
    "drephip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "drephip_create": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "drephip_destroy": (C.c_int, [vp]),
    "drephip_max_sketch": (C.c_uint32, []),
    "drephip_tile_bases": (C.c_uint64, []),
    "drephip_padded_bases": (C.c_uint64, [u64p, C.c_uint32]),
    "drephip_fasta_info": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "drephip_fasta_pack": (C.c_int, [C.c_char_p, C.c_int, u32p, u32p, C.c_uint64, C.c_uint64,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "drephip_sketch": (C.c_int, [vp, u8p, u64p, C.c_uint32, u64p, C.c_uint32, u64p, u32p, u64p]),
    "drephip_sketch_files": (C.c_int, [vp, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, u64p, u32p, u64p]),
    "drephip_last_ingest_stats": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "drephip_last_ingest_phases": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_uint32)]),
    "drephip_text_tile_bytes": (C.c_uint32, []),
    "drephip_fasta_pack_device": (C.c_int, [vp, vp, u64p, C.c_uint32, u64p, u64p, vp, vp, vp, vp, vp, vp, vp, vp]),
    "drephip_set_ingest_path": (C.c_int, [vp, C.c_int]),
    "drephip_get_ingest_path": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "drephip_last_ingest_paths": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint64)]),
    "drephip_sketch_device": (C.c_int, [vp, vp, vp, u64p, u64p, u64p, C.c_uint32, vp, vp, vp]),
    "drephip_sketch_device_async": (C.c_int, [vp, vp, vp, u64p, u64p, u64p, C.c_uint32, vp, vp, vp]),
    "drephip_sketch_wait": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "drephip_synth_device": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                       vp, vp, vp]),
    "drephip_prefilter_eval": (C.c_int, [u64p, u64p, C.c_uint64, C.c_uint64, u8p, u8p]),
    "drephip_canon_eval": (C.c_int, [u32p, C.c_uint64, C.c_uint32, u32p, u32p]),
    "drephip_allpairs": (C.c_int, [vp, u64p, u32p, C.c_uint32, u16p, vp]),
    "drephip_allpairs_rows": (C.c_int, [vp, u64p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]),
    "drephip_allpairs_device": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
    "drephip_allpairs_device_async": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
    "drephip_allpairs_wait": (C.c_int, [vp]),
    "drephip_screen_geometry": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
    "drephip_screen_part": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp]),
    "drephip_screen_part_copy": (C.c_int, [vp, vp, vp, vp]),
    "drephip_screen_worth": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "drephip_allpairs_device_marked": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp,
                                                 C.c_uint64, vp, C.c_uint64, vp]),
    "drephip_allpairs_merge_device": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
    "drephip_allpairs_sparse_device": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64,
                                                 C.POINTER(C.c_uint64), vp]),
    "drephip_allpairs_sparse_device_marked": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64,
                                                        vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]),
    "drephip_allpairs_sparse": (C.c_int, [vp, u64p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64,
                                          C.POINTER(C.c_uint64)]),
    "drephip_dist_rect_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                           vp, vp, vp]),
    "drephip_dist_rect_merge_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 vp, vp, vp]),
    "drephip_dist_rect": (C.c_int, [vp, u64p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                    vp, vp]),
    "drephip_dist_rect_sparse_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  vp, C.c_uint64, C.POINTER(C.c_uint64), vp]),
    "drephip_dist_rect_sparse": (C.c_int, [vp, u64p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, C.c_uint32,
                                           C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "drephip_dist_rect_top_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.c_uint32, vp, vp, vp]),
    "drephip_dist_rect_top": (C.c_int, [vp, u64p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_uint32, vp, vp]),
    "drephip_pvalue_eval": (C.c_int, [C.c_int, C.c_uint32, u32p, u64p, u64p, C.c_uint64, f64p, vp, vp]),
    "drephip_pvalue_records_device": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, vp, vp]),
    "drephip_pvalue_records": (C.c_int, [vp, vp, C.c_uint64, u64p, C.c_uint32, u64p, C.c_uint32, vp]),
    "drephip_pvalue_hits_device": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp]),
    "drephip_records_filter_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_double, vp, vp, vp,
                                                C.POINTER(C.c_uint64), vp]),
    "drephip_allpairs_sparse_sig": (C.c_int, [vp, u64p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.c_double,
                                              vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "drephip_dist_rect_sparse_sig": (C.c_int, [vp, u64p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, C.c_uint32,
                                               C.c_uint32, u64p, u64p, C.c_double, vp, vp, C.c_uint64, vp,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "drephip_write_mash_table_rect": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p),
                                                C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_int]),
    "drephip_last_sparse_stats": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]),
    "drephip_distance_lut": (C.c_int, [C.c_int, C.c_uint32, f64p]),
    "drephip_write_mash_table": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, vp, vp, C.c_uint32,
                                           vp, vp, u16p, f64p, C.c_int]),
    "drephip_set_allpairs_path": (C.c_int, [vp, C.c_int, C.c_uint32]),
    "drephip_set_rect_band": (C.c_int, [vp, C.c_int, C.c_uint32]),
    "drephip_last_rect_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "drephip_set_rect_screen": (C.c_int, [vp, C.c_int]),
    "drephip_last_rect_screen_stats": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint32)]),
    "drephip_last_rect_screen_ms": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "drephip_rect_screen_mode_of": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "drephip_linkage": (C.c_int, [vp, f64p, C.c_uint32, C.c_int, f64p]),
    "drephip_linkage_counts_device": (C.c_int, [vp, vp, vp, C.c_uint32, u32p, f64p, C.c_uint32,
                                                np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS"),
                                                C.c_int, f64p, vp]),
    "drephip_linkage_square": (C.c_int, [vp, np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS"),
                                         C.c_uint32, C.c_int, f64p]),
    "drephip_mdb_square": (C.c_int, [C.c_uint32, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_int, vp, vp, vp,
                                     vp, C.c_int]),
    "drephip_pivot_scan": (C.c_int, [C.c_uint64, vp, vp, C.c_int, C.c_uint32, u8p, u8p, C.POINTER(C.c_uint64),
                                     C.c_int]),
    "drephip_pivot_fill": (C.c_int, [C.c_uint64, vp, vp, C.c_int, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32,
                                     C.c_uint64, vp, C.c_int]),
    "drephip_linkage_reserve": (C.c_int, [vp, C.c_uint32]),
    "drephip_set_linkage_path": (C.c_int, [vp, C.c_int]),
    "drephip_linkage_sparse": (C.c_int, [C.c_uint32, C.c_uint64, u32p, u32p, f64p, C.c_int, f64p]),
    "drephip_last_linkage_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint32)]),
    "drephip_last_linkage_stats": (C.c_int, [vp] + [C.POINTER(C.c_double)] * 5),
    "drephip_last_linkage_launches": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "drephip_set_timing": (C.c_int, [vp, C.c_int]),
    "drephip_last_kernel_ms": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "drephip_set_allpairs_screen": (C.c_int, [vp, C.c_int]),
    "drephip_last_screen_stats": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
}


def _preload_torch_hip_runtime() -> None:
    if "torch" in sys.modules:
        return  # torch already put its runtime in the process
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for root in spec.submodule_search_locations:
        cand = os.path.join(root, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def lib():
    """Load libdrephip.so (once).  Raises DrepHipError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise DrepHipError(
                "libdrephip.so not found at %s -- build it (make -C drep_amd/csrc); "
                "drep_amd has no CPU fallback" % LIB_PATH)
        _preload_torch_hip_runtime()
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:
            raise DrepHipError("cannot load %s: %s" % (LIB_PATH, e)) from e
        for name, (res, args) in SIGNATURES.items():
            # an older build loaded for a same-box A/B (DREPHIP_LIB) may lack
            # entry points added since; the product library has them all
            # (tests/test_host.py checks the export list)
            if "DREPHIP_LIB" in os.environ and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
        return L


def source_digest(root: Optional[str] = None) -> str:
    """sha256 of the library's sources as drep_amd/csrc/Makefile computes it
    for drephip_build_id: the `sha256sum` listing of include/drephip.h and the
    sorted drep_amd/csrc/*.{cpp,h,hip} + Makefile, hashed again."""
    import glob
    import hashlib
    root = root or os.path.dirname(_HERE)
    csrc = os.path.join(root, "drep_amd", "csrc")
    names = sorted([os.path.basename(p) for ext in ("*.hip", "*.cpp", "*.h")
                    for p in glob.glob(os.path.join(csrc, ext))] + ["Makefile"])
    files = ["include/drephip.h"] + ["drep_amd/csrc/" + n for n in names]
    listing = "".join("%s  %s\n" % (hashlib.sha256(open(os.path.join(root, f), "rb").read()).hexdigest(), f)
                      for f in files)
    return hashlib.sha256(listing.encode()).hexdigest()


def build_id() -> dict:
    """The loaded library's build identity (drephip_build_id) as a dict."""
    raw = lib().drephip_build_id().decode()
    return dict(kv.split("=", 1) for kv in raw.split(";") if "=" in kv)


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().drephip_last_error().decode("utf-8", "replace")
        raise DrepHipError("%s failed (%s): %s" % (what, ERR.get(rc, rc), msg))


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().drephip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def max_sketch() -> int:
    """Largest supported sketch size s."""
    return int(lib().drephip_max_sketch())


def tile_bases() -> int:
    return int(lib().drephip_tile_bases())


def text_tile_bytes() -> int:
    """Bytes of FASTA text per tile of the device ingest kernels (a power of two)."""
    return int(lib().drephip_text_tile_bytes())


def text_layout(sizes: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """Where files of the given byte sizes go in a device text buffer for
    Context.fasta_pack_device: (starts, text_off).  File f is written at
    starts[f] (16-byte aligned); text_off (n + 1 entries) is what the call
    takes: file f ends at text_off[f + 1] and the next one starts at the
    16-byte boundary at or after it.  The buffer holds text_off[-1] bytes."""
    starts = np.zeros(len(sizes), np.uint64)
    off = np.zeros(len(sizes) + 1, np.uint64)
    at = 0
    for f, sz in enumerate(sizes):
        at = (at + 15) // 16 * 16
        starts[f] = at
        at += int(sz)
        off[f + 1] = at
    return starts, off


INGEST_PATHS = {"host": 0, "device": 1}


def padded_bases(rec_len: Sequence[int]) -> int:
    a = np.ascontiguousarray(rec_len, dtype=np.uint64)
    return int(lib().drephip_padded_bases(a if len(a) else np.zeros(1, np.uint64), len(a)))


def distance_lut(denom: int, k: int = 21) -> np.ndarray:
    out = np.zeros(denom + 1, dtype=np.float64)
    check(lib().drephip_distance_lut(k, denom, out), "drephip_distance_lut")
    return out


def prefilter_eval(q1: np.ndarray, q2: np.ndarray, T: int) -> Tuple[np.ndarray, np.ndarray]:
    """drephip_prefilter_eval (host): (pass, exact) bits of the sketch kernel's
    reject-early test and of h1 <= T for the fmix64 state pairs (q1, q2)."""
    q1 = np.ascontiguousarray(q1, dtype=np.uint64)
    q2 = np.ascontiguousarray(q2, dtype=np.uint64)
    if q1.shape != q2.shape or q1.ndim != 1:
        raise ValueError("q1 and q2 must be equal-length vectors")
    n = len(q1)
    ok = np.zeros(max(n, 1), np.uint8)
    exact = np.zeros(max(n, 1), np.uint8)
    z = np.zeros(1, np.uint64)
    check(lib().drephip_prefilter_eval(q1 if n else z, q2 if n else z, n, int(T), ok, exact),
          "drephip_prefilter_eval")
    return ok[:n].astype(bool), exact[:n].astype(bool)


def canon_eval(words: np.ndarray, r: int) -> Tuple[np.ndarray, np.ndarray]:
    """drephip_canon_eval (host): (high word, tail index) of the canonical 21-mer
    ending at base 32 + r of each row of words (n x 3 code words).  The tail is
    the natural index (base 16 on top): the kernel's table index -- the other
    strand's bases 0-4 -- mapped back by the function the table is stored by."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    if words.ndim != 2 or words.shape[1] != 3:
        raise ValueError("words must be n x 3")
    n = len(words)
    hi = np.zeros(max(n, 1), np.uint32)
    tail = np.zeros(max(n, 1), np.uint32)
    check(lib().drephip_canon_eval(words if n else np.zeros((1, 3), np.uint32), n, int(r), hi, tail),
          "drephip_canon_eval")
    return hi[:n], tail[:n]


def write_mash_table(path: str, names: Sequence[str], common: np.ndarray, denom: Optional[np.ndarray], s: int,
                     dist: np.ndarray, pval: np.ndarray, self_count: np.ndarray, self_pval: np.ndarray,
                     threads: int = 0) -> None:
    """drephip_write_mash_table: condensed arrays (i < j), names of the N genomes."""
    N = len(names)
    npairs = N * (N - 1) // 2
    common = np.ascontiguousarray(common, dtype=np.uint16)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    pval = np.ascontiguousarray(pval, dtype=np.float64)
    for a in (common, dist, pval) + ((denom,) if denom is not None else ()):
        if len(a) != npairs:
            raise ValueError("condensed arrays must hold N(N-1)/2 = %d entries" % npairs)
    den = None if denom is None else np.ascontiguousarray(denom, dtype=np.uint16)
    arr = (C.c_char_p * max(N, 1))(*[os.fsencode(n) for n in names])
    check(lib().drephip_write_mash_table(os.fsencode(path), arr, N, common.ctypes.data,
                                         None if den is None else den.ctypes.data, int(s), dist.ctypes.data,
                                         pval.ctypes.data, np.ascontiguousarray(self_count, dtype=np.uint16),
                                         np.ascontiguousarray(self_pval, dtype=np.float64), int(threads)),
          "drephip_write_mash_table(%s)" % path)


def write_mash_table_rect(path: str, rnames: Sequence[str], qnames: Sequence[str], common: np.ndarray,
                          denom: Optional[np.ndarray], s: int, dist: np.ndarray, pval: np.ndarray,
                          threads: int = 0) -> None:
    """drephip_write_mash_table_rect: the [Q, N] rectangle's arrays (row-major,
    query rows), names of the N references and the Q queries."""
    N, Q = len(rnames), len(qnames)
    common = np.ascontiguousarray(common, dtype=np.uint16)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    pval = np.ascontiguousarray(pval, dtype=np.float64)
    den = None if denom is None else np.ascontiguousarray(denom, dtype=np.uint16)
    for a in (common, dist, pval) + ((den,) if den is not None else ()):
        if a.size != Q * N:
            raise ValueError("rectangle arrays must hold Q x N = %d entries" % (Q * N))
    ra = (C.c_char_p * max(N, 1))(*[os.fsencode(n) for n in rnames])
    qa = (C.c_char_p * max(Q, 1))(*[os.fsencode(n) for n in qnames])
    check(lib().drephip_write_mash_table_rect(os.fsencode(path), ra, N, qa, Q, common.ctypes.data,
                                              None if den is None else den.ctypes.data, int(s), dist.ctypes.data,
                                              pval.ctypes.data, int(threads)),
          "drephip_write_mash_table_rect(%s)" % path)


def pvalue_eval(common: np.ndarray, len_a: np.ndarray, len_b: np.ndarray, s: int, k: int = 21,
                want_rn: bool = False):
    """drephip_pvalue_eval (host, no GPU): Mash's p-value of each (common,
    len_a, len_b) at sketch size s and k-mer size k, through the inline
    functions the kernels call (drep_amd/csrc/pvalue.h).  want_rn: also the
    binomial's r (float64) and n (uint32) of every pair."""
    common = np.ascontiguousarray(common, dtype=np.uint32)
    len_a = np.ascontiguousarray(len_a, dtype=np.uint64)
    len_b = np.ascontiguousarray(len_b, dtype=np.uint64)
    if not (common.ndim == 1 and common.shape == len_a.shape == len_b.shape):
        raise ValueError("common, len_a and len_b must be equal-length vectors")
    n = len(common)
    m = max(n, 1)
    p = np.zeros(m, np.float64)
    r = np.zeros(m, np.float64) if want_rn else None
    nn = np.zeros(m, np.uint32) if want_rn else None
    z32, z64 = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    check(lib().drephip_pvalue_eval(int(k), int(s), common if n else z32, len_a if n else z64, len_b if n else z64,
                                    n, p, _ptr(r), _ptr(nn)), "drephip_pvalue_eval")
    return (p[:n], r[:n], nn[:n]) if want_rn else p[:n]


def _records(records: np.ndarray) -> np.ndarray:
    records = np.ascontiguousarray(records, dtype=np.uint32)
    if records.ndim != 2 or records.shape[1] != 4:
        raise ValueError("records must be a uint32 [n, 4] array")
    return records


def _lengths(length, n: int) -> np.ndarray:
    length = np.ascontiguousarray(length, dtype=np.uint64)
    if length.shape != (n,):
        raise ValueError("lengths must hold one entry per sketch row (%d), got %s" % (n, length.shape))
    return length


def _sorted_sig(rec: np.ndarray, pv: np.ndarray):
    """Records and their p-values sorted by (first, second) index, as columns."""
    order = np.lexsort((rec[:, 1], rec[:, 0]))
    rec = rec[order]
    return (np.ascontiguousarray(rec[:, 0]), np.ascontiguousarray(rec[:, 1]), rec[:, 2].astype(np.uint16),
            rec[:, 3].astype(np.uint16), np.ascontiguousarray(pv[order]))


def fasta_info(path: str, k: int = 21):
    length = C.c_uint64(0)
    padded = C.c_uint64(0)
    nrec = C.c_uint32(0)
    nk = C.c_uint64(0)
    check(lib().drephip_fasta_info(path.encode(), k, C.byref(length), C.byref(padded), C.byref(nrec),
                                   C.byref(nk)), "drephip_fasta_info(%s)" % path)
    return {"length": length.value, "padded": padded.value, "n_records": nrec.value, "n_kmers": nk.value}


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def mdb_square(N: int, common: np.ndarray, denom: Optional[np.ndarray], s: int, lut32: np.ndarray,
               lut_off: np.ndarray, codes: np.ndarray, threads: int = 0, want_sim: bool = True):
    """drephip_mdb_square (host): the N^2-row Mdb columns from the condensed
    counts -- (g1 codes, g2 codes, dist, similarity) in all_vs_all_MASH's row
    order; codes' dtype (int8/16/32) is the category code width."""
    common = np.ascontiguousarray(common, dtype=np.uint16)
    den = None if denom is None else np.ascontiguousarray(denom, dtype=np.uint16)
    lut32 = np.ascontiguousarray(lut32, dtype=np.float32)
    lut_off = np.ascontiguousarray(lut_off, dtype=np.int32)
    codes = np.ascontiguousarray(codes)
    if codes.dtype not in (np.int8, np.int16, np.int32) or len(codes) != N or len(lut_off) != s + 1:
        raise ValueError("codes must be N int8/int16/int32 category codes and lut_off s+1 offsets")
    npairs = N * (N - 1) // 2
    if len(common) != npairs or (den is not None and len(den) != npairs):
        raise ValueError("condensed arrays must hold N(N-1)/2 = %d entries" % npairs)
    codes32 = codes.astype(np.int32)
    g1 = np.empty(N * N, dtype=codes.dtype)
    g2 = np.empty(N * N, dtype=codes.dtype)
    dist = np.empty(N * N, dtype=np.float32)
    sim = np.empty(N * N, dtype=np.float32) if want_sim else None
    check(lib().drephip_mdb_square(N, _ptr(common) if npairs else None, _ptr(den) if npairs else None, int(s),
                                   _ptr(lut32), len(lut32), _ptr(lut_off), _ptr(codes32), codes.dtype.itemsize,
                                   _ptr(g1), _ptr(g2), _ptr(dist), _ptr(sim), int(threads)), "drephip_mdb_square")
    return g1, g2, dist, sim


def pivot_scan(codes1: np.ndarray, codes2: np.ndarray, ncat: int, threads: int = 0):
    """drephip_pivot_scan: (present1, present2, period) of two category-code
    columns; raises DrepHipError(-5) on a missing (negative) code."""
    codes1 = np.ascontiguousarray(codes1)
    codes2 = np.ascontiguousarray(codes2)
    if codes1.dtype != codes2.dtype or codes1.dtype not in (np.int8, np.int16, np.int32) or len(codes1) != len(codes2):
        raise ValueError("codes1/codes2 must be equal-length int8/int16/int32 arrays")
    p1 = np.zeros(max(ncat, 1), np.uint8)
    p2 = np.zeros(max(ncat, 1), np.uint8)
    period = C.c_uint64(0)
    check(lib().drephip_pivot_scan(len(codes1), _ptr(codes1), _ptr(codes2), codes1.dtype.itemsize, int(ncat), p1, p2,
                                   C.byref(period), int(threads)), "drephip_pivot_scan")
    return p1[:ncat].astype(bool), p2[:ncat].astype(bool), int(period.value)


def pivot_fill(codes1: np.ndarray, codes2: np.ndarray, pos1: np.ndarray, pos2: np.ndarray, vals: np.ndarray,
               n1: int, n2: int, period: int = 0, threads: int = 0) -> np.ndarray:
    """drephip_pivot_fill: the n1 x n2 float32 pivot of `vals`; raises
    DrepHipError(-1, "Index contains duplicate entries...") like pandas."""
    codes1 = np.ascontiguousarray(codes1)
    codes2 = np.ascontiguousarray(codes2)
    pos1 = np.ascontiguousarray(pos1, dtype=np.int32)
    pos2 = np.ascontiguousarray(pos2, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    if not (len(codes1) == len(codes2) == len(vals)) or len(pos1) != len(pos2):
        raise ValueError("codes/vals lengths or pos lengths differ")
    out = np.empty((n1, n2), dtype=np.float32)
    check(lib().drephip_pivot_fill(len(vals), _ptr(codes1), _ptr(codes2), codes1.dtype.itemsize, _ptr(pos1), _ptr(pos2),
                                   len(pos1), _ptr(vals), int(n1), int(n2), int(period), _ptr(out), int(threads)),
          "drephip_pivot_fill")
    return out


# scipy linkage method codes (include/drephip.h DREPHIP_LINK_*): the methods
# with a sparse form (linkage_sparse), and those of the context's linkage
# calls -- ward runs on the dense path only
LINK_METHODS = {"single": 0, "complete": 1, "average": 2, "weighted": 6}
DENSE_LINK_METHODS = {**LINK_METHODS, "ward": 5}


def linkage_sparse(n: int, i: np.ndarray, j: np.ndarray, v: np.ndarray, method: str) -> np.ndarray:
    """drephip_linkage_sparse (host only, no GPU): scipy's linkage Z of the n x n
    distance matrix that holds v[t] at (i[t], j[t]) and 1.0 at every pair not
    listed (each unordered pair at most once, v in [0, 1))."""
    i = np.ascontiguousarray(i, dtype=np.uint32)
    j = np.ascontiguousarray(j, dtype=np.uint32)
    v = np.ascontiguousarray(v, dtype=np.float64)
    if not (len(i) == len(j) == len(v)):
        raise ValueError("i, j and v must have one entry per pair")
    Z = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
    if n >= 2:
        e = np.zeros(1, np.uint32)
        check(lib().drephip_linkage_sparse(int(n), len(v), i if len(i) else e, j if len(j) else e,
                                           v if len(v) else np.zeros(1), LINK_METHODS[method], Z.reshape(-1)),
              "drephip_linkage_sparse")
    return Z


def rect_arrays(qhashes, qnhash, rhashes, rnhash, s: int):
    """The two sketch matrices of a query-against-reference call, contiguous:
    hashes uint64 [rows, s], nhash uint32 [rows].  ValueError for any other
    dtype or shape (no conversion: a float or signed matrix is a caller's
    mistake, not a sketch); needs no library and no GPU."""
    out = []
    for side, h, n in (("query", qhashes, qnhash), ("reference", rhashes, rnhash)):
        h, n = np.asarray(h), np.asarray(n)
        if h.dtype != np.uint64 or n.dtype != np.uint32:
            raise ValueError("%s hashes / nhash must be uint64 / uint32, got %s / %s" % (side, h.dtype, n.dtype))
        if n.ndim != 1 or h.ndim != 2 or h.shape != (len(n), int(s)):
            raise ValueError("%s hashes must be [rows, s] = [%d, %d] with nhash [rows], got %s and %s"
                             % (side, len(n) if n.ndim == 1 else -1, int(s), h.shape, n.shape))
        out += [np.ascontiguousarray(h), np.ascontiguousarray(n)]
    return tuple(out)


def tri_arrays(hashes, nhash, s: int, length=None):
    """The sketch matrix of an all-pairs call, contiguous: hashes uint64 [N, s],
    nhash uint32 [N], and with `length` the genome lengths uint64 [N] of a
    _sig call.  Converts (unlike rect_arrays); ValueError for any other shape."""
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    nhash = np.ascontiguousarray(nhash, dtype=np.uint32)
    N = len(nhash)
    if length is None:
        if hashes.shape != (N, s):
            raise ValueError("hashes must be [N, s] = [%d, %d], got %s" % (N, s, hashes.shape))
        return hashes, nhash
    length = np.ascontiguousarray(length, dtype=np.uint64)
    if hashes.shape != (N, s) or length.shape != (N,):
        raise ValueError("hashes must be [N, s] and length [N]")
    return hashes, nhash, length


def _pairs_cap(pairs: Optional[np.ndarray]) -> int:
    """Records a caller's `pairs` buffer holds (None: 0, a count-only call)."""
    if pairs is None:
        return 0
    if pairs.dtype != np.uint32 or not pairs.flags.c_contiguous or pairs.ndim != 2 or pairs.shape[1] != 4:
        raise ValueError("pairs must be a contiguous uint32 [cap, 4] array")
    return len(pairs)


ERR_NOMEM = -4


def _nomem_ok(rc: int, what: str) -> int:
    """A record call's return code: raises on every error but
    DREPHIP_ERR_NOMEM (the buffer is too small; n_pairs says by how much)."""
    if rc != ERR_NOMEM:
        check(rc, what)
    return rc


def _sorted_records(raw_call, what: str, cap: int):
    """The record calls' retry: raw_call(pairs or None) -> (rc, n) into a
    buffer of `cap` records, once more with the reported size when that was
    too small; the records sorted by their two indices, as columns."""
    buf = np.empty((max(cap, 1), 4), dtype=np.uint32)
    rc, n = raw_call(buf[:cap] if cap else None)
    if rc == ERR_NOMEM:
        buf = np.empty((n, 4), dtype=np.uint32)
        rc, n = raw_call(buf)
        check(rc, what)
    rec = buf[:n]
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
    return (np.ascontiguousarray(rec[:, 0]), np.ascontiguousarray(rec[:, 1]),
            rec[:, 2].astype(np.uint16), rec[:, 3].astype(np.uint16))


class Context:
    """One libdrephip context: a HIP device plus (k, s, seed)."""

    def __init__(self, device: int = 0, k: int = 21, s: int = 1000, seed: int = 42):
        L = lib()
        self.k, self.s, self.seed, self.device = int(k), int(s), int(seed), int(device)
        h = vp()
        check(L.drephip_create(self.device, self.k, self.s, self.seed, C.byref(h)), "drephip_create")
        self._h = h

    # -- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().drephip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    # all-pairs kernel selection (include/drephip.h DREPHIP_AP_*)
    AP_AUTO, AP_TABLE, AP_BAND, AP_MERGE = 0, 1, 2, 3

    SCREEN_AUTO, SCREEN_ON, SCREEN_OFF = 0, 1, 2

    def set_allpairs_screen(self, mode: int) -> None:
        """The shared-hash screen in front of the all-pairs kernels
        (include/drephip.h: auto / on / off)."""
        check(lib().drephip_set_allpairs_screen(self._h, mode), "drephip_set_allpairs_screen")
        self._screen_mode = mode

    @property
    def allpairs_screen(self) -> int:
        return getattr(self, "_screen_mode", self.SCREEN_AUTO)

    def screen_stats(self) -> dict:
        u = C.c_int(0)
        e, r, c, m, sp = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().drephip_last_screen_stats(self._h, C.byref(u), C.byref(e), C.byref(r), C.byref(c), C.byref(m),
                                              C.byref(sp)), "drephip_last_screen_stats")
        return {"used": bool(u.value), "entries": e.value, "runs": r.value, "checks": c.value, "marked": m.value,
                "simple": sp.value}

    def set_allpairs_path(self, path: int, band_cap: int = 1024) -> None:
        check(lib().drephip_set_allpairs_path(self._h, path, band_cap), "drephip_set_allpairs_path")

    # the rectangle's band kernel (include/drephip.h DREPHIP_RECT_BAND_*)
    RECT_BAND_AUTO, RECT_BAND_OFF, RECT_BAND_FORCE = 0, 1, 2

    def set_rect_band(self, mode: int, band_cap: int = 768) -> None:
        """Which kernel the query-against-reference calls take above the
        whole-row tables (auto: the band kernel; off: the literal merge;
        force: the band kernel at every s) and its elements per row per band."""
        check(lib().drephip_set_rect_band(self._h, int(mode), int(band_cap)), "drephip_set_rect_band")

    def last_rect_info(self) -> Tuple[int, int]:
        """(kernel, fallback) of the last rectangle call: AP_TABLE / AP_BAND /
        AP_MERGE, and 1 when rows were rerun by the merge kernel after an
        unbuildable band table."""
        k, f = C.c_int(0), C.c_int(0)
        check(lib().drephip_last_rect_info(self._h, C.byref(k), C.byref(f)), "drephip_last_rect_info")
        return k.value, f.value

    # the rectangle's two-set shared-hash screen (include/drephip.h DREPHIP_RECT_SCREEN_*)
    RECT_SCREEN_AUTO, RECT_SCREEN_OFF, RECT_SCREEN_FORCE = 0, 1, 2

    def set_rect_screen(self, mode: int) -> None:
        """The screen in front of the query-against-reference kernels: auto
        (from 4096 references and 2048 query rows on, unless its count pass
        finds the block too dense), off, or force (any size, no verdict)."""
        check(lib().drephip_set_rect_screen(self._h, int(mode)), "drephip_set_rect_screen")

    def last_rect_screen_stats(self) -> dict:
        """{used, blocks, query_entries, distinct, checks, marked, dense_blocks}
        of the last rectangle call's screen (zeros when it did not run)."""
        u, b, d = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        qe, di, ch, mk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().drephip_last_rect_screen_stats(self._h, C.byref(u), C.byref(b), C.byref(qe), C.byref(di),
                                                   C.byref(ch), C.byref(mk), C.byref(d)),
              "drephip_last_rect_screen_stats")
        return {"used": bool(u.value), "blocks": b.value, "query_entries": qe.value, "distinct": di.value,
                "checks": ch.value, "marked": mk.value, "dense_blocks": d.value}

    def last_rect_screen_ms(self) -> dict:
        """The screen's phase times (ms) of the last rectangle call, measured
        while set_timing covers kernel 4: sort, count, mark, lists, fill."""
        v = (C.c_double * 5)()
        check(lib().drephip_last_rect_screen_ms(self._h, v), "drephip_last_rect_screen_ms")
        return dict(zip(("sort", "count", "mark", "lists", "fill"), (float(x) for x in v)))

    LINK_METHODS = LINK_METHODS
    DENSE_LINK_METHODS = DENSE_LINK_METHODS
    # linkage path (include/drephip.h DREPHIP_LINK_PATH_*)
    LINK_AUTO, LINK_DENSE, LINK_SPARSE = 0, 1, 2

    def set_linkage_path(self, path: int) -> None:
        check(lib().drephip_set_linkage_path(self._h, int(path)), "drephip_set_linkage_path")

    def linkage_info(self):
        """{sparse, pairs, components, largest} of the last linkage call."""
        sp, npairs, nc, lg = C.c_int(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().drephip_last_linkage_info(self._h, C.byref(sp), C.byref(npairs), C.byref(nc), C.byref(lg)),
              "drephip_last_linkage_info")
        return {"sparse": bool(sp.value), "pairs": npairs.value, "components": nc.value, "largest": lg.value}

    def linkage(self, y: np.ndarray, method: str) -> np.ndarray:
        """scipy.cluster.hierarchy.linkage(y, method) on the GPU, bit-identical
        (y: condensed float64 distances).  method: single, complete, average,
        weighted, or ward (dense path only; a negative distance is refused)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        n = int(round((1 + (1 + 8 * len(y)) ** 0.5) / 2))
        if n * (n - 1) // 2 != len(y):
            raise ValueError("y is not a condensed distance vector")
        Z = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
        if n >= 2:
            check(lib().drephip_linkage(self._h, y, n, self.DENSE_LINK_METHODS[method], Z.reshape(-1)),
                  "drephip_linkage")
        return Z

    def linkage_square(self, M: np.ndarray, method: str) -> np.ndarray:
        """scipy.cluster.hierarchy.linkage(squareform(M), method) on the GPU,
        bit-identical, with squareform's and linkage's checks (DrepHipError
        carrying scipy's message when one fails); M: n x n float32."""
        M = np.ascontiguousarray(M, dtype=np.float32)
        if M.ndim != 2 or M.shape[0] != M.shape[1]:
            raise ValueError("M must be a square matrix")
        n = M.shape[0]
        Z = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
        if n >= 2:
            check(lib().drephip_linkage_square(self._h, M, n, self.DENSE_LINK_METHODS[method], Z.reshape(-1)),
                  "drephip_linkage_square")
        return Z

    def linkage_counts_device(self, d_common: int, d_denom: Optional[int], n: int, perm: np.ndarray,
                              lut: np.ndarray, lut_off: np.ndarray, method: str,
                              stream: Optional[int] = None) -> np.ndarray:
        """linkage() of the distances given by device-resident all-pairs counts
        (see drephip_linkage_counts_device); the counts are read after the work
        queued on `stream`."""
        Z = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
        if n >= 2:
            check(lib().drephip_linkage_counts_device(
                self._h, d_common, d_denom, n, np.ascontiguousarray(perm, dtype=np.uint32),
                np.ascontiguousarray(lut, dtype=np.float64), len(lut),
                np.ascontiguousarray(lut_off, dtype=np.int32), self.DENSE_LINK_METHODS[method], Z.reshape(-1), stream),
                "drephip_linkage_counts_device")
        return Z

    def linkage_reserve(self, n: int) -> None:
        """Allocate the n x n linkage matrix now (drephip_linkage_reserve)."""
        check(lib().drephip_linkage_reserve(self._h, int(n)), "drephip_linkage_reserve")

    def linkage_stats(self):
        """{alloc_s, matrix_s, chain_s, finish_s, wall_s} of the last linkage call."""
        v = [C.c_double(0) for _ in range(5)]
        check(lib().drephip_last_linkage_stats(self._h, *[C.byref(x) for x in v]), "drephip_last_linkage_stats")
        return dict(zip(("alloc_s", "matrix_s", "chain_s", "finish_s", "wall_s"), (x.value for x in v)))

    def linkage_launches(self) -> int:
        """Step launches of the last dense-chain linkage call."""
        v = C.c_uint64(0)
        check(lib().drephip_last_linkage_launches(self._h, C.byref(v)), "drephip_last_linkage_launches")
        return int(v.value)

    def set_timing(self, on: bool = True, kernels=None) -> None:
        """HIP-event timing of kernel launches: all kernels, or only the
        `which` indices in `kernels` (see kernel_ms)."""
        mask = 0 if not on else (-1 if kernels is None else sum(1 << int(w) for w in kernels))
        check(lib().drephip_set_timing(self._h, mask), "drephip_set_timing")

    def kernel_ms(self, which: int):
        ms = C.c_double(0)
        n = C.c_int(0)
        check(lib().drephip_last_kernel_ms(self._h, which, C.byref(ms), C.byref(n)), "drephip_last_kernel_ms")
        return ms.value, n.value

    # -- sketch
    def sketch_files(self, paths: Sequence[str], threads: int = 0):
        n = len(paths)
        hashes = np.zeros((n, self.s), dtype=np.uint64)
        nhash = np.zeros(n, dtype=np.uint32)
        length = np.zeros(n, dtype=np.uint64)
        if n == 0:
            return hashes, nhash, length
        arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
        check(lib().drephip_sketch_files(self._h, arr, n, int(threads), hashes.reshape(-1), nhash, length),
              "drephip_sketch_files")
        return hashes, nhash, length

    def set_ingest_path(self, path: str) -> None:
        """Who parses and packs the files of sketch_files: "host" (worker
        threads; the default) or "device" (kernels on the raw text)."""
        if path not in INGEST_PATHS:
            raise ValueError("ingest must be 'host' or 'device', got %r" % (path,))
        check(lib().drephip_set_ingest_path(self._h, INGEST_PATHS[path]), "drephip_set_ingest_path")

    @property
    def ingest_path(self) -> str:
        v = C.c_int(0)
        check(lib().drephip_get_ingest_path(self._h, C.byref(v)), "drephip_get_ingest_path")
        return {0: "host", 1: "device"}[v.value]

    def ingest_paths(self) -> dict:
        """{path, device_files, host_files, text_bytes}: the context's ingest
        path, and for the last sketch_files call the files the device packed,
        the files that took the host reader and the text bytes copied."""
        d, h, t = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        check(lib().drephip_last_ingest_paths(self._h, C.byref(d), C.byref(h), C.byref(t)),
              "drephip_last_ingest_paths")
        return {"path": self.ingest_path, "device_files": d.value, "host_files": h.value, "text_bytes": t.value}

    def fasta_pack_device(self, text, text_off, base_off, cap_bases, d_codes, d_valid,
                          stream: Optional[int] = None) -> dict:
        """drephip_fasta_pack_device: parse and pack FASTA text that is in
        device memory.  `text`: a torch.uint8 CUDA tensor or a device pointer;
        `text_off`: n + 1 offsets (see text_layout); `base_off` / `cap_bases`:
        each file's region in `d_codes` / `d_valid` (torch tensors or device
        pointers).  Returns numpy arrays {length, padded, n_records, n_kmers,
        status} (status 0 packed, 1 needs the host reader, 2 region too small)."""
        def ptr(x):
            return int(x.data_ptr()) if hasattr(x, "data_ptr") else (None if x is None else int(x))
        text_off = np.ascontiguousarray(text_off, dtype=np.uint64)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        cap_bases = np.ascontiguousarray(cap_bases, dtype=np.uint64)
        n = len(base_off)
        if len(text_off) != n + 1 or len(cap_bases) != n:
            raise ValueError("text_off must hold n + 1 and cap_bases n entries")
        m = max(n, 1)
        out = {"length": np.zeros(m, np.uint64), "padded": np.zeros(m, np.uint64),
               "n_records": np.zeros(m, np.uint32), "n_kmers": np.zeros(m, np.uint64),
               "status": np.zeros(m, np.uint8)}
        z = np.zeros(1, np.uint64)
        check(lib().drephip_fasta_pack_device(self._h, ptr(text), text_off, n, base_off if n else z,
                                              cap_bases if n else z, ptr(d_codes), ptr(d_valid),
                                              out["length"].ctypes.data, out["padded"].ctypes.data,
                                              out["n_records"].ctypes.data, out["n_kmers"].ctypes.data,
                                              out["status"].ctypes.data, stream), "drephip_fasta_pack_device")
        return {k: v[:n] for k, v in out.items()}

    def ingest_stats(self):
        """{produce_s, gpu_s, wall_s, batches} of the last sketch_files call."""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        n = C.c_uint32(0)
        check(lib().drephip_last_ingest_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)),
              "drephip_last_ingest_stats")
        r, p = C.c_double(0), C.c_double(0)
        o = C.c_uint32(0)
        check(lib().drephip_last_ingest_phases(self._h, C.byref(r), C.byref(p), C.byref(o)),
              "drephip_last_ingest_phases")
        return {"produce_s": a.value, "gpu_s": b.value, "wall_s": c.value, "batches": n.value,
                "read_thread_s": r.value, "pack_thread_s": p.value, "overflow_genomes": o.value}

    def sketch_records(self, seq: np.ndarray, rec_off: np.ndarray, genome_rec_off: np.ndarray):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        genome_rec_off = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        n = len(genome_rec_off) - 1
        hashes = np.zeros((max(n, 0), self.s), dtype=np.uint64)
        nhash = np.zeros(max(n, 0), dtype=np.uint32)
        length = np.zeros(max(n, 0), dtype=np.uint64)
        if n <= 0:
            return hashes, nhash, length
        check(lib().drephip_sketch(self._h, seq if len(seq) else np.zeros(1, np.uint8), rec_off,
                                   len(rec_off) - 1, genome_rec_off, n, hashes.reshape(-1), nhash, length),
              "drephip_sketch")
        return hashes, nhash, length

    def sketch_device(self, d_codes: int, d_valid: int, base_off, padded, nkmers, n: int,
                      d_hashes: int, d_nhash: int, stream: Optional[int] = None) -> None:
        check(lib().drephip_sketch_device(self._h, d_codes, d_valid,
                                          np.ascontiguousarray(base_off, dtype=np.uint64),
                                          np.ascontiguousarray(padded, dtype=np.uint64),
                                          np.ascontiguousarray(nkmers, dtype=np.uint64), n,
                                          d_hashes, d_nhash, stream), "drephip_sketch_device")

    def sketch_device_async(self, d_codes: int, d_valid: int, base_off, padded, nkmers, n: int,
                            d_hashes: int, d_nhash: int, stream: Optional[int] = None) -> None:
        """sketch_device without the wait: the sketches are final after
        sketch_wait() (include/drephip.h)."""
        check(lib().drephip_sketch_device_async(self._h, d_codes, d_valid,
                                                np.ascontiguousarray(base_off, dtype=np.uint64),
                                                np.ascontiguousarray(padded, dtype=np.uint64),
                                                np.ascontiguousarray(nkmers, dtype=np.uint64), n,
                                                d_hashes, d_nhash, stream), "drephip_sketch_device_async")

    def sketch_wait(self) -> bool:
        """Completes sketch_device_async; True if the sketches were recomputed
        (results derived from them in between must be recomputed)."""
        redone = C.c_int(0)
        check(lib().drephip_sketch_wait(self._h, C.byref(redone)), "drephip_sketch_wait")
        return bool(redone.value)

    def synth_device(self, seed: int, g0: int, n: int, family_size: int, L: int, d_codes: int,
                     d_valid: int, stream: Optional[int] = None) -> None:
        check(lib().drephip_synth_device(self._h, seed, g0, n, family_size, L, d_codes, d_valid, stream),
              "drephip_synth_device")

    # -- all-pairs
    def allpairs(self, hashes: np.ndarray, nhash: np.ndarray, want_denom: Optional[bool] = None):
        hashes, nhash = tri_arrays(hashes, nhash, self.s)
        N = len(nhash)
        npairs = N * (N - 1) // 2
        if want_denom is None:
            want_denom = bool((nhash < self.s).any())
        common = np.zeros(max(npairs, 1), dtype=np.uint16)
        denom = np.zeros(max(npairs, 1), dtype=np.uint16) if want_denom else None
        if N >= 2:
            check(lib().drephip_allpairs(self._h, hashes.reshape(-1), nhash, N, common,
                                         denom.ctypes.data if denom is not None else None),
                  "drephip_allpairs")
        common = common[:npairs]
        if denom is None:
            denom = np.full(npairs, self.s, dtype=np.uint16)
        else:
            denom = denom[:npairs]
        return common, denom

    def allpairs_rows(self, hashes: np.ndarray, nhash: np.ndarray, row0: int, row1: int,
                      common_out: np.ndarray, denom_out: Optional[np.ndarray] = None) -> None:
        """Rows [row0, row1) of the triangle into the given condensed segment
        views (uint16, contiguous; length = pairs of those rows)."""
        hashes, nhash = tri_arrays(hashes, nhash, self.s)
        N = len(nhash)
        r1 = min(row1, N - 1)

        def start(i):
            return i * N - i * (i + 1) // 2
        n = max(0, start(r1) - start(row0)) if row0 < r1 else 0
        for arr in (common_out, denom_out):
            if arr is not None and (arr.dtype != np.uint16 or not arr.flags.c_contiguous or len(arr) < n):
                raise ValueError("segment buffers must be contiguous uint16 of length >= %d" % n)
        if n == 0:
            return
        check(lib().drephip_allpairs_rows(self._h, hashes.reshape(-1), nhash, N, row0, row1,
                                          common_out.ctypes.data,
                                          denom_out.ctypes.data if denom_out is not None else None),
              "drephip_allpairs_rows")

    # -- sparse all-pairs (include/drephip.h: drephip_allpairs_sparse ...)
    ERR_NOMEM = ERR_NOMEM                # the module's constant, kept as Context.ERR_NOMEM for callers

    def allpairs_sparse_raw(self, hashes: np.ndarray, nhash: np.ndarray, row0: int, row1: int,
                            pairs: Optional[np.ndarray]) -> Tuple[int, int]:
        """One drephip_allpairs_sparse call into `pairs` (uint32 [cap, 4],
        contiguous; None: count only): (return code, records the rows hold).
        Raises on every error but DREPHIP_ERR_NOMEM (the buffer is too small)."""
        hashes, nhash = tri_arrays(hashes, nhash, self.s)
        cap = _pairs_cap(pairs)
        n = C.c_uint64(0)
        rc = lib().drephip_allpairs_sparse(self._h, hashes.reshape(-1), nhash, len(nhash), int(row0), int(row1),
                                           pairs.ctypes.data if cap else None, cap, C.byref(n))
        return _nomem_ok(rc, "drephip_allpairs_sparse"), n.value

    def allpairs_sparse(self, hashes: np.ndarray, nhash: np.ndarray, row0: int = 0, row1: Optional[int] = None,
                        cap: Optional[int] = None):
        """The pairs of rows [row0, row1) that share a hash, as (i, j, common,
        denom) -- uint32, uint32, uint16, uint16 -- sorted by (i, j); every
        pair not listed has common 0.  `cap`: records to make room for at
        first (default 8 per genome + 4096); when the rows hold more, the call
        is repeated once with the size the library reports."""
        N = len(nhash)
        row1 = N if row1 is None else int(row1)
        cap = int(cap) if cap is not None else 8 * N + 4096
        return _sorted_records(lambda pairs: self.allpairs_sparse_raw(hashes, nhash, row0, row1, pairs),
                               "drephip_allpairs_sparse", cap)

    def allpairs_sparse_device(self, d_hashes: int, d_nhash: int, N: int, row0: int, row1: int,
                               d_pairs: Optional[int], cap: int, stream: Optional[int] = None) -> Tuple[int, int]:
        """drephip_allpairs_sparse_device: (return code, records the rows hold);
        raises on every error but DREPHIP_ERR_NOMEM."""
        n = C.c_uint64(0)
        rc = lib().drephip_allpairs_sparse_device(self._h, d_hashes, d_nhash, N, row0, row1, d_pairs, cap,
                                                  C.byref(n), stream)
        return _nomem_ok(rc, "drephip_allpairs_sparse_device"), n.value

    def allpairs_sparse_device_marked(self, d_hashes: int, d_nhash: int, N: int, row0: int, row1: int,
                                      d_cells: Optional[int], n_cells: int, d_records: Optional[int], n_records: int,
                                      d_pairs: Optional[int], cap: int, stream: Optional[int] = None) -> Tuple[int, int]:
        """drephip_allpairs_sparse_device_marked (rows [row0, row1) screened from
        every hash part's cells and records): (return code, records the rows
        hold); raises on every error but DREPHIP_ERR_NOMEM."""
        n = C.c_uint64(0)
        rc = lib().drephip_allpairs_sparse_device_marked(self._h, d_hashes, d_nhash, N, row0, row1, d_cells, n_cells,
                                                         d_records, n_records, d_pairs, cap, C.byref(n), stream)
        return _nomem_ok(rc, "drephip_allpairs_sparse_device_marked"), n.value

    # -- query against reference (include/drephip.h: drephip_dist_rect ...)
    def _rect_range(self, Q: int, q0: int, q1: Optional[int]) -> Tuple[int, int]:
        q0 = int(q0)
        q1 = Q if q1 is None else min(int(q1), Q)
        if q0 < 0 or q1 < 0:
            raise ValueError("q0 and q1 must not be negative")
        return q0, q1

    def dist_rect(self, qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray,
                  q0: int = 0, q1: Optional[int] = None, common_out: Optional[np.ndarray] = None,
                  denom_out: Optional[np.ndarray] = None):
        """`mash dist <reference> <query>` as counts: (common, denom), uint16
        [q1 - q0, N], for query rows [q0, q1) against every reference row
        (drephip_dist_rect).  common_out / denom_out: contiguous uint16 buffers
        of at least (q1 - q0) * N entries to write into instead."""
        qhashes, qnhash, rhashes, rnhash = rect_arrays(qhashes, qnhash, rhashes, rnhash, self.s)
        Q, N = len(qnhash), len(rnhash)
        q0, q1 = self._rect_range(Q, q0, q1)
        rows = max(0, q1 - q0)
        for arr in (common_out, denom_out):
            if arr is not None and (arr.dtype != np.uint16 or not arr.flags.c_contiguous or arr.size < rows * N):
                raise ValueError("output buffers must be contiguous uint16 of at least %d entries" % (rows * N))
        common = common_out if common_out is not None else np.zeros((rows, N), dtype=np.uint16)
        denom = denom_out if denom_out is not None else np.zeros((rows, N), dtype=np.uint16)
        check(lib().drephip_dist_rect(self._h, qhashes.reshape(-1), qnhash, Q, rhashes.reshape(-1), rnhash, N, q0, q1,
                                      common.ctypes.data, denom.ctypes.data), "drephip_dist_rect")
        return common, denom

    def dist_rect_device(self, d_qhashes: int, d_qnhash: int, Q: int, d_rhashes: int, d_rnhash: int, N: int,
                         q0: int, q1: int, d_common: int, d_denom: Optional[int] = None,
                         stream: Optional[int] = None, merge: bool = False) -> None:
        fn = lib().drephip_dist_rect_merge_device if merge else lib().drephip_dist_rect_device
        check(fn(self._h, d_qhashes, d_qnhash, Q, d_rhashes, d_rnhash, N, q0, q1, d_common, d_denom, stream),
              "drephip_dist_rect_merge_device" if merge else "drephip_dist_rect_device")

    def dist_rect_merge(self, qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray,
                        q0: int = 0, q1: Optional[int] = None):
        """dist_rect by the literal merge kernel (drephip_dist_rect_merge_device;
        the cross-check): the matrices are staged with torch on this context's
        device."""
        import torch
        qhashes, qnhash, rhashes, rnhash = rect_arrays(qhashes, qnhash, rhashes, rnhash, self.s)
        Q, N = len(qnhash), len(rnhash)
        q0, q1 = self._rect_range(Q, q0, q1)
        rows = max(0, q1 - q0)
        if rows == 0 or N == 0:
            return np.zeros((rows, N), dtype=np.uint16), np.zeros((rows, N), dtype=np.uint16)
        dev = torch.device("cuda", self.device)

        def up(a, view):
            return torch.tensor(a.view(view), device=dev)      # (a copy: the input may be read-only)
        with torch.cuda.device(dev):
            d_qh, d_qn = up(qhashes, np.int64), up(qnhash, np.int32)
            d_rh, d_rn = up(rhashes, np.int64), up(rnhash, np.int32)
            d_c = torch.zeros((rows, N), dtype=torch.int16, device=dev)
            d_d = torch.zeros((rows, N), dtype=torch.int16, device=dev)
            torch.cuda.synchronize(dev)
            self.dist_rect_device(d_qh.data_ptr(), d_qn.data_ptr(), Q, d_rh.data_ptr(), d_rn.data_ptr(), N, q0, q1,
                                  d_c.data_ptr(), d_d.data_ptr(), merge=True)
            return d_c.cpu().numpy().view(np.uint16), d_d.cpu().numpy().view(np.uint16)

    def dist_rect_sparse_raw(self, qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray,
                             q0: int, q1: Optional[int], pairs: Optional[np.ndarray]) -> Tuple[int, int]:
        """One drephip_dist_rect_sparse call into `pairs` (uint32 [cap, 4],
        contiguous; None: count only): (return code, records the rows hold).
        Raises on every error but DREPHIP_ERR_NOMEM (the buffer is too small)."""
        qhashes, qnhash, rhashes, rnhash = rect_arrays(qhashes, qnhash, rhashes, rnhash, self.s)
        Q, N = len(qnhash), len(rnhash)
        q0, q1 = self._rect_range(Q, q0, q1)
        cap = _pairs_cap(pairs)
        n = C.c_uint64(0)
        rc = lib().drephip_dist_rect_sparse(self._h, qhashes.reshape(-1), qnhash, Q, rhashes.reshape(-1), rnhash, N,
                                            q0, q1, pairs.ctypes.data if cap else None, cap, C.byref(n))
        return _nomem_ok(rc, "drephip_dist_rect_sparse"), n.value

    def dist_rect_sparse_device(self, d_qhashes: int, d_qnhash: int, Q: int, d_rhashes: int, d_rnhash: int, N: int,
                                q0: int, q1: int, d_pairs: Optional[int], cap: int,
                                stream: Optional[int] = None) -> Tuple[int, int]:
        """drephip_dist_rect_sparse_device: (return code, records the rows hold);
        raises on every error but DREPHIP_ERR_NOMEM."""
        n = C.c_uint64(0)
        rc = lib().drephip_dist_rect_sparse_device(self._h, d_qhashes, d_qnhash, Q, d_rhashes, d_rnhash, N, q0, q1,
                                                   d_pairs, cap, C.byref(n), stream)
        return _nomem_ok(rc, "drephip_dist_rect_sparse_device"), n.value

    def dist_rect_sparse(self, qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray,
                         q0: int = 0, q1: Optional[int] = None, cap: Optional[int] = None):
        """The (query, reference) pairs of query rows [q0, q1) that share a hash,
        as (q, r, common, denom) -- uint32, uint32, uint16, uint16 -- sorted by
        (q, r); every pair not listed has common 0.  `cap`: records to make room
        for at first (default 8 per query + 4096); when the rows hold more, the
        call is repeated once with the size the library reports."""
        cap = int(cap) if cap is not None else 8 * len(qnhash) + 4096
        return _sorted_records(lambda pairs: self.dist_rect_sparse_raw(qhashes, qnhash, rhashes, rnhash, q0, q1, pairs),
                               "drephip_dist_rect_sparse", cap)

    def dist_rect_top_raw(self, qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray,
                          top: int, q0: int, q1: Optional[int], hits: np.ndarray, count: np.ndarray) -> int:
        """One drephip_dist_rect_top call into `hits` (contiguous uint32, at
        least rows * top * 4 entries) and `count` (contiguous uint32, at least
        rows entries), rows = q1 - q0 after clamping; returns rows.  Only the
        rows' slots are written."""
        qhashes, qnhash, rhashes, rnhash = rect_arrays(qhashes, qnhash, rhashes, rnhash, self.s)
        Q, N = len(qnhash), len(rnhash)
        q0, q1 = self._rect_range(Q, q0, q1)
        rows, top = max(0, q1 - q0), int(top)
        for arr, need in ((hits, rows * max(top, 0) * 4), (count, rows)):
            if arr.dtype != np.uint32 or not arr.flags.c_contiguous or arr.size < need:
                raise ValueError("output buffers must be contiguous uint32 of at least %d entries" % need)
        if top < 0:
            raise ValueError("top must not be negative")
        check(lib().drephip_dist_rect_top(self._h, qhashes.reshape(-1), qnhash, Q, rhashes.reshape(-1), rnhash, N,
                                          q0, q1, top, hits.ctypes.data, count.ctypes.data), "drephip_dist_rect_top")
        return rows

    def dist_rect_top(self, qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray,
                      top: int, q0: int = 0, q1: Optional[int] = None):
        """The `top` (1..64) nearest references of query rows [q0, q1) among
        those sharing a hash with the row (drephip_dist_rect_top): (ref int64
        [rows, top], common uint16 [rows, top], denom uint16 [rows, top], count
        uint32 [rows]).  Nearest first: larger common / denom as exact
        rationals, ties by the smaller reference row.  Slots at or past
        count[row] hold ref -1, common 0, denom 0."""
        Q = len(np.asarray(qnhash))
        a, b = self._rect_range(Q, q0, q1)
        rows, top = max(0, b - a), int(top)
        hits = np.empty((rows, max(top, 0), 4), dtype=np.uint32)
        hits[:] = (0xFFFFFFFF, 0, 0, 0)                  # (an empty call writes nothing)
        count = np.zeros(rows, dtype=np.uint32)
        self.dist_rect_top_raw(qhashes, qnhash, rhashes, rnhash, top, q0, q1, hits, count)
        ref = hits[:, :, 0].astype(np.int64)
        ref[ref == 0xFFFFFFFF] = -1
        return ref, hits[:, :, 1].astype(np.uint16), hits[:, :, 2].astype(np.uint16), count

    def dist_rect_top_device(self, d_qhashes: int, d_qnhash: int, Q: int, d_rhashes: int, d_rnhash: int, N: int,
                             q0: int, q1: int, top: int, d_hits: Optional[int], d_count: Optional[int],
                             stream: Optional[int] = None) -> None:
        """drephip_dist_rect_top_device: d_hits uint32 [(q1 - q0), top, 4],
        d_count uint32 [q1 - q0], device pointers."""
        check(lib().drephip_dist_rect_top_device(self._h, d_qhashes, d_qnhash, Q, d_rhashes, d_rnhash, N, q0, q1,
                                                 int(top), d_hits, d_count, stream), "drephip_dist_rect_top_device")

    # -- significance (include/drephip.h: drephip_pvalue_records ...)
    def pvalue_records(self, records: np.ndarray, len_a: np.ndarray, len_b: Optional[np.ndarray] = None,
                       out: Optional[np.ndarray] = None) -> np.ndarray:
        """drephip_pvalue_records: Mash's p-value of each record {a, b, common,
        denom} (uint32 [n, 4]) on the GPU; a indexes len_a, b indexes len_b
        (default: len_a, the triangle's records).  `out`: a contiguous float64
        buffer of at least n entries to write into."""
        records = _records(records)
        len_a = np.ascontiguousarray(len_a, dtype=np.uint64)
        len_b = len_a if len_b is None else np.ascontiguousarray(len_b, dtype=np.uint64)
        n = len(records)
        if out is None:
            out = np.empty(n, dtype=np.float64)
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size < n:
            raise ValueError("out must be contiguous float64 of at least %d entries" % n)
        z = np.zeros(1, np.uint64)
        check(lib().drephip_pvalue_records(self._h, records.ctypes.data, n, len_a if len(len_a) else z, len(len_a),
                                           len_b if len(len_b) else z, len(len_b), out.ctypes.data),
              "drephip_pvalue_records")
        return out[:n]

    def pvalue_records_device(self, d_records: Optional[int], n: int, d_len_a: Optional[int], n_a: int,
                              d_len_b: Optional[int], n_b: int, d_pval: Optional[int],
                              stream: Optional[int] = None) -> None:
        """drephip_pvalue_records_device: device pointers (records uint32 [n, 4],
        lengths uint64, d_pval float64 [n])."""
        check(lib().drephip_pvalue_records_device(self._h, d_records, int(n), d_len_a, int(n_a), d_len_b, int(n_b),
                                                  d_pval, stream), "drephip_pvalue_records_device")

    def pvalue_hits_device(self, d_hits: Optional[int], d_count: Optional[int], rows: int, top: int,
                           d_qlen: Optional[int], d_rlen: Optional[int], N: int, d_pval: Optional[int],
                           stream: Optional[int] = None) -> None:
        """drephip_pvalue_hits_device: device pointers (the hits and counts of
        dist_rect_top_device, uint64 lengths, d_pval float64 [rows, top])."""
        check(lib().drephip_pvalue_hits_device(self._h, d_hits, d_count, int(rows), int(top), d_qlen, d_rlen, int(N),
                                               d_pval, stream), "drephip_pvalue_hits_device")

    def _torch_dev(self):
        import torch
        return torch, torch.device("cuda", self.device)

    def pvalue_hits(self, ref: np.ndarray, common: np.ndarray, denom: np.ndarray, count: np.ndarray,
                    qlen: np.ndarray, rlen: np.ndarray) -> np.ndarray:
        """The p-values of the best hits dist_rect_top returned ((ref, common,
        denom) [rows, top], count [rows]; qlen: the rows' query lengths, rlen:
        every reference's): float64 [rows, top], 1.0 in the slots at or past
        count[row].  Staged with torch on this context's device
        (drephip_pvalue_hits_device)."""
        ref = np.asarray(ref)
        rows, top = ref.shape
        hits = np.zeros((rows, top, 4), dtype=np.uint32)
        hits[:, :, 0] = np.where(ref < 0, 0xFFFFFFFF, ref).astype(np.uint32)
        hits[:, :, 1] = common
        hits[:, :, 2] = denom
        qlen = np.ascontiguousarray(qlen, dtype=np.uint64)
        rlen = np.ascontiguousarray(rlen, dtype=np.uint64)
        if len(qlen) != rows:
            raise ValueError("qlen must hold one length per row")
        if rows == 0 or top == 0:
            return np.ones((rows, top), dtype=np.float64)
        torch, dev = self._torch_dev()
        with torch.cuda.device(dev):
            d_h = torch.tensor(hits.view(np.int32), device=dev)
            d_c = torch.tensor(np.ascontiguousarray(count, dtype=np.uint32).view(np.int32), device=dev)
            d_q = torch.tensor(qlen.view(np.int64), device=dev)
            d_r = torch.tensor(rlen.view(np.int64) if len(rlen) else np.zeros(1, np.int64), device=dev)
            d_p = torch.zeros((rows, top), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            self.pvalue_hits_device(d_h.data_ptr(), d_c.data_ptr(), rows, top, d_q.data_ptr(), d_r.data_ptr(),
                                    len(rlen), d_p.data_ptr())
            return d_p.cpu().numpy()

    def filter_records_device(self, d_records: Optional[int], d_pval: Optional[int], n: int, max_p: float,
                              d_cmin: Optional[int], d_out: Optional[int], d_pval_out: Optional[int],
                              stream: Optional[int] = None) -> int:
        """drephip_records_filter_device (device pointers): the survivors' count."""
        kept = C.c_uint64(0)
        check(lib().drephip_records_filter_device(self._h, d_records, d_pval, int(n), float(max_p), d_cmin, d_out,
                                                  d_pval_out, C.byref(kept), stream), "drephip_records_filter_device")
        return int(kept.value)

    def filter_records(self, records: np.ndarray, pval: Optional[np.ndarray] = None, max_p: float = 1.0,
                       cmin: Optional[np.ndarray] = None):
        """The records (uint32 [n, 4]) with pval <= max_p (no test without
        pval) and common >= cmin[denom] (cmin: s + 1 entries, see
        d_cluster.min_common_table; no test without it), in their order:
        (records, pval or None).  Staged with torch on this context's device
        (drephip_records_filter_device)."""
        records = _records(records)
        n = len(records)
        if pval is not None:
            pval = np.ascontiguousarray(pval, dtype=np.float64)
            if pval.shape != (n,):
                raise ValueError("pval must hold one value per record")
        if cmin is not None:
            cmin = np.ascontiguousarray(cmin, dtype=np.uint32)
            if cmin.shape != (self.s + 1,):
                raise ValueError("cmin must hold s + 1 entries")
        torch, dev = self._torch_dev()
        with torch.cuda.device(dev):
            d_r = torch.tensor(records.view(np.int32) if n else np.zeros((1, 4), np.int32), device=dev)
            d_p = None if pval is None else torch.tensor(pval if n else np.zeros(1), device=dev)
            d_c = None if cmin is None else torch.tensor(cmin.view(np.int32), device=dev)
            d_o = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
            d_po = None if pval is None else torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            kept = self.filter_records_device(d_r.data_ptr(), None if d_p is None else d_p.data_ptr(), n, max_p,
                                              None if d_c is None else d_c.data_ptr(), d_o.data_ptr(),
                                              None if d_po is None else d_po.data_ptr())
            out = d_o[:kept].cpu().numpy().view(np.uint32)
            return out, (None if d_po is None else d_po[:kept].cpu().numpy())

    def _sig_call(self, call, what: str, n_first: int, length_arrays, max_p: float, cmin, cap: Optional[int],
                  want_pval: bool):
        """One _sig host call with the retry of the record calls: (records
        uint32 [n, 4] in the device call's order, pval or None, n_listed)."""
        if cmin is not None:
            cmin = np.ascontiguousarray(cmin, dtype=np.uint32)
            if cmin.shape != (self.s + 1,):
                raise ValueError("cmin must hold s + 1 entries")
        cap = int(cap) if cap is not None else 8 * n_first + 4096
        n, listed = C.c_uint64(0), C.c_uint64(0)
        for _ in range(2):
            buf = np.empty((max(cap, 1), 4), dtype=np.uint32)
            pv = np.empty(max(cap, 1), dtype=np.float64) if want_pval else None
            rc = call(*length_arrays, float(max_p), _ptr(cmin), buf.ctypes.data if cap else None, cap, _ptr(pv),
                      C.byref(n), C.byref(listed))
            if rc != self.ERR_NOMEM:
                break
            cap = n.value
        check(rc, what)
        return buf[:n.value], (None if pv is None else pv[:n.value]), int(listed.value)

    def allpairs_sparse_sig_raw(self, hashes: np.ndarray, nhash: np.ndarray, length: np.ndarray, row0: int, row1: int,
                                max_p: float, cmin: Optional[np.ndarray], pairs: Optional[np.ndarray],
                                pval: Optional[np.ndarray]) -> Tuple[int, int, int]:
        """One drephip_allpairs_sparse_sig call into `pairs` (uint32 [cap, 4];
        None: count only) and `pval` (float64 [cap] or None): (return code,
        records that pass the filter, records listed before it).  Raises on
        every error but DREPHIP_ERR_NOMEM."""
        hashes, nhash, length = tri_arrays(hashes, nhash, self.s, length)
        N = len(nhash)
        cap = 0 if pairs is None else len(pairs)
        cm = None if cmin is None else np.ascontiguousarray(cmin, dtype=np.uint32)
        n, listed = C.c_uint64(0), C.c_uint64(0)
        rc = lib().drephip_allpairs_sparse_sig(self._h, hashes.reshape(-1), nhash, N, int(row0), int(row1), length,
                                               float(max_p), _ptr(cm), pairs.ctypes.data if cap else None, cap,
                                               _ptr(pval), C.byref(n), C.byref(listed))
        return _nomem_ok(rc, "drephip_allpairs_sparse_sig"), n.value, listed.value

    def allpairs_sparse_sig(self, hashes: np.ndarray, nhash: np.ndarray, length: np.ndarray, max_p: float = 1.0,
                            cmin: Optional[np.ndarray] = None, row0: int = 0, row1: Optional[int] = None,
                            cap: Optional[int] = None):
        """allpairs_sparse with Mash's p-value per record and the -v / -d
        filters applied on the GPU before the copy
        (drephip_allpairs_sparse_sig): (i, j, common, denom, p, n_listed), the
        records sorted by (i, j); n_listed counts them before the filter."""
        hashes, nhash, length = tri_arrays(hashes, nhash, self.s, length)
        N = len(nhash)
        row1 = N if row1 is None else int(row1)

        def call(ln, *rest):
            return lib().drephip_allpairs_sparse_sig(self._h, hashes.reshape(-1), nhash, N, int(row0), row1, ln, *rest)
        rec, pv, listed = self._sig_call(call, "drephip_allpairs_sparse_sig", N, (length,), max_p, cmin, cap, True)
        return _sorted_sig(rec, pv) + (listed,)

    def dist_rect_sparse_sig_raw(self, qhashes, qnhash, rhashes, rnhash, qlength, rlength, q0: int, q1: Optional[int],
                                 max_p: float, cmin: Optional[np.ndarray], pairs: Optional[np.ndarray],
                                 pval: Optional[np.ndarray]) -> Tuple[int, int, int]:
        """One drephip_dist_rect_sparse_sig call (see allpairs_sparse_sig_raw)."""
        qhashes, qnhash, rhashes, rnhash = rect_arrays(qhashes, qnhash, rhashes, rnhash, self.s)
        Q, N = len(qnhash), len(rnhash)
        ql, rl = _lengths(qlength, Q), _lengths(rlength, N)
        q0, q1 = self._rect_range(Q, q0, q1)
        cap = 0 if pairs is None else len(pairs)
        cm = None if cmin is None else np.ascontiguousarray(cmin, dtype=np.uint32)
        n, listed = C.c_uint64(0), C.c_uint64(0)
        rc = lib().drephip_dist_rect_sparse_sig(self._h, qhashes.reshape(-1), qnhash, Q, rhashes.reshape(-1), rnhash, N,
                                                q0, q1, ql, rl, float(max_p), _ptr(cm),
                                                pairs.ctypes.data if cap else None, cap, _ptr(pval), C.byref(n),
                                                C.byref(listed))
        return _nomem_ok(rc, "drephip_dist_rect_sparse_sig"), n.value, listed.value

    def dist_rect_sparse_sig(self, qhashes, qnhash, rhashes, rnhash, qlength, rlength, max_p: float = 1.0,
                             cmin: Optional[np.ndarray] = None, q0: int = 0, q1: Optional[int] = None,
                             cap: Optional[int] = None):
        """dist_rect_sparse with Mash's p-value per record and the -v / -d
        filters applied on the GPU before the copy
        (drephip_dist_rect_sparse_sig): (q, r, common, denom, p, n_listed), the
        records sorted by (q, r)."""
        qhashes, qnhash, rhashes, rnhash = rect_arrays(qhashes, qnhash, rhashes, rnhash, self.s)
        Q, N = len(qnhash), len(rnhash)
        ql, rl = _lengths(qlength, Q), _lengths(rlength, N)
        a, b = self._rect_range(Q, q0, q1)

        def call(qlen, rlen, *rest):
            return lib().drephip_dist_rect_sparse_sig(self._h, qhashes.reshape(-1), qnhash, Q, rhashes.reshape(-1),
                                                      rnhash, N, a, b, qlen, rlen, *rest)
        rec, pv, listed = self._sig_call(call, "drephip_dist_rect_sparse_sig", Q, (ql, rl), max_p, cmin, cap, True)
        return _sorted_sig(rec, pv) + (listed,)

    def sparse_stats(self) -> dict:
        """{blocks, direct, fallback, scratch_bytes} of the last sparse all-pairs call."""
        b, d, f, sb = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().drephip_last_sparse_stats(self._h, C.byref(b), C.byref(d), C.byref(f), C.byref(sb)),
              "drephip_last_sparse_stats")
        return {"blocks": b.value, "direct": d.value, "fallback": f.value, "scratch_bytes": sb.value}

    def allpairs_device(self, d_hashes: int, d_nhash: int, N: int, row0: int, row1: int, d_common: int,
                        d_denom: Optional[int] = None, stream: Optional[int] = None, merge: bool = False):
        fn = lib().drephip_allpairs_merge_device if merge else lib().drephip_allpairs_device
        check(fn(self._h, d_hashes, d_nhash, N, row0, row1, d_common, d_denom, stream),
              "drephip_allpairs_device")

    # ---- the sharded screen (include/drephip.h: drephip_screen_part ...)
    def screen_geometry(self) -> int:
        """Rows per row tile of the sharded screen's marks (tile T = rows [T R, (T + 1) R))."""
        r = C.c_uint32()
        check(lib().drephip_screen_geometry(self._h, C.byref(r)), "drephip_screen_geometry")
        return r.value

    def screen_part(self, d_hashes: int, d_nhash: int, N: int, part: int, nparts: int,
                    stream: Optional[int] = None) -> Tuple[int, int, int]:
        """Group hash part `part` of `nparts`: (its pair checks, its cell words, its records)."""
        c, nc, n = C.c_uint64(), C.c_uint32(), C.c_uint32()
        check(lib().drephip_screen_part(self._h, d_hashes, d_nhash, N, part, nparts, C.byref(c), C.byref(nc),
                                        C.byref(n), stream), "drephip_screen_part")
        return c.value, nc.value, n.value

    def screen_part_copy(self, d_cells: Optional[int], d_records: Optional[int], stream: Optional[int] = None) -> None:
        check(lib().drephip_screen_part_copy(self._h, d_cells, d_records, stream), "drephip_screen_part_copy")

    def screen_worth(self, N: int, checks: int) -> Tuple[bool, bool]:
        """(the screen applies to N genomes at all, it would run with these checks)."""
        a, u = C.c_int(), C.c_int()
        check(lib().drephip_screen_worth(self._h, N, checks, C.byref(a), C.byref(u)), "drephip_screen_worth")
        return bool(a.value), bool(u.value)

    def allpairs_device_marked(self, d_hashes: int, d_nhash: int, N: int, row0: int, row1: int, d_common: int,
                               d_denom: Optional[int], d_cells: Optional[int], n_cells: int, d_records: Optional[int],
                               n_records: int, stream: Optional[int] = None) -> None:
        check(lib().drephip_allpairs_device_marked(self._h, d_hashes, d_nhash, N, row0, row1, d_common, d_denom,
                                                   d_cells, n_cells, d_records, n_records, stream),
              "drephip_allpairs_device_marked")

    def allpairs_device_async(self, d_hashes: int, d_nhash: int, N: int, row0: int, row1: int,
                              d_common: int, d_denom: Optional[int] = None, stream: Optional[int] = None):
        """allpairs_device whose failure-count check is deferred to
        allpairs_wait() (include/drephip.h)."""
        check(lib().drephip_allpairs_device_async(self._h, d_hashes, d_nhash, N, row0, row1, d_common,
                                                  d_denom, stream), "drephip_allpairs_device_async")

    def allpairs_wait(self) -> None:
        check(lib().drephip_allpairs_wait(self._h), "drephip_allpairs_wait")
