"""drep_amd -- MI355X-native drop-in for dRep's primary-clustering Mash step.

The reference (SilasK/drep, drep/d_cluster.py:481-630) shells out to the Mash
binary to sketch every genome and compute all-vs-all Mash distances, then
clusters the resulting Mdb table with scipy.  This package keeps that Python
surface (``d_cluster.all_vs_all_MASH`` -> Mdb, ``cluster_mash_database`` ->
Cdb) and runs the sketch and all-pairs arithmetic in hand-written HIP kernels
for gfx950 (libdrephip.so, C ABI in include/drephip.h).  There is no CPU
fallback: without the HIP library every compute call raises.
"""
from . import mash_io
from ._lib import Context, DrepHipError

__all__ = ["Context", "DrepHipError", "mash_io", "d_cluster", "SparseMash", "all_vs_all_MASH_sparse",
           "cluster_mash_sparse", "mdb_from_sparse", "store_sparse", "load_sparse", "RectMash", "query_vs_MASH",
           "query_vs_MASH_rect", "rect_allpairs", "rect_allpairs_sparse", "mdb_from_rect", "union_condensed",
           "rect_top_hits", "query_best_hits", "place_queries", "mash_pvalue_device", "min_common_table",
           "write_mash_table_rect", "sparse_allpairs_sig", "rect_allpairs_sparse_sig"]
__version__ = "0.1.0"


def __getattr__(name):
    if name == "d_cluster":   # lazy: pulls in pandas/scipy
        import importlib
        return importlib.import_module(".d_cluster", __name__)
    if name in ("SparseMash", "all_vs_all_MASH_sparse", "cluster_mash_sparse", "mdb_from_sparse"):
        import importlib           # the sparse pipeline (>~2x10^5 genomes), lazy for the same reason
        return getattr(importlib.import_module(".d_cluster", __name__), name)
    if name in ("RectMash", "query_vs_MASH", "query_vs_MASH_rect", "rect_allpairs", "rect_allpairs_sparse",
                "mdb_from_rect", "union_condensed", "rect_top_hits", "query_best_hits", "place_queries"):
        import importlib           # query against reference (`mash dist <reference> <query>`)
        return getattr(importlib.import_module(".d_cluster", __name__), name)
    if name in ("mash_pvalue_device", "min_common_table", "write_mash_table_rect", "sparse_allpairs_sig",
                "rect_allpairs_sparse_sig"):
        import importlib           # significance: Mash's p-value and its -v / -d filters on the GPU
        return getattr(importlib.import_module(".d_cluster", __name__), name)
    if name in ("store_sparse", "load_sparse"):
        import importlib
        return getattr(importlib.import_module(".store", __name__), name)
    raise AttributeError(name)
