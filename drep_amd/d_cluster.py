"""Drop-in for the Mash half of dRep's primary clustering, on MI355X.

Mirrors the reference functions of ``drep/d_cluster.py`` that sit on the hot
path -- same names, arguments, return values and side effects on the work
directory -- with the external ``mash sketch`` / ``mash paste`` /
``mash dist`` processes replaced by libdrephip.so (HIP kernels, gfx950):

===============================  ==========================================
reference (drep/d_cluster.py)    here
===============================  ==========================================
all_vs_all_MASH       481-596    :func:`all_vs_all_MASH`
cluster_mash_database 598-630    :func:`cluster_mash_database` (its
  cluster_hierarchical 429-461 /  linkage + fcluster + Cdb steps inline)
  _gen_cdb_from_fclust 463-479
_get_genome_name_from_fasta 632  :func:`_get_genome_name_from_fasta`
===============================  ==========================================

dRep's own ``load_genomes`` (1483-1518) builds the Bdb these functions take;
it is not on the hot path and stays dRep's.

Beyond the reference (needed at 10^4-10^5 genomes, where an N^2-row Mdb does
not fit): :func:`all_vs_all_MASH_condensed` returns the condensed
``common``/``denom`` vectors and :func:`mdb_from_condensed` /
:func:`cluster_mash_condensed` build the Mdb / primary clusters from them with
the same float32 arithmetic the reference applies; with ``gpu=`` the linkage
itself (scipy's algorithm, bit-identical Z) runs on the GPU.
"""
from __future__ import annotations

import io
import logging
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import pandas as pd
import scipy.cluster.hierarchy
import scipy.spatial.distance as ssd

from . import _lib
from .mash_io import MashReference, read_msh, write_msh
from .parallel import cond_start, row_partition, segment_size

MASH_K = 21          # Mash default, never overridden by dRep (d_cluster.py:543)
MASH_SEED = 42       # Mash default hash seed

# host wall-clock seconds of the stages of the last all_vs_all_MASH /
# cluster_mash_database call in this process (tools/dropin_bench.py reports
# them; nothing reads them on the product path)
STAGE_TIMES: Dict[str, float] = {}


class _Stage:
    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        import time
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        import time
        STAGE_TIMES[self.name] = time.perf_counter() - self.t0


# --------------------------------------------------------------- genomes
def _get_genome_name_from_fasta(fasta):
    """os.path.basename (reference drep/d_cluster.py:632-642)."""
    return str(os.path.basename(fasta))


# ----------------------------------------------------------- distances
def mash_distance_float32(common: np.ndarray, denom: np.ndarray, k: int = MASH_K) -> np.ndarray:
    """float32 "dist" values exactly as the reference obtains them.

    The reference parses Mash's text output: ``mash dist`` prints the double
    distance with C++ ostream defaults (= ``%g``, 6 significant digits) and
    ``pd.read_csv(..., dtype={'dist': np.float32})`` parses it
    (d_cluster.py:570-581).  Distance is a pure function of (common, denom), so
    the at most (s+1) x (#denominators) distinct values are formatted and
    pushed through the same ``read_csv`` call, then gathered.
    """
    common = np.asarray(common)
    denom = np.asarray(denom)
    out = np.empty(common.shape, dtype=np.float32)
    if common.size == 0:
        return out
    for d in np.unique(denom):
        d = int(d)
        sel = denom == d
        if d == 0:
            lut = np.zeros(1, dtype=np.float64)   # common == denom == 0 -> 0 (Mash)
        else:
            lut = _lib.distance_lut(d, k)
        txt = "\n".join("%g" % v for v in lut) + "\n"
        lut32 = pd.read_csv(io.StringIO(txt), header=None, names=['dist'],
                            dtype={'dist': np.float32}, sep='\t')['dist'].to_numpy()
        out[sel] = lut32[common[sel]]
    return out


def float32_tables(denominators, s: int, k: int = MASH_K):
    """(lut32, lut_off) for every denominator d that occurs: lut32[lut_off[d] +
    c] = the float32 "dist" of (common c, denominator d) as the reference
    parses it (mash_distance_float32); lut_off has s + 1 entries, -1 where d
    does not occur."""
    lut_off = np.full(s + 1, -1, dtype=np.int32)
    parts, pos = [], 0
    for d in np.asarray(denominators, dtype=np.int64):
        d = int(d)
        c = np.arange(d + 1, dtype=np.uint16)
        parts.append(mash_distance_float32(c, np.full(d + 1, d, dtype=np.uint16), k))
        lut_off[d] = pos
        pos += d + 1
    lut32 = np.concatenate(parts).astype(np.float32) if parts else np.zeros(1, np.float32)
    return lut32, lut_off


def _denominators(denom: np.ndarray, s: int):
    """(distinct denominators, whether every pair has denominator s) without
    sorting the condensed vector (5x10^7 entries at 10^4 genomes)."""
    denom = np.asarray(denom)
    if denom.size == 0 or (denom == s).all():
        return np.array([s]), True
    seen = np.bincount(denom.astype(np.int64, copy=False), minlength=s + 1) > 0
    return np.nonzero(seen)[0], False


def mdb_from_condensed(names: Sequence[str], common: np.ndarray, denom: np.ndarray,
                       nhash: np.ndarray, s: int, k: int = MASH_K, threads: int = 0) -> pd.DataFrame:
    """Long-form Mdb (genome1, genome2, dist, similarity) from the condensed
    all-pairs result, with the reference's row order (outer loop = query =
    genome2, inner = reference = genome1, as `mash dist` prints), dtypes
    (ordered categoricals sorted by name; float32) and values
    (d_cluster.py:575-596).

    The N^2 rows are filled by libdrephip on host threads
    (drephip_mdb_square): the float32 distances from one table per
    denominator (the reference's %g / read_csv values, float32_tables), the
    diagonal 0 -- a genome against itself has common = denom = its hash count
    (or 0 for an empty sketch), distance 0 either way --, similarity = 1 - dist
    in float32, and the category codes of both columns; the DataFrame wraps
    those arrays without copying them."""
    N = len(names)
    common = np.asarray(common, dtype=np.uint16)
    dens, full = _denominators(np.asarray(denom, dtype=np.uint16), s)
    lut32, lut_off = float32_tables(dens, s, k)
    cats = sorted(set(names))
    dtype = pd.CategoricalDtype(cats, ordered=True)
    code_t = pd.Categorical([], dtype=dtype).codes.dtype        # pandas' code width for len(cats)
    pos = {n: i for i, n in enumerate(cats)}
    codes = np.array([pos[n] for n in names], dtype=code_t)
    g1, g2, dist, sim = _lib.mdb_square(N, common, None if full else denom, s, lut32, lut_off, codes, threads)
    return pd.DataFrame({'genome1': pd.Categorical.from_codes(g1, dtype=dtype, validate=False),
                         'genome2': pd.Categorical.from_codes(g2, dtype=dtype, validate=False),
                         'dist': dist, 'similarity': sim}, copy=False)


# ---------------------------------------------------------- devices
def _devices(kwargs) -> List[int]:
    """HIP devices for the Mash step: kwargs `gpus` (a count, a list, or
    "0,1,..."), else $DREPHIP_DEVICES, else the single `gpu` /
    $DREPHIP_DEVICE (default 0)."""
    g = kwargs.get('gpus', os.environ.get('DREPHIP_DEVICES'))
    if g is None or g == '':
        return [int(kwargs.get('gpu', os.environ.get('DREPHIP_DEVICE', 0)))]
    if isinstance(g, int):
        return list(range(g))
    if isinstance(g, str):
        return [int(x) for x in g.split(',') if x.strip() != '']
    return [int(x) for x in g]


def _on_devices(devs: Sequence[int], fn) -> list:
    """fn(i, device) for every device, one host thread each (the C ABI calls
    release the GIL); first exception re-raised."""
    from concurrent.futures import ThreadPoolExecutor
    if len(devs) == 1:
        return [fn(0, devs[0])]
    with ThreadPoolExecutor(max_workers=len(devs)) as ex:
        futs = [ex.submit(fn, i, d) for i, d in enumerate(devs)]
        return [f.result() for f in futs]


def _balanced_shards(weights: Sequence[int], n: int) -> List[List[int]]:
    """Contiguous index shards with near-equal total weight (genome bytes)."""
    w = np.asarray(weights, dtype=np.float64)
    cum = np.concatenate([[0.0], np.cumsum(w)])
    cuts = [0] + [int(np.searchsorted(cum, cum[-1] * k / n)) for k in range(1, n)] + [len(w)]
    cuts = np.maximum.accumulate(np.minimum(cuts, len(w)))
    return [list(range(cuts[k], cuts[k + 1])) for k in range(n)]


# ---------------------------------------------------------- sketch cache
def _load_cached(path: str, s: int) -> Optional[MashReference]:
    try:
        m = read_msh(path)
    except Exception:
        return None
    if m.kmer != MASH_K or m.sketch_size != s or m.seed != MASH_SEED or len(m.references) != 1:
        return None
    return m.references[0]


@dataclass
class SketchSet:
    names: List[str]          # genome (basename), Bdb order
    locations: List[str]
    hashes: np.ndarray        # uint64 [N, s], rows padded with UINT64_MAX
    nhash: np.ndarray         # uint32 [N]
    length: np.ndarray        # uint64 [N]
    s: int


def _check_ingest(kwargs) -> str:
    """The `ingest` kwarg ('host' by default), or ValueError."""
    ingest = kwargs.get('ingest', 'host')
    if ingest not in _lib.INGEST_PATHS:
        raise ValueError("ingest must be 'host' or 'device', got %r" % (ingest,))
    return ingest


def sketch_genomes(Bdb: pd.DataFrame, data_folder: str, **kwargs) -> SketchSet:
    """The sketch + paste half of all_vs_all_MASH (d_cluster.py:499-567):
    same folders and files (MASH_files/sketches/chunk_<i>/<genome>.msh,
    chunk_all.msh, ALL.msh), sketches cached across runs by file existence
    (d_cluster.py:541-542), new ones computed on the GPU in one batch.
    `ingest`: 'host' (the default; worker threads parse and pack the FASTA
    files) or 'device' (the GPU does, from the raw text); same sketches."""
    MASH_s = int(kwargs.get('MASH_sketch', 1000))
    ingest = _check_ingest(kwargs)
    p = int(kwargs.get('processors', 6))
    groupSize = int(kwargs.get('groupSize', 1000))
    write_sketches = kwargs.get('write_sketches', True)

    MASH_folder = os.path.join(data_folder, 'MASH_files/')
    sketch_folder = os.path.join(MASH_folder, 'sketches/')
    os.makedirs(sketch_folder, exist_ok=True)

    l2g = Bdb.set_index('location')['genome'].to_dict()
    locations = list(Bdb['location'].unique())
    chunks = [locations[x:x + groupSize] for x in range(0, len(locations), groupSize)]
    N = len(locations)
    names = [l2g[loc] for loc in locations]
    hashes = np.full((N, MASH_s), np.iinfo(np.uint64).max, dtype=np.uint64)
    nhash = np.zeros(N, dtype=np.uint32)
    length = np.zeros(N, dtype=np.uint64)
    msh_path: Dict[int, str] = {}
    todo: List[int] = []
    idx = 0
    chunk_members: List[List[int]] = []
    cache = _Stage('sketch_cache_s')
    cache.__enter__()
    for i, chunk in enumerate(chunks):
        chunk_folder = os.path.join(sketch_folder, "chunk_{0}".format(i))
        os.makedirs(chunk_folder, exist_ok=True)
        members = []
        for _ in chunk:
            f = os.path.join(chunk_folder, names[idx]) + '.msh'
            msh_path[idx] = f
            ref = _load_cached(f, MASH_s) if os.path.isfile(f) else None
            if ref is not None:
                n = min(len(ref.hashes), MASH_s)
                hashes[idx, :n] = ref.hashes[:n]
                nhash[idx] = n
                length[idx] = ref.length
            else:
                todo.append(idx)
            members.append(idx)
            idx += 1
        chunk_members.append(members)
    cache.__exit__()
    STAGE_TIMES['sketched_genomes'] = len(todo)

    sk = _Stage('sketch_gpu_s')
    sk.__enter__()
    if todo:
        devs = _devices(kwargs)
        sizes = [os.path.getsize(locations[i]) if os.path.exists(locations[i]) else 1 for i in todo]
        shards = [[todo[j] for j in sh] for sh in _balanced_shards(sizes, len(devs))]
        threads = max(1, p // len(devs))

        def run(k, dev):
            if not shards[k]:
                return
            with _lib.Context(device=dev, k=MASH_K, s=MASH_s, seed=MASH_SEED) as ctx:
                ctx.set_ingest_path(ingest)
                h, nh, ln = ctx.sketch_files([locations[i] for i in shards[k]], threads=threads)
            hashes[shards[k]] = h
            nhash[shards[k]] = nh
            length[shards[k]] = ln
        _on_devices(devs, run)
        logging.debug("sketched %d genomes on HIP devices %s", len(todo), devs)
    sk.__exit__()

    wr = _Stage('sketch_write_s')
    wr.__enter__()
    if write_sketches:
        def ref_of(i):
            return MashReference(locations[i], '', int(length[i]), hashes[i, :nhash[i]])
        for i in todo:
            write_msh(msh_path[i], [ref_of(i)], MASH_K, MASH_s, MASH_SEED)
        alls = []
        for ci, members in enumerate(chunk_members):
            all_file = os.path.join(sketch_folder, "chunk_{0}".format(ci), 'chunk_all.msh')
            write_msh(all_file, [ref_of(i) for i in members], MASH_K, MASH_s, MASH_SEED)
            alls.append(all_file)
        write_msh(os.path.join(MASH_folder, 'ALL.msh'), [ref_of(i) for i in range(N)],
                  MASH_K, MASH_s, MASH_SEED)
    wr.__exit__()
    return SketchSet(names, locations, hashes, nhash, length, MASH_s)


@dataclass
class CondensedMash:
    names: List[str]
    locations: List[str]
    common: np.ndarray     # uint16, condensed i<j (scipy squareform order)
    denom: np.ndarray      # uint16, same layout
    nhash: np.ndarray
    length: np.ndarray
    s: int


def all_vs_all_MASH_condensed(Bdb, data_folder, **kwargs) -> CondensedMash:
    """Sketch (or load cached sketches) and run the HIP all-pairs kernel;
    return the condensed shared-hash counts instead of an N^2-row table."""
    sk = sketch_genomes(Bdb, data_folder, **kwargs)
    with _Stage('allpairs_s'):
        common, denom = condensed_allpairs(sk.hashes, sk.nhash, sk.s, _devices(kwargs))
    return CondensedMash(sk.names, sk.locations, common, denom, sk.nhash, sk.length, sk.s)


def condensed_allpairs(hashes: np.ndarray, nhash: np.ndarray, s: int, devices: Sequence[int] = (0,)):
    """(common, denom) for the whole condensed triangle.  With several devices
    the rows are split into contiguous ranges of near-equal pair count
    (parallel.row_partition), one context and host thread per device, each
    writing its own segment of the host buffers (no collective)."""
    N = len(nhash)
    npairs = N * (N - 1) // 2
    partial = bool((np.asarray(nhash) < s).any())
    common = np.zeros(npairs, dtype=np.uint16)
    denom = np.zeros(npairs, dtype=np.uint16) if partial else None
    parts = row_partition(N, len(devices))

    def run(k, dev):
        r0, r1 = parts[k]
        a = cond_start(r0, N)
        b = a + segment_size(N, r0, r1)
        if b <= a:
            return
        with _lib.Context(device=dev, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
            ctx.allpairs_rows(hashes, nhash, r0, r1, common[a:b], denom[a:b] if denom is not None else None)
    if npairs:
        _on_devices(list(devices), run)
    if denom is None:
        denom = np.full(npairs, s, dtype=np.uint16)
    return common, denom


def all_vs_all_MASH(Bdb, data_folder, **kwargs):
    """
    Run MASH pairwise within all samples in Bdb (reference
    drep/d_cluster.py:481-596), with sketching and the all-vs-all distance on
    the GPU.

    Args:
        Bdb: dataframe with genome, location
        data_folder: location to store output files

    Keyword Args:
        MASH_sketch: size of mash sketches (int or str, as the CLI passes it)
        dry: dont actually run anything (parses an existing MASH_table.tsv, as
            the reference does after printing its commands)
        processors: CPU threads for FASTA ingest
        groupSize: max number of mash sketches to hold in each folder
        debug / wd: accepted for compatibility (no external commands to log)
        exe_loc / mash_exe: accepted and ignored (no mash executable is used)
        gpu: HIP device index (default $DREPHIP_DEVICE or 0)
        gpus: several HIP devices (count, list or "0,1,..."; default
            $DREPHIP_DEVICES): sketch shards and all-pairs row ranges run on
            all of them from this process, one host thread per device
        write_sketches: write the .msh files (default True)
        write_table: also write MASH_table.tsv like `mash dist` (default False)
        ingest: 'host' (default; CPU threads parse and pack the FASTA files) or
            'device' (the GPU does, from the raw text); the same result.
            Anything else raises ValueError, also on a dry run

    Returns:
        Mdb DataFrame [genome1, genome2, dist, similarity]
    """
    _check_ingest(kwargs)
    MASH_folder = os.path.join(data_folder, 'MASH_files/')
    if kwargs.get('dry', False):
        table = MASH_folder + 'MASH_table.tsv'
        print("# drep_amd: dry run -- would sketch %d genomes and run all-pairs on HIP device %s"
              % (len(Bdb), kwargs.get('gpu', os.environ.get('DREPHIP_DEVICE', 0))))
        return _parse_mash_table(table, Bdb)

    STAGE_TIMES.clear()
    cm = all_vs_all_MASH_condensed(Bdb, data_folder, **kwargs)
    if kwargs.get('write_table', False):
        with _Stage('mash_table_s'):
            write_mash_table(MASH_folder + 'MASH_table.tsv', cm)
    with _Stage('mdb_s'):
        Mdb = mdb_from_condensed(cm.names, cm.common, cm.denom, cm.nhash, cm.s,
                                 threads=int(kwargs.get('processors', 6)))

    # Filter out those genomes that are not in Bdb (reference 586-594).  When
    # every sketched genome is in Bdb (the drop-in sketches Bdb's own genomes)
    # the block is the identity: no row is dropped and the categories already
    # are the sorted names, ordered (mdb_from_condensed) -- skip its 10^6-row
    # isin passes
    genomes = Bdb['genome'].unique()
    if set(cm.names).issubset(set(genomes)):
        return Mdb
    Mdb = Mdb[Mdb['genome1'].isin(genomes)]
    Mdb = Mdb[Mdb['genome2'].isin(genomes)]
    for g in ['genome1', 'genome2']:
        Mdb[g] = Mdb[g].cat.remove_unused_categories()
        Mdb[g] = Mdb[g].cat.reorder_categories(sorted((Mdb[g].unique())), ordered=True)
    return Mdb


def _parse_mash_table(file, Bdb):
    """The reference's TSV -> Mdb parse (d_cluster.py:575-596)."""
    iniCols = ['genome1', 'genome2', 'dist', 'p', 'kmers']
    uCols = ['genome1', 'genome2', 'dist']
    dTypes = {'genome1': 'category', 'genome2': 'category', 'dist': np.float32}
    Mdb = pd.read_csv(file, names=iniCols, usecols=uCols, dtype=dTypes, sep='\t')
    Mdb['genome1'] = Mdb['genome1'].apply(_get_genome_name_from_fasta)
    Mdb['genome2'] = Mdb['genome2'].apply(_get_genome_name_from_fasta)
    Mdb['similarity'] = 1 - Mdb['dist']
    genomes = Bdb['genome'].unique()
    Mdb = Mdb[Mdb['genome1'].isin(genomes)]
    Mdb = Mdb[Mdb['genome2'].isin(genomes)]
    for g in ['genome1', 'genome2']:
        Mdb[g] = Mdb[g].astype('category').cat.remove_unused_categories()
        Mdb[g] = Mdb[g].cat.reorder_categories(sorted((Mdb[g].unique())), ordered=True)
    return Mdb


def mash_pvalue(common: np.ndarray, len_r: np.ndarray, len_q: np.ndarray, s: int,
                k: int = MASH_K) -> np.ndarray:
    """Mash's p-value column (binomial upper tail; Mash uses GSL's
    gsl_cdf_binomial_Q, restated with scipy): 1 if common == 0, else
    Q(common-1; r, trunc(min(M, s)))."""
    from scipy.stats import binom
    kspace = 4.0 ** k
    px = 1.0 / (1.0 + kspace / np.asarray(len_r, dtype=np.float64))
    py = 1.0 / (1.0 + kspace / np.asarray(len_q, dtype=np.float64))
    r = px * py / (px + py - px * py)
    M = kspace * (px + py) / (1.0 + r)
    n = np.floor(np.minimum(M, s))
    c = np.asarray(common, dtype=np.float64)
    p = binom.sf(c - 1, n, r)
    return np.where(c == 0, 1.0, p)


def mash_pvalue_device(common: np.ndarray, len_a: np.ndarray, len_b: np.ndarray, s: int, gpu: int = 0) -> np.ndarray:
    """mash_pvalue on the GPU (libdrephip drephip_pvalue_records, kernel
    k_pvalue_records): Mash's own arithmetic restated with IEEE operations
    only, bit for bit _lib.pvalue_eval; against mash_pvalue (scipy) the values
    agree to about 1e-12 relative, and values below 2^-1022 are 0.0."""
    common = np.ascontiguousarray(common, dtype=np.uint32).reshape(-1)
    n = len(common)
    if n == 0:
        return np.zeros(0, dtype=np.float64)
    if int(common.max()) > s:
        raise ValueError("common must not exceed s")
    rec = np.empty((n, 4), dtype=np.uint32)
    rec[:, 0] = rec[:, 1] = np.arange(n, dtype=np.uint32)
    rec[:, 2] = common
    rec[:, 3] = s
    la = np.broadcast_to(np.asarray(len_a, dtype=np.uint64).reshape(-1), (n,))
    lb = np.broadcast_to(np.asarray(len_b, dtype=np.uint64).reshape(-1), (n,))
    with _lib.Context(device=gpu, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
        return ctx.pvalue_records(rec, la, lb)


_CMIN_CACHE = {}


def min_common_table(max_dist: float, s: int, k: int = MASH_K) -> np.ndarray:
    """Mash's -d <max_dist> as a rule on counts: uint32 [s + 1], entry d the
    smallest common with float64 Mash distance (drephip_distance_lut at
    denominator d) <= max_dist, or d + 1 when no count reaches it.  A pair
    passes when common >= table[denom]: the comparison mdb_from_rect makes,
    bit for bit, since the distance falls as common grows.  Entry 0 (two empty
    sketches, distance 0) is 0."""
    key = (float(max_dist), int(s), int(k))
    if key not in _CMIN_CACHE:
        out = np.empty(s + 1, dtype=np.uint32)
        out[0] = 0 if 0.0 <= key[0] else 1
        for d in range(1, s + 1):
            ok = np.nonzero(_lib.distance_lut(d, k) <= key[0])[0]
            out[d] = ok[0] if len(ok) else d + 1
        _CMIN_CACHE[key] = out
    return _CMIN_CACHE[key].copy()


def _pvalue_by(how: str, common, len_a, len_b, s: int, gpu: int = 0) -> np.ndarray:
    """The p-values by 'host' (scipy, mash_pvalue), 'device' (the GPU kernel)
    or 'eval' (the kernel's arithmetic on the host, no GPU)."""
    if how == 'host':
        return mash_pvalue(common, len_a, len_b, s)
    if how == 'device':
        return mash_pvalue_device(common, len_a, len_b, s, gpu)
    if how == 'eval':
        return _lib.pvalue_eval(common, len_a, len_b, s, MASH_K)
    raise ValueError("pvalue must be 'host', 'device' or 'eval', got %r" % (how,))


def write_mash_table(path: str, cm: CondensedMash, threads: int = 0, pvalue: str = 'host', gpu: int = 0) -> None:
    """MASH_table.tsv as `mash dist ALL ALL` prints it (d_cluster.py:570-572):
    reference, query, %g distance, %g p-value, common/denom; outer loop over
    queries.  N^2 lines (10^8 at 10^4 genomes).  Distances (per-denominator
    tables) and p-values are computed once per unordered pair -- both are
    symmetric in (reference, query) -- and only for pairs sharing a hash (the
    p-value of c = 0 is 1); libdrephip formats the text on `threads` host
    threads (drephip_write_mash_table).  pvalue: 'host' (scipy, the
    default), 'device' (the p-values on GPU `gpu`, mash_pvalue_device) or
    'eval' (the same arithmetic on the host)."""
    N = len(cm.names)
    common = np.asarray(cm.common, dtype=np.uint16)
    denom = np.asarray(cm.denom, dtype=np.uint16)
    length = np.asarray(cm.length, dtype=np.float64 if pvalue == 'host' else np.uint64)
    dist = np.empty(len(common), dtype=np.float64)
    for d in np.unique(denom):
        sel = denom == d
        lut = _lib.distance_lut(int(d), MASH_K) if d else np.zeros(1)
        dist[sel] = lut[common[sel]]
    pval = np.ones(len(common), dtype=np.float64)
    nz = np.nonzero(common)[0]
    if len(nz):
        iu, ju = _condensed_ij(nz, N)
        pval[nz] = _pvalue_by(pvalue, common[nz], length[iu], length[ju], cm.s, gpu)
    self_count = np.minimum(np.asarray(cm.nhash, dtype=np.int64), cm.s).astype(np.uint16)
    self_pval = _pvalue_by(pvalue, self_count, length, length, cm.s, gpu)
    full = bool((denom == cm.s).all())
    _lib.write_mash_table(path, list(cm.locations), common, None if full else denom, cm.s, dist, pval,
                          self_count, self_pval, threads)


def _condensed_ij(t: np.ndarray, N: int):
    """(i, j), i < j, of condensed indices t (scipy squareform order)."""
    t = np.asarray(t, dtype=np.int64)
    Mf = 2.0 * N - 1.0
    i = np.floor((Mf - np.sqrt(np.maximum(Mf * Mf - 8.0 * t, 0.0))) / 2.0).astype(np.int64)
    i = np.clip(i, 0, max(N - 2, 0))
    for _ in range(2):
        i = np.where(i * N - i * (i + 1) // 2 > t, i - 1, i)
        i = np.where((i + 1) * N - (i + 1) * (i + 2) // 2 <= t, i + 1, i)
    j = t - (i * N - i * (i + 1) // 2) + i + 1
    return i, j


# ------------------------------------------------------ primary clustering
def _primary_cdb(labels, names) -> pd.DataFrame:
    """Cdb [primary_cluster, genome]: fcluster labels in the pivot's genome
    order (what dRep's _gen_cdb_from_fclust + rename give,
    d_cluster.py:463-479, 623)."""
    return pd.DataFrame({'primary_cluster': np.asarray(labels), 'genome': list(names)})


def _pivot_dist(db: pd.DataFrame) -> pd.DataFrame:
    """db.pivot(index="genome1", columns="genome2", values="dist")
    (d_cluster.py:620; keyword form -- pandas >= 2 rejects the positional one),
    the same DataFrame, filled by libdrephip on category codes
    (drephip_pivot_scan / drephip_pivot_fill) when the table is what the
    Mash step produces: both genome columns categorical over one sorted list
    of names (the reference's parse sorts them, d_cluster.py:591-594) and a
    float32 dist.  Index and columns are then the names that occur, in
    category order, as CategoricalIndex of the column's dtype (pandas' pivot of
    a categorical); missing cells NaN; a cell named twice raises pandas'
    ValueError.  Any other table goes through pandas itself."""
    g1, g2, dist = db['genome1'], db['genome2'], db['dist']
    fast = (isinstance(g1.dtype, pd.CategoricalDtype) and isinstance(g2.dtype, pd.CategoricalDtype)
            and g1.dtype.categories.equals(g2.dtype.categories) and g1.dtype.ordered == g2.dtype.ordered
            and g1.dtype.categories.is_monotonic_increasing and dist.dtype == np.float32 and len(db) > 0)
    if fast:
        c1 = g1.cat.codes.to_numpy()
        c2 = g2.cat.codes.to_numpy()
        fast = c1.dtype == c2.dtype and c1.dtype in (np.int8, np.int16, np.int32)
    if not fast:
        return db.pivot(index="genome1", columns="genome2", values="dist")
    ncat = len(g1.dtype.categories)
    try:
        p1, p2, period = _lib.pivot_scan(c1, c2, ncat)
    except _lib.DrepHipError:                   # a missing genome (NaN category): pandas' own handling
        return db.pivot(index="genome1", columns="genome2", values="dist")
    if not (p1.all() and p2.all()):
        # a category unused in either column: pandas' unstack then orders the
        # names in a way of its own (not the category order) -- leave it to pandas
        return db.pivot(index="genome1", columns="genome2", values="dist")
    pos1 = np.where(p1, np.cumsum(p1) - 1, -1).astype(np.int32)
    pos2 = np.where(p2, np.cumsum(p2) - 1, -1).astype(np.int32)
    n1, n2 = int(p1.sum()), int(p2.sum())
    try:
        M = _lib.pivot_fill(c1, c2, pos1, pos2, dist.to_numpy(), n1, n2, period)
    except _lib.DrepHipError as e:
        raise ValueError("Index contains duplicate entries, cannot reshape") from e

    def index(present, name, dtype):
        return pd.CategoricalIndex(pd.Categorical.from_codes(np.nonzero(present)[0], dtype=dtype), name=name)
    return pd.DataFrame(M, index=index(p1, "genome1", g1.dtype), columns=index(p2, "genome2", g2.dtype), copy=False)


def _linkage_gpu(kwargs) -> Optional[int]:
    """The HIP device of the primary linkage: kwargs `gpu` (None = scipy on
    the host), else $DREPHIP_DEVICE, else 0."""
    if 'gpu' in kwargs:
        return None if kwargs['gpu'] is None else int(kwargs['gpu'])
    return int(os.environ.get('DREPHIP_DEVICE', 0))


def _square_linkage(M: np.ndarray, method: str, gpu: int) -> np.ndarray:
    """scipy.cluster.hierarchy.linkage(squareform(M), method) on the GPU (Z
    bit-identical): float32 M through drephip_linkage_square (squareform's and
    linkage's checks on the device), float64 M through squareform +
    drephip_linkage.  A failed check raises scipy's ValueError.  Ward on a
    negative distance, which the GPU refuses (scipy's ward gives NaN rows
    there), is run by scipy, so the result is still the reference's."""
    with _lib.Context(device=gpu, k=MASH_K, s=1, seed=MASH_SEED) as ctx:
        try:
            if M.dtype == np.float32:
                return ctx.linkage_square(M, method)
            y = ssd.squareform(np.asarray(M, dtype=np.float64))
            if not np.all(np.isfinite(y)):
                raise ValueError("The condensed distance matrix must contain only finite values.")
            return ctx.linkage(y, method)
        except _lib.DrepHipError as e:
            msg = _lib.lib().drephip_last_error().decode("utf-8", "replace")
            if msg in ("Distance matrix 'X' must be symmetric.", "Distance matrix 'X' diagonal must be zero.",
                       "The condensed distance matrix must contain only finite values."):
                raise ValueError(msg) from e
            if method == 'ward' and "ward needs distances >= 0" in msg:
                return scipy.cluster.hierarchy.linkage(ssd.squareform(M), method=method)
            raise


def cluster_mash_database(db, **kwargs):
    """
    From a Mash database, cluster and return Cdb (reference
    drep/d_cluster.py:598-630, with its cluster_hierarchical 429-461).  Same
    in-place update of db['dist'] from db['similarity'] as the reference, the
    same pivot (pandas' DataFrame, filled from the category codes by
    libdrephip: _pivot_dist) and the same linkage of its squareform -- run on
    the GPU for single / complete / average / weighted / ward (scipy's
    algorithms restated, Z bit-identical; drephip_linkage_square), by scipy for
    the other methods (centroid, median) and for ward on a negative distance --
    so Cdb, linkage and linkage_db equal the reference's.

    Keyword arguments:
        clusterAlg: how to cluster database (default = single)
        P_ani: threshold to cluster at (default = 0.9)
        gpu: HIP device of the linkage (default $DREPHIP_DEVICE or 0); None
            runs scipy's linkage on the host, as the reference does

    Returns:
        list: [Cdb, [linkage, linkage_db, arguments]]
    """
    logging.debug('Clustering MASH database')
    method = kwargs.get('clusterAlg', 'single')
    cutoff = 1 - kwargs.get('P_ani', .9)
    with _Stage('dist_update_s'):
        db['dist'] = 1 - db['similarity']
    with _Stage('pivot_s'):
        linkage_db = _pivot_dist(db)
    gpu = _linkage_gpu(kwargs)
    M = np.asarray(linkage_db)
    link = _Stage('linkage_s')
    link.__enter__()
    try:
        if (gpu is not None and method in GPU_DENSE_LINKAGE_METHODS and M.ndim == 2 and M.shape[0] == M.shape[1]
                and M.shape[0] >= 2 and M.dtype in (np.float32, np.float64)):
            linkage = _square_linkage(M, method, gpu)
        else:
            y = ssd.squareform(M)       # raises unless symmetric with a zero diagonal
            linkage = scipy.cluster.hierarchy.linkage(y, method=method)
    except ValueError as e:
        if "symmetric" in str(e) or "diagonal" in str(e) or "square" in str(e):    # squareform's checks
            logging.error("The database passed in is not symmetrical!")
        raise
    link.__exit__()
    labels = scipy.cluster.hierarchy.fcluster(linkage, cutoff, criterion='distance')
    Cdb = _primary_cdb(labels, linkage_db.columns)
    arguments = {'linkage_method': method, 'linkage_cutoff': cutoff, 'comparison_algorithm': 'MASH'}
    return Cdb, [linkage, linkage_db, arguments]


def _linkage_values(common: np.ndarray, denom: np.ndarray) -> np.ndarray:
    """float64 linkage input for (common, denom) pairs, bit-identical to what
    the reference feeds scipy: dist32 (the %g / read_csv path) -> 1 - (1 -
    dist32) in float32 (d_cluster.py:584, 619) -> float64."""
    d32 = mash_distance_float32(common, denom)
    one = np.float32(1)
    return (one - (one - d32)).astype(np.float32).astype(np.float64)


def condensed_cluster_distances(cm: CondensedMash) -> np.ndarray:
    """float64 condensed linkage input, rows/columns in sorted-name order (the
    pivot's order)."""
    N = len(cm.names)
    after = _linkage_values(cm.common, cm.denom)
    order = np.argsort(np.array(cm.names, dtype=object), kind='stable')
    if np.all(order == np.arange(N)):
        return after
    M = ssd.squareform(after, checks=False)[np.ix_(order, order)]
    return ssd.squareform(M, checks=False).astype(np.float64)


def linkage_tables(denominators: np.ndarray, s: int):
    """(lut, lut_off) for drephip_linkage_counts_device: for every denominator
    d that occurs, lut[lut_off[d] + c] = linkage input value of (c, d)."""
    lut_off = np.full(s + 1, -1, dtype=np.int32)
    parts, pos = [], 0
    for d in np.unique(np.asarray(denominators)):
        d = int(d)
        c = np.arange(d + 1)
        parts.append(_linkage_values(c, np.full(d + 1, d)))
        lut_off[d] = pos
        pos += d + 1
    lut = np.concatenate(parts) if parts else np.zeros(1)
    return lut, lut_off


def linkage_order(names: Sequence[str]) -> np.ndarray:
    """perm[i] = row of genome i in the linkage input (sorted names, as the
    reference's pivot orders them)."""
    order = np.argsort(np.array(names, dtype=object), kind='stable')
    perm = np.empty(len(names), dtype=np.uint32)
    perm[order] = np.arange(len(names), dtype=np.uint32)
    return perm


# the methods with a sparse form (cluster_mash_sparse), and those of the dense
# GPU chain: ward's update moves a pair at 1.0, so it has no sparse form
GPU_LINKAGE_METHODS = ('single', 'complete', 'average', 'weighted')
GPU_DENSE_LINKAGE_METHODS = GPU_LINKAGE_METHODS + ('ward',)


def cluster_mash_condensed(cm: CondensedMash, **kwargs):
    """Primary clustering straight from the condensed result (no N^2 Mdb):
    same linkage input as cluster_mash_database builds via pivot+squareform.

    The linkage runs on the GPU (libdrephip drephip_linkage_counts_device:
    scipy's nn_chain / MST restated, Z bit-identical; the n x n matrix is
    built in HBM from the counts; ward always on that dense chain) on device
    `gpu` (default $DREPHIP_DEVICE or 0); other methods (centroid, median), or
    gpu=None, use scipy on the host."""
    P_Lmethod = kwargs.get('clusterAlg', 'single')
    P_Lcutoff = 1 - kwargs.get('P_ani', .9)
    gpu = _linkage_gpu(kwargs)
    names = sorted(cm.names)
    N = len(cm.names)
    if gpu is not None and P_Lmethod in GPU_DENSE_LINKAGE_METHODS and N >= 2:
        import torch
        dev = torch.device('cuda', int(gpu))
        lut, lut_off = linkage_tables(cm.denom, cm.s)
        d_c = torch.from_numpy(np.ascontiguousarray(cm.common, dtype=np.uint16).view(np.int16)).to(dev)
        full = bool((cm.denom == cm.s).all())
        d_d = None if full else torch.from_numpy(np.ascontiguousarray(cm.denom, dtype=np.uint16).view(np.int16)).to(dev)
        torch.cuda.synchronize(dev)
        with _lib.Context(device=int(gpu), k=MASH_K, s=cm.s, seed=MASH_SEED) as ctx:
            linkage = ctx.linkage_counts_device(d_c.data_ptr(), None if d_d is None else d_d.data_ptr(), N,
                                                linkage_order(cm.names), lut, lut_off, P_Lmethod)
    else:
        arr = condensed_cluster_distances(cm)
        linkage = scipy.cluster.hierarchy.linkage(arr, method=P_Lmethod)
    fclust = scipy.cluster.hierarchy.fcluster(linkage, P_Lcutoff, criterion='distance')
    Cdb = _primary_cdb(fclust, names)
    arguments = {'linkage_method': P_Lmethod, 'linkage_cutoff': P_Lcutoff,
                 'comparison_algorithm': 'MASH'}
    return Cdb, [linkage, None, arguments]


# ------------------------------------------------------- the sparse pipeline
# Beyond ~2x10^5 genomes the condensed triangle itself no longer fits (1 TB per
# array at 10^6): the all-pairs step then lists only the pairs that share a
# hash (libdrephip drephip_allpairs_sparse), and everything downstream works on
# that list -- a pair that is not listed has common 0, Mash distance 1.
@dataclass
class SparseMash:
    names: List[str]
    locations: List[str]
    i: np.ndarray          # uint32, i < j, sorted by (i, j)
    j: np.ndarray          # uint32
    common: np.ndarray     # uint16, > 0
    denom: np.ndarray      # uint16
    nhash: np.ndarray
    length: np.ndarray
    s: int
    pval: Optional[np.ndarray] = None   # float64 per listed pair (all_vs_all_MASH_sparse with max_p / max_dist)


def sparse_allpairs(hashes: np.ndarray, nhash: np.ndarray, s: int, devices: Sequence[int] = (0,)):
    """(i, j, common, denom) of the pairs sharing a hash, sorted by (i, j).
    With several devices the rows are split as condensed_allpairs splits them
    (parallel.row_partition), one context and host thread per device; a row
    range's list holds the pairs whose smaller genome is one of its rows, so
    the ranges' lists are concatenated in order."""
    N = len(nhash)
    parts = row_partition(N, len(devices))

    def run(k, dev):
        r0, r1 = parts[k]
        if r1 <= r0:
            return tuple(np.zeros(0, t) for t in (np.uint32, np.uint32, np.uint16, np.uint16))
        with _lib.Context(device=dev, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
            return ctx.allpairs_sparse(hashes, nhash, r0, r1)
    res = _on_devices(list(devices), run) if N >= 2 else []
    if not res:
        return tuple(np.zeros(0, t) for t in (np.uint32, np.uint32, np.uint16, np.uint16))
    return tuple(np.concatenate([r[k] for r in res]) for k in range(4))


def _check_sig(max_p, max_dist):
    if max_p is not None and not (0 <= float(max_p) <= 1):
        raise ValueError("max_p must be in [0, 1]")
    if max_dist is not None and not (0 <= float(max_dist) < 1):
        raise ValueError("max_dist must be in [0, 1): the record form lists only pairs that share a hash")


def sparse_allpairs_sig(hashes: np.ndarray, nhash: np.ndarray, length: np.ndarray, s: int,
                        max_p: Optional[float] = None, max_dist: Optional[float] = None,
                        devices: Sequence[int] = (0,)):
    """sparse_allpairs with Mash's p-value per pair and its -v <max_p> /
    -d <max_dist> filters applied on the GPU, before the list comes to the host
    (libdrephip drephip_allpairs_sparse_sig): (i, j, common, denom, p), sorted
    by (i, j).  Rows split over the devices as sparse_allpairs splits them."""
    _check_sig(max_p, max_dist)
    N = len(nhash)
    parts = row_partition(N, len(devices))
    cmin = None if max_dist is None else min_common_table(max_dist, s)
    mp = 1.0 if max_p is None else float(max_p)
    none = tuple(np.zeros(0, t) for t in (np.uint32, np.uint32, np.uint16, np.uint16, np.float64))

    def run(k, dev):
        r0, r1 = parts[k]
        if r1 <= r0:
            return none
        with _lib.Context(device=dev, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
            return ctx.allpairs_sparse_sig(hashes, nhash, length, mp, cmin, r0, r1)[:5]
    res = _on_devices(list(devices), run) if N >= 2 else []
    if not res:
        return none
    return tuple(np.concatenate([r[k] for r in res]) for k in range(5))


def all_vs_all_MASH_sparse(Bdb, data_folder, max_p=None, max_dist=None, **kwargs) -> SparseMash:
    """Sketch (or load cached sketches) and run the sparse HIP all-pairs: the
    pairs that share a hash instead of the condensed triangle (reference
    drep/d_cluster.py:481-596 keeps every pair as a row of MASH_table.tsv).
    Same keyword arguments as all_vs_all_MASH_condensed.

    max_p / max_dist (default None: every pair that shares a hash, as before):
    Mash's -v and -d.  With either one the p-values are computed on the GPU,
    only the pairs with p <= max_p and float64 Mash distance <= max_dist are
    listed, and the result's pval holds their p-values."""
    sk = sketch_genomes(Bdb, data_folder, **kwargs)
    if max_p is None and max_dist is None:
        with _Stage('allpairs_s'):
            i, j, common, denom = sparse_allpairs(sk.hashes, sk.nhash, sk.s, _devices(kwargs))
        return SparseMash(sk.names, sk.locations, i, j, common, denom, sk.nhash, sk.length, sk.s)
    with _Stage('allpairs_s'):
        i, j, common, denom, p = sparse_allpairs_sig(sk.hashes, sk.nhash, sk.length, sk.s, max_p, max_dist,
                                                     _devices(kwargs))
    return SparseMash(sk.names, sk.locations, i, j, common, denom, sk.nhash, sk.length, sk.s, p)


def _sparse_pairs(sm: SparseMash):
    """The listed pairs plus the pairs of two empty sketches: Mash gives those
    common = denom = 0 and distance 0 (mash_distance_float32), below 1 like
    the listed ones although they share no hash."""
    i, j = np.asarray(sm.i, dtype=np.uint32), np.asarray(sm.j, dtype=np.uint32)
    c, d = np.asarray(sm.common, dtype=np.uint16), np.asarray(sm.denom, dtype=np.uint16)
    empty = np.nonzero(np.asarray(sm.nhash) == 0)[0].astype(np.uint32)
    if len(empty) >= 2:
        a, b = np.triu_indices(len(empty), 1)
        i, j = np.concatenate([i, empty[a]]), np.concatenate([j, empty[b]])
        c = np.concatenate([c, np.zeros(len(a), np.uint16)])
        d = np.concatenate([d, np.zeros(len(a), np.uint16)])
    return i, j, c, d


def cluster_mash_sparse(sm: SparseMash, **kwargs):
    """cluster_mash_condensed from the pair list: the same Cdb and the same
    linkage Z, bit for bit (reference cluster_mash_database,
    drep/d_cluster.py:598-630).  The linkage input holds the listed pairs'
    values (_linkage_values) at the rows linkage_order gives the genomes and
    1.0 everywhere else, which is what libdrephip's sparse linkage
    (drephip_linkage_sparse: scipy's algorithm over the pairs below 1.0, on
    the host) takes."""
    P_Lmethod = kwargs.get('clusterAlg', 'single')
    P_Lcutoff = 1 - kwargs.get('P_ani', .9)
    if P_Lmethod not in GPU_LINKAGE_METHODS:
        raise ValueError("cluster_mash_sparse supports clusterAlg in %s" % (GPU_LINKAGE_METHODS,))
    names = sorted(sm.names)
    N = len(sm.names)
    i, j, c, d = _sparse_pairs(sm)
    vals = _linkage_values(c, d)
    perm = linkage_order(sm.names)
    keep = vals < 1.0
    linkage = _lib.linkage_sparse(N, perm[i[keep]], perm[j[keep]], vals[keep], P_Lmethod)
    fclust = scipy.cluster.hierarchy.fcluster(linkage, P_Lcutoff, criterion='distance') if N >= 2 \
        else np.ones(N, dtype=np.int32)
    Cdb = _primary_cdb(fclust, names)
    arguments = {'linkage_method': P_Lmethod, 'linkage_cutoff': P_Lcutoff,
                 'comparison_algorithm': 'MASH'}
    return Cdb, [linkage, None, arguments]


def mdb_from_sparse(sm: SparseMash, k: int = MASH_K) -> pd.DataFrame:
    """The rows of the Mdb all_vs_all_MASH returns (drep/d_cluster.py:575-596)
    whose dist is below 1, the diagonal included: same row order (and index:
    row t = q N + r of the full table is genome1 = genome r, genome2 = genome
    q), dtypes, ordered categories and float32 dist / similarity bits as
    mdb_from_condensed(...)[dist < 1], built from the same float32 tables."""
    N = len(sm.names)
    i, j, c, d = _sparse_pairs(sm)
    dens = np.unique(d) if len(d) else np.array([sm.s])
    lut32, lut_off = float32_tables(dens, sm.s, k)
    dp = lut32[lut_off[d.astype(np.int64)].astype(np.int64) + c.astype(np.int64)] if len(d) \
        else np.zeros(0, np.float32)
    diag = np.arange(N, dtype=np.int64)
    r = np.concatenate([i.astype(np.int64), j.astype(np.int64), diag])
    q = np.concatenate([j.astype(np.int64), i.astype(np.int64), diag])
    dist = np.concatenate([dp, dp, np.zeros(N, np.float32)]).astype(np.float32)
    t = q * N + r
    order = np.argsort(t, kind='stable')
    order = order[dist[order] < 1]
    dist = dist[order]
    cats = sorted(set(sm.names))
    dtype = pd.CategoricalDtype(cats, ordered=True)
    code_t = pd.Categorical([], dtype=dtype).codes.dtype
    pos = {n: x for x, n in enumerate(cats)}
    codes = np.array([pos[n] for n in sm.names], dtype=code_t)
    return pd.DataFrame({'genome1': pd.Categorical.from_codes(codes[r[order]], dtype=dtype, validate=False),
                         'genome2': pd.Categorical.from_codes(codes[q[order]], dtype=dtype, validate=False),
                         'dist': dist, 'similarity': np.float32(1) - dist}, index=t[order], copy=False)


# ------------------------------------------------- query against reference
# `mash dist <reference.msh> <query.msh>`, the two-file form of the call at
# drep/d_cluster.py:569-573: new genomes against a sketch database that an
# earlier all_vs_all_MASH run left behind, without redoing reference x reference.
@dataclass
class RectMash:
    qnames: List[str]          # queries (basename), Qdb order
    qlocations: List[str]
    rnames: List[str]          # references (basename), order of the .msh file
    rlocations: List[str]      # their names as the .msh file holds them
    common: Optional[np.ndarray]   # uint16 [Q, N] (dense form), else None
    denom: Optional[np.ndarray]    # uint16 [Q, N]
    q: Optional[np.ndarray]        # record form: uint32 query rows, sorted by (q, r); else None
    r: Optional[np.ndarray]        # uint32 reference rows
    rec_common: Optional[np.ndarray]   # uint16, > 0
    rec_denom: Optional[np.ndarray]    # uint16
    qnhash: np.ndarray
    rnhash: np.ndarray
    qlength: np.ndarray
    rlength: np.ndarray
    s: int
    pval: Optional[np.ndarray] = None  # record form with pvalue / max_p: float64 per record


def _query_ranges(Q: int, n: int) -> List[tuple]:
    """Q query rows in n contiguous ranges of near-equal size (every row of
    the rectangle costs the same: N pairs)."""
    return [(Q * k // n, Q * (k + 1) // n) for k in range(n)]


def rect_allpairs(qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray, s: int,
                  devices: Sequence[int] = (0,)):
    """(common[Q, N], denom[Q, N]) of `mash dist <reference> <query>`: every
    query sketch against every reference sketch (libdrephip
    drephip_dist_rect).  With several devices the query rows are split into
    contiguous ranges, one context and host thread per device, each writing
    its own rows of the host buffers, as condensed_allpairs splits the
    triangle.  denom is always filled.  ValueError for mismatched dtypes or
    shapes, before any GPU call."""
    qhashes, qnhash, rhashes, rnhash = _lib.rect_arrays(qhashes, qnhash, rhashes, rnhash, s)
    Q, N = len(qnhash), len(rnhash)
    common = np.zeros((Q, N), dtype=np.uint16)
    denom = np.zeros((Q, N), dtype=np.uint16)
    parts = _query_ranges(Q, len(devices))

    def run(k, dev):
        a, b = parts[k]
        if b <= a:
            return
        with _lib.Context(device=dev, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
            ctx.dist_rect(qhashes, qnhash, rhashes, rnhash, a, b, common[a:b], denom[a:b])
    if Q and N:
        _on_devices(list(devices), run)
    return common, denom


def rect_allpairs_sparse(qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray, s: int,
                         devices: Sequence[int] = (0,)):
    """(q, r, common, denom) of the (query, reference) pairs sharing a hash,
    sorted by (q, r) (libdrephip drephip_dist_rect_sparse); query rows split
    over the devices as rect_allpairs splits them."""
    qhashes, qnhash, rhashes, rnhash = _lib.rect_arrays(qhashes, qnhash, rhashes, rnhash, s)
    Q, N = len(qnhash), len(rnhash)
    none = tuple(np.zeros(0, t) for t in (np.uint32, np.uint32, np.uint16, np.uint16))
    parts = _query_ranges(Q, len(devices))

    def run(k, dev):
        a, b = parts[k]
        if b <= a:
            return none
        with _lib.Context(device=dev, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
            return ctx.dist_rect_sparse(qhashes, qnhash, rhashes, rnhash, a, b)
    if not (Q and N):
        return none
    res = _on_devices(list(devices), run)
    return tuple(np.concatenate([x[k] for x in res]) for k in range(4))


def rect_allpairs_sparse_sig(qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray,
                             qlength: np.ndarray, rlength: np.ndarray, s: int, max_p: Optional[float] = None,
                             max_dist: Optional[float] = None, devices: Sequence[int] = (0,)):
    """rect_allpairs_sparse with Mash's p-value per pair and its -v <max_p> /
    -d <max_dist> filters applied on the GPU, before the list comes to the host
    (libdrephip drephip_dist_rect_sparse_sig): (q, r, common, denom, p), sorted
    by (q, r)."""
    _check_sig(max_p, max_dist)
    qhashes, qnhash, rhashes, rnhash = _lib.rect_arrays(qhashes, qnhash, rhashes, rnhash, s)
    Q, N = len(qnhash), len(rnhash)
    none = tuple(np.zeros(0, t) for t in (np.uint32, np.uint32, np.uint16, np.uint16, np.float64))
    parts = _query_ranges(Q, len(devices))
    cmin = None if max_dist is None else min_common_table(max_dist, s)
    mp = 1.0 if max_p is None else float(max_p)

    def run(k, dev):
        a, b = parts[k]
        if b <= a:
            return none
        with _lib.Context(device=dev, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
            return ctx.dist_rect_sparse_sig(qhashes, qnhash, rhashes, rnhash, qlength, rlength, mp, cmin, a, b)[:5]
    if not (Q and N):
        return none
    res = _on_devices(list(devices), run)
    return tuple(np.concatenate([x[k] for x in res]) for k in range(5))


_MAX_SKETCH = 32767      # drephip_max_sketch(): counts and denominators are uint16


def _read_reference(path: str, kwargs):
    """The reference .msh of a query call: (names, locations, hashes, nhash,
    length, s).  It must be a k = 21, seed 42 sketch file of one sketch size,
    which is the call's s; a MASH_sketch kwarg that differs raises."""
    m = read_msh(path)
    if m.kmer != MASH_K or m.seed != MASH_SEED:
        raise ValueError("%s: reference sketches must have k = %d and seed %d, got k = %d, seed %d"
                         % (path, MASH_K, MASH_SEED, m.kmer, m.seed))
    s = int(m.sketch_size)
    if s < 1 or s > _MAX_SKETCH or any(len(ref.hashes) > s for ref in m.references):
        raise ValueError("%s: reference sketches must share one sketch size in 1..%d" % (path, _MAX_SKETCH))
    if 'MASH_sketch' in kwargs and int(kwargs['MASH_sketch']) != s:
        raise ValueError("MASH_sketch = %s, but the reference %s was sketched with s = %d"
                         % (kwargs['MASH_sketch'], path, s))
    N = len(m.references)
    hashes = np.full((N, s), np.iinfo(np.uint64).max, dtype=np.uint64)
    nhash = np.zeros(N, dtype=np.uint32)
    length = np.zeros(N, dtype=np.uint64)
    for i, ref in enumerate(m.references):
        n = len(ref.hashes)
        hashes[i, :n] = ref.hashes
        nhash[i] = n
        length[i] = ref.length
    locations = [ref.name for ref in m.references]
    return [_get_genome_name_from_fasta(x) for x in locations], locations, hashes, nhash, length, s


def _rect_distance64(common: np.ndarray, denom: np.ndarray, k: int = MASH_K) -> np.ndarray:
    """float64 Mash distance per (common, denom) (drephip_distance_lut)."""
    common, denom = np.asarray(common), np.asarray(denom)
    out = np.zeros(common.shape, dtype=np.float64)       # denominator 0 (two empty sketches): 0
    for d in np.unique(denom):
        if int(d) == 0:
            continue
        sel = denom == d
        out[sel] = _lib.distance_lut(int(d), k)[common[sel]]
    return out


def _query_inputs(Qdb, data_folder, reference, max_dist, kwargs):
    """What every query-against-reference call starts from: the reference
    sketches (_read_reference's tuple), the queries' SketchSet -- sketched or
    loaded from their cache in kwargs['query_folder'] at the reference's s --
    and the devices.  Checks ingest and max_dist first."""
    _check_ingest(kwargs)
    if max_dist is not None and not (0 <= float(max_dist) < 1):
        raise ValueError("max_dist must be in [0, 1): the record form lists only pairs that share a hash")
    if reference is None:
        reference = os.path.join(data_folder, 'MASH_files', 'ALL.msh')
    ref = _read_reference(reference, kwargs)
    qfolder = kwargs.get('query_folder', os.path.join(data_folder, 'MASH_query'))
    _check_sig(kwargs.get('max_p', None), None)
    skw = {k: v for k, v in kwargs.items()
           if k not in ('query_folder', 'max_dist', 'max_p', 'pvalue', 'write_table')}
    skw['MASH_sketch'] = ref[5]
    sk = sketch_genomes(Qdb, qfolder, **skw)
    return ref, sk, _devices(kwargs)


def query_vs_MASH_rect(Qdb, data_folder, reference=None, **kwargs) -> RectMash:
    """The genomes of Qdb against a reference sketch file: the counts behind
    `mash dist <reference.msh> <query.msh>` (the two-file form of
    drep/d_cluster.py:569-573).

    reference: a .msh path; default <data_folder>/MASH_files/ALL.msh, the file
    every earlier all_vs_all_MASH run left there.  It must hold k = 21, seed 42
    sketches of one size, which becomes the call's s (a differing MASH_sketch
    kwarg raises ValueError).  The queries are sketched (or loaded from their
    cache) by sketch_genomes into kwargs['query_folder'] (default
    <data_folder>/MASH_query), so <data_folder>/MASH_files is never modified.
    max_dist (default None: the dense Q x N form): the record form, only the
    pairs that share a hash.  max_p (default None), Mash's -v: selects the
    record form as max_dist does; pvalue=True with either: the records carry
    their p-values (the result's pval).  With max_p or pvalue the record form
    runs drephip_dist_rect_sparse_sig: the p-values are computed on the GPU and
    the records above max_p, or beyond max_dist, are dropped there, before the
    list comes to the host.  write_table=<path> (dense form only): the text of
    `mash dist <reference.msh> <query.msh>` written by write_mash_table_rect.
    gpu, gpus, processors and ingest as in all_vs_all_MASH."""
    max_dist, max_p = kwargs.get('max_dist', None), kwargs.get('max_p', None)
    want_p = bool(kwargs.get('pvalue', False)) or max_p is not None
    table = kwargs.get('write_table', None)
    record_form = max_dist is not None or max_p is not None
    if table is not None and record_form:
        raise ValueError("write_table needs the dense form: no max_dist, no max_p")
    (rnames, rlocs, rh, rn, rlen, s), sk, devs = _query_inputs(Qdb, data_folder, reference, max_dist, kwargs)
    pval = None
    with _Stage('rect_s'):
        if not record_form:
            common, denom = rect_allpairs(sk.hashes, sk.nhash, rh, rn, s, devs)
            rec = (None, None, None, None)
        elif want_p:
            common = denom = None
            rec = rect_allpairs_sparse_sig(sk.hashes, sk.nhash, rh, rn, sk.length, rlen, s, max_p, max_dist, devs)
            pval = rec[4]
        else:
            common = denom = None
            rec = rect_allpairs_sparse(sk.hashes, sk.nhash, rh, rn, s, devs)
    rm = RectMash(sk.names, sk.locations, rnames, rlocs, common, denom, rec[0], rec[1], rec[2], rec[3],
                  sk.nhash, rn, sk.length, rlen, s, pval)
    if table is not None:
        with _Stage('table_s'):
            write_mash_table_rect(table, rm, kwargs.get('processors', 0) or 0, gpu=devs[0])
    return rm


def write_mash_table_rect(path: str, rm: RectMash, threads: int = 0, pvalue: str = 'device', gpu: int = 0) -> None:
    """The text `mash dist <reference.msh> <query.msh>` prints (the two-file
    form of drep/d_cluster.py:569-573) from the dense rectangle: Q x N lines,
    query outer, reference inner: reference, query, %g distance, %g p-value,
    common/denom, the names as the sketch files hold them.  No diagonal rule: a
    query that is also a reference prints its cell as computed.  The p-values
    are computed for the cells that share a hash (1 elsewhere) by `pvalue`:
    'device' (GPU `gpu`, the default), 'eval' (the same arithmetic on the host)
    or 'host' (scipy); libdrephip formats the text on `threads` host threads
    (drephip_write_mash_table_rect)."""
    if rm.common is None:
        raise ValueError("write_mash_table_rect needs the dense form of the rectangle")
    Q, N = len(rm.qnames), len(rm.rnames)
    common = np.ascontiguousarray(rm.common, dtype=np.uint16).reshape(Q, N)
    denom = np.ascontiguousarray(rm.denom, dtype=np.uint16).reshape(Q, N)
    dist = _rect_distance64(common, denom)
    pval = np.ones((Q, N), dtype=np.float64)
    q, r = np.nonzero(common)
    if len(q):
        pval[q, r] = _pvalue_by(pvalue, common[q, r], np.asarray(rm.qlength, dtype=np.uint64)[q],
                                np.asarray(rm.rlength, dtype=np.uint64)[r], rm.s, gpu)
    full = bool((denom == rm.s).all())
    _lib.write_mash_table_rect(path, list(rm.rlocations), list(rm.qlocations), common, None if full else denom, rm.s,
                               dist, pval, threads)


def mdb_from_rect(rm: RectMash, k: int = MASH_K, max_dist: Optional[float] = None, max_p: Optional[float] = None,
                  pvalue: bool = False) -> pd.DataFrame:
    """The table dRep's parse (drep/d_cluster.py:575-585) makes of `mash dist
    <reference> <queries>`: rows query-outer, reference-inner; genome1 the
    reference name, genome2 the query name, each an ordered categorical over
    that side's sorted names; dist float32 through the %g / read_csv route
    (float32_tables), similarity = 1 - dist.  The record form gives the rows of
    the listed pairs (plus empty query against empty reference, distance 0 to
    Mash), in the same order; max_dist keeps the rows whose float64 Mash
    distance (drephip_distance_lut) is <= max_dist.  max_p keeps the rows with
    p <= max_p and pvalue=True adds the float64 column p; both need the
    record form's p-values (rm.pval, from drephip_dist_rect_sparse_sig; a pair
    of two empty sketches has p = 1)."""
    Q, N = len(rm.qnames), len(rm.rnames)
    want_p = pvalue or max_p is not None
    if want_p and (rm.common is not None or rm.pval is None):
        raise ValueError("p-values need the record form computed with pvalue=True or max_p")
    p = np.asarray(rm.pval, dtype=np.float64) if want_p else None
    if rm.common is not None:
        q = np.repeat(np.arange(Q, dtype=np.int64), N)
        r = np.tile(np.arange(N, dtype=np.int64), Q)
        c = np.asarray(rm.common, dtype=np.uint16).reshape(-1)
        d = np.asarray(rm.denom, dtype=np.uint16).reshape(-1)
    else:
        q, r = np.asarray(rm.q, dtype=np.int64), np.asarray(rm.r, dtype=np.int64)
        c, d = np.asarray(rm.rec_common, dtype=np.uint16), np.asarray(rm.rec_denom, dtype=np.uint16)
        eq = np.nonzero(np.asarray(rm.qnhash) == 0)[0]
        er = np.nonzero(np.asarray(rm.rnhash) == 0)[0]
        if len(eq) and len(er):
            q = np.concatenate([q, np.repeat(eq, len(er))])
            r = np.concatenate([r, np.tile(er, len(eq))])
            c = np.concatenate([c, np.zeros(len(eq) * len(er), np.uint16)])
            d = np.concatenate([d, np.zeros(len(eq) * len(er), np.uint16)])
            order = np.argsort(q * max(N, 1) + r, kind='stable')
            if p is not None:
                p = np.concatenate([p, np.ones(len(eq) * len(er))])[order]
            q, r, c, d = q[order], r[order], c[order], d[order]
    if max_dist is not None or max_p is not None:
        keep = np.ones(len(c), dtype=bool)
        if max_dist is not None:
            keep &= _rect_distance64(c, d, k) <= float(max_dist)
        if max_p is not None:
            keep &= p <= float(max_p)
        q, r, c, d = q[keep], r[keep], c[keep], d[keep]
        p = p[keep] if p is not None else None
    dens = np.unique(d) if len(d) else np.array([rm.s])
    lut32, lut_off = float32_tables(dens, rm.s, k)
    dist = lut32[lut_off[d.astype(np.int64)].astype(np.int64) + c.astype(np.int64)].astype(np.float32) if len(d) \
        else np.zeros(0, np.float32)
    cols = {'genome1': _name_categorical(rm.rnames, r), 'genome2': _name_categorical(rm.qnames, q),
            'dist': dist, 'similarity': np.float32(1) - dist}
    if pvalue:
        cols['p'] = p
    return pd.DataFrame(cols, copy=False)


def _name_categorical(names, idx):
    """names[idx] as an ordered categorical over the sorted names."""
    cats = sorted(set(names))
    dtype = pd.CategoricalDtype(cats, ordered=True)
    code_t = pd.Categorical([], dtype=dtype).codes.dtype
    pos = {n: x for x, n in enumerate(cats)}
    codes = np.array([pos[n] for n in names], dtype=code_t)
    return pd.Categorical.from_codes(codes[idx] if len(codes) else np.zeros(0, code_t), dtype=dtype, validate=False)


def query_vs_MASH(Qdb, data_folder, reference=None, **kwargs):
    """`mash dist <reference.msh> <queries>` parsed as dRep parses its table
    (drep/d_cluster.py:569-585), with sketching and the distances on the GPU:
    the genomes of Qdb (genome, location) against the reference sketches.

    Args and keyword args as query_vs_MASH_rect.  max_dist (default None: all
    Q x N rows): only the rows whose float64 Mash distance is <= max_dist,
    from the record form of the kernel.  This is this library's own filter:
    Mash's -d option cannot be pinned here, because no Mash binary is available
    to compare against.  max_p (default None), Mash's -v: only the rows with
    p-value <= max_p; it selects the record form as max_dist does.  pvalue=True
    (with max_dist or max_p): a float64 column p.  With either one the p-values
    and both filters run on the GPU (drephip_dist_rect_sparse_sig).

    Returns:
        DataFrame [genome1 (reference), genome2 (query), dist, similarity
        (, p)], rows query-outer, reference-inner
    """
    rm = query_vs_MASH_rect(Qdb, data_folder, reference, **kwargs)
    with _Stage('mdb_s'):
        return mdb_from_rect(rm, max_dist=kwargs.get('max_dist', None), max_p=kwargs.get('max_p', None),
                             pvalue=bool(kwargs.get('pvalue', False)))


def union_condensed(cm_ref: CondensedMash, rm: RectMash, cm_query: CondensedMash) -> CondensedMash:
    """The condensed triangle of (references, then queries) from the
    references' triangle, the query x reference rectangle and the queries'
    triangle: extends a stored run by new genomes for cluster_mash_condensed
    without redoing reference x reference.  Pure numpy."""
    Nr, Nq = len(cm_ref.names), len(cm_query.names)
    if rm.common is None:
        raise ValueError("union_condensed needs the dense form of the rectangle")
    if not (cm_ref.s == rm.s == cm_query.s):
        raise ValueError("the three parts must share one sketch size")
    if list(rm.rnames) != list(cm_ref.names) or list(rm.qnames) != list(cm_query.names):
        raise ValueError("the rectangle's reference / query names must be the two triangles' names, in order")
    rc, rd = np.asarray(rm.common), np.asarray(rm.denom)
    if rc.shape != (Nq, Nr) or rd.shape != (Nq, Nr):
        raise ValueError("the rectangle must be [queries, references] = [%d, %d]" % (Nq, Nr))
    N = Nr + Nq
    out = []
    for src_ref, src_q, rect in ((cm_ref.common, cm_query.common, rc), (cm_ref.denom, cm_query.denom, rd)):
        src_ref, src_q = np.asarray(src_ref, dtype=np.uint16), np.asarray(src_q, dtype=np.uint16)
        v = np.empty(N * (N - 1) // 2, dtype=np.uint16)
        rect_t = np.ascontiguousarray(rect.T, dtype=np.uint16)       # [references, queries]
        pos = 0
        for i in range(Nr):                                          # row i: its references, then every query
            a, n = cond_start(i, Nr), Nr - 1 - i
            v[pos:pos + n] = src_ref[a:a + n]
            pos += n
            v[pos:pos + Nq] = rect_t[i]
            pos += Nq
        v[pos:] = src_q                                              # the queries' rows: their own triangle
        out.append(v)
    return CondensedMash(list(cm_ref.names) + list(cm_query.names), list(cm_ref.locations) + list(cm_query.locations),
                         out[0], out[1], np.concatenate([np.asarray(cm_ref.nhash), np.asarray(cm_query.nhash)]),
                         np.concatenate([np.asarray(cm_ref.length), np.asarray(cm_query.length)]), cm_ref.s)


# ------------------------------------------------- best hits and placement
# What a caller of `mash dist <reference.msh> <queries>` usually keeps: each
# query's nearest references, and from them the primary cluster a new genome
# falls into.  The selection runs on the GPU (drephip_dist_rect_top), so neither
# the Q x N rectangle nor the record list comes to the host.
def rect_top_hits(qhashes: np.ndarray, qnhash: np.ndarray, rhashes: np.ndarray, rnhash: np.ndarray, s: int,
                  top: int, devices: Sequence[int] = (0,)):
    """(ref int64 [Q, top], common uint16 [Q, top], denom uint16 [Q, top],
    count uint32 [Q]): per query the `top` (1..64) nearest references among
    those that share a hash with it, nearest first, ties by the smaller
    reference row (libdrephip drephip_dist_rect_top); unused slots hold ref -1.
    Query rows are split over the devices as rect_allpairs splits them."""
    qhashes, qnhash, rhashes, rnhash = _lib.rect_arrays(qhashes, qnhash, rhashes, rnhash, s)
    top = int(top)
    if not 1 <= top <= 64:
        raise ValueError("top must be in 1..64")
    Q, N = len(qnhash), len(rnhash)
    ref = np.full((Q, top), -1, dtype=np.int64)
    common = np.zeros((Q, top), dtype=np.uint16)
    denom = np.zeros((Q, top), dtype=np.uint16)
    count = np.zeros(Q, dtype=np.uint32)
    parts = _query_ranges(Q, len(devices))

    def run(k, dev):
        a, b = parts[k]
        if b <= a:
            return
        with _lib.Context(device=dev, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
            ref[a:b], common[a:b], denom[a:b], count[a:b] = ctx.dist_rect_top(qhashes, qnhash, rhashes, rnhash,
                                                                               top, a, b)
    if Q and N:
        _on_devices(list(devices), run)
    return ref, common, denom, count


def best_hits_frame(qnames: Sequence[str], rnames: Sequence[str], ref: np.ndarray, common: np.ndarray,
                    denom: np.ndarray, count: np.ndarray, s: int, k: int = MASH_K,
                    max_dist: Optional[float] = None, pval: Optional[np.ndarray] = None,
                    max_p: Optional[float] = None) -> pd.DataFrame:
    """rect_top_hits' arrays as the table query_best_hits returns (its
    docstring).  Pure pandas/numpy plus the distance tables.  pval (float64
    [Q, top]): the hits' p-values, added as column p; max_p drops the listed
    hits above it (their ranks stay as selected)."""
    ref, count = np.asarray(ref, dtype=np.int64), np.asarray(count, dtype=np.int64)
    top = ref.shape[1] if ref.ndim == 2 else 0
    listed = np.arange(top, dtype=np.int64)[None, :] < count[:, None]
    q, rank = np.nonzero(listed)                                   # query-outer, rank-inner
    r = ref[q, rank]
    c = np.asarray(common, dtype=np.uint16)[q, rank]
    d = np.asarray(denom, dtype=np.uint16)[q, rank]
    p = None if pval is None else np.asarray(pval, dtype=np.float64)[q, rank]
    if max_p is not None and p is None:
        raise ValueError("max_p needs the hits' p-values")
    if max_dist is not None or max_p is not None:
        keep = np.ones(len(c), dtype=bool)
        if max_dist is not None:
            keep &= _rect_distance64(c, d, k) <= float(max_dist)
        if max_p is not None:
            keep &= p <= float(max_p)
        q, rank, r, c, d = q[keep], rank[keep], r[keep], c[keep], d[keep]
        p = p[keep] if p is not None else None
    dens = np.unique(d) if len(d) else np.array([s])
    lut32, lut_off = float32_tables(dens, s, k)
    dist = lut32[lut_off[d.astype(np.int64)].astype(np.int64) + c.astype(np.int64)].astype(np.float32) if len(d) \
        else np.zeros(0, np.float32)
    cols = {'genome1': _name_categorical(rnames, r), 'genome2': _name_categorical(qnames, q),
            'rank': rank.astype(np.int32), 'dist': dist, 'similarity': np.float32(1) - dist, 'common': c, 'denom': d}
    if p is not None:
        cols['p'] = p
    return pd.DataFrame(cols, copy=False)


def rect_top_pvalues(ref: np.ndarray, common: np.ndarray, denom: np.ndarray, count: np.ndarray, qlength: np.ndarray,
                     rlength: np.ndarray, s: int, gpu: int = 0) -> np.ndarray:
    """Mash's p-value of every hit rect_top_hits listed, float64 [Q, top], 1.0
    in the unused slots, computed on GPU `gpu` (libdrephip
    drephip_pvalue_hits_device)."""
    with _lib.Context(device=gpu, k=MASH_K, s=s, seed=MASH_SEED) as ctx:
        return ctx.pvalue_hits(ref, common, denom, count, qlength, rlength)


def query_best_hits(Qdb, data_folder, reference=None, top=1, max_dist=None, pvalue=False, max_p=None,
                    **kwargs) -> pd.DataFrame:
    """Each genome of Qdb against a reference sketch file: its `top` (1..64)
    nearest references, selected on the GPU.

    Args and keyword args as query_vs_MASH_rect (reference, query_folder, gpu,
    gpus, processors, ingest).  Only references that share a hash with the
    query are ever listed (Mash distance < 1).  max_dist keeps the rows whose
    float64 Mash distance (drephip_distance_lut) is <= max_dist, the rule of
    mdb_from_rect.  pvalue=True adds Mash's p-value of every hit as the float64
    column p (computed on the GPU); max_p (Mash's -v; implies the column) drops
    the rows with p > max_p.  Both filters apply to the listed hits: the `top`
    nearest are selected first, so a dropped hit is not replaced by a farther
    one, and the ranks stay as selected.

    Returns:
        DataFrame [genome1 (reference), genome2 (query), rank (0-based, nearest
        first; ties by the reference's row in the .msh file), dist, similarity,
        common, denom], rows query-outer, rank-inner.  dist is float32 through
        the %g / read_csv route (float32_tables), so a row's dist and
        similarity are bit for bit those of the same pair in query_vs_MASH.
    """
    _check_sig(max_p, None)
    (rnames, _, rh, rn, rlen, s), sk, devs = _query_inputs(Qdb, data_folder, reference, max_dist, kwargs)
    with _Stage('rect_top_s'):
        ref, common, denom, count = rect_top_hits(sk.hashes, sk.nhash, rh, rn, s, top, devs)
        pval = None
        if pvalue or max_p is not None:
            pval = rect_top_pvalues(ref, common, denom, count, sk.length, rlen, s, devs[0])
    with _Stage('mdb_s'):
        return best_hits_frame(sk.names, rnames, ref, common, denom, count, s, max_dist=max_dist, pval=pval,
                               max_p=max_p)


def place_queries(hits: pd.DataFrame, Cdb: pd.DataFrame, P_ani: float = 0.9) -> pd.DataFrame:
    """Which existing primary cluster each query of a query_best_hits table
    falls into, by its listed hits.

    hits: the frame of query_best_hits; Cdb: [genome, primary_cluster] of the
    references (clusters numbered from 1, as cluster_mash_database numbers
    them).  A hit is within the threshold when its float64 Mash distance
    (drephip_distance_lut of its common / denom) is <= 1 - P_ani.

    Returns one row per query: the queries with rows in hits in the order of
    their first rows, then the queries without any hit (they have no row in
    hits, but query_best_hits keeps every query's name among genome2's
    categories):
        genome, nearest (the rank-0 reference, None without one), dist (its
        float32 dist, NaN without one), primary_cluster (that of the rank-0 hit
        when it is within the threshold, else 0), n_clusters (the distinct
        primary clusters among the listed hits within the threshold; use it
        with top > 1: a value above 1 means the genome bridges clusters).
    A hit whose reference is missing from Cdb raises ValueError.

    What this is: for clusterAlg='single' it is exactly the cluster the query
    gets when the references and the query are re-clustered, provided every
    hit within the threshold is listed (count < top, or the last listed hit is
    already outside) and they all fall in one cluster (n_clusters <= 1).  What
    it is not: for n_clusters > 1 single linkage would merge those clusters,
    which a placement cannot express; for average, complete and the other
    methods this is the nearest-reference rule, not a re-clustering.
    union_condensed plus cluster_mash_condensed remains the exact route."""
    for col in ('genome1', 'genome2', 'rank', 'dist', 'common', 'denom'):
        if col not in hits.columns:
            raise ValueError("hits must be a query_best_hits table: no column %r" % col)
    cluster = dict(zip(Cdb['genome'].astype(str), Cdb['primary_cluster'].astype(np.int64)))
    g1 = hits['genome1'].astype(str).to_numpy()
    g2 = hits['genome2'].astype(str).to_numpy()
    missing = sorted(set(g1) - set(cluster))
    if missing:
        raise ValueError("hits name references that Cdb does not hold: %s" % ", ".join(missing[:5]))
    within = _rect_distance64(hits['common'].to_numpy(), hits['denom'].to_numpy()) <= 1.0 - float(P_ani)
    cl = np.array([cluster[n] for n in g1], dtype=np.int64)
    q, order = pd.factorize(g2)                                    # queries in the order of their first rows
    order = list(order)
    if isinstance(hits['genome2'].dtype, pd.CategoricalDtype):
        seen = set(order)
        order += [n for n in hits['genome2'].cat.categories if n not in seen]
    nq = len(order)
    nearest = np.full(nq, None, dtype=object)
    dist = np.full(nq, np.nan, dtype=np.float32)
    primary = np.zeros(nq, dtype=np.int64)
    first = hits['rank'].to_numpy() == 0
    nearest[q[first]] = g1[first]
    dist[q[first]] = hits['dist'].to_numpy()[first]
    primary[q[first & within]] = cl[first & within]
    pairs = np.unique(np.stack([q[within], cl[within]], axis=1), axis=0) if within.any() else np.zeros((0, 2), np.int64)
    n_clusters = np.bincount(pairs[:, 0], minlength=nq).astype(np.int64)
    return pd.DataFrame({'genome': order, 'nearest': nearest, 'dist': dist, 'primary_cluster': primary,
                         'n_clusters': n_clusters})
