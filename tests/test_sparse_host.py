"""CPU-only tests of the sparse pipeline (the pairs that share a hash instead
of the condensed triangle): the new C ABI symbols, the .npy store, and the
Python layers -- cluster_mash_sparse against scipy through
cluster_mash_condensed(gpu=None), mdb_from_sparse against the filtered dense
Mdb -- on pair lists taken from the C oracle's Mash merge (reference: `mash
dist`, drep/d_cluster.py:569-573, and cluster_mash_database, 598-630).  The
two argument checks at the end need a context, hence a device."""
import numpy as np
import pytest

import oracle
from drep_amd import _lib
from drep_amd import d_cluster, store

UMAX = np.iinfo(np.uint64).max


def family_sketches(N, s, seed, fam=7):
    """N sorted sketches: families of `fam` genomes drawing from a shared pool
    at varying rates (distances spread over the linkage cutoff), chance hashes
    between unrelated genomes, every 11th genome partial, two genomes empty."""
    rng = np.random.default_rng(seed)
    H = np.full((N, s), UMAX, dtype=np.uint64)
    NH = np.zeros(N, dtype=np.uint32)
    stray = rng.integers(1, UMAX, size=N // 2, dtype=np.uint64)
    pools = {}
    for g in range(N):
        f = g // fam
        if f not in pools:
            pools[f] = rng.integers(1, UMAX, size=2 * s, dtype=np.uint64)
        take = rng.random(2 * s) < rng.choice([0.15, 0.3, 0.45])
        own = rng.integers(1, UMAX, size=s, dtype=np.uint64)
        vals = np.unique(np.concatenate([pools[f][take], own, rng.choice(stray, 3)]))
        n = s if g % 11 else int(rng.integers(1, s))
        if g in (5, N - 3):
            n = 0
        vals = vals[:n]
        H[g, :len(vals)] = vals
        NH[g] = len(vals)
    return H, NH


def sparse_from_oracle(H, NH, s, names):
    N = len(NH)
    oc, od = oracle.allpairs(H, NH, s, threads=8)
    ii, jj = np.triu_indices(N, 1)
    keep = oc > 0
    sm = d_cluster.SparseMash(names, names, ii[keep].astype(np.uint32), jj[keep].astype(np.uint32), oc[keep], od[keep],
                              NH, np.full(N, 10 ** 6, np.uint64), s)
    cm = d_cluster.CondensedMash(names, names, oc, od, NH, np.full(N, 10 ** 6, np.uint64), s)
    return sm, cm


@pytest.fixture(scope="module")
def data300():
    s, N = 200, 300
    H, NH = family_sketches(N, s, seed=3)
    names = ["g%04d.fa" % ((i * 37) % N) for i in range(N)]          # not in sorted order
    sm, cm = sparse_from_oracle(H, NH, s, names)
    assert (cm.common > 0).sum() > N and (cm.common == 0).sum() > N
    return sm, cm


def test_sparse_symbols_exported():
    L = _lib.lib()
    for name in ("drephip_allpairs_sparse_device", "drephip_allpairs_sparse", "drephip_last_sparse_stats"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.drephip_version() >= 200
    import drep_amd
    for name in ("SparseMash", "all_vs_all_MASH_sparse", "cluster_mash_sparse", "mdb_from_sparse", "store_sparse",
                 "load_sparse"):
        assert getattr(drep_amd, name) is not None


@pytest.mark.parametrize("mmap", [True, False])
def test_sparse_store_roundtrip(tmp_path, data300, mmap):
    sm, _ = data300
    d = store.store_sparse(str(tmp_path), sm)
    assert d == store.sparse_dir(str(tmp_path)) and d != store.condensed_dir(str(tmp_path))
    back = store.load_sparse(str(tmp_path), mmap=mmap)
    assert isinstance(back.i, np.memmap) == mmap
    assert back.names == sm.names and back.locations == sm.locations and back.s == sm.s
    for f, dt in (("i", np.uint32), ("j", np.uint32), ("common", np.uint16), ("denom", np.uint16),
                  ("nhash", np.uint32), ("length", np.uint64)):
        a, b = getattr(back, f), getattr(sm, f)
        assert a.dtype == dt and np.array_equal(a, b), f


@pytest.mark.parametrize("alg", ["single", "average"])
def test_cluster_mash_sparse_equals_scipy(data300, alg):
    sm, cm = data300
    Cdb, ret = d_cluster.cluster_mash_condensed(cm, clusterAlg=alg, P_ani=0.9, gpu=None)     # scipy on the host
    Cdb2, ret2 = d_cluster.cluster_mash_sparse(sm, clusterAlg=alg, P_ani=0.9)
    assert np.array_equal(ret[0], ret2[0])
    assert ret2[0].tobytes() == ret[0].tobytes()
    assert Cdb2.equals(Cdb) and Cdb.to_dict("list") == Cdb2.to_dict("list")
    assert ret2[1] is None and ret2[2] == ret[2]
    assert 1 < Cdb["primary_cluster"].nunique() < len(sm.names)


def test_mdb_from_sparse_equals_filtered_dense(data300):
    sm, cm = data300
    dense = d_cluster.mdb_from_condensed(cm.names, cm.common, cm.denom, cm.nhash, cm.s)
    want = dense[dense["dist"] < 1]
    got = d_cluster.mdb_from_sparse(sm)
    assert len(got) == len(want) > len(sm.names)
    assert list(got.columns) == list(want.columns) and (got.dtypes == want.dtypes).all()
    for g in ("genome1", "genome2"):
        assert got[g].cat.ordered and list(got[g].cat.categories) == list(want[g].cat.categories)
        assert got[g].cat.codes.dtype == want[g].cat.codes.dtype
    for c in ("dist", "similarity"):
        assert got[c].to_numpy().dtype == np.float32
        assert np.array_equal(got[c].to_numpy().view(np.uint32), want[c].to_numpy().view(np.uint32)), c
    assert got.equals(want)


@pytest.mark.gpu
def test_sparse_argument_checks():
    s, N = 64, 12
    H, NH = family_sketches(N, s, seed=1)
    with _lib.Context(0, 21, s, 42) as ctx:
        buf = np.zeros((64, 4), np.uint32)
        bad = H.copy()
        bad[3, [4, 9]] = bad[3, [9, 4]]                               # row 3 no longer ascending
        n = _lib.C.c_uint64(0)
        rc = _lib.lib().drephip_allpairs_sparse(ctx.handle, bad.reshape(-1), NH, N, 0, N, buf.ctypes.data, len(buf),
                                                _lib.C.byref(n))
        assert rc == -1 and b"ascending" in _lib.lib().drephip_last_error()       # DREPHIP_ERR_ARG
        dup = H.copy()
        dup[4, 7] = dup[4, 6]                                         # not distinct
        rc = _lib.lib().drephip_allpairs_sparse(ctx.handle, dup.reshape(-1), NH, N, 0, N, buf.ctypes.data, len(buf),
                                                _lib.C.byref(n))
        assert rc == -1
        for r0, r1 in ((5, 5), (7, 3), (N - 1, N), (N, N + 4)):
            rc, cnt = ctx.allpairs_sparse_raw(H, NH, r0, r1, buf)
            assert rc == 0 and cnt == 0, (r0, r1)
            i, j, c, d = ctx.allpairs_sparse(H, NH, r0, r1)
            assert len(i) == len(j) == len(c) == len(d) == 0
