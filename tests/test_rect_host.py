"""Query against reference, the parts that need no GPU: the library exports
the rectangle's entry points, argument checks come before any context, the
reference .msh is vetted, and the table / condensed assemblies
(mdb_from_rect, union_condensed) are plain numpy and pandas."""
import os

import numpy as np
import pandas as pd
import pytest

import edge_cases
from drep_amd import _lib
from drep_amd import d_cluster
from drep_amd.mash_io import MashReference, write_msh

UMAX = np.iinfo(np.uint64).max
RECT_SYMBOLS = ("drephip_dist_rect_device", "drephip_dist_rect_merge_device", "drephip_dist_rect",
                "drephip_dist_rect_sparse_device", "drephip_dist_rect_sparse")


def test_library_exports_rect_symbols():
    L = _lib.lib()
    for name in RECT_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.drephip_version() >= 400
    for m in ("dist_rect", "dist_rect_merge", "dist_rect_sparse"):
        assert callable(getattr(_lib.Context, m))


def _mats(Q=3, N=4, s=8):
    qh = np.full((Q, s), UMAX, np.uint64)
    rh = np.full((N, s), UMAX, np.uint64)
    return qh, np.zeros(Q, np.uint32), rh, np.zeros(N, np.uint32)


def test_rect_allpairs_rejects_bad_arguments(monkeypatch):
    """ValueError before any GPU call: no context is ever created."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    qh, qn, rh, rn = _mats()
    s = 8
    bad = [
        (qh.astype(np.int64), qn, rh, rn),            # signed hashes
        (qh.astype(np.float64), qn, rh, rn),
        (qh, qn.astype(np.int32), rh, rn),
        (qh, qn, rh, rn.astype(np.uint64)),
        (qh[:, :7], qn, rh, rn),                      # another sketch size
        (qh, qn, rh[:, :7], rn),
        (qh[:2], qn, rh, rn),                         # rows and counts disagree
        (qh, qn, rh, rn[:3]),
        (qh.reshape(-1), qn, rh, rn),                 # not a matrix
    ]
    for args in bad:
        with pytest.raises(ValueError):
            d_cluster.rect_allpairs(*args, s)
        with pytest.raises(ValueError):
            d_cluster.rect_allpairs_sparse(*args, s)
    # an empty side needs no GPU either
    c, d = d_cluster.rect_allpairs(qh[:0], qn[:0], rh, rn, s)
    assert c.shape == (0, 4) and d.shape == (0, 4) and c.dtype == np.uint16
    c, d = d_cluster.rect_allpairs(qh, qn, rh[:0], rn[:0], s)
    assert c.shape == (3, 0)
    assert all(len(a) == 0 for a in d_cluster.rect_allpairs_sparse(qh, qn, rh[:0], rn[:0], s))


@pytest.mark.parametrize("k,seed,s,kwargs", [(20, 42, 64, {}), (21, 7, 64, {}), (21, 42, 64, {"MASH_sketch": 1000}),
                                             (21, 42, 64, {"MASH_sketch": "65"})])
def test_reference_with_other_parameters_raises(tmp_path, monkeypatch, k, seed, s, kwargs):
    def no_sketch(*a, **kw):
        raise AssertionError("queries were sketched")
    monkeypatch.setattr(d_cluster, "sketch_genomes", no_sketch)
    ref = str(tmp_path / "ref.msh")
    write_msh(ref, [MashReference("/g/a.fa", "", 1000, np.arange(1, s + 1, dtype=np.uint64))], k, s, seed)
    Qdb = pd.DataFrame({"genome": ["q.fa"], "location": ["/q/q.fa"]})
    with pytest.raises(ValueError):
        d_cluster.query_vs_MASH(Qdb, str(tmp_path), reference=ref, **kwargs)
    with pytest.raises(ValueError):
        d_cluster.query_vs_MASH_rect(Qdb, str(tmp_path), reference=ref, **kwargs)


def test_reference_defaults_and_matching_sketch_size(tmp_path, monkeypatch):
    """The default reference is <data_folder>/MASH_files/ALL.msh, its sketch
    size is the call's s, and the queries go to <data_folder>/MASH_query."""
    seen = {}

    class Stop(Exception):
        pass

    def fake_sketch(Bdb, folder, **kw):
        seen.update(folder=folder, kw=kw)
        raise Stop()
    monkeypatch.setattr(d_cluster, "sketch_genomes", fake_sketch)
    os.makedirs(tmp_path / "MASH_files")
    write_msh(str(tmp_path / "MASH_files" / "ALL.msh"),
              [MashReference("/g/a.fa", "", 1000, np.arange(1, 65, dtype=np.uint64))], 21, 64, 42)
    Qdb = pd.DataFrame({"genome": ["q.fa"], "location": ["/q/q.fa"]})
    with pytest.raises(Stop):
        d_cluster.query_vs_MASH(Qdb, str(tmp_path), MASH_sketch="64", processors=3)
    assert seen["folder"] == os.path.join(str(tmp_path), "MASH_query")
    assert seen["kw"]["MASH_sketch"] == 64 and seen["kw"]["processors"] == 3
    with pytest.raises(ValueError):
        d_cluster.query_vs_MASH(Qdb, str(tmp_path), max_dist=1.0)
    with pytest.raises(ValueError):
        d_cluster.query_vs_MASH(Qdb, str(tmp_path), ingest="fpga")


def _hand_rect(dense=True):
    s = 1000
    common = np.array([[1000, 3, 0], [561, 0, 700]], dtype=np.uint16)
    denom = np.array([[1000, 1000, 1000], [1000, 1000, 700]], dtype=np.uint16)
    q, r = np.nonzero(common)
    return d_cluster.RectMash(
        qnames=["zq.fa", "aq.fa"], qlocations=["/q/zq.fa", "/q/aq.fa"],
        rnames=["m.fa", "b.fa", "x.fa"], rlocations=["/r/m.fa", "/r/b.fa", "/r/x.fa"],
        common=common if dense else None, denom=denom if dense else None,
        q=None if dense else q.astype(np.uint32), r=None if dense else r.astype(np.uint32),
        rec_common=None if dense else common[q, r], rec_denom=None if dense else denom[q, r],
        qnhash=np.array([1000, 700], np.uint32), rnhash=np.array([1000, 1000, 700], np.uint32),
        qlength=np.array([5, 6], np.uint64), rlength=np.array([7, 8, 9], np.uint64), s=s)


def test_mdb_from_rect_order_dtypes_categories():
    rm = _hand_rect()
    Mdb = d_cluster.mdb_from_rect(rm)
    assert list(Mdb.columns) == ["genome1", "genome2", "dist", "similarity"]
    # query-outer, reference-inner; genome1 the reference, genome2 the query
    assert list(Mdb["genome1"].astype(str)) == ["m.fa", "b.fa", "x.fa"] * 2
    assert list(Mdb["genome2"].astype(str)) == ["zq.fa"] * 3 + ["aq.fa"] * 3
    assert list(Mdb["genome1"].cat.categories) == ["b.fa", "m.fa", "x.fa"] and Mdb["genome1"].cat.ordered
    assert list(Mdb["genome2"].cat.categories) == ["aq.fa", "zq.fa"] and Mdb["genome2"].cat.ordered
    assert Mdb["dist"].dtype == np.float32 and Mdb["similarity"].dtype == np.float32
    exp = d_cluster.mash_distance_float32(rm.common.reshape(-1), rm.denom.reshape(-1))
    assert np.array_equal(Mdb["dist"].to_numpy().view(np.uint32), exp.view(np.uint32))
    assert Mdb["dist"].iloc[0] == 0 and Mdb["dist"].iloc[2] == 1 and Mdb["dist"].iloc[5] == 0
    assert np.array_equal(Mdb["similarity"].to_numpy(), np.float32(1) - exp)
    # the record form: the listed rows, same order and bits; max_dist on the float64 distance
    rec = d_cluster.mdb_from_rect(_hand_rect(dense=False))
    keep = rm.common.reshape(-1) > 0
    assert list(rec["genome1"].astype(str)) == list(Mdb["genome1"].astype(str)[keep])
    assert list(rec["genome2"].astype(str)) == list(Mdb["genome2"].astype(str)[keep])
    assert np.array_equal(rec["dist"].to_numpy().view(np.uint32), Mdb["dist"].to_numpy()[keep].view(np.uint32))
    assert list(rec["genome1"].cat.categories) == ["b.fa", "m.fa", "x.fa"]
    d64 = np.array([_lib.distance_lut(int(d))[int(c)] for c, d in zip(rm.common.reshape(-1), rm.denom.reshape(-1))])
    cut = d_cluster.mdb_from_rect(_hand_rect(dense=False), max_dist=0.02)
    assert len(cut) == int((d64 <= 0.02).sum()) == 3
    assert np.array_equal(cut["dist"].to_numpy(), Mdb["dist"].to_numpy()[d64 <= 0.02])


def test_union_condensed_equals_stacked_allpairs():
    s, nr, nq = 64, 18, 12
    H, NH = edge_cases.geometry_sketches(nr + nq, s, seed=5)
    ec, ed = edge_cases.ref_allpairs(H, NH, s)
    names = ["g%02d.fa" % i for i in range(nr + nq)]
    locs = ["/x/" + n for n in names]
    length = np.arange(nr + nq, dtype=np.uint64) + 100

    def cm(a, b):
        c, d = edge_cases.ref_allpairs(H[a:b], NH[a:b], s)
        return d_cluster.CondensedMash(names[a:b], locs[a:b], c, d, NH[a:b], length[a:b], s)
    rc = np.zeros((nq, nr), np.uint16)
    rd = np.zeros((nq, nr), np.uint16)
    for q in range(nq):
        for r in range(nr):
            rc[q, r], rd[q, r] = edge_cases.ref_pair(H[nr + q, :NH[nr + q]], H[r, :NH[r]], s)
    rm = d_cluster.RectMash(names[nr:], locs[nr:], names[:nr], locs[:nr], rc, rd, None, None, None, None,
                            NH[nr:], NH[:nr], length[nr:], length[:nr], s)
    u = d_cluster.union_condensed(cm(0, nr), rm, cm(nr, nr + nq))
    assert u.names == names and u.locations == locs and u.s == s
    assert u.common.dtype == np.uint16 and u.denom.dtype == np.uint16
    assert np.array_equal(u.common, ec) and np.array_equal(u.denom, ed)
    assert np.array_equal(u.nhash, NH) and np.array_equal(u.length, length)
    assert (ed < s).any() and (ec > 0).any()
    with pytest.raises(ValueError):
        d_cluster.union_condensed(cm(0, nr), rm, cm(nr + 1, nr + nq))
