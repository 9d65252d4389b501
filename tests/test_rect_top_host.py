"""Best hits and placement, the parts that need no GPU: the library exports
the entry points, the selection kernel's 64-bit key orders (common, denom, r)
as the contract does (exact rationals, then the smaller r), the hit table
(best_hits_frame) and place_queries are plain numpy and pandas."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

from drep_amd import _lib
from drep_amd import d_cluster

S = 1000


def test_library_exports_rect_top_symbols():
    L = _lib.lib()
    for name in ("drephip_dist_rect_top_device", "drephip_dist_rect_top"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    for m in ("dist_rect_top", "dist_rect_top_device", "dist_rect_top_raw"):
        assert callable(getattr(_lib.Context, m))
    import drep_amd
    for name in ("rect_top_hits", "query_best_hits", "place_queries"):
        assert name in drep_amd.__all__ and getattr(drep_amd, name) is getattr(d_cluster, name)


def test_rect_top_hits_rejects_bad_arguments(monkeypatch):
    """ValueError before any GPU call: no context is ever created."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    umax = np.iinfo(np.uint64).max
    qh, qn = np.full((3, 8), umax, np.uint64), np.zeros(3, np.uint32)
    rh, rn = np.full((4, 8), umax, np.uint64), np.zeros(4, np.uint32)
    for top in (0, 65, -1):
        with pytest.raises(ValueError):
            d_cluster.rect_top_hits(qh, qn, rh, rn, 8, top)
    with pytest.raises(ValueError):
        d_cluster.rect_top_hits(qh.astype(np.int64), qn, rh, rn, 8, 1)
    with pytest.raises(ValueError):
        d_cluster.rect_top_hits(qh, qn, rh[:, :7], rn, 8, 1)
    # no references, or no queries: nothing to run
    ref, c, d, n = d_cluster.rect_top_hits(qh, qn, rh[:0], rn[:0], 8, 3)
    assert ref.shape == (3, 3) and (ref == -1).all() and (c == 0).all() and (d == 0).all() and (n == 0).all()
    ref, c, d, n = d_cluster.rect_top_hits(qh[:0], qn[:0], rh, rn, 8, 3)
    assert ref.shape == (0, 3) and n.shape == (0,)


def kernel_key(c, d, r):
    """top_key of allpairs.hip, restated: floor(c (2^32 - 1) / d) << 32 | ~r."""
    return ((c * 0xFFFFFFFF // d) << 32) | (~r & 0xFFFFFFFF)


def test_key_preserves_fraction_order():
    """Random (common, denom, r) with denom <= 32767, ties of the ratio
    (multiples of one reduced fraction) and of everything but r included: the
    keys, largest first, give the order of (-Fraction(c, d), r); and the
    closest two distinct ratios the denominators allow stay apart."""
    rng = np.random.default_rng(5)
    cells = []
    for _ in range(4000):
        d = int(rng.integers(1, 32768))
        cells.append((int(rng.integers(1, d + 1)), d))
    for _ in range(500):                                    # ties: one ratio under several denominators
        b = int(rng.integers(1, 200))
        a = int(rng.integers(1, b + 1))
        for m in rng.integers(1, 32767 // b + 1, size=4):
            cells.append((a * int(m), b * int(m)))
    cells += [(1, 32767), (32767, 32767), (1, 1), (32766, 32767), (32765, 32766), (16383, 32767), (16383, 32766),
              (1, 32766), (2, 32767)]
    cells += cells[:300]                                    # the same cell at two reference rows
    r = rng.permutation(len(cells))
    items = [(c, d, int(x)) for (c, d), x in zip(cells, r)]
    by_key = sorted(items, key=lambda t: kernel_key(*t), reverse=True)
    by_contract = sorted(items, key=lambda t: (-Fraction(t[0], t[1]), t[2]))
    assert by_key == by_contract
    assert len({Fraction(c, d) for c, d, _ in items}) < len(items) - 300          # ratio ties across denominators
    assert all(kernel_key(c, d, x) > 0 and kernel_key(c, d, x) < 1 << 64 for c, d, x in items)
    # neighbours in the Farey sequence of order 32767 differ by 1 / (d1 d2) > 2^-30
    for (c1, d1), (c2, d2) in (((32765, 32766), (32766, 32767)), ((1, 32767), (1, 32766)), ((16383, 32767), (1, 2))):
        assert Fraction(c1, d1) < Fraction(c2, d2) and kernel_key(c1, d1, 0) >> 32 < kernel_key(c2, d2, 0) >> 32


def _hits(rows):
    """A query_best_hits table from (reference, query, rank, common, denom) rows."""
    qn = sorted({r[1] for r in rows}) + ["lonely.fa"]
    rn = sorted({r[0] for r in rows})
    q = np.array([qn.index(r[1]) for r in rows], dtype=np.int64)
    ref = np.full((len(qn), 4), -1, np.int64)
    common = np.zeros((len(qn), 4), np.uint16)
    denom = np.zeros((len(qn), 4), np.uint16)
    count = np.zeros(len(qn), np.uint32)
    for (g1, g2, rank, c, d), qi in zip(rows, q):
        ref[qi, rank], common[qi, rank], denom[qi, rank] = rn.index(g1), c, d
        count[qi] = max(count[qi], rank + 1)
    return d_cluster.best_hits_frame(qn, rn, ref, common, denom, count, S), qn, rn


def test_best_hits_frame_columns_and_max_dist():
    rows = [("r1", "a.fa", 0, 1000, 1000), ("r2", "a.fa", 1, 500, 1000), ("r3", "a.fa", 2, 3, 997),
            ("r2", "b.fa", 0, 40, 1000)]
    f, qn, rn = _hits(rows)
    assert list(f.columns) == ["genome1", "genome2", "rank", "dist", "similarity", "common", "denom"]
    assert list(f["genome2"].astype(str)) == ["a.fa"] * 3 + ["b.fa"] and list(f["rank"]) == [0, 1, 2, 0]
    assert list(f["genome1"].astype(str)) == ["r1", "r2", "r3", "r2"]
    assert f["dist"].dtype == np.float32 and f["similarity"].dtype == np.float32
    assert list(f["genome2"].cat.categories) == qn                 # the query without hits keeps its name
    exp = d_cluster.mash_distance_float32(np.array([1000, 500, 3, 40]), np.array([1000, 1000, 997, 1000]))
    assert np.array_equal(f["dist"].to_numpy().view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(f["similarity"].to_numpy().view(np.uint32), (np.float32(1) - exp).view(np.uint32))
    assert list(f["common"]) == [1000, 500, 3, 40] and list(f["denom"]) == [1000, 1000, 997, 1000]
    # max_dist: the float64 distance decides, the edge is inside
    d64 = [_lib.distance_lut(d)[c] for _, _, _, c, d in rows]
    ref = np.array([[0, 1, 2], [1, -1, -1], [-1, -1, -1]])
    common = np.array([[1000, 500, 3], [40, 0, 0], [0, 0, 0]], np.uint16)
    denom = np.array([[1000, 1000, 997], [1000, 0, 0], [0, 0, 0]], np.uint16)
    count = np.array([3, 1, 0], np.uint32)
    for cut, want in ((d64[1], [0, 1]), (np.nextafter(d64[1], 0), [0]), (d64[3], [0, 1, 3]), (0.0, [0])):
        g = d_cluster.best_hits_frame(qn, rn, ref, common, denom, count, S, max_dist=cut)
        assert list(g["genome1"].astype(str)) == [rows[t][0] for t in want], cut
        assert list(g["rank"]) == [rows[t][2] for t in want]
    empty = d_cluster.best_hits_frame(qn, rn, ref, common, denom, np.zeros(3, np.uint32), S)
    assert len(empty) == 0 and list(empty.columns) == list(f.columns)


def _edge_pair():
    """(common, P_ani) with 1 - P_ani exactly the float64 distance of common / S."""
    lut = _lib.distance_lut(S)
    for c in range(S - 1, 0, -1):
        p = 1.0 - lut[c]
        if 1.0 - p == lut[c] and 0.05 < lut[c] < 0.2:
            return c, p
    raise AssertionError("no exactly representable threshold")


def test_place_queries():
    c_edge, p_edge = _edge_pair()
    rows = [("r1", "a.fa", 0, 900, 1000), ("r2", "a.fa", 1, 800, 1000), ("r3", "a.fa", 2, 700, 1000),
            ("r3", "b.fa", 0, c_edge, S), ("r1", "b.fa", 1, c_edge - 1, S),
            ("r2", "c.fa", 0, 2, 1000)]
    hits, qn, rn = _hits(rows)
    Cdb = pd.DataFrame({"genome": ["r1", "r2", "r3", "other"], "primary_cluster": [1, 1, 2, 3]})
    lut = _lib.distance_lut(S)
    assert lut[900] < 0.1 and lut[700] < 0.1 and lut[2] > 0.1
    out = d_cluster.place_queries(hits, Cdb, P_ani=0.9)
    assert list(out.columns) == ["genome", "nearest", "dist", "primary_cluster", "n_clusters"]
    assert list(out["genome"]) == ["a.fa", "b.fa", "c.fa", "lonely.fa"]
    assert list(out["nearest"]) == ["r1", "r3", "r2", None]
    assert out["dist"].dtype == np.float32
    assert np.array_equal(out["dist"].to_numpy()[:3].view(np.uint32),
                          hits["dist"].to_numpy()[[0, 3, 5]].view(np.uint32)) and np.isnan(out["dist"][3])
    # a: r1, r2 (cluster 1) and r3 (cluster 2) within 0.1 -> bridges; c: its only hit is outside; lonely: none
    assert list(out["primary_cluster"]) == [1, 2 if lut[c_edge] <= 1 - 0.9 else 0, 0, 0]
    assert out["n_clusters"][0] == 2 and out["n_clusters"][2] == 0 and out["n_clusters"][3] == 0
    # the edge: dist == 1 - P_ani is inside, one ulp tighter is outside (and the next hit already is)
    at = d_cluster.place_queries(hits, Cdb, P_ani=p_edge)
    assert 1.0 - p_edge == lut[c_edge]
    assert at["primary_cluster"][1] == 2 and at["n_clusters"][1] == 1
    tight = d_cluster.place_queries(hits, Cdb, P_ani=np.nextafter(p_edge, 2.0))
    assert 1.0 - np.nextafter(p_edge, 2.0) < lut[c_edge]
    assert tight["primary_cluster"][1] == 0 and tight["n_clusters"][1] == 0 and tight["nearest"][1] == "r3"
    # a reference that Cdb does not hold
    with pytest.raises(ValueError):
        d_cluster.place_queries(hits, Cdb[Cdb["genome"] != "r2"])
    with pytest.raises(ValueError):
        d_cluster.place_queries(hits.drop(columns=["common"]), Cdb)
