"""Mash's p-value and its -v / -d rules, the parts that need no GPU: the
library exports the entry points; drephip_pvalue_eval -- the inline functions of
drep_amd/csrc/pvalue.h that the kernels call, so these are the kernels'
numerics -- against 80-digit values (tests/golden/pvalue_grid.json, written by
tools/make_pvalue_grid.py) and against the golden MASH_table.tsv; the
rectangle's table writer; min_common_table against the distance comparison it
stands for."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import oracle
from drep_amd import _lib
from drep_amd import d_cluster
from drep_amd.mash_io import read_msh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 21
TINY = Fraction(1, 2 ** 1022)
# relative error allowed against the exact value: derived, not measured.  %g
# keeps 6 digits, so an error e flips a printed row with probability about
# 2 e / 1e-6: 2e-5 per row at 1e-11.  The scheme's own error is about
# (n + 3 common) 2^-53 <= 4e-12 at s = 32767.
REL_BOUND = 1e-11


@pytest.fixture(scope="module")
def grid():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "pvalue_grid.json")))
    assert g["k"] == K
    rows = g["rows"]
    out = {"common": np.array([r["common"] for r in rows], np.uint32),
           "len_a": np.array([r["len_a"] for r in rows], np.uint64),
           "len_b": np.array([r["len_b"] for r in rows], np.uint64),
           "s": np.array([r["s"] for r in rows], np.uint32),
           "exact": [Fraction(r["exact"]) for r in rows]}
    out["normal"] = np.array([e >= TINY for e in out["exact"]])
    assert out["normal"].sum() >= 300 and (~out["normal"]).sum() >= 100 and len(rows) <= 1000
    return out


def eval_grid(g, want_rn=False):
    """pvalue_eval over the grid, one call per sketch size."""
    n = len(g["common"])
    p, r, nn = np.zeros(n), np.zeros(n), np.zeros(n, np.uint32)
    for s in np.unique(g["s"]):
        sel = g["s"] == s
        p[sel], r[sel], nn[sel] = _lib.pvalue_eval(g["common"][sel], g["len_a"][sel], g["len_b"][sel], int(s), K,
                                                   want_rn=True)
    return (p, r, nn) if want_rn else p


def numpy_rn(len_a, len_b, s, k=K):
    """r and n by the formulas of d_cluster.mash_pvalue, in numpy float64."""
    kspace = 4.0 ** k
    px = 1.0 / (1.0 + kspace / np.asarray(len_a, dtype=np.float64))
    py = 1.0 / (1.0 + kspace / np.asarray(len_b, dtype=np.float64))
    r = px * py / (px + py - px * py)
    M = kspace * (px + py) / (1.0 + r)
    return r, np.floor(np.minimum(M, s))


def test_library_exports_significance_symbols():
    L = _lib.lib()
    assert L.drephip_version() >= 500
    for name in ("drephip_pvalue_eval", "drephip_pvalue_records_device", "drephip_pvalue_records",
                 "drephip_pvalue_hits_device", "drephip_records_filter_device", "drephip_allpairs_sparse_sig",
                 "drephip_dist_rect_sparse_sig", "drephip_write_mash_table_rect"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    for m in ("pvalue_records", "pvalue_records_device", "pvalue_hits", "filter_records", "allpairs_sparse_sig",
              "dist_rect_sparse_sig"):
        assert callable(getattr(_lib.Context, m))
    assert callable(_lib.pvalue_eval) and callable(_lib.write_mash_table_rect)
    import drep_amd
    for name in ("mash_pvalue_device", "min_common_table", "write_mash_table_rect"):
        assert name in drep_amd.__all__ and getattr(drep_amd, name) is getattr(d_cluster, name)


def test_accuracy_against_exact_values(grid):
    """Every normal-range row: relative error <= 1e-11 and the same %g text."""
    p = eval_grid(grid)
    worst, bad = Fraction(0), []
    for t in np.nonzero(grid["normal"])[0]:
        ex = grid["exact"][t]
        err = abs(Fraction(float(p[t])) - ex) / ex
        worst = max(worst, err)
        if err > Fraction(REL_BOUND) or "%g" % p[t] != "%g" % float(ex):
            bad.append((int(t), float(err), "%g" % p[t], "%g" % float(ex)))
    print("worst relative error over %d rows: %.3g" % (grid["normal"].sum(), float(worst)))
    assert not bad, bad[:5]


def test_rows_below_the_normal_range_are_zero(grid):
    p = eval_grid(grid)
    low = ~grid["normal"]
    assert (p[low] == 0.0).all()
    assert (p[grid["normal"]] >= float(TINY)).all() and (p <= 1.0).all()


def test_r_and_n_are_numpys_bit_for_bit(grid):
    _, r, n = eval_grid(grid, want_rn=True)
    for s in np.unique(grid["s"]):
        sel = grid["s"] == s
        er, en = numpy_rn(grid["len_a"][sel], grid["len_b"][sel], int(s))
        assert np.array_equal(r[sel].view(np.uint64), er.view(np.uint64))
        assert np.array_equal(n[sel], en.astype(np.uint32))


def test_common_zero_and_common_above_n():
    la = np.array([3_000_000, 25, 40, 2 * 10 ** 11], np.uint64)
    lb = np.array([5_000_000, 30, 2_000_000, 25], np.uint64)
    assert (_lib.pvalue_eval(np.zeros(4, np.uint32), la, lb, 1000) == 1.0).all()
    # tiny genomes: n = floor(M) < s
    _, _, n = _lib.pvalue_eval(np.ones(4, np.uint32), la, lb, 1000, want_rn=True)
    assert n[0] == 1000 and n[1] == 54 and n[2] == 1000 and n[3] == 1000     # (M is about len_a + len_b)
    above = (n + 1).astype(np.uint32)
    assert (_lib.pvalue_eval(above, la, lb, 1000) == 0.0).all()
    at = _lib.pvalue_eval(n.astype(np.uint32), la, lb, 1000)
    assert (at >= 0.0).all() and (at < 1.0).all()
    # a zero length with a shared hash cannot occur; without one it is p = 1
    with pytest.raises(_lib.DrepHipError):
        _lib.pvalue_eval(np.array([1], np.uint32), np.array([0], np.uint64), np.array([100], np.uint64), 1000)
    assert _lib.pvalue_eval(np.array([0], np.uint32), np.array([0], np.uint64), np.array([100], np.uint64), 1000)[0] == 1.0
    assert len(_lib.pvalue_eval(np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), 1000)) == 0


@pytest.mark.parametrize("la,lb,s", [(2_900_000, 4_100_000, 1000), (150_000, 8_000_000, 400),
                                     (2 * 10 ** 11, 10 ** 11, 32767), (60, 5_000_000, 1000)])
def test_monotone_in_common(la, lb, s):
    c = np.arange(0, min(200, s) + 1, dtype=np.uint32)
    p = _lib.pvalue_eval(c, np.full(len(c), la, np.uint64), np.full(len(c), lb, np.uint64), s)
    assert p[0] == 1.0 and (np.diff(p) <= 0).all()


def _golden_all(golden):
    m = read_msh(os.path.join(golden, "MASH_files", "ALL.msh"))
    N = len(m.references)
    H = np.full((N, 1000), np.iinfo(np.uint64).max, dtype=np.uint64)
    NH = np.zeros(N, dtype=np.uint32)
    L = np.zeros(N, dtype=np.uint64)
    for i, ref in enumerate(m.references):
        H[i, :len(ref.hashes)] = ref.hashes
        NH[i] = len(ref.hashes)
        L[i] = ref.length
    return [ref.name for ref in m.references], H, NH, L


def _oracle_rect(H, NH, s):
    """The N x N rectangle of a set against itself from the oracle's triangle."""
    N = len(NH)
    c, d = oracle.allpairs(H, NH, s)
    C = np.zeros((N, N), np.uint16)
    D = np.zeros((N, N), np.uint16)
    iu = np.triu_indices(N, 1)
    C[iu], D[iu] = c, d
    C, D = C + C.T, D + D.T
    C[np.arange(N), np.arange(N)] = D[np.arange(N), np.arange(N)] = np.minimum(NH, s)
    return C, D


def test_golden_table_p_values(golden):
    """The p text of all 25 rows of MASH_table.tsv from pvalue_eval."""
    names, H, NH, L = _golden_all(golden)
    C, _ = _oracle_rect(H, NH, 1000)
    rows = [ln.split("\t") for ln in open(os.path.join(golden, "MASH_files", "MASH_table.tsv")).read().splitlines()]
    assert len(rows) == 25
    idx = {n: i for i, n in enumerate(names)}
    r = np.array([idx[x[0]] for x in rows])
    q = np.array([idx[x[1]] for x in rows])
    p = _lib.pvalue_eval(C[q, r].astype(np.uint32), L[q], L[r], 1000)
    assert ["%g" % v for v in p] == [x[3] for x in rows]
    assert sum(1 for x in rows if "e-" in x[3]) >= 6           # real values among the 0s and 1s


def test_write_mash_table_rect_equals_golden_table(golden, tmp_path):
    """ALL x ALL from the oracle's counts: the golden table, byte for byte (a
    query that is a reference prints its own cell: 0, p, 1000/1000)."""
    names, H, NH, L = _golden_all(golden)
    C, D = _oracle_rect(H, NH, 1000)
    base = [os.path.basename(n) for n in names]
    rm = d_cluster.RectMash(base, names, base, names, C, D, None, None, None, None, NH, NH, L, L, 1000)
    out = tmp_path / "rect.tsv"
    d_cluster.write_mash_table_rect(str(out), rm, threads=3, pvalue='eval')
    want = open(os.path.join(golden, "MASH_files", "MASH_table.tsv"), "rb").read()
    assert out.read_bytes() == want
    # a 2 x 5 slice, one thread, explicit denominators through the C entry point
    dist = d_cluster._rect_distance64(C, D)
    qi, ri = np.nonzero(np.ones_like(C))
    P = _lib.pvalue_eval(C[qi, ri].astype(np.uint32), L[qi], L[ri], 1000).reshape(C.shape)
    _lib.write_mash_table_rect(str(out), names, names[1:3], C[1:3], D[1:3], 1000, dist[1:3], P[1:3], threads=1)
    assert out.read_bytes() == b"".join(want.splitlines(keepends=True)[5:15])
    with pytest.raises(ValueError):
        _lib.write_mash_table_rect(str(out), names, names[1:3], C, D, 1000, dist, P)


@pytest.mark.parametrize("s", [64, 1000])
def test_min_common_table_is_the_distance_comparison(s):
    c = np.arange(s + 1)
    for max_dist in (0.0, 0.05, 0.3):
        cmin = d_cluster.min_common_table(max_dist, s, K)
        assert cmin.dtype == np.uint32 and cmin.shape == (s + 1,)
        for d in range(s + 1):
            cc = c[:d + 1]
            brute = d_cluster._rect_distance64(cc, np.full(d + 1, d), K) <= max_dist
            assert np.array_equal(cc >= cmin[d], brute), (max_dist, d)
