"""Mash's p-value and its -v / -d filters on the GPU (drep_amd/csrc/pvalue.hip):
k_pvalue_records and k_pvalue_hits against the host evaluator of the same
arithmetic (drephip_pvalue_eval) bit for bit, the stable record filter against
a numpy mask, the two _sig record calls against the existing record calls
followed by the evaluator and the mask on the host, and the table writers
against the golden MASH_table.tsv."""
import functools
import os
import shutil

import numpy as np
import pandas as pd
import pytest

import edge_cases
from drep_amd import _lib
from drep_amd import d_cluster
from drep_amd.mash_io import read_msh

pytestmark = pytest.mark.gpu

K = 21
POISON = -7.25


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


# ------------------------------------------------------------ 1. records
LEN_A = np.array([2_900_000, 25, 4_100_000, 5_200_000, 60, 2 * 10 ** 11, 1_800_000, 3_300_000, 7_700_000, 40,
                  10 ** 11, 2_000_000, 6_100_000], np.uint64)
LEN_B = np.array([3_100_000, 30, 5_500_000, 10 ** 11, 2_400_000, 1_000_000, 8_000_000], np.uint64)


def wave_records(n, s=1000, seed=5):
    """n records whose neighbours differ as much as records can: per group of
    five lanes common = 0, 1, about 900, above the binomial's n (a pair of tiny
    genomes, n = 54) and a value far below 2^-1022; the rest random.  a indexes
    LEN_A, b indexes LEN_B."""
    rng = np.random.default_rng(seed + n)
    rec = np.zeros((n, 4), np.uint32)
    rec[:, 0] = rng.integers(0, len(LEN_A), n)
    rec[:, 1] = rng.integers(0, len(LEN_B), n)
    rec[:, 2] = rng.integers(0, 201, n)
    rec[:, 3] = s
    t = np.arange(n)
    rec[t % 10 == 0, 2] = 0
    rec[t % 10 == 1, 2] = 1
    rec[t % 10 == 2, 2] = 900 - (t[t % 10 == 2] % 7)
    tiny = t % 10 == 3
    rec[tiny, 0], rec[tiny, 1], rec[tiny, 2] = 1, 1, 55 + (t[tiny] % 5)          # lengths 25 and 30: n = 54
    low = t % 10 == 4
    rec[low, 0], rec[low, 1], rec[low, 2] = 0, 0, 150                             # ~1e-900
    return rec


def host_p(rec, la, lb, s):
    return _lib.pvalue_eval(rec[:, 2], la[rec[:, 0]], lb[rec[:, 1]], s, K)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4099])
def test_pvalue_records_equal_host_evaluator(ctx1000, n):
    torch, dev = torch_dev()
    rec = wave_records(n)
    want = host_p(rec, LEN_A, LEN_B, 1000)
    if n >= 63:
        _, _, nn = _lib.pvalue_eval(rec[:5, 2], LEN_A[rec[:5, 0]], LEN_B[rec[:5, 1]], 1000, K, want_rn=True)
        assert want[0] == 1.0 and 0 < want[1] < 1 and want[2] == 0.0
        assert rec[3, 2] > nn[3] == 54 and want[3] == 0.0 and rec[4, 2] < nn[4] and want[4] == 0.0
    # the host form, into a guarded buffer
    buf = np.full(n + 2, POISON)
    got = ctx1000.pvalue_records(rec, LEN_A, LEN_B, out=buf[1:-1])
    assert buf[0] == POISON and buf[-1] == POISON
    assert np.array_equal(bits(got), bits(want))
    # the device form: guards before and after the output on the device
    d_r = torch.tensor(rec.view(np.int32), device=dev)
    d_a = torch.tensor(LEN_A.view(np.int64), device=dev)
    d_b = torch.tensor(LEN_B.view(np.int64), device=dev)
    d_p = torch.full((n + 2,), POISON, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ctx1000.pvalue_records_device(d_r.data_ptr(), n, d_a.data_ptr(), len(LEN_A), d_b.data_ptr(), len(LEN_B),
                                  d_p.data_ptr() + 8)
    out = d_p.cpu().numpy()
    assert out[0] == POISON and out[-1] == POISON
    assert np.array_equal(bits(out[1:-1]), bits(want))


def test_pvalue_records_arguments(ctx1000):
    rec = wave_records(8)
    assert len(ctx1000.pvalue_records(rec[:0], LEN_A, LEN_B)) == 0
    ctx1000.pvalue_records_device(None, 0, None, 0, None, 0, None)              # n == 0: nothing to do
    with pytest.raises(_lib.DrepHipError):
        ctx1000.pvalue_records_device(None, 4, None, 0, None, 0, None)
    for col, val in ((0, len(LEN_A)), (1, len(LEN_B)), (3, 1001)):
        bad = rec.copy()
        bad[5, col] = val
        with pytest.raises(_lib.DrepHipError):
            ctx1000.pvalue_records(bad, LEN_A, LEN_B)
    bad = rec.copy()
    bad[2, 2], bad[2, 3] = 30, 20                                                # common > denom
    with pytest.raises(_lib.DrepHipError):
        ctx1000.pvalue_records(bad, LEN_A, LEN_B)
    la = LEN_A.copy()
    la[rec[1, 0]] = 0                                                            # record 1 has common 1
    with pytest.raises(_lib.DrepHipError):
        ctx1000.pvalue_records(rec, la, LEN_B)
    # one array for both sides (the triangle's records)
    tri = rec.copy()
    tri[:, 1] = tri[:, 1] % len(LEN_A)
    assert np.array_equal(bits(ctx1000.pvalue_records(tri, LEN_A)), bits(host_p(tri, LEN_A, LEN_A, 1000)))


# ------------------------------------------------------------ 2. hits
@pytest.mark.parametrize("top", [3, 64])
def test_pvalue_hits_equal_host_evaluator(ctx1000, top):
    torch, dev = torch_dev()
    rows, N = 41, 29
    rng = np.random.default_rng(top)
    qlen = rng.integers(100_000, 9_000_000, rows).astype(np.uint64)
    rlen = rng.integers(100_000, 9_000_000, N).astype(np.uint64)
    count = rng.integers(0, top + 1, rows).astype(np.uint32)
    count[:3] = (0, top, 1)
    assert (count < top).sum() >= rows // 2
    hits = np.zeros((rows, top, 4), np.uint32)
    hits[:, :, 0] = rng.integers(0, N, (rows, top))
    hits[:, :, 1] = rng.integers(1, 30, (rows, top))
    hits[:, :, 2] = 1000
    listed = np.arange(top)[None, :] < count[:, None]
    hits[~listed] = (0xFFFFFFFF, 0, 0, 0)
    want = np.ones((rows, top))
    q, t = np.nonzero(listed)
    want[q, t] = _lib.pvalue_eval(hits[q, t, 1], qlen[q], rlen[hits[q, t, 0]], 1000, K)
    assert (want[listed] < 1).all()
    d_h = torch.tensor(hits.view(np.int32), device=dev)
    d_c = torch.tensor(count.view(np.int32), device=dev)
    d_q = torch.tensor(qlen.view(np.int64), device=dev)
    d_r = torch.tensor(rlen.view(np.int64), device=dev)
    d_p = torch.full((rows * top + 2,), POISON, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ctx1000.pvalue_hits_device(d_h.data_ptr(), d_c.data_ptr(), rows, top, d_q.data_ptr(), d_r.data_ptr(), N,
                               d_p.data_ptr() + 8)
    out = d_p.cpu().numpy()
    assert out[0] == POISON and out[-1] == POISON
    assert np.array_equal(bits(out[1:-1].reshape(rows, top)), bits(want))
    # the array form d_cluster uses
    ref = hits[:, :, 0].astype(np.int64)
    ref[~listed] = -1
    got = ctx1000.pvalue_hits(ref, hits[:, :, 1], hits[:, :, 2], count, qlen, rlen)
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------ 3. the filter
def filter_case(n, seed=3):
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 4), np.uint32)
    rec[:, 0] = np.arange(n)                       # distinct records: the order is visible
    rec[:, 1] = rng.integers(0, 1 << 20, n)
    rec[:, 3] = rng.integers(1, 1001, n)
    rec[:, 2] = (rng.random(n) * (rec[:, 3] + 1)).astype(np.uint32)
    p = 10.0 ** rng.uniform(-30, 0, n)
    p[rng.random(n) < 0.1] = 0.0
    p[rng.random(n) < 0.1] = 1.0
    return rec, p


@pytest.mark.parametrize("n", [0, 1, 4099])
def test_filter_records_equals_numpy_mask(ctx1000, n, monkeypatch):
    rec, p = filter_case(n)
    cmin = d_cluster.min_common_table(0.05, 1000, K)
    none = np.full(1001, 1002, np.uint32)
    cases = [("all kept", p, 1.0, None), ("none kept", p, 0.0, none), ("p only", p, 1e-10, None),
             ("cmin only", None, 1.0, cmin), ("both", p, 1e-10, cmin), ("no test at all", None, 1.0, None)]
    for chunk in (None, "1000"):
        if chunk:
            monkeypatch.setenv("DREPHIP_FILTER_CHUNK", chunk)
        for name, pv, max_p, cm in cases:
            mask = np.ones(n, bool)
            if pv is not None:
                mask &= pv <= max_p
            if cm is not None:
                mask &= rec[:, 2] >= cm[rec[:, 3]]
            out, pout = ctx1000.filter_records(rec, pv, max_p, cm)
            assert np.array_equal(out, rec[mask]), name
            if pv is None:
                assert pout is None
            else:
                assert np.array_equal(bits(pout), bits(pv[mask])), name
            if n == 4099 and name in ("p only", "cmin only", "both"):
                assert 0 < mask.sum() < n, name
            if name == "none kept":
                assert len(out) == 0
            if name == "all kept":
                assert len(out) == n


def test_filter_records_arguments(ctx1000):
    torch, dev = torch_dev()
    rec, p = filter_case(16)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.DrepHipError):
            ctx1000.filter_records(rec, p, bad)
    d_r = torch.tensor(rec.view(np.int32), device=dev)
    with pytest.raises(_lib.DrepHipError):                    # the output must not alias the input
        ctx1000.filter_records_device(d_r.data_ptr(), None, 16, 1.0, None, d_r.data_ptr(), None)
    with pytest.raises(_lib.DrepHipError):
        ctx1000.filter_records_device(None, None, 16, 1.0, None, None, None)


# ------------------------------------------------------------ 4. the _sig calls
NQ = 41


@functools.lru_cache(maxsize=None)
def sig_set(s):
    H, NH = edge_cases.geometry_sketches(97, s, seed=2000 + s)
    H.setflags(write=False)
    NH.setflags(write=False)
    rng = np.random.default_rng(s)
    length = np.exp(rng.uniform(np.log(2_000), np.log(2e11), 97)).astype(np.uint64)
    length.setflags(write=False)
    return H, NH, length


def sig_filters(s):
    cmin = d_cluster.min_common_table(0.12, s, K)
    return [(1.0, None), (1e-10, None), (1.0, cmin), (1e-10, cmin), (1e-300, None), (0.0, cmin)]


def expect(rec4, la, lb, s, max_p, cmin):
    """The existing call's sorted records through the evaluator and the mask."""
    a, b, c, d = rec4
    p = _lib.pvalue_eval(c, la[a], lb[b], s, K)
    keep = p <= max_p
    if cmin is not None:
        keep &= c >= cmin[d]
    return a[keep], b[keep], c[keep], d[keep], p[keep]


def same(got, want):
    assert all(np.array_equal(g, w) for g, w in zip(got[:4], want[:4]))
    assert np.array_equal(bits(got[4]), bits(want[4]))


@pytest.mark.parametrize("s", [64, 1000, 4096])
@pytest.mark.parametrize("how", ["plain", "blocks", "screen"])
def test_dist_rect_sparse_sig(s, how, monkeypatch):
    H, NH, L = sig_set(s)
    if how == "blocks":
        monkeypatch.setenv("DREPHIP_RECT_BLOCK_ROWS", "7")
        monkeypatch.setenv("DREPHIP_RECT_SCREEN_BLOCK_ROWS", "7")
    with _lib.Context(0, K, s, 42) as ctx:
        if how == "screen":
            ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        base = ctx.dist_rect_sparse(H[:NQ], NH[:NQ], H, NH)
        assert len(base[0]) > 100
        kept = []
        for max_p, cmin in sig_filters(s):
            want = expect(base, L[:NQ], L, s, max_p, cmin)
            got = ctx.dist_rect_sparse_sig(H[:NQ], NH[:NQ], H, NH, L[:NQ], L, max_p, cmin)
            same(got, want)
            assert got[5] == len(base[0])                         # n_listed: before the filter
            kept.append(len(want[0]))
        assert kept[0] == len(base[0]) and 0 < kept[3] < kept[0]
        if how == "screen":
            assert ctx.last_rect_screen_stats()["used"]
        # a query range, and a cap one too small: NOMEM, the filtered count, then the retry
        max_p, cmin = sig_filters(s)[3]
        want = expect(ctx.dist_rect_sparse(H[:NQ], NH[:NQ], H, NH, 5, 30), L[:NQ], L, s, max_p, cmin)
        n = len(want[0])
        assert n > 1
        pairs = np.full((n + 1, 4), 0xABCDEF01, np.uint32)
        pv = np.full(n + 1, POISON)
        rc, cnt, listed = ctx.dist_rect_sparse_sig_raw(H[:NQ], NH[:NQ], H, NH, L[:NQ], L, 5, 30, max_p, cmin,
                                                       pairs[:n - 1], pv[:n - 1])
        assert (rc, cnt) == (ctx.ERR_NOMEM, n) and listed > n
        assert (pairs[n - 1:] == 0xABCDEF01).all() and (pv[n - 1:] == POISON).all()
        rc, cnt, _ = ctx.dist_rect_sparse_sig_raw(H[:NQ], NH[:NQ], H, NH, L[:NQ], L, 5, 30, max_p, cmin, pairs[:n],
                                                  pv[:n])
        assert (rc, cnt) == (0, n) and (pairs[n] == 0xABCDEF01).all() and pv[n] == POISON
        same(_lib._sorted_sig(pairs[:n], pv[:n]), want)
        # count only
        rc, cnt, _ = ctx.dist_rect_sparse_sig_raw(H[:NQ], NH[:NQ], H, NH, L[:NQ], L, 5, 30, max_p, cmin, None, None)
        assert (rc, cnt) == (ctx.ERR_NOMEM, n)


@pytest.mark.parametrize("s", [64, 1000, 4096])
@pytest.mark.parametrize("how", ["plain", "blocks", "screen"])
def test_allpairs_sparse_sig(s, how, monkeypatch):
    H, NH, L = sig_set(s)
    if how == "blocks":
        monkeypatch.setenv("DREPHIP_SPARSE_BLOCK_ROWS", "7")
    with _lib.Context(0, K, s, 42) as ctx:
        if how == "screen":
            ctx.set_allpairs_screen(ctx.SCREEN_ON)
        base = ctx.allpairs_sparse(H, NH)
        assert len(base[0]) > 100
        kept = []
        for max_p, cmin in sig_filters(s):
            want = expect(base, L, L, s, max_p, cmin)
            got = ctx.allpairs_sparse_sig(H, NH, L, max_p, cmin)
            same(got, want)
            assert got[5] == len(base[0])
            kept.append(len(want[0]))
        assert kept[0] == len(base[0]) and 0 < kept[3] < kept[0]
        if how == "blocks":
            assert ctx.sparse_stats()["blocks"] > 1
        max_p, cmin = sig_filters(s)[3]
        want = expect(ctx.allpairs_sparse(H, NH, 10, 60), L, L, s, max_p, cmin)
        n = len(want[0])
        assert n > 1
        pairs = np.full((n + 1, 4), 0xABCDEF01, np.uint32)
        pv = np.full(n + 1, POISON)
        rc, cnt, listed = ctx.allpairs_sparse_sig_raw(H, NH, L, 10, 60, max_p, cmin, pairs[:n - 1], pv[:n - 1])
        assert (rc, cnt) == (ctx.ERR_NOMEM, n) and listed > n
        assert (pairs[n - 1:] == 0xABCDEF01).all() and (pv[n - 1:] == POISON).all()
        rc, cnt, _ = ctx.allpairs_sparse_sig_raw(H, NH, L, 10, 60, max_p, cmin, pairs[:n], pv[:n])
        assert (rc, cnt) == (0, n) and (pairs[n] == 0xABCDEF01).all() and pv[n] == POISON
        same(_lib._sorted_sig(pairs[:n], pv[:n]), want)


def test_sig_calls_reject_bad_arguments():
    H, NH, L = sig_set(64)
    with _lib.Context(0, K, 64, 42) as ctx:
        for bad in (-1e-3, 1.0001, float("nan")):
            with pytest.raises(_lib.DrepHipError):
                ctx.allpairs_sparse_sig(H, NH, L, bad)
            with pytest.raises(_lib.DrepHipError):
                ctx.dist_rect_sparse_sig(H[:NQ], NH[:NQ], H, NH, L[:NQ], L, bad)
        zero = L.copy()
        zero[0] = 0                                     # genome 0 holds hashes
        assert NH[0] > 0
        with pytest.raises(_lib.DrepHipError):
            ctx.allpairs_sparse_sig(H, NH, zero)
        with pytest.raises(_lib.DrepHipError):
            ctx.dist_rect_sparse_sig(H[:NQ], NH[:NQ], H, NH, zero[:NQ], L)


# ------------------------------------------------------------ 5. the fixture
def _golden_refs(golden):
    return read_msh(os.path.join(golden, "MASH_files", "ALL.msh")).references


def _query_cache(golden, folder, names):
    chunk = os.path.join(folder, "MASH_files", "sketches", "chunk_0")
    os.makedirs(chunk)
    for n in names:
        shutil.copy(os.path.join(golden, "MASH_files", "sketches", n + ".msh"), os.path.join(chunk, n + ".msh"))


def test_best_hits_p_values(golden, tmp_path):
    refs = _golden_refs(golden)
    names = [os.path.basename(r.name) for r in refs]
    length = {os.path.basename(r.name): r.length for r in refs}
    ref = os.path.join(golden, "MASH_files", "ALL.msh")
    qfolder = str(tmp_path / "queries")
    _query_cache(golden, qfolder, names)
    Qdb = pd.DataFrame({"genome": names, "location": ["/nowhere/" + n for n in names]})
    kw = dict(reference=ref, top=5, query_folder=qfolder)
    plain = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd"), **kw)
    hits = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd"), pvalue=True, **kw)
    assert list(hits.columns) == list(plain.columns) + ["p"] and hits["p"].dtype == np.float64
    pd.testing.assert_frame_equal(hits.drop(columns="p"), plain)
    assert len(hits) == 17                                         # 25 rows less the 8 without a shared hash
    want = _lib.pvalue_eval(hits["common"].to_numpy(), np.array([length[g] for g in hits["genome2"].astype(str)]),
                            np.array([length[g] for g in hits["genome1"].astype(str)]), 1000, K)
    assert np.array_equal(bits(hits["p"].to_numpy()), bits(want))
    three = (hits["common"] == 3).to_numpy()
    assert three.sum() == 6 and ((want[three] > 8e-12) & (want[three] < 1e-11)).all() and (want[~three] == 0).all()
    # -v keeps p <= max_p: the 3/1000 rows (p about 9e-12) pass 1e-10 and fail 1e-12; the ranks stay
    kept = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd"), max_p=1e-10, **kw)
    pd.testing.assert_frame_equal(kept, hits)
    cut = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd"), max_p=1e-12, **kw)
    pd.testing.assert_frame_equal(cut.reset_index(drop=True), hits[~three].reset_index(drop=True))
    with pytest.raises(ValueError):
        d_cluster.query_best_hits(Qdb, str(tmp_path / "wd"), max_p=2.0, **kw)


def test_query_vs_mash_p_values_and_table(golden, tmp_path):
    refs = _golden_refs(golden)
    names = [os.path.basename(r.name) for r in refs]
    ref = os.path.join(golden, "MASH_files", "ALL.msh")
    table = os.path.join(golden, "MASH_files", "MASH_table.tsv")
    qfolder = str(tmp_path / "queries")
    _query_cache(golden, qfolder, names)
    Qdb = pd.DataFrame({"genome": names, "location": [r.name for r in refs]})
    # the rectangle's table from a GPU rectangle: the golden file, byte for byte
    out = tmp_path / "rect.tsv"
    rm = d_cluster.query_vs_MASH_rect(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder,
                                      write_table=str(out))
    assert out.read_bytes() == open(table, "rb").read()
    out2 = tmp_path / "rect2.tsv"
    d_cluster.write_mash_table_rect(str(out2), rm, threads=2)
    assert out2.read_bytes() == open(table, "rb").read()
    # the record form with p-values: the table's rows that share a hash, and -v / -d on the device
    rows = [ln.split("\t") for ln in open(table).read().splitlines()]
    listed = [x for x in rows if not x[4].startswith("0/")]
    full = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_dist=0.99,
                                   pvalue=True)
    assert len(full) == len(listed) == 17
    assert ["%g" % v for v in full["p"]] == [x[3] for x in listed]
    assert list(full["genome1"].astype(str)) == [os.path.basename(x[0]) for x in listed]
    nop = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_dist=0.99)
    pd.testing.assert_frame_equal(full.drop(columns="p"), nop)
    cut = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_p=1e-12)
    assert len(cut) == 11 and list(cut.columns) == list(nop.columns)
    near = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_dist=0.1,
                                   max_p=1e-12, pvalue=True)
    old = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_dist=0.1)
    pd.testing.assert_frame_equal(near.drop(columns="p"), old)
    with pytest.raises(ValueError):
        d_cluster.query_vs_MASH_rect(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_dist=0.1,
                                     write_table=str(out))


def test_write_mash_table_device_equals_host(golden, tmp_path, ctx1000):
    refs = _golden_refs(golden)
    N = len(refs)
    H = np.full((N, 1000), np.iinfo(np.uint64).max, dtype=np.uint64)
    NH = np.zeros(N, dtype=np.uint32)
    for i, r in enumerate(refs):
        H[i, :len(r.hashes)] = r.hashes
        NH[i] = len(r.hashes)
    c, d = ctx1000.allpairs(H, NH)
    names = [r.name for r in refs]
    cm = d_cluster.CondensedMash(names, names, c, d, NH, np.array([r.length for r in refs], np.uint64), 1000)
    host, dev = tmp_path / "host.tsv", tmp_path / "device.tsv"
    d_cluster.write_mash_table(str(host), cm)
    d_cluster.write_mash_table(str(dev), cm, pvalue='device')
    assert dev.read_bytes() == host.read_bytes()
    assert host.read_bytes() == open(os.path.join(golden, "MASH_files", "MASH_table.tsv"), "rb").read()


def test_sparse_mash_with_filters(golden, tmp_path):
    """all_vs_all_MASH_sparse(max_p, max_dist) on the golden sketches: the
    unfiltered list through the evaluator and both rules."""
    refs = _golden_refs(golden)
    names = [os.path.basename(r.name) for r in refs]
    wd = str(tmp_path / "wd")
    _query_cache(golden, wd, names)
    Bdb = pd.DataFrame({"genome": names, "location": ["/nowhere/" + n for n in names]})
    base = d_cluster.all_vs_all_MASH_sparse(Bdb, wd)
    assert base.pval is None and len(base.i) == 6
    L = np.asarray(base.length, np.uint64)
    p = _lib.pvalue_eval(base.common, L[base.i], L[base.j], 1000, K)
    for max_p, max_dist in ((1e-12, None), (None, 0.1), (1.0, 0.99), (1e-12, 0.001)):
        keep = np.ones(6, bool)
        if max_p is not None:
            keep &= p <= max_p
        if max_dist is not None:
            keep &= d_cluster._rect_distance64(base.common, base.denom) <= max_dist
        sm = d_cluster.all_vs_all_MASH_sparse(Bdb, wd, max_p=max_p, max_dist=max_dist)
        assert np.array_equal(sm.i, base.i[keep]) and np.array_equal(sm.j, base.j[keep])
        assert np.array_equal(sm.common, base.common[keep]) and np.array_equal(sm.denom, base.denom[keep])
        assert np.array_equal(bits(sm.pval), bits(p[keep]))
