"""Query against reference (drephip_dist_rect*, the RECT flavour of
k_allpairs_q and k_rect_merge in allpairs.hip): `mash dist <reference.msh>
<query.msh>`, the two-file form of drep/d_cluster.py:569-573.  Every (query,
reference) cell is checked bit for bit on common and denom against the C
oracle's Mash merge -- self pairs included, which the triangle kernels never
produce --, through every kernel variant the whole-row path selects, the merge
kernel, row ranges, the record form, and end to end against the golden
MASH_table.tsv (a 5 x 5 rectangle of ALL.msh against itself)."""
import glob
import os
import shutil

import numpy as np
import pandas as pd
import pytest

import edge_cases
import oracle
from drep_amd import _lib
from drep_amd import d_cluster
from drep_amd.mash_io import read_msh

pytestmark = pytest.mark.gpu
UMAX = np.iinfo(np.uint64).max
ERR_NOMEM = -4
NQ = 41           # not a multiple of any R (1, 2, 4, 8)
NREF = 97         # not a multiple of the 16-column tile


def oracle_rect(Hq, NHq, Hr, NHr, s):
    """(common, denom) [Q, N] of every (query, reference) pair by the oracle's
    merge (oracle_dist_pair, run over the pairs of the stacked matrix by
    oracle.allpairs: a query that is also a reference is two rows there, so the
    self pairs are ordinary pairs of the stack)."""
    Q, N = len(NHq), len(NHr)
    if Q == 0 or N == 0:
        return np.zeros((Q, N), np.uint16), np.zeros((Q, N), np.uint16)
    H = np.concatenate([Hq, Hr])
    NH = np.concatenate([NHq, NHr]).astype(np.uint32)
    oc, od = oracle.allpairs(H, NH, s, threads=8)
    M = Q + N
    q = np.arange(Q, dtype=np.int64)[:, None]
    r = np.arange(N, dtype=np.int64)[None, :] + Q
    t = q * M - q * (q + 1) // 2 + (r - q - 1)
    return oc[t], od[t]


_CASES = {}


def case(s):
    """The case-1 sets at sketch size s and their expected rectangle, computed
    once and shared (read-only): geometry_sketches(97, s) as references, its
    rows 0..40 as queries -- zero-key tiles, twin rows 7 / 23 / 39, partial and
    empty rows, and every query also a reference.  s = 4096: 40 references,
    21 queries (the merge route)."""
    if s not in _CASES:
        n, nq = (NREF, NQ) if s <= 2048 else (40, 21)
        H, NH = edge_cases.geometry_sketches(n, s, seed=1000 + s)
        exp = oracle_rect(H[:nq], NH[:nq], H, NH, s)
        for a in (H, NH) + exp:
            a.setflags(write=False)
        _CASES[s] = (H, NH, nq, exp)
    return _CASES[s]


def test_oracle_self_pairs():
    """What the expected values say of the cells the triangle never had."""
    A = np.arange(1, 65, dtype=np.uint64)
    assert oracle.dist_pair(A, A, 64) == (64, 64)
    assert oracle.dist_pair(A[:10], A[:10], 64) == (10, 10)
    assert oracle.dist_pair(A[:0], A[:0], 64) == (0, 0)
    assert edge_cases.ref_pair(A[:10], A[:10], 64) == (10, 10)


# ------------------------------------------------------------ 1. variant matrix
_VARIANTS = [(s, None, None) for s in (64, 100, 600, 1000, 1025, 2048)]
_VARIANTS += [(s, r, None) for s in (64, 1000) for r in (1, 2, 4, 8)]
_VARIANTS += [(s, None, 0) for s in (64, 1000)]


@pytest.mark.parametrize("s,R,hit", _VARIANTS)
def test_rect_variants_vs_oracle(s, R, hit, monkeypatch):
    H, NH, nq, (ec, ed) = case(s)
    if R is not None:
        monkeypatch.setenv("DREPHIP_AP_R", str(R))
    if hit is not None:
        monkeypatch.setenv("DREPHIP_AP_HIT", str(hit))
    with _lib.Context(0, 21, s, 42) as ctx:
        c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
    assert c.shape == (nq, NREF) and c.dtype == np.uint16 and d.dtype == np.uint16
    assert np.array_equal(c, ec), np.argwhere(c != ec)[:8]
    assert np.array_equal(d, ed), np.argwhere(d != ed)[:8]
    # the sets do hold what the variants are for
    full = (NH[:nq] == s)
    assert (ec[np.arange(nq)[full], np.arange(nq)[full]] == s).all()      # self rows: s / s
    assert (NH[:nq] == 0).any() and ((NH[:nq] > 0) & (NH[:nq] < s)).any() and (H[:nq, 0] == 0).any()


@pytest.mark.parametrize("s", [64, 100, 600, 1000, 1025, 2048, 4096])
def test_rect_merge_kernel_vs_oracle(s):
    """k_rect_merge: through drephip_dist_rect_merge_device at every s, and as
    the route DREPHIP_AP_AUTO takes above the tables (s = 4096)."""
    H, NH, nq, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        c, d = ctx.dist_rect_merge(H[:nq], NH[:nq], H, NH)
        assert np.array_equal(c, ec) and np.array_equal(d, ed)
        if s > 2048:
            c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
            assert np.array_equal(c, ec) and np.array_equal(d, ed)
            ctx.set_allpairs_path(ctx.AP_MERGE)
            c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
            assert np.array_equal(c, ec) and np.array_equal(d, ed)


def test_rect_band_path_is_unsupported():
    H, NH, nq, _ = case(100)
    with _lib.Context(0, 21, 100, 42) as ctx:
        ctx.set_allpairs_path(ctx.AP_BAND, 64)
        with pytest.raises(_lib.DrepHipError):
            ctx.dist_rect(H[:nq], NH[:nq], H, NH)


# ------------------------------------------------------------ 2. rank edges
@pytest.mark.parametrize("s", [64, 1000])
def test_rect_rank_edges(s):
    """Every planted pair (a shared hash at union rank s - 2, s - 1, s around
    every chunk edge of the column): the A sides as queries against the B sides
    as references, then swapped.  The diagonal is the planted pair; every
    other cell is checked against the oracle too."""
    pp = edge_cases.planted_rank_pairs(s, seed=s)
    want = edge_cases.rank_pair_expected(pp)
    P = len(want)
    with _lib.Context(0, 21, s, 42) as ctx:
        for p0 in range(0, P, 100):                     # blocks as rank_pair_matrices cuts them
            p1 = min(P, p0 + 100)
            A, B = pp["A"][p0:p1], pp["B"][p0:p1]
            nh = np.full(p1 - p0, s, dtype=np.uint32)
            ec, ed = oracle_rect(A, nh, B, nh, s)
            assert np.array_equal(np.diag(ec), want[p0:p1])
            c, d = ctx.dist_rect(A, nh, B, nh)
            assert np.array_equal(np.diag(c), want[p0:p1]), (p0, np.nonzero(np.diag(c) != want[p0:p1])[0][:8])
            assert np.array_equal(c, ec) and np.array_equal(d, ed)
            c, d = ctx.dist_rect(B, nh, A, nh)
            assert np.array_equal(np.diag(c), want[p0:p1])
            assert np.array_equal(c, ec.T) and np.array_equal(d, ed.T)


# ------------------------------------------------------------ 3. row ranges, bounds
def test_rect_row_range_writes_only_its_cells():
    s = 100
    H, NH, nq, (ec, ed) = case(s)
    q0, q1 = 3, 38
    with _lib.Context(0, 21, s, 42) as ctx:
        bc = np.full((q1 - q0 + 2, NREF), 0xBEEF, dtype=np.uint16)    # a guard row before and after
        bd = np.full((q1 - q0 + 2, NREF), 0xBEEF, dtype=np.uint16)
        ctx.dist_rect(H[:nq], NH[:nq], H, NH, q0, q1, bc[1:-1], bd[1:-1])
        assert (bc[0] == 0xBEEF).all() and (bc[-1] == 0xBEEF).all()
        assert (bd[0] == 0xBEEF).all() and (bd[-1] == 0xBEEF).all()
        assert np.array_equal(bc[1:-1], ec[q0:q1]) and np.array_equal(bd[1:-1], ed[q0:q1])
        # q1 is clamped to Q
        c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH, 30, 1000)
        assert np.array_equal(c, ec[30:]) and np.array_equal(d, ed[30:])


@pytest.mark.parametrize("n", [1, 15, 17])
def test_rect_one_query_few_references(n):
    s = 100
    H, NH, _, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        for q in (0, 5, 11):                                     # zero key, partial, empty
            c, d = ctx.dist_rect(H[q:q + 1], NH[q:q + 1], H[:n], NH[:n])
            assert np.array_equal(c, ec[q:q + 1, :n]) and np.array_equal(d, ed[q:q + 1, :n])


def test_rect_device_empty_calls_write_nothing():
    """Q == 0, N == 0 and q0 >= q1 return OK and leave the outputs alone
    (device entry points, both kernels)."""
    import torch
    s = 100
    H, NH, nq, _ = case(s)
    dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    out = torch.full((nq * NREF,), 0x7EEF, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _lib.Context(0, 21, s, 42) as ctx:
        for merge in (False, True):
            for Q, N, q0, q1 in ((0, NREF, 0, 5), (nq, 0, 0, nq), (nq, NREF, 7, 7), (nq, NREF, 9, 3), (nq, NREF, nq, nq + 4)):
                ctx.dist_rect_device(dh.data_ptr(), dn.data_ptr(), Q, dh.data_ptr(), dn.data_ptr(), N, q0, q1,
                                     out.data_ptr(), out.data_ptr(), merge=merge)
        rc, n = ctx.dist_rect_sparse_device(dh.data_ptr(), dn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), 0, 0, nq,
                                            None, 0)
        assert (rc, n) == (0, 0)
    assert (out.cpu().numpy() == 0x7EEF).all()


# ------------------------------------------------------------ 4. symmetry
@pytest.mark.parametrize("s", [100, 1000])
def test_rect_symmetry(s):
    H, NH, nq, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        c1, d1 = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
        c2, d2 = ctx.dist_rect(H, NH, H[:nq], NH[:nq])
    assert np.array_equal(c1, c2.T) and np.array_equal(d1, d2.T)
    assert np.array_equal(c1, ec)


# ------------------------------------------------------------ 5. failed table build
def unbuildable_rows(S=1000):
    """Rows 0 and 7 hold three hashes with one low word (no cuckoo table can
    hold them); rows 1 and 8 share two of them.  (The construction of
    tests/test_gpu.py's failed-build test, restated here.)"""
    rng = np.random.default_rng(3)
    N = 24
    base = np.sort(rng.choice(2 ** 62, size=(N, 2000), replace=False).astype(np.uint64), axis=1)
    h = np.full((N, S), UMAX, dtype=np.uint64)
    for i in range(N):                                   # families: shared prefixes
        pool = base[i // 6]
        keep = np.sort(rng.choice(len(pool), S, replace=False))
        h[i] = pool[keep]
    lo = np.uint64(0x12345678)
    bad = np.array([(np.uint64(k) << np.uint64(40)) | lo for k in (1, 2, 3)], dtype=np.uint64)
    for i in (0, 7):
        row = np.unique(np.concatenate([h[i][:S - 3], bad]))
        h[i] = row[:S]
        h[i + 1] = np.unique(np.concatenate([h[i + 1][:S - 2], bad[:2]]))[:S]
    return h, np.full(N, S, np.uint32)


@pytest.mark.parametrize("partial", [False, True])
def test_rect_failed_table_build(partial):
    """Query rows whose table cannot be built are merged literally inside the
    RECT kernel, against every reference (themselves included)."""
    S = 1000
    h, nh = unbuildable_rows(S)
    rh, rnh = h.copy(), nh.copy()
    if partial:
        for i in (1, 7, 12):
            rnh[i] = 300 + i
            rh[i, rnh[i]:] = UMAX
    qh, qnh = rh[:10], rnh[:10]                       # rows 0, 7 fail; 1, 8 share their bad keys
    ec, ed = oracle_rect(qh, qnh, rh, rnh, S)
    with _lib.Context(0, 21, S, 42) as ctx:
        c, d = ctx.dist_rect(qh, qnh, rh, rnh)
        q, r, rc_, rd_ = ctx.dist_rect_sparse(qh, qnh, rh, rnh)
    assert np.array_equal(c, ec) and np.array_equal(d, ed)
    assert ec[0, 0] == S and ec[0, 1] >= 2 and (not partial or (ed < S).any())
    k = ec > 0
    qq, rr = np.nonzero(k)
    assert np.array_equal(q, qq) and np.array_equal(r, rr) and np.array_equal(rc_, ec[k]) and np.array_equal(rd_, ed[k])


# ------------------------------------------------------------ 6. record form
@pytest.mark.parametrize("s", [64, 1000, 2048, 4096])
def test_rect_records_are_the_nonzero_cells(s):
    import torch
    H, NH, nq, (ec, ed) = case(s)
    nref = len(NH)
    k = ec > 0
    qq, rr = np.nonzero(k)
    need = int(k.sum())
    assert need > nq
    with _lib.Context(0, 21, s, 42) as ctx:
        q, r, c, d = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, cap=need + 5)
        assert np.array_equal(q, qq) and np.array_equal(r, rr) and np.array_equal(c, ec[k]) and np.array_equal(d, ed[k])
        # the default buffer is too small at these sizes or not: either way the same list
        q2, r2, c2, d2 = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, cap=7)
        assert np.array_equal(q2, qq) and np.array_equal(r2, rr) and np.array_equal(c2, ec[k])
        # a row range
        q3, r3, c3, d3 = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, 3, 17, cap=need)
        k3 = (qq >= 3) & (qq < 17)
        assert np.array_equal(q3, qq[k3]) and np.array_equal(r3, rr[k3]) and np.array_equal(d3, ed[k][k3])
        # cap = 0 counts; cap = need - 1: NOMEM, the size needed, nothing past cap
        dqh = torch.from_numpy(H[:nq].copy().view(np.int64)).cuda()
        dqn = torch.from_numpy(NH[:nq].copy().view(np.int32)).cuda()
        drh = torch.from_numpy(H.copy().view(np.int64)).cuda()
        drn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
        args = (dqh.data_ptr(), dqn.data_ptr(), nq, drh.data_ptr(), drn.data_ptr(), nref, 0, nq)
        torch.cuda.synchronize()
        assert ctx.dist_rect_sparse_device(*args, None, 0) == (ERR_NOMEM, need)
        buf = torch.full((need + 8, 4), 0x7EADBEEF, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ctx.dist_rect_sparse_device(*args, buf.data_ptr(), need - 1) == (ERR_NOMEM, need)
        got = buf.cpu().numpy()
        assert (got[need - 1:] == 0x7EADBEEF).all()
        rec = got[:need - 1].view(np.uint32)
        assert len(set(map(tuple, rec[:, :2]))) == need - 1                 # each pair at most once
        assert all(ec[a, b] == cc and ed[a, b] == dd and cc > 0 for a, b, cc, dd in rec)
        buf.fill_(0x7EADBEEF)
        torch.cuda.synchronize()
        assert ctx.dist_rect_sparse_device(*args, buf.data_ptr(), need) == (0, need)
        rec = buf.cpu().numpy()[:need].view(np.uint32)
        rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
        assert np.array_equal(rec[:, 0], qq) and np.array_equal(rec[:, 1], rr) and np.array_equal(rec[:, 2], ec[k])


@pytest.mark.parametrize("s", [64, 4096])
def test_rect_records_of_disjoint_sets(s):
    rng = np.random.default_rng(s)
    v = np.unique(rng.integers(1, UMAX - 1, size=40 * s, dtype=np.uint64))[:30 * s]
    rng.shuffle(v)
    M = np.sort(v.reshape(30, s), axis=1)
    nh = np.full(30, s, np.uint32)
    with _lib.Context(0, 21, s, 42) as ctx:
        q, r, c, d = ctx.dist_rect_sparse(M[:9], nh[:9], M[9:], nh[9:])
        assert len(q) == len(r) == len(c) == len(d) == 0
        c2, d2 = ctx.dist_rect(M[:9], nh[:9], M[9:], nh[9:])
        assert (c2 == 0).all() and (d2 == s).all()


# ------------------------------------------------------------ 7. the fixture
def _golden_names(golden):
    return [os.path.basename(r.name) for r in read_msh(os.path.join(golden, "MASH_files", "ALL.msh")).references]


def _query_cache(golden, folder, names):
    """The golden .msh sketches of `names` where sketch_genomes looks for its
    cache, so nothing is sketched."""
    chunk = os.path.join(folder, "MASH_files", "sketches", "chunk_0")
    os.makedirs(chunk)
    for n in names:
        shutil.copy(os.path.join(golden, "MASH_files", "sketches", n + ".msh"), os.path.join(chunk, n + ".msh"))


def test_query_vs_mash_equals_golden_table(golden, tmp_path):
    names = _golden_names(golden)
    ref = os.path.join(golden, "MASH_files", "ALL.msh")
    table = os.path.join(golden, "MASH_files", "MASH_table.tsv")
    qfolder = str(tmp_path / "queries")
    _query_cache(golden, qfolder, names)
    Qdb = pd.DataFrame({"genome": names, "location": ["/nowhere/" + n for n in names]})
    Mdb = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder)
    assert d_cluster.STAGE_TIMES['sketched_genomes'] == 0
    exp = d_cluster._parse_mash_table(table, Qdb)
    assert len(Mdb) == len(exp) == 25
    assert list(Mdb.columns) == list(exp.columns)
    for col in ("genome1", "genome2"):
        assert list(Mdb[col].astype(str)) == list(exp[col].astype(str))
        assert list(Mdb[col].cat.categories) == list(exp[col].cat.categories) and Mdb[col].cat.ordered
    for col in ("dist", "similarity"):
        assert Mdb[col].dtype == np.float32 and exp[col].dtype == np.float32
        assert np.array_equal(Mdb[col].to_numpy().view(np.uint32), exp[col].to_numpy().view(np.uint32))
    # the 25 common/denom pairs are the table's kmers column, self rows included
    rm = d_cluster.query_vs_MASH_rect(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder)
    kmers = [ln.split("\t")[4] for ln in open(table).read().splitlines()]
    got = ["%d/%d" % (rm.common[q, r], rm.denom[q, r]) for q in range(5) for r in range(5)]
    assert got == kmers and [got[6 * i] for i in range(5)] == ["1000/1000"] * 5
    # the record form keeps the rows at or below max_dist
    sub = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_dist=0.1)
    keep = exp["dist"].to_numpy() <= 0.1
    assert keep.sum() > 5 and len(sub) == keep.sum()
    assert np.array_equal(sub["dist"].to_numpy().view(np.uint32), exp["dist"].to_numpy()[keep].view(np.uint32))
    assert list(sub["genome1"].astype(str)) == list(exp["genome1"].astype(str)[keep])
    assert not os.path.exists(tmp_path / "wd" / "MASH_files")          # the reference's folder is never touched


# ------------------------------------------------------------ 8. end to end
def test_query_vs_mash_sketches_fasta_queries(golden, tmp_path):
    """Two golden FASTA genomes sketched on the GPU as queries against ALL.msh:
    the same rows as the golden table's; one and two contexts."""
    ref = os.path.join(golden, "MASH_files", "ALL.msh")
    table = os.path.join(golden, "MASH_files", "MASH_table.tsv")
    fas = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))[1:3]
    locs = []
    for f in fas:                                       # under the names the table knows them by
        dst = tmp_path / os.path.basename(f)
        shutil.copy(f, dst)
        locs.append(str(dst))
    qn = [os.path.basename(f)[:-3] for f in fas]
    Qdb = pd.DataFrame({"genome": qn, "location": locs})
    allnames = _golden_names(golden)
    full = d_cluster._parse_mash_table(table, pd.DataFrame({"genome": allnames}))
    exp = full[full["genome2"].astype(str).isin(qn)]
    for k, gpus in enumerate((None, [0, 0])):
        kw = {} if gpus is None else {"gpus": gpus}
        Mdb = d_cluster.query_vs_MASH(Qdb, str(tmp_path / ("wd%d" % k)), reference=ref, **kw)
        assert d_cluster.STAGE_TIMES['sketched_genomes'] == 2
        assert len(Mdb) == 10
        assert list(Mdb["genome2"].astype(str)) == list(exp["genome2"].astype(str))
        assert list(Mdb["genome1"].astype(str)) == list(exp["genome1"].astype(str))
        assert np.array_equal(Mdb["dist"].to_numpy().view(np.uint32), exp["dist"].to_numpy().view(np.uint32))
        assert os.path.isdir(tmp_path / ("wd%d" % k) / "MASH_query" / "MASH_files")
