"""Best hits of a query against a reference (drephip_dist_rect_top*, k_rect_top
in allpairs.hip) and the placement built on them.  Expected hits: the C
oracle's Mash merge of every (query, reference) pair (test_rect.oracle_rect),
then a Python sort by (-Fraction(common, denom), r) -- the contract's order,
stated without the kernel's 64-bit key."""
import os
import shutil
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import edge_cases
import oracle
from drep_amd import _lib
from drep_amd import d_cluster
from drep_amd.mash_io import MashReference, read_msh, write_msh
from test_rect import oracle_rect

pytestmark = pytest.mark.gpu
UMAX = np.iinfo(np.uint64).max
EMPTY = 0xFFFFFFFF
POISON = 0xDEADBEEF


def expected_top(ec, ed, top):
    """(ref [Q, top] with -1 past count, common, denom, count) from a rectangle."""
    Q = ec.shape[0]
    ref = np.full((Q, top), -1, np.int64)
    common = np.zeros((Q, top), np.uint16)
    denom = np.zeros((Q, top), np.uint16)
    count = np.zeros(Q, np.uint32)
    for q in range(Q):
        nz = [int(r) for r in np.nonzero(ec[q])[0]]
        best = sorted(nz, key=lambda r: (-Fraction(int(ec[q, r]), int(ed[q, r])), r))[:top]
        n = len(best)
        ref[q, :n], common[q, :n], denom[q, :n], count[q] = best, ec[q, best], ed[q, best], n
    return ref, common, denom, count


def same(got, exp):
    return all(np.array_equal(g, e) and g.dtype == e.dtype and g.shape == e.shape for g, e in zip(got, exp))


_SETS = {}


def sets(s):
    """geometry_sketches(n, s, seed = 1000 + s) stacked twice as references
    (every hit r ties with r + n), its first rows as queries, and the oracle's
    rectangle; computed once and shared, read-only."""
    if s not in _SETS:
        n, nq = (97, 41) if s <= 2048 else (40, 21)
        H, NH = edge_cases.geometry_sketches(n, s, seed=1000 + s)
        RH, RN = np.concatenate([H, H]), np.concatenate([NH, NH])
        QH, QN = H[:nq].copy(), NH[:nq].copy()
        ec, ed = oracle_rect(QH, QN, RH, RN, s)
        for a in (QH, QN, RH, RN, ec, ed):
            a.setflags(write=False)
        _SETS[s] = (QH, QN, RH, RN, n, ec, ed)
    return _SETS[s]


# ------------------------------------------------------------ 1. variant matrix
@pytest.mark.parametrize("top", [1, 3, 64])
@pytest.mark.parametrize("s", [64, 1000, 4096])
def test_top_variants_vs_oracle(s, top):
    QH, QN, RH, RN, n, ec, ed = sets(s)
    exp = expected_top(ec, ed, top)
    nz = (ec > 0).sum(axis=1)
    # the sets hold what the cases are for
    assert (nz > 64).any() and (nz < top).any() and (nz == 0).any()
    assert len(np.unique(ed[ec > 0])) > 1 and len(np.unique(exp[2][exp[0] >= 0])) > 1
    assert np.array_equal(ec[:, :n], ec[:, n:]) and np.array_equal(ed[:, :n], ed[:, n:])     # r ties with r + n
    if top % 2:                                             # an odd top cuts inside a tie: the next hit has the ratio
        more = expected_top(ec, ed, top + 1)
        cut = [q for q in range(len(QN)) if more[3][q] > top]
        assert cut and all(Fraction(int(more[1][q, top - 1]), int(more[2][q, top - 1])) ==
                           Fraction(int(more[1][q, top]), int(more[2][q, top])) for q in cut)
    with _lib.Context(0, 21, s, 42) as ctx:
        got = ctx.dist_rect_top(QH, QN, RH, RN, top)
        assert same(got, exp), [(q, got[0][q], exp[0][q]) for q in range(len(QN)) if not np.array_equal(got[0][q], exp[0][q])][:3]
        ctx.set_allpairs_path(ctx.AP_MERGE)
        assert same(ctx.dist_rect_top(QH, QN, RH, RN, top), got)
    q_self = [q for q in range(len(QN)) if QN[q] > 0]
    # a query that is also a reference lists itself first (or an identical sketch of a smaller row)
    assert all(got[0][q, 0] <= q and got[1][q, 0] == got[2][q, 0] == QN[q] for q in q_self)
    assert any(got[0][q, 0] == q for q in q_self)


# ------------------------------------------------------------ 2. blocks, ranges
@pytest.mark.parametrize("s", [64, 4096])
def test_top_row_blocks_give_identical_hits(s, monkeypatch):
    QH, QN, RH, RN, n, ec, ed = sets(s)
    exp = expected_top(ec, ed, 5)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_timing(True, kernels=[5])
        for rows in (None, 1, 7):
            if rows is not None:
                monkeypatch.setenv("DREPHIP_RECT_TOP_BLOCK_ROWS", str(rows))
            assert same(ctx.dist_rect_top(QH, QN, RH, RN, 5), exp), rows
            ms, launches = ctx.kernel_ms(5)
            assert launches == (1 if rows is None else -(-len(QN) // rows)) and ms > 0


def test_top_row_range_writes_only_its_slots(monkeypatch):
    s, top = 1000, 3
    QH, QN, RH, RN, n, ec, ed = sets(s)
    ref, common, denom, count = expected_top(ec, ed, top)
    monkeypatch.setenv("DREPHIP_RECT_TOP_BLOCK_ROWS", "7")
    with _lib.Context(0, 21, s, 42) as ctx:
        for q0, q1 in ((3, 38), (30, 1000), (0, 1), (40, 41)):
            rows = min(q1, len(QN)) - q0
            hits = np.full((rows + 2) * top * 4, POISON, np.uint32)     # a guard row before and after
            cnt = np.full(rows + 2, POISON, np.uint32)
            assert ctx.dist_rect_top_raw(QH, QN, RH, RN, top, q0, q1, hits[top * 4:], cnt[1:]) == rows
            hits = hits.reshape(rows + 2, top, 4)
            assert (hits[0] == POISON).all() and (hits[-1] == POISON).all() and cnt[0] == POISON and cnt[-1] == POISON
            assert np.array_equal(cnt[1:-1], count[q0:q0 + rows])
            got = hits[1:-1]
            r = got[:, :, 0].astype(np.int64)
            r[r == EMPTY] = -1
            assert np.array_equal(r, ref[q0:q0 + rows]) and np.array_equal(got[:, :, 1], common[q0:q0 + rows])
            assert np.array_equal(got[:, :, 2], denom[q0:q0 + rows]) and (got[:, :, 3] == 0).all()


# ------------------------------------------------------------ 3. the rectangle
@pytest.mark.parametrize("s", [64, 1000, 4096])
def test_top_hits_are_rectangle_cells(s):
    QH, QN, RH, RN, n, _, _ = sets(s)
    top = 7
    with _lib.Context(0, 21, s, 42) as ctx:
        c, d = ctx.dist_rect(QH, QN, RH, RN)
        hits = np.full((len(QN), top, 4), POISON, np.uint32)
        cnt = np.full(len(QN), POISON, np.uint32)
        ctx.dist_rect_top_raw(QH, QN, RH, RN, top, 0, None, hits, cnt)
    assert np.array_equal(cnt, np.minimum(top, (c > 0).sum(axis=1)))
    for q in range(len(QN)):
        for t in range(top):
            r, hc, hd, z = (int(x) for x in hits[q, t])
            if t < cnt[q]:
                assert (hc, hd, z) == (c[q, r], d[q, r], 0) and hc > 0
            else:
                assert (r, hc, hd, z) == (EMPTY, 0, 0, 0)
        assert len(set(hits[q, :cnt[q], 0])) == cnt[q]                    # each reference at most once


# ------------------------------------------------------------ 4. long rows
def test_top_long_row_past_the_lds_list():
    """One query against 70,000 references at s = 64, more than 20,000 of them
    sharing a hash with it -- several times the kernel's LDS list, so the list
    is cut to its top many times over --, partial sketches among them (mixed
    denominators) and hundreds of equal ratios around the cut."""
    s, N, top = 64, 70000, 64
    rng = np.random.default_rng(64)
    nq = 50                                                              # a partial query: the union decides the denominator
    q = np.sort(rng.choice(np.arange(1, 1 << 20, dtype=np.uint64), size=nq, replace=False))
    R = rng.integers(1 << 21, UMAX - 1, size=(N, s), dtype=np.uint64)
    planted = rng.permutation(N)[:25000]
    for r in planted:
        m = int(rng.integers(1, 41))
        R[r, :m] = rng.choice(q, size=m, replace=False)
    R.sort(axis=1)
    assert (R[:, 1:] != R[:, :-1]).all()
    RN = np.full(N, s, np.uint32)
    part = rng.permutation(N)[:9000]                                     # partial sketches: the smallest hashes kept
    RN[part] = rng.integers(1, s, size=len(part))
    R[np.arange(s)[None, :] >= RN[:, None]] = UMAX
    QH, QN = np.full((1, s), UMAX, np.uint64), np.array([nq], np.uint32)
    QH[0, :nq] = q
    oc, od = oracle.allpairs(np.concatenate([QH, R]), np.concatenate([QN, RN]), s, r0=0, r1=1, threads=8)
    ec, ed = oc[None, :], od[None, :]
    assert ec.shape == (1, N) and (ec > 0).sum() > 20000 and len(np.unique(ed[ec > 0])) > 1
    exp = expected_top(ec, ed, top)
    ratio = [Fraction(int(c), int(d)) for c, d in zip(exp[1][0], exp[2][0])]
    assert len(set(ratio)) < top                                         # ties inside the list
    with _lib.Context(0, 21, s, 42) as ctx:
        assert same(ctx.dist_rect_top(QH, QN, R, RN, top), exp)
        ctx.set_allpairs_path(ctx.AP_MERGE)
        assert same(ctx.dist_rect_top(QH, QN, R, RN, top), exp)


# ------------------------------------------------------------ 5. arguments
def test_top_argument_checks():
    import torch
    s = 64
    QH, QN, RH, RN, n, ec, ed = sets(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        for top in (0, 65):
            with pytest.raises(_lib.DrepHipError):
                ctx.dist_rect_top(QH, QN, RH, RN, top)
        # Q = 1, N = 1
        for q in (0, 5, 11):
            for r in (q, 1):
                got = ctx.dist_rect_top(QH[q:q + 1], QN[q:q + 1], RH[r:r + 1], RN[r:r + 1], 2)
                assert same(got, expected_top(ec[q:q + 1, r:r + 1], ed[q:q + 1, r:r + 1], 2))
        # empty calls write nothing (the device entry point)
        dh = torch.from_numpy(RH.copy().view(np.int64)).cuda()
        dn = torch.from_numpy(RN.copy().view(np.int32)).cuda()
        out = torch.full((len(RN) * 4 * 4,), 0x7EADBEEF, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        N = len(RN)
        for Q, Nr, q0, q1 in ((0, N, 0, 5), (N, 0, 0, N), (N, N, 7, 7), (N, N, 9, 3), (N, N, N, N + 4)):
            ctx.dist_rect_top_device(dh.data_ptr(), dn.data_ptr(), Q, dh.data_ptr(), dn.data_ptr(), Nr, q0, q1, 4,
                                     out.data_ptr(), out.data_ptr())
        ctx.dist_rect_top_device(dh.data_ptr(), dn.data_ptr(), N, dh.data_ptr(), dn.data_ptr(), 0, 0, N, 4, None, None)
        assert (out.cpu().numpy() == 0x7EADBEEF).all()
        with pytest.raises(_lib.DrepHipError):
            ctx.dist_rect_top_device(dh.data_ptr(), dn.data_ptr(), N, dh.data_ptr(), dn.data_ptr(), N, 0, N, 4, None,
                                     out.data_ptr())
        # the device form, filled
        ctx.dist_rect_top_device(dh.data_ptr(), dn.data_ptr(), N, dh.data_ptr(), dn.data_ptr(), N, 2, 6, 4,
                                 out.data_ptr(), out.data_ptr() + 4 * 4 * 4 * 4)
        got = out.cpu().numpy().view(np.uint32)
        exp = expected_top(ec[2:6], ed[2:6], 4)
        r = got[:64].reshape(4, 4, 4)[:, :, 0].astype(np.int64)
        r[r == EMPTY] = -1
        assert np.array_equal(r, exp[0]) and np.array_equal(got[64:68], exp[3]) and (got[68:] == 0x7EADBEEF).all()
        ctx.set_allpairs_path(ctx.AP_BAND, 64)
        with pytest.raises(_lib.DrepHipError):
            ctx.dist_rect_top(QH, QN, RH, RN, 3)


def test_top_two_contexts():
    s = 1000
    QH, QN, RH, RN, n, ec, ed = sets(s)
    one = d_cluster.rect_top_hits(QH, QN, RH, RN, s, 4)
    assert same(one, expected_top(ec, ed, 4))
    assert same(d_cluster.rect_top_hits(QH, QN, RH, RN, s, 4, devices=(0, 0)), one)


# ------------------------------------------------------------ 6. the fixture
def _golden_refs(golden):
    return read_msh(os.path.join(golden, "MASH_files", "ALL.msh")).references


def _query_cache(golden, folder, names):
    """The golden .msh sketches of `names` where sketch_genomes looks for its
    cache, so nothing is sketched."""
    chunk = os.path.join(folder, "MASH_files", "sketches", "chunk_0")
    os.makedirs(chunk)
    for n in names:
        shutil.copy(os.path.join(golden, "MASH_files", "sketches", n + ".msh"), os.path.join(chunk, n + ".msh"))


def test_query_best_hits_rows_are_query_vs_mash_rows(golden, tmp_path):
    names = [os.path.basename(r.name) for r in _golden_refs(golden)]
    ref = os.path.join(golden, "MASH_files", "ALL.msh")
    qfolder = str(tmp_path / "queries")
    _query_cache(golden, qfolder, names)
    Qdb = pd.DataFrame({"genome": names, "location": ["/nowhere/" + n for n in names]})
    hits = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd"), reference=ref, top=5, query_folder=qfolder)
    assert d_cluster.STAGE_TIMES['sketched_genomes'] == 0
    Mdb = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder)
    assert list(hits.columns) == ["genome1", "genome2", "rank", "dist", "similarity", "common", "denom"]
    full = {(a, b): (x, y) for a, b, x, y in zip(Mdb["genome1"].astype(str), Mdb["genome2"].astype(str),
                                                  Mdb["dist"].to_numpy().view(np.uint32),
                                                  Mdb["similarity"].to_numpy().view(np.uint32))}
    got = list(zip(hits["genome1"].astype(str), hits["genome2"].astype(str), hits["dist"].to_numpy().view(np.uint32),
                   hits["similarity"].to_numpy().view(np.uint32)))
    assert len(got) == 17 and all(full[(a, b)] == (x, y) for a, b, x, y in got)      # 25 pairs, 8 of them with Sakai
    assert hits["dist"].dtype == np.float32 and hits["similarity"].dtype == np.float32
    # query-outer in Qdb order, rank-inner, nearest first, itself at rank 0
    assert list(dict.fromkeys(hits["genome2"].astype(str))) == names
    for name, grp in hits.groupby(hits["genome2"].astype(str), sort=False):
        assert list(grp["rank"]) == list(range(len(grp))) and grp["genome1"].astype(str).iloc[0] == name
        assert (np.diff(grp["dist"].to_numpy()) >= 0).all() and grp["common"].iloc[0] == grp["denom"].iloc[0] == 1000
    # max_dist: the rows of query_vs_MASH(max_dist), which are the pairs at or below it
    sub = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd"), reference=ref, top=5, max_dist=0.1, query_folder=qfolder)
    near = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder, max_dist=0.1)
    assert len(sub) == len(near) == 11
    assert sorted(zip(sub["genome2"].astype(str), sub["genome1"].astype(str))) == \
        sorted(zip(near["genome2"].astype(str), near["genome1"].astype(str)))
    assert not os.path.exists(tmp_path / "wd" / "MASH_files")


def test_leave_one_out_placement_is_the_single_linkage_clustering(golden, tmp_path):
    """Each golden genome as the query against the other four, Cdb from their
    single-linkage clustering: place_queries gives the cluster the genome has
    in the single-linkage clustering of all five."""
    refs = _golden_refs(golden)
    names = [os.path.basename(r.name) for r in refs]
    S = 1000
    H = np.full((5, S), UMAX, np.uint64)
    NH = np.zeros(5, np.uint32)
    for i, r in enumerate(refs):
        H[i, :len(r.hashes)], NH[i] = r.hashes, len(r.hashes)
    ln = np.array([r.length for r in refs], np.uint64)

    def cdb_of(idx):
        c, d = oracle.allpairs(H[idx], NH[idx], S)
        cm = d_cluster.CondensedMash([names[i] for i in idx], [names[i] for i in idx], c, d, NH[idx], ln[idx], S)
        return d_cluster.cluster_mash_condensed(cm, clusterAlg='single', P_ani=0.9, gpu=None)[0]
    all5 = cdb_of(list(range(5)))
    members5 = {n: set(all5["genome"][all5["primary_cluster"] == c]) for n, c in zip(all5["genome"], all5["primary_cluster"])}
    placed = {}
    for i in range(5):
        rest = [j for j in range(5) if j != i]
        Cdb = cdb_of(rest)
        msh = str(tmp_path / ("ref%d.msh" % i))
        write_msh(msh, [MashReference(refs[j].name, '', int(ln[j]), H[j, :NH[j]]) for j in rest], 21, S, 42)
        qfolder = str(tmp_path / ("q%d" % i))
        _query_cache(golden, qfolder, [names[i]])
        Qdb = pd.DataFrame({"genome": [names[i]], "location": ["/nowhere/" + names[i]]})
        hits = d_cluster.query_best_hits(Qdb, str(tmp_path / ("wd%d" % i)), reference=msh, top=4, query_folder=qfolder)
        out = d_cluster.place_queries(hits, Cdb, P_ani=0.9)
        assert len(out) == 1 and out["genome"][0] == names[i]
        k = int(out["primary_cluster"][0])
        mates = set(Cdb["genome"][Cdb["primary_cluster"] == k]) if k else set()
        assert mates | {names[i]} == members5[names[i]] and out["n_clusters"][0] == (1 if k else 0)
        placed[names[i]] = (k, mates, out["nearest"][0], out["dist"][0])
    faecalis = {n for n in names if "faecalis" in n}
    assert len(faecalis) == 3
    for n in faecalis:                                              # T2, TX0104, YI6-1 join each other's cluster
        assert placed[n][0] > 0 and placed[n][1] == faecalis - {n}
    ec20 = placed["Enterococcus_casseliflavus_EC20.fasta"]
    assert ec20[0] == 0 and ec20[2] in faecalis and abs(float(ec20[3]) - 0.2438) < 5e-5
    sakai = placed["Escherichia_coli_Sakai.fna"]
    assert sakai[0] == 0 and sakai[2] is None and np.isnan(sakai[3])
