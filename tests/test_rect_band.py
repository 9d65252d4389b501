"""The RECT flavour of k_allpairs_band (allpairs.hip): the query-against-
reference rectangle above the whole-row tables (s > 2048 under DREPHIP_AP_AUTO)
and, forced, at small sketches where small caps make many bands.  Expected
values: the C oracle's Mash merge of every (query, reference) pair, bit for bit
on common and denom.  Every test asserts the kernel the call reports
(drephip_last_rect_info), except where the merge rerun is the point."""
import glob
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import edge_cases
import oracle
from drep_amd import _lib
from drep_amd import d_cluster
from drep_amd.mash_io import MashReference, write_msh

pytestmark = pytest.mark.gpu
UMAX = np.iinfo(np.uint64).max
ERR_NOMEM = -4
AP_TABLE, AP_BAND, AP_MERGE = 1, 2, 3
NQ = 41            # 10 row tiles of 4 and one of a single row
NREF = 257         # 2 x 128 + 1: three column tiles, the last of one column
POISON = 0x7EEF
_PLAN = re.compile(r"\[drephip\] rect band plan: R 4 C 128 cap (\d+) items (\d+) slots (\d+) pieces (\d+)")


def oracle_rect(Hq, NHq, Hr, NHr, s):
    """(common, denom) [Q, N] of every (query, reference) pair by the oracle's
    merge, run over the pairs of the stacked matrix (test_rect.py's, restated:
    a query that is also a reference is two rows of the stack, so the self
    pairs are ordinary pairs there)."""
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


def case(s, n=NREF, nq=NQ):
    """geometry_sketches(n, s) as references, its first nq rows as queries, and
    the oracle's rectangle; computed once and shared, read-only."""
    key = (s, n, nq)
    if key not in _CASES:
        H, NH = edge_cases.geometry_sketches(n, s, seed=1000 + s)
        exp = oracle_rect(H[:nq], NH[:nq], H, NH, s)
        for a in (H, NH) + exp:
            a.setflags(write=False)
        _CASES[key] = (H, NH, nq, exp)
    return _CASES[key]


def band_rect(ctx, QH, QN, H, NH, *a, **kw):
    """dist_rect, with the kernel it reports checked: the band kernel, no rerun."""
    out = ctx.dist_rect(QH, QN, H, NH, *a, **kw)
    assert ctx.last_rect_info() == (AP_BAND, 0)
    return out


# ------------------------------------------------------------ 1. the natural route
@pytest.mark.parametrize("cap", [768, 64, 300])
def test_band_natural_route_vs_oracle(cap):
    s = 4096
    H, NH, nq, (ec, ed) = case(s)
    QH, QN = H[:nq], NH[:nq]
    # the set holds what it is for
    assert (QH[:4, 0] == 0).all() and QN[11] == 0 and QN[28] == 0 and 0 < QN[5] < s and 0 < QN[12] < s
    assert ((ed < s) & (ed > 0)).any() and nq % 4 == 1 and NREF % 128 == 1
    full = np.nonzero(QN == s)[0]
    assert (ec[full, full] == s).all() and (ed[full, full] == s).all()
    part = np.nonzero(QN < s)[0]
    assert np.array_equal(ec[part, part], QN[part]) and np.array_equal(ed[part, part], QN[part])   # n / n, 0 / 0
    with _lib.Context(0, 21, s, 42) as ctx:
        assert ctx.last_rect_info() == (0, 0)
        if cap != 768:
            ctx.set_rect_band(ctx.RECT_BAND_AUTO, cap)
        c, d = band_rect(ctx, QH, QN, H, NH)
        assert c.shape == (nq, NREF) and c.dtype == np.uint16 and d.dtype == np.uint16
        assert np.array_equal(c, ec), np.argwhere(c != ec)[:8]
        assert np.array_equal(d, ed), np.argwhere(d != ed)[:8]
        # denom = None (device form: a null pointer)
        import torch
        dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
        dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
        out = torch.full((nq * NREF,), POISON, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ctx.dist_rect_device(dh.data_ptr(), dn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), NREF, 0, nq,
                             out.data_ptr(), None)
        assert ctx.last_rect_info() == (AP_BAND, 0)
        assert np.array_equal(out.cpu().numpy().view(np.uint16).reshape(nq, NREF), ec)


# ------------------------------------------------------------ 2. forced at small sketches
@pytest.mark.parametrize("cap", [64, 300])
@pytest.mark.parametrize("s", [100, 1000, 2049])
def test_band_forced_at_small_sketches(s, cap):
    H, NH, nq, (ec, ed) = case(s, 97, 41)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_band(ctx.RECT_BAND_FORCE, cap)
        c, d = band_rect(ctx, H[:nq], NH[:nq], H, NH)
        assert np.array_equal(c, ec), np.argwhere(c != ec)[:8]
        assert np.array_equal(d, ed), np.argwhere(d != ed)[:8]
        if s <= 2048:                                   # the table route on the same context
            ctx.set_rect_band(ctx.RECT_BAND_AUTO, cap)
            ct, dt = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
            assert ctx.last_rect_info() == (AP_TABLE, 0)
            assert np.array_equal(c, ct) and np.array_equal(d, dt)


@pytest.mark.parametrize("cap", [64, 300])
def test_band_forced_at_the_largest_sketch(cap):
    """s = 32767: counts and denominators at the uint16 edge on the self cells."""
    s = 32767
    H, NH, nq, (ec, ed) = case(s, 9, 5)
    full = np.nonzero(NH[:nq] == s)[0]
    assert len(full) and (ec[full, full] == s).all() and (ed[full, full] == s).all()
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_band(ctx.RECT_BAND_FORCE, cap)
        c, d = band_rect(ctx, H[:nq], NH[:nq], H, NH)
    assert np.array_equal(c, ec), np.argwhere(c != ec)[:8]
    assert np.array_equal(d, ed), np.argwhere(d != ed)[:8]


# ------------------------------------------------------------ 3. rank edges
def test_band_rank_edges_forced():
    """test_rect.py's rank-edge sweep at s = 1000 through the band kernel at cap
    64: the A sides against the B sides, then swapped, in blocks of 100."""
    s = 1000
    pp = edge_cases.planted_rank_pairs(s, seed=s)
    want = edge_cases.rank_pair_expected(pp)
    P = len(want)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        for p0 in range(0, P, 100):
            p1 = min(P, p0 + 100)
            A, B = pp["A"][p0:p1], pp["B"][p0:p1]
            nh = np.full(p1 - p0, s, dtype=np.uint32)
            ec, ed = oracle_rect(A, nh, B, nh, s)
            assert np.array_equal(np.diag(ec), want[p0:p1])
            c, d = band_rect(ctx, A, nh, B, nh)
            assert np.array_equal(np.diag(c), want[p0:p1]), (p0, np.nonzero(np.diag(c) != want[p0:p1])[0][:8])
            assert np.array_equal(c, ec) and np.array_equal(d, ed)
            c, d = band_rect(ctx, B, nh, A, nh)
            assert np.array_equal(np.diag(c), want[p0:p1])
            assert np.array_equal(c, ec.T) and np.array_equal(d, ed.T)


def test_band_rank_edges_natural():
    """The same construction at s = 4096 under AUTO.  A planted pair shares
    nothing with another pair, so every off-diagonal cell is 0 / s and the
    diagonal is rank_pair_expected: no oracle run."""
    s = 4096
    pp = edge_cases.planted_rank_pairs(s, seed=s)
    want = edge_cases.rank_pair_expected(pp)
    P = len(want)
    with _lib.Context(0, 21, s, 42) as ctx:
        for p0 in range(0, P, 1000):
            p1 = min(P, p0 + 1000)
            A, B = pp["A"][p0:p1], pp["B"][p0:p1]
            nh = np.full(p1 - p0, s, dtype=np.uint32)
            off = ~np.eye(p1 - p0, dtype=bool)
            for X, Y in ((A, B), (B, A)):
                c, d = band_rect(ctx, X, nh, Y, nh)
                assert np.array_equal(np.diag(c), want[p0:p1]), (p0, np.nonzero(np.diag(c) != want[p0:p1])[0][:8])
                assert (c[off] == 0).all() and (d == s).all()


# ------------------------------------------------------------ 4. row ranges, edges
def _device_sets(H, NH):
    import torch
    dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    torch.cuda.synchronize()
    return dh, dn


@pytest.mark.parametrize("q0,q1", [(3, 38), (0, 1), (40, 41)])
def test_band_row_range_writes_only_its_cells(q0, q1):
    """Poisoned device buffers with a guard region before and after the rows."""
    import torch
    s = 4096
    H, NH, nq, (ec, ed) = case(s)
    dh, dn = _device_sets(H, NH)
    G = 2 * NREF + 5                                    # guard cells on either side (not a whole row)
    cells = (q1 - q0) * NREF
    bc = torch.full((cells + 2 * G,), POISON, dtype=torch.int16, device="cuda")
    bd = torch.full((cells + 2 * G,), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.dist_rect_device(dh.data_ptr(), dn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), NREF, q0, q1,
                             bc.data_ptr() + 2 * G, bd.data_ptr() + 2 * G)
        assert ctx.last_rect_info() == (AP_BAND, 0)
    for buf, exp in ((bc, ec), (bd, ed)):
        got = buf.cpu().numpy().view(np.uint16)
        assert (got[:G] == POISON).all() and (got[G + cells:] == POISON).all()
        assert np.array_equal(got[G:G + cells].reshape(q1 - q0, NREF), exp[q0:q1])


@pytest.mark.parametrize("n", [1, 128, 129])
def test_band_one_query_and_tile_edges(n):
    s = 4096
    H, NH, nq, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        for q in (0, 5, 11):                                     # zero key, partial, empty
            c, d = band_rect(ctx, H[q:q + 1], NH[q:q + 1], H[:n], NH[:n])
            assert np.array_equal(c, ec[q:q + 1, :n]) and np.array_equal(d, ed[q:q + 1, :n])
        # q1 is clamped to Q
        c, d = band_rect(ctx, H[:nq], NH[:nq], H[:n], NH[:n], 30, 1000)
        assert np.array_equal(c, ec[30:, :n]) and np.array_equal(d, ed[30:, :n])


def test_band_empty_calls_write_nothing():
    import torch
    s = 4096
    H, NH, nq, _ = case(s)
    dh, dn = _device_sets(H, NH)
    out = torch.full((nq * NREF,), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _lib.Context(0, 21, s, 42) as ctx:
        for Q, N, q0, q1 in ((0, NREF, 0, 5), (nq, 0, 0, nq), (nq, NREF, 7, 7), (nq, NREF, 9, 3), (nq, NREF, nq, nq + 4)):
            ctx.dist_rect_device(dh.data_ptr(), dn.data_ptr(), Q, dh.data_ptr(), dn.data_ptr(), N, q0, q1,
                                 out.data_ptr(), out.data_ptr())
        assert ctx.last_rect_info() == (0, 0)           # an empty call chooses no kernel
    assert (out.cpu().numpy().view(np.uint16) == POISON).all()


# ------------------------------------------------------------ 5. split launches
def test_band_split_launches(monkeypatch, capfd):
    s = 4096
    H, NH, nq, (ec, ed) = case(s)
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    with _lib.Context(0, 21, s, 42) as ctx:
        capfd.readouterr()
        band_rect(ctx, H[:nq], NH[:nq], H, NH)
        (cap, items, slots, pieces), = [tuple(map(int, m)) for m in _PLAN.findall(capfd.readouterr().err)]
        assert (cap, items, pieces) == (768, 11 * 3, 1) and slots >= items and slots % 8 == 0
        monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", "8192")      # 8 items per dispatch of the 1024-lane kernel
        c, d = band_rect(ctx, H[:nq], NH[:nq], H, NH)
        (cap, items, slots2, pieces), = [tuple(map(int, m)) for m in _PLAN.findall(capfd.readouterr().err)]
        assert slots2 == slots and pieces == -(-slots // 8) and pieces > 1
    assert np.array_equal(c, ec) and np.array_equal(d, ed)


# ------------------------------------------------------------ 6. unbuildable band table
def unbuildable_rows(S=1000):
    """Rows 0 and 7 hold three hashes with one low word (no cuckoo table can
    hold them), the three smallest of the row: they sit in its first band at
    any cap.  Rows 1 and 8 share two of them.  (The construction of
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
def test_band_unbuildable_table_reruns_by_merge(partial):
    S = 1000
    h, nh = unbuildable_rows(S)
    rh, rnh = h.copy(), nh.copy()
    if partial:
        for i in (1, 7, 12):
            rnh[i] = 300 + i
            rh[i, rnh[i]:] = UMAX
    qh, qnh = rh[:10], rnh[:10]
    assert np.array_equal(qh[0, :3] & np.uint64(0xFFFFFFFF), np.full(3, 0x12345678, np.uint64))
    ec, ed = oracle_rect(qh, qnh, rh, rnh, S)
    assert ec[0, 0] == S and ec[0, 1] >= 2 and (not partial or (ed < S).any())
    with _lib.Context(0, 21, S, 42) as ctx:
        ctx.set_rect_band(ctx.RECT_BAND_FORCE, 256)
        c, d = ctx.dist_rect(qh, qnh, rh, rnh)
        assert ctx.last_rect_info()[1] == 1
        assert np.array_equal(c, ec) and np.array_equal(d, ed)
        # a clean call on the same context (rows 2..5: their tables build)
        c2, d2 = band_rect(ctx, qh[2:6], qnh[2:6], rh, rnh)
        assert np.array_equal(c2, ec[2:6]) and np.array_equal(d2, ed[2:6])
        # and the failing call again
        c, d = ctx.dist_rect(qh, qnh, rh, rnh)
        assert ctx.last_rect_info()[1] == 1
        assert np.array_equal(c, ec) and np.array_equal(d, ed)


# ------------------------------------------------------------ 7. records and best hits
def expected_top(ec, ed, top):
    """(ref [Q, top] with -1 past count, common, denom, count) from a rectangle:
    the contract's order, (-Fraction(common, denom), r) (test_rect_top.py's)."""
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


@pytest.mark.parametrize("rows", [None, 7])
def test_band_records(rows, monkeypatch):
    import torch
    s = 4096
    H, NH, nq, (ec, ed) = case(s)
    k = ec > 0
    qq, rr = np.nonzero(k)
    need = int(k.sum())
    assert need > nq
    if rows is not None:
        monkeypatch.setenv("DREPHIP_RECT_BLOCK_ROWS", str(rows))
    dh, dn = _device_sets(H, NH)
    args = (dh.data_ptr(), dn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), NREF, 0, nq)
    lists = []
    with _lib.Context(0, 21, s, 42) as ctx:
        for mode, kern in ((ctx.RECT_BAND_AUTO, AP_BAND), (ctx.RECT_BAND_OFF, AP_MERGE)):
            ctx.set_rect_band(mode)
            assert ctx.dist_rect_sparse_device(*args, None, 0) == (ERR_NOMEM, need)
            assert ctx.last_rect_info() == (kern, 0)
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
            assert ctx.last_rect_info() == (kern, 0)
            assert (buf.cpu().numpy()[need:] == 0x7EADBEEF).all()
            rec = buf.cpu().numpy()[:need].view(np.uint32)
            rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
            assert np.array_equal(rec[:, 0], qq) and np.array_equal(rec[:, 1], rr)
            assert np.array_equal(rec[:, 2], ec[k]) and np.array_equal(rec[:, 3], ed[k])
            lists.append(rec)
    assert np.array_equal(lists[0], lists[1])


@pytest.mark.parametrize("rows", [None, 7])
@pytest.mark.parametrize("top", [1, 3, 64])
def test_band_best_hits(top, rows, monkeypatch):
    s = 4096
    H, NH, nq, (ec, ed) = case(s)
    exp = expected_top(ec, ed, top)
    if rows is not None:
        monkeypatch.setenv("DREPHIP_RECT_TOP_BLOCK_ROWS", str(rows))
    got = []
    with _lib.Context(0, 21, s, 42) as ctx:
        for mode, kern in ((ctx.RECT_BAND_AUTO, AP_BAND), (ctx.RECT_BAND_OFF, AP_MERGE)):
            ctx.set_rect_band(mode)
            got.append(ctx.dist_rect_top(H[:nq], NH[:nq], H, NH, top))
            assert ctx.last_rect_info() == (kern, 0)
            assert all(np.array_equal(g, e) and g.dtype == e.dtype and g.shape == e.shape for g, e in zip(got[-1], exp))
    assert all(np.array_equal(a, b) for a, b in zip(*got))


# ------------------------------------------------------------ 8. selection
def test_band_selection(monkeypatch):
    H, NH, nq, (ec, ed) = case(4096)
    QH, QN = H[:8], NH[:8]
    Hs, NHs, _, (ecs, eds) = case(1000, 97, 41)
    with _lib.Context(0, 21, 4096, 42) as ctx:
        ctx.set_rect_band(ctx.RECT_BAND_OFF)
        c, d = ctx.dist_rect(QH, QN, H, NH)
        assert ctx.last_rect_info() == (AP_MERGE, 0) and np.array_equal(c, ec[:8]) and np.array_equal(d, ed[:8])
        for mode in (ctx.RECT_BAND_AUTO, ctx.RECT_BAND_OFF, ctx.RECT_BAND_FORCE):
            ctx.set_rect_band(mode)
            ctx.set_allpairs_path(ctx.AP_MERGE)
            c, d = ctx.dist_rect(QH, QN, H, NH)
            assert ctx.last_rect_info() == (AP_MERGE, 0) and np.array_equal(c, ec[:8])
            ctx.set_allpairs_path(ctx.AP_AUTO)
            c, d = ctx.dist_rect_merge(QH, QN, H, NH)           # the cross-check stays the merge
            assert ctx.last_rect_info() == (AP_MERGE, 0) and np.array_equal(c, ec[:8]) and np.array_equal(d, ed[:8])
            ctx.set_allpairs_path(ctx.AP_BAND, 64)              # the triangle's selector stays unsupported
            with pytest.raises(_lib.DrepHipError):
                ctx.dist_rect(QH, QN, H, NH)
            ctx.set_allpairs_path(ctx.AP_AUTO)
        for mode, cap in ((3, 64), (-1, 64), (ctx.RECT_BAND_AUTO, 0), (ctx.RECT_BAND_AUTO, 1025)):
            with pytest.raises(_lib.DrepHipError):
                ctx.set_rect_band(mode, cap)
        assert _lib.lib().drephip_set_rect_band(ctx.handle, 3, 64) == -1           # DREPHIP_ERR_ARG
        assert _lib.lib().drephip_set_rect_band(ctx.handle, 0, 0) == -1
        ctx.set_rect_band(ctx.RECT_BAND_AUTO, 1024)             # clamped to 768
        c, d = band_rect(ctx, QH, QN, H, NH)
        assert np.array_equal(c, ec[:8]) and np.array_equal(d, ed[:8])
    with _lib.Context(0, 21, 1000, 42) as ctx:
        c, d = ctx.dist_rect(Hs[:8], NHs[:8], Hs, NHs)
        assert ctx.last_rect_info() == (AP_TABLE, 0) and np.array_equal(c, ecs[:8])
        ctx.set_allpairs_path(ctx.AP_TABLE)
        ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)              # DREPHIP_AP_TABLE keeps its meaning
        ctx.dist_rect(Hs[:8], NHs[:8], Hs, NHs)
        assert ctx.last_rect_info() == (AP_TABLE, 0)
    # the environment sets a new context's mode and cap
    monkeypatch.setenv("DREPHIP_RECT_BAND", "off")
    with _lib.Context(0, 21, 4096, 42) as ctx:
        c, d = ctx.dist_rect(QH, QN, H, NH)
        assert ctx.last_rect_info() == (AP_MERGE, 0) and np.array_equal(c, ec[:8])
    monkeypatch.setenv("DREPHIP_RECT_BAND", "force")
    monkeypatch.setenv("DREPHIP_RECT_BAND_CAP", "64")
    with _lib.Context(0, 21, 1000, 42) as ctx:
        c, d = band_rect(ctx, Hs[:8], NHs[:8], Hs, NHs)
        assert np.array_equal(c, ecs[:8]) and np.array_equal(d, eds[:8])


def test_band_cap_from_environment_is_the_one_run(monkeypatch, capfd):
    H, NH, nq, _ = case(4096)
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    monkeypatch.setenv("DREPHIP_RECT_BAND_CAP", "300")
    with _lib.Context(0, 21, 4096, 42) as ctx:
        capfd.readouterr()
        band_rect(ctx, H[:4], NH[:4], H[:5], NH[:5])
        assert [int(m[0]) for m in _PLAN.findall(capfd.readouterr().err)] == [300]


# ------------------------------------------------------------ 9. end to end
def test_band_end_to_end_on_the_golden_genomes(golden, tmp_path, monkeypatch):
    """The four golden FASTAs sketched on the GPU at MASH_sketch = 4096; each
    genome against the other three: DREPHIP_RECT_BAND=off against unset, row
    for row, float32 bit patterns; the counts against the oracle's merge."""
    S = 4096
    fas = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))
    assert len(fas) == 4
    locs = []
    for f in fas:
        dst = tmp_path / os.path.basename(f)
        shutil.copy(f, dst)
        locs.append(str(dst))
    names = [os.path.basename(f) for f in fas]
    Bdb = pd.DataFrame({"genome": names, "location": locs})
    cache = str(tmp_path / "sk")                        # the queries' sketch cache of every call below
    sk = d_cluster.sketch_genomes(Bdb, cache, MASH_sketch=S)
    assert sk.s == S and (sk.nhash > 2048).all()
    monkeypatch.delenv("DREPHIP_RECT_BAND", raising=False)
    for i in range(4):
        rest = [j for j in range(4) if j != i]
        ref = str(tmp_path / ("ref%d.msh" % i))
        write_msh(ref, [MashReference(locs[j], "", int(sk.length[j]), sk.hashes[j, :sk.nhash[j]]) for j in rest], 21, S, 42)
        Qdb = Bdb.iloc[[i]].reset_index(drop=True)
        res = []
        for env in (None, "off"):
            if env is not None:
                monkeypatch.setenv("DREPHIP_RECT_BAND", env)
            wd = str(tmp_path / ("wd%d%s" % (i, env)))
            rm = d_cluster.query_vs_MASH_rect(Qdb, wd, reference=ref, query_folder=cache)
            Mdb = d_cluster.query_vs_MASH(Qdb, wd, reference=ref, query_folder=cache)
            top = d_cluster.query_best_hits(Qdb, wd, reference=ref, top=5, query_folder=cache)
            res.append((rm, Mdb, top))
            monkeypatch.delenv("DREPHIP_RECT_BAND", raising=False)
        (rm_a, M_a, t_a), (rm_b, M_b, t_b) = res
        ec, ed = oracle_rect(sk.hashes[i:i + 1], sk.nhash[i:i + 1], sk.hashes[rest], sk.nhash[rest], S)
        for rm in (rm_a, rm_b):
            assert np.array_equal(rm.common, ec) and np.array_equal(rm.denom, ed)
        for a, b in ((M_a, M_b), (t_a, t_b)):
            assert list(a.columns) == list(b.columns) and len(a) == len(b)
            for col in a.columns:
                if a[col].dtype == np.float32:
                    assert np.array_equal(a[col].to_numpy().view(np.uint32), b[col].to_numpy().view(np.uint32)), col
                else:
                    assert list(a[col].astype(str)) == list(b[col].astype(str)), col
        assert len(M_a) == 3 and M_a["dist"].dtype == np.float32
        eref, ecom, eden, ecnt = expected_top(ec, ed, 5)
        n = int(ecnt[0])
        assert len(t_a) == n and list(t_a["common"]) == list(ecom[0, :n]) and list(t_a["denom"]) == list(eden[0, :n])
        assert list(t_a["genome1"].astype(str)) == [names[rest[r]] for r in eref[0, :n]]
