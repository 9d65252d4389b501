"""The two-set shared-hash screen of the query-against-reference rectangle
(rect_screen.hip) and the RECT, LIST flavours of k_allpairs_q / k_allpairs_band
it feeds.  Expected values: the C oracle's Mash merge of every (query,
reference) pair, bit for bit on common and denom, every cell.  Every case
asserts from drephip_last_rect_screen_stats that the screen really ran, or
really did not."""
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
from drep_amd.mash_io import read_msh

pytestmark = pytest.mark.gpu
UMAX = np.iinfo(np.uint64).max
U = np.uint64
ERR_NOMEM = -4
AP_TABLE, AP_BAND, AP_MERGE = 1, 2, 3
NQ, NREF = 41, 97
POISON = 0x7EEF
_PLAN = re.compile(r"\[drephip\] rect screen plan: R (\d+) C (\d+) tiles (\d+) marked (\d+) items (\d+) slots (\d+) "
                   r"pieces (\d+)")
_OLD_PLAN = re.compile(r"\[drephip\] rect (?:band )?plan:")


def oracle_rect(Hq, NHq, Hr, NHr, s):
    """(common, denom) [Q, N] of every (query, reference) pair by the oracle's
    merge over the pairs of the stacked matrix (tests/test_rect.py's helper,
    restated)."""
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
    """Case 1's sets at sketch size s with the expected rectangle, computed
    once and shared (read-only): geometry_sketches(97, s) as references and its
    rows 0..40 as queries (every query is a reference: n / n self cells; zero
    hashes; twin rows 7 / 23 / 39; low-word twins split between even and odd
    genomes, so across the two sets; partial rows 5, 12, ..; empty rows 11, 28
    on both sides; rows 0, 4, .. end in 2^64 - 2, the largest hash the
    sketcher admits)."""
    if s not in _CASES:
        H, NH = edge_cases.geometry_sketches(NREF, s, seed=1000 + s)
        exp = oracle_rect(H[:NQ], NH[:NQ], H, NH, s)
        for a in (H, NH) + exp:
            a.setflags(write=False)
        _CASES[s] = (H, NH, NQ, exp)
    return _CASES[s]


def check_case_holds_its_edges(H, NH, nq, ec, ed, s):
    QH, QN = H[:nq], NH[:nq]
    assert (QH[:4, 0] == 0).all() and QN[0] == s                      # a zero hash among valid entries
    assert QH[0, s - 1] == UMAX - 1 and H[44, s - 1] == UMAX - 1      # the largest hash the sketcher admits
    part = np.nonzero((NH > 0) & (NH < s))[0]
    assert len(part) and (H[part, -1] == UMAX).all()                  # partial rows: padded with 2^64 - 1
    empty_q, empty_r = np.nonzero(QN == 0)[0], np.nonzero(NH == 0)[0]
    assert len(empty_q) and len(empty_r) > len(empty_q)
    assert (ec[np.ix_(empty_q, empty_r)] == 0).all() and (ed[np.ix_(empty_q, empty_r)] == 0).all()   # 0 / 0
    lo = U(0xFFFFFFFF)
    qv = np.unique(np.concatenate([QH[g, :QN[g]] for g in range(0, nq, 2)]))          # even queries, odd references
    rv = np.unique(np.concatenate([H[g, :NH[g]] for g in range(1, len(NH), 2)]))
    cand = rv[np.isin(rv & lo, qv & lo)]
    assert any((qv[(qv & lo) == (y & lo)] != y).any() for y in cand)  # low-word twins across the sets
    assert (np.diff((QH[7, :s] & lo)[np.argsort(QH[7, :s] & lo)]) == 0).any()     # twins within a row
    i = np.arange(nq)
    assert np.array_equal(ec[i, i], QN) and np.array_equal(ed[i, i], QN)          # n / n self cells


def ran(ctx, blocks=None):
    st = ctx.last_rect_screen_stats()
    assert st["used"] and st["blocks"] >= 1 and st["dense_blocks"] == 0, st
    if blocks is not None:
        assert st["blocks"] == blocks, st
    return st


def did_not_run(ctx):
    st = ctx.last_rect_screen_stats()
    assert not st["used"] and st["blocks"] == 0 and st["marked"] == 0 and st["query_entries"] == 0, st


def both_routes(ctx, QH, QN, H, NH, ec, ed, kernel, blocks=None):
    """dist_rect under FORCE against the oracle, then under _OFF: equal."""
    ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
    c, d = ctx.dist_rect(QH, QN, H, NH)
    st = ran(ctx, blocks)
    assert ctx.last_rect_info() == (kernel, 0)
    assert np.array_equal(c, ec), np.argwhere(c != ec)[:8]
    assert np.array_equal(d, ed), np.argwhere(d != ed)[:8]
    ctx.set_rect_screen(ctx.RECT_SCREEN_OFF)
    c0, d0 = ctx.dist_rect(QH, QN, H, NH)
    did_not_run(ctx)
    assert ctx.last_rect_info() == (kernel, 0)
    assert np.array_equal(c, c0) and np.array_equal(d, d0)
    ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
    return st


def no_denom(ctx, QH, QN, H, NH, ec):
    """The device form with a null denom pointer into a poisoned buffer."""
    import torch
    nq, n = len(QN), len(NH)
    dqh = torch.from_numpy(QH.copy().view(np.int64)).cuda()
    dqn = torch.from_numpy(QN.copy().view(np.int32)).cuda()
    dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    out = torch.full((nq * n,), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.dist_rect_device(dqh.data_ptr(), dqn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), n, 0, nq, out.data_ptr(), None)
    assert np.array_equal(out.cpu().numpy().view(np.uint16).reshape(nq, n), ec)


# ------------------------------------------------------------ 1. FORCE on the variant matrix
@pytest.mark.parametrize("s", [64, 100, 600, 1000, 1025, 2048])
def test_forced_screen_table_kernel_vs_oracle(s):
    """The five LIST geometries of the table kernel: (R, chunks, workgroups per
    CU) = (8, 8, 2) at s = 64 and 100, (8, 16, 1) at 600, (4, 16, 2) at 1000,
    (4, 32, 1) at 1025, (2, 32, 2) at 2048."""
    H, NH, nq, (ec, ed) = case(s)
    check_case_holds_its_edges(H, NH, nq, ec, ed, s)
    with _lib.Context(0, 21, s, 42) as ctx:
        st = both_routes(ctx, H[:nq], NH[:nq], H, NH, ec, ed, AP_TABLE, blocks=1)
        assert st["query_entries"] == int(NH[:nq].sum()) and 0 < st["distinct"] <= st["query_entries"]
        assert st["checks"] == 0                                       # FORCE skips the count pass
        R = {64: 8, 100: 8, 600: 8, 1000: 4, 1025: 4, 2048: 2}[s]
        tiles = -(-nq // R)
        # a tile's marked columns: at least the references sharing a hash with one of its rows
        assert (ec > 0).reshape(-1).sum() / R <= st["marked"] <= tiles * NREF
        no_denom(ctx, H[:nq], NH[:nq], H, NH, ec)
        ran(ctx, 1)


@pytest.mark.parametrize("s,band", [(64, False), (1000, False), (64, True), (4096, True)])
def test_largest_value_among_valid_entries(s, band):
    """2^64 - 1 as a valid entry -- the last hash of the full rows 2 (a query
    and a reference) and 50 (a reference) of case 1's sets -- which is also the
    padding of every partial and empty row: the screen must ignore entries at
    k >= nhash, and every cell equals the oracle's, screened and unscreened.

    No sketcher admits that value (it is the padding), and the table and band
    kernels read whole rows: a query row that ends in it is merged literally
    inside the table kernel (k_build_q32 marks it as it marks a failed row),
    and sends a band call's rows to k_rect_merge (fallback = 1).  It is kept
    out of case() so that the band cases there do run the band kernel."""
    H, NH, nq, _ = case(s)
    H = H.copy()
    for g in (2, 50):
        assert NH[g] == s and H[g, s - 2] < UMAX - 1
        H[g, s - 1] = UMAX
    ec, ed = oracle_rect(H[:nq], NH[:nq], H, NH, s)
    part = np.nonzero((NH > 0) & (NH < s))[0]
    assert (H[part, -1] == UMAX).all() and ec[2, 50] >= 1 and len(part) > 3
    kernel = (AP_BAND, 1) if band else (AP_TABLE, 0)
    with _lib.Context(0, 21, s, 42) as ctx:
        if band and s <= 2048:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
        st = ran(ctx, 1)
        assert ctx.last_rect_info() == kernel
        assert st["query_entries"] == int(NH[:nq].sum())             # padding is no entry
        assert np.array_equal(c, ec), np.argwhere(c != ec)[:8]
        assert np.array_equal(d, ed), np.argwhere(d != ed)[:8]
        q, r, cc, dd = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH)
        ran(ctx, 1)
        k = ec > 0
        assert np.array_equal(q, np.nonzero(k)[0]) and np.array_equal(r, np.nonzero(k)[1])
        assert np.array_equal(cc, ec[k]) and np.array_equal(dd, ed[k])
        ctx.set_rect_screen(ctx.RECT_SCREEN_OFF)
        c0, d0 = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
        did_not_run(ctx)
        assert ctx.last_rect_info() == kernel
        assert np.array_equal(c0, ec) and np.array_equal(d0, ed)
        # the rows that do not hold it still run the band kernel
        c1, d1 = ctx.dist_rect(H[:nq], NH[:nq], H, NH, 4, 40)
        assert ctx.last_rect_info() == ((AP_BAND, 0) if band else (AP_TABLE, 0))
        assert np.array_equal(c1, ec[4:40]) and np.array_equal(d1, ed[4:40])


@pytest.mark.parametrize("s,cap", [(4096, 768), (100, 64), (100, 300)])
def test_forced_screen_band_kernel_vs_oracle(s, cap):
    H, NH, nq, (ec, ed) = case(s)
    check_case_holds_its_edges(H, NH, nq, ec, ed, s)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_band(ctx.RECT_BAND_AUTO if s > 2048 else ctx.RECT_BAND_FORCE, cap)
        st = both_routes(ctx, H[:nq], NH[:nq], H, NH, ec, ed, AP_BAND, blocks=1)
        assert st["marked"] <= -(-nq // 4) * NREF
        no_denom(ctx, H[:nq], NH[:nq], H, NH, ec)
        ran(ctx, 1)


# ------------------------------------------------------------ 2. nothing shared
def disjoint_sets(s, seed=5):
    """12 queries from the low half of the value range, 40 references from the
    high half, partial sketches of several lengths on both sides."""
    rng = np.random.default_rng(seed)
    half = 1 << 62
    lo = np.unique(rng.integers(1, half, size=14 * s, dtype=np.uint64))[:12 * s]
    hi = np.unique(rng.integers(2 * half, 3 * half, size=44 * s, dtype=np.uint64))[:40 * s]
    rng.shuffle(lo)
    rng.shuffle(hi)
    QH, RH = np.sort(lo.reshape(12, s), axis=1), np.sort(hi.reshape(40, s), axis=1)
    QN, RN = np.full(12, s, np.uint32), np.full(40, s, np.uint32)
    for g, n in ((1, s // 4), (6, 3), (9, 0)):
        QN[g] = n
        QH[g, n:] = UMAX
    for g, n in ((0, s // 8), (17, s // 2), (33, 1), (39, 0)):
        RN[g] = n
        RH[g, n:] = UMAX
    return QH, QN, RH, RN


@pytest.mark.parametrize("s,band", [(64, False), (64, True), (4096, True)])
def test_nothing_shared_launches_no_kernel(s, band, monkeypatch, capfd):
    QH, QN, RH, RN = disjoint_sets(s)
    ec, ed = oracle_rect(QH, QN, RH, RN, s)
    want = np.minimum(s, QN[:, None].astype(np.int64) + RN[None, :].astype(np.int64)).astype(np.uint16)
    assert (ec == 0).all() and np.array_equal(ed, want) and len(np.unique(ed)) >= 6
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_timing(True)
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        if band and s <= 2048:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        capfd.readouterr()
        c, d = ctx.dist_rect(QH, QN, RH, RN)
        err = capfd.readouterr().err
        st = ran(ctx, 1)
        assert st["marked"] == 0 and st["query_entries"] == int(QN.sum())
        (R, C, tiles, marked, items, slots, pieces), = [tuple(map(int, m)) for m in _PLAN.findall(err)]
        assert (marked, items, slots, pieces) == (0, 0, 0, 0) and C == (128 if band else 512) and tiles == -(-12 // R)
        assert not _OLD_PLAN.search(err)
        assert ctx.kernel_ms(2)[1] == 0 and ctx.kernel_ms(3)[1] == 0       # neither the kernel nor a table build
        assert np.array_equal(c, ec) and np.array_equal(d, ed)
        q, r, cc, dd = ctx.dist_rect_sparse(QH, QN, RH, RN)
        assert len(q) == 0 and ran(ctx)["marked"] == 0
        ref, _, _, cnt = ctx.dist_rect_top(QH, QN, RH, RN, 3)
        assert (cnt == 0).all() and (ref == -1).all() and ran(ctx)["marked"] == 0


@pytest.mark.parametrize("s,band", [(64, False), (64, True), (4096, True)])
def test_one_planted_shared_hash(s, band):
    """The disjoint sets with exactly one shared hash per planted pair, at ranks
    i + j on both sides of s: it counts when the union rank i + j is below s."""
    QH, QN, RH, RN = disjoint_sets(s)
    QH, RH = QH.copy(), RH.copy()
    mid = U(1) << U(63)                                 # between the two ranges ...
    top = U(0xF) << U(60)                               # ... and above both
    # query 2 gets `mid` as its last element: rank s - 1 in the query, 0 in reference 5 -> i + j = s - 1 < s
    QH[2, s - 1] = mid
    RH[5] = np.sort(np.concatenate([[mid], RH[5, 1:]]))
    assert RH[5, 0] == mid
    # query 4 gets `top` as its last element, reference 8 too: i + j = 2 s - 2 >= s
    QH[4, s - 1] = top
    RH[8, s - 1] = top
    ec, ed = oracle_rect(QH, QN, RH, RN, s)
    assert ec[2, 5] == 1 and ec[4, 8] == 0 and ec.sum() == 1
    with _lib.Context(0, 21, s, 42) as ctx:
        if band and s <= 2048:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        st = both_routes(ctx, QH, QN, RH, RN, ec, ed, AP_BAND if band else AP_TABLE, blocks=1)
        assert st["marked"] == 2                       # cells (tile of query 2, ref 5) and (tile of query 4, ref 8)
        q, r, cc, dd = ctx.dist_rect_sparse(QH, QN, RH, RN)
        assert (list(q), list(r), list(cc), list(dd)) == ([2], [5], [1], [int(ed[2, 5])])


# ------------------------------------------------------------ 3. bitmap edges
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_bitmap_word_edges(n):
    s = 100
    H, NH, nq, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        for lo in (0, 97 - n):                                      # the first n references, and the last n
            c, d = ctx.dist_rect(H[:nq], NH[:nq], H[lo:lo + n], NH[lo:lo + n])
            ran(ctx, 1)
            assert np.array_equal(c, ec[:, lo:lo + n]) and np.array_equal(d, ed[:, lo:lo + n])
        for q in (0, 5, 11):                                        # Q = 1: zero key, partial, empty
            c, d = ctx.dist_rect(H[q:q + 1], NH[q:q + 1], H[:n], NH[:n])
            ran(ctx, 1)
            assert np.array_equal(c, ec[q:q + 1, :n]) and np.array_equal(d, ed[q:q + 1, :n])


@pytest.mark.parametrize("band", [False, True])
@pytest.mark.parametrize("q0,q1", [(3, 38), (0, 1), (40, 41)])
def test_row_ranges_write_only_their_cells(q0, q1, band):
    import torch
    s = 100
    H, NH, nq, (ec, ed) = case(s)
    dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    rows = q1 - q0
    bc = torch.full((rows + 2, NREF), POISON, dtype=torch.int16, device="cuda")     # a guard row before and after
    bd = torch.full((rows + 2, NREF), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        if band:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        ctx.dist_rect_device(dh.data_ptr(), dn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), NREF, q0, q1,
                             bc[1].data_ptr(), bd[1].data_ptr())
        ran(ctx, 1)
        assert ctx.last_rect_info() == (AP_BAND if band else AP_TABLE, 0)
    gc, gd = bc.cpu().numpy().view(np.uint16), bd.cpu().numpy().view(np.uint16)
    for g in (gc, gd):
        assert (g[0] == POISON).all() and (g[-1] == POISON).all()
    assert np.array_equal(gc[1:-1], ec[q0:q1]) and np.array_equal(gd[1:-1], ed[q0:q1])


def test_clamped_and_empty_calls():
    """q1 clamped to Q; Q == 0, N == 0 and q0 >= q1 return OK, write nothing and
    leave the screen's figures at zero (tests/test_rect.py's empty calls)."""
    import torch
    s = 100
    H, NH, nq, (ec, ed) = case(s)
    dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    out = torch.full((nq * NREF,), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH, 30, 1000)
        ran(ctx, 1)
        assert np.array_equal(c, ec[30:]) and np.array_equal(d, ed[30:])
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        for Q, N, q0, q1 in ((0, NREF, 0, 5), (nq, 0, 0, nq), (nq, NREF, 7, 7), (nq, NREF, 9, 3), (nq, NREF, nq, nq + 4)):
            ctx.dist_rect_device(dh.data_ptr(), dn.data_ptr(), Q, dh.data_ptr(), dn.data_ptr(), N, q0, q1,
                                 out.data_ptr(), out.data_ptr())
            did_not_run(ctx)
        rc, n = ctx.dist_rect_sparse_device(dh.data_ptr(), dn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), 0, 0, nq,
                                            None, 0)
        assert (rc, n) == (0, 0)
    assert (out.cpu().numpy() == POISON).all()


# ------------------------------------------------------------ 4. long runs
def hub_sets(s, nq=200, nref=300, hubq=150, seed=11):
    """Disjoint random sets, then: one hash held by the first `hubq` queries and
    every reference (more than a wave on each side), and a second hash held by
    queries hubq + 11 and hubq + 12 (one tile at R = 4 and 8) and references 3, 77."""
    rng = np.random.default_rng(seed)
    v = np.unique(rng.integers(1 << 20, 1 << 62, size=(nq + nref + 8) * s, dtype=np.uint64))[:(nq + nref) * s]
    rng.shuffle(v)
    M = np.sort(v.reshape(nq + nref, s), axis=1)
    QH, RH = M[:nq].copy(), M[nq:].copy()
    hub, second = U(77), U(99)                          # below every random value: ranks 0 and 1
    QH[:hubq, 0] = hub
    RH[:, 0] = hub
    for g in (hubq + 11, hubq + 12):
        QH[g, 0] = second
    for g in (3, 77):
        RH[g, 1] = second
    assert (np.diff(QH.astype(object), axis=1) > 0).all() and (np.diff(RH.astype(object), axis=1) > 0).all()
    return QH, np.full(nq, s, np.uint32), RH, np.full(nref, s, np.uint32)


@pytest.mark.parametrize("band", [False, True])
def test_long_runs_hub_and_one_tile_pair(band):
    s, hubq = 64, 150
    QH, QN, RH, RN = hub_sets(s, hubq=hubq)
    ec, ed = oracle_rect(QH, QN, RH, RN, s)
    R = 4 if band else 8
    tiles = ec.shape[0] // R
    per_tile = (ec.reshape(tiles, R, -1) > 0).any(axis=1).sum(axis=1)        # columns a tile must hold
    assert (per_tile == 0).any() and (per_tile == 300).any() and (per_tile == 2).sum() == 1
    assert (ec[:hubq] == 1).all() and ec[hubq:].sum() == 4
    with _lib.Context(0, 21, s, 42) as ctx:
        if band:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        st = both_routes(ctx, QH, QN, RH, RN, ec, ed, AP_BAND if band else AP_TABLE, blocks=1)
        assert st["marked"] == int(per_tile.sum())                   # nothing else is shared: the marks are exact


# ------------------------------------------------------------ 5. item splitting
@pytest.mark.parametrize("band", [False, True])
def test_item_splitting_and_split_launches(band, monkeypatch, capfd):
    """One row tile with more marked columns than an item holds (512 for the
    table kernel, 128 for the band kernel), then the launch cut into pieces."""
    s, nref = (100, 300) if band else (64, 1100)
    QH, QN, RH, RN = hub_sets(s, nq=20, nref=nref, hubq=1, seed=13)
    ec, ed = oracle_rect(QH, QN, RH, RN, s)
    assert (ec[0] == 1).all() and ec[1:].sum() == 4
    C, R, lanes = (128, 4, 1024) if band else (512, 8, 1024)
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        if band:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        capfd.readouterr()
        c, d = ctx.dist_rect(QH, QN, RH, RN)
        (r_, c_, tiles, marked, items, slots, pieces), = [tuple(map(int, m)) for m in _PLAN.findall(capfd.readouterr().err)]
        assert (r_, c_, tiles, marked) == (R, C, -(-20 // R), nref + 2)
        assert items == -(-nref // C) + 1 == 4 and slots >= items and slots % 8 == 0 and pieces == 1
        assert np.array_equal(c, ec) and np.array_equal(d, ed)
        monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", str(8 * lanes))         # eight items per dispatch, the least
        c, d = ctx.dist_rect(QH, QN, RH, RN)
        (_, _, _, _, items2, slots2, pieces), = [tuple(map(int, m)) for m in _PLAN.findall(capfd.readouterr().err)]
        assert (items2, slots2) == (items, slots) and pieces == -(-slots // 8) and pieces > 1
        assert np.array_equal(c, ec) and np.array_equal(d, ed)
        ran(ctx, 1)
        q, r, cc, dd = ctx.dist_rect_sparse(QH, QN, RH, RN)
        k = ec > 0
        assert np.array_equal(q, np.nonzero(k)[0]) and np.array_equal(r, np.nonzero(k)[1]) and np.array_equal(cc, ec[k])


# ------------------------------------------------------------ 6. several blocks
@pytest.mark.parametrize("s,band", [(64, False), (1000, False), (100, True)])
def test_several_blocks_equal_one_block(s, band, monkeypatch):
    H, NH, nq, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        if band:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        c1, d1 = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
        one = ran(ctx, 1)
        monkeypatch.setenv("DREPHIP_RECT_SCREEN_BLOCK_ROWS", "7")
        c7, d7 = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
        st = ran(ctx, 6)
        assert st["query_entries"] == one["query_entries"]
        assert np.array_equal(c1, ec) and np.array_equal(d1, ed)
        assert np.array_equal(c7, c1) and np.array_equal(d7, d1)
        c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH, 3, 38)        # 35 rows: five blocks of 7
        ran(ctx, 5)
        assert np.array_equal(c, ec[3:38]) and np.array_equal(d, ed[3:38])


# ------------------------------------------------------------ 7. records and best hits
def expected_top(ec, ed, top):
    """(ref [Q, top] with -1 past count, common, denom, count) from a rectangle
    in the contract's order (tests/test_rect_top.py's)."""
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
@pytest.mark.parametrize("s", [64, 4096])
def test_records_and_best_hits(s, rows, monkeypatch):
    import torch
    H, NH, nq, (ec, ed) = case(s)
    QH, QN = H[:nq], NH[:nq]
    k = ec > 0
    qq, rr = np.nonzero(k)
    need = int(k.sum())
    if rows:
        monkeypatch.setenv("DREPHIP_RECT_SCREEN_BLOCK_ROWS", str(rows))
    nblocks = -(-nq // rows) if rows else 1
    dqh = torch.from_numpy(QH.copy().view(np.int64)).cuda()
    dqn = torch.from_numpy(QN.copy().view(np.int32)).cuda()
    drh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    drn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    args = (dqh.data_ptr(), dqn.data_ptr(), nq, drh.data_ptr(), drn.data_ptr(), NREF, 0, nq)
    with _lib.Context(0, 21, s, 42) as ctx:
        got = {}
        for mode in (ctx.RECT_SCREEN_FORCE, ctx.RECT_SCREEN_OFF):
            ctx.set_rect_screen(mode)
            check = (lambda: ran(ctx, nblocks)) if mode == ctx.RECT_SCREEN_FORCE else (lambda: did_not_run(ctx))
            q, r, c, d = ctx.dist_rect_sparse(QH, QN, H, NH, cap=need)
            check()
            assert ctx.last_rect_info() == (AP_TABLE if s <= 2048 else AP_BAND, 0)
            assert np.array_equal(q, qq) and np.array_equal(r, rr) and np.array_equal(c, ec[k]) and np.array_equal(d, ed[k])
            torch.cuda.synchronize()
            assert ctx.dist_rect_sparse_device(*args, None, 0) == (ERR_NOMEM, need)
            check()
            buf = torch.full((need + 8, 4), 0x7EADBEEF, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert ctx.dist_rect_sparse_device(*args, buf.data_ptr(), need - 1) == (ERR_NOMEM, need)
            check()
            rec = buf.cpu().numpy()
            assert (rec[need - 1:] == 0x7EADBEEF).all()
            rec = rec[:need - 1].view(np.uint32)
            assert len(set(map(tuple, rec[:, :2]))) == need - 1
            assert all(ec[a, b] == cc and ed[a, b] == dd and cc > 0 for a, b, cc, dd in rec)
            tops = []
            for top in (1, 3, 64):
                t = ctx.dist_rect_top(QH, QN, H, NH, top)
                check()
                for a, b in zip(t, expected_top(ec, ed, top)):
                    assert np.array_equal(a, b)
                tops.append(t)
            got[mode] = tops
        for a, b in zip(got[ctx.RECT_SCREEN_FORCE], got[ctx.RECT_SCREEN_OFF]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------ 8. verdict and gates
def family_sets(nq, nref, s, fam, seed, keep=0.9):
    """Families of `fam` genomes: each keeps `keep` of its family's pool of
    hashes; queries and references are drawn from the same families."""
    rng = np.random.default_rng(seed)
    nfam = -(-max(nq, nref) // fam)
    pool = np.unique(rng.integers(1, UMAX - 1, size=nfam * 2 * s + 64, dtype=np.uint64))[:nfam * 2 * s]
    rng.shuffle(pool)
    pool = pool.reshape(nfam, 2 * s)

    def draw(n):
        M = np.empty((n, s), np.uint64)
        for g in range(n):
            p = pool[g // fam]
            fixed = p[:int(keep * s)]
            M[g] = np.sort(np.concatenate([fixed, rng.choice(p[int(keep * s):], s - len(fixed), replace=False)]))
        return M, np.full(n, s, np.uint32)
    return draw(nq) + draw(nref)


def test_dense_set_is_declined_by_the_verdict(monkeypatch):
    """One family: every query shares most hashes with every reference."""
    s = 64
    QH, QN, RH, RN = family_sets(24, 130, s, fam=1000, seed=3)
    ec, ed = oracle_rect(QH, QN, RH, RN, s)
    assert (ec > s // 2).all()
    monkeypatch.setenv("DREPHIP_RECT_SCREEN_MIN_N", "100")
    monkeypatch.setenv("DREPHIP_RECT_SCREEN_MIN_Q", "8")
    with _lib.Context(0, 21, s, 42) as ctx:
        c, d = ctx.dist_rect(QH, QN, RH, RN)                            # AUTO, floors lowered
        st = ctx.last_rect_screen_stats()
        assert not st["used"] and st["blocks"] == 1 and st["dense_blocks"] == 1 and st["marked"] == 0, st
        # the marking's bit tests: every (query entry, reference entry) match
        assert st["checks"] == sum(len(np.intersect1d(a, b)) for a in QH for b in RH)
        assert st["checks"] * 16 > 24 * 130 * s
        assert np.array_equal(c, ec) and np.array_equal(d, ed)
        both_routes(ctx, QH, QN, RH, RN, ec, ed, AP_TABLE, blocks=1)    # FORCE: screened, exact
    # below either floor AUTO does not look at all
    monkeypatch.setenv("DREPHIP_RECT_SCREEN_MIN_Q", "25")
    with _lib.Context(0, 21, s, 42) as ctx:
        c, d = ctx.dist_rect(QH, QN, RH, RN)
        did_not_run(ctx)
        assert np.array_equal(c, ec)


def test_auto_floors(monkeypatch):
    """AUTO with the shipped floors (4096 references, 2048 query rows: the row
    floor was raised from 256 by the measurement in profiles/rect_screen.json):
    not at 24 x 6149, not at 255 or 256 x 4096, not at 2047 x 4096; at
    2048 x 4096 on a family-structured set it runs (and the merge routes never)."""
    for v in ("DREPHIP_RECT_SCREEN_MIN_N", "DREPHIP_RECT_SCREEN_MIN_Q", "DREPHIP_RECT_SCREEN"):
        monkeypatch.delenv(v, raising=False)
    s = 64
    QH, QN, RH, RN = family_sets(2048, 6149, s, fam=16, seed=9)
    ec, ed = oracle_rect(QH, QN, RH[:4096], RN[:4096], s)
    tile_any = (ec.reshape(256, 8, -1) > 0).any(axis=1)
    assert 0 < tile_any.sum() < tile_any.size // 50                     # sparse: the screen is worth it
    with _lib.Context(0, 21, s, 42) as ctx:
        assert ctx.last_rect_screen_stats()["blocks"] == 0
        c, d = ctx.dist_rect(QH[:24], QN[:24], RH, RN)
        did_not_run(ctx)
        for rows in (255, 256, 2047):
            c, d = ctx.dist_rect(QH[:rows], QN[:rows], RH[:4096], RN[:4096])
            did_not_run(ctx)
            assert np.array_equal(c, ec[:rows]) and np.array_equal(d, ed[:rows])
        c, d = ctx.dist_rect(QH, QN, RH[:4095], RN[:4095])
        did_not_run(ctx)
        c, d = ctx.dist_rect(QH, QN, RH[:4096], RN[:4096])
        st = ran(ctx, 1)
        assert st["checks"] > 0 and st["checks"] * 16 <= 2048 * 4096 * s
        assert st["marked"] == int(tile_any.sum())                      # families only: the marks are exact
        assert ctx.last_rect_info() == (AP_TABLE, 0)
        assert np.array_equal(c, ec) and np.array_equal(d, ed)
        q, r, cc, dd = ctx.dist_rect_sparse(QH, QN, RH[:4096], RN[:4096])
        ran(ctx, 1)
        k = ec > 0
        assert np.array_equal(q, np.nonzero(k)[0]) and np.array_equal(r, np.nonzero(k)[1]) and np.array_equal(cc, ec[k])
        ref, tc, td, cnt = ctx.dist_rect_top(QH, QN, RH[:4096], RN[:4096], 1)
        ran(ctx, 1)
        assert np.array_equal(cnt, k.any(axis=1).astype(np.uint32))
        # never screened: the merge entry point, DREPHIP_AP_MERGE
        c, d = ctx.dist_rect_merge(QH, QN, RH[:4096], RN[:4096])
        did_not_run(ctx)
        assert ctx.last_rect_info() == (AP_MERGE, 0) and np.array_equal(c, ec) and np.array_equal(d, ed)
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        ctx.set_allpairs_path(ctx.AP_MERGE)
        c, d = ctx.dist_rect(QH[:40], QN[:40], RH[:4096], RN[:4096])
        did_not_run(ctx)
        assert ctx.last_rect_info() == (AP_MERGE, 0) and np.array_equal(c, ec[:40])


def test_band_off_above_the_tables_is_never_screened():
    s = 4096
    H, NH, nq, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        ctx.set_rect_band(ctx.RECT_BAND_OFF)
        c, d = ctx.dist_rect(H[:9], NH[:9], H, NH)
        did_not_run(ctx)
        assert ctx.last_rect_info() == (AP_MERGE, 0)
        assert np.array_equal(c, ec[:9]) and np.array_equal(d, ed[:9])


def test_mode_argument_and_environment(monkeypatch):
    s = 64
    H, NH, nq, (ec, ed) = case(s)
    with _lib.Context(0, 21, s, 42) as ctx:
        for mode in (3, -1):
            with pytest.raises(_lib.DrepHipError):
                ctx.set_rect_screen(mode)
        assert _lib.lib().drephip_set_rect_screen(ctx.handle, 3) == -1
    for word, runs in (("force", True), ("off", False), ("auto", False)):
        monkeypatch.setenv("DREPHIP_RECT_SCREEN", word)
        with _lib.Context(0, 21, s, 42) as ctx:                       # read at creation
            monkeypatch.delenv("DREPHIP_RECT_SCREEN")
            c, d = ctx.dist_rect(H[:nq], NH[:nq], H, NH)
            ran(ctx, 1) if runs else did_not_run(ctx)
            assert np.array_equal(c, ec) and np.array_equal(d, ed)


# ------------------------------------------------------------ 9. failed tables
def unbuildable_rows(S=1000):
    """Rows 0 and 7 hold three hashes with one low word (no cuckoo table can
    hold them), the three smallest of the row; rows 1 and 8 share two of them
    (tests/test_rect_band.py's construction, restated)."""
    rng = np.random.default_rng(3)
    N = 24
    base = np.sort(rng.choice(2 ** 62, size=(N, 2000), replace=False).astype(np.uint64), axis=1)
    h = np.full((N, S), UMAX, dtype=np.uint64)
    for i in range(N):
        pool = base[i // 6]
        keep = np.sort(rng.choice(len(pool), S, replace=False))
        h[i] = pool[keep]
    lo = U(0x12345678)
    bad = np.array([(U(k) << U(40)) | lo for k in (1, 2, 3)], dtype=np.uint64)
    for i in (0, 7):
        row = np.unique(np.concatenate([h[i][:S - 3], bad]))
        h[i] = row[:S]
        h[i + 1] = np.unique(np.concatenate([h[i + 1][:S - 2], bad[:2]]))[:S]
    return h, np.full(N, S, np.uint32)


@pytest.mark.parametrize("band", [False, True])
@pytest.mark.parametrize("partial", [False, True])
def test_failed_tables_under_the_screen(partial, band):
    S = 1000
    h, nh = unbuildable_rows(S)
    rh, rnh = h.copy(), nh.copy()
    if partial:
        for i in (1, 7, 12):
            rnh[i] = 300 + i
            rh[i, rnh[i]:] = UMAX
    qh, qnh = rh[:10], rnh[:10]
    ec, ed = oracle_rect(qh, qnh, rh, rnh, S)
    assert ec[0, 0] == S and ec[0, 1] >= 2 and (not partial or (ed < S).any())
    assert (ec[:, 12:] == 0).all() and (ec[:6, :6] > 0).all()          # marked and unmarked columns
    with _lib.Context(0, 21, S, 42) as ctx:
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        if band:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 256)
        for _ in range(2):
            c, d = ctx.dist_rect(qh, qnh, rh, rnh)
            ran(ctx, 1)
            assert ctx.last_rect_info() == ((AP_BAND, 1) if band else (AP_TABLE, 0))   # band: rows rerun by the merge
            assert np.array_equal(c, ec) and np.array_equal(d, ed)
            q, r, rc_, rd_ = ctx.dist_rect_sparse(qh, qnh, rh, rnh)
            ran(ctx, 1)
            k = ec > 0
            assert np.array_equal(q, np.nonzero(k)[0]) and np.array_equal(r, np.nonzero(k)[1])
            assert np.array_equal(rc_, ec[k]) and np.array_equal(rd_, ed[k])
            # a clean call on the same context (rows 2..5: their tables build)
            c2, d2 = ctx.dist_rect(qh[2:6], qnh[2:6], rh, rnh)
            ran(ctx, 1)
            assert ctx.last_rect_info() == (AP_BAND if band else AP_TABLE, 0)
            assert np.array_equal(c2, ec[2:6]) and np.array_equal(d2, ed[2:6])


# ------------------------------------------------------------ 10. end to end
def _golden_names(golden):
    return [os.path.basename(r.name) for r in read_msh(os.path.join(golden, "MASH_files", "ALL.msh")).references]


def _query_cache(golden, folder, names):
    chunk = os.path.join(folder, "MASH_files", "sketches", "chunk_0")
    os.makedirs(chunk)
    for n in names:
        shutil.copy(os.path.join(golden, "MASH_files", "sketches", n + ".msh"), os.path.join(chunk, n + ".msh"))


def test_golden_table_through_the_forced_screen(golden, tmp_path, monkeypatch):
    names = _golden_names(golden)
    ref = os.path.join(golden, "MASH_files", "ALL.msh")
    table = os.path.join(golden, "MASH_files", "MASH_table.tsv")
    qfolder = str(tmp_path / "queries")
    _query_cache(golden, qfolder, names)
    Qdb = pd.DataFrame({"genome": names, "location": ["/nowhere/" + n for n in names]})
    monkeypatch.delenv("DREPHIP_RECT_SCREEN", raising=False)
    plain = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd0"), reference=ref, query_folder=qfolder, top=5)
    monkeypatch.setenv("DREPHIP_RECT_SCREEN", "force")
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    Mdb = d_cluster.query_vs_MASH(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder)
    exp = d_cluster._parse_mash_table(table, Qdb)
    assert len(Mdb) == len(exp) == 25
    for col in ("genome1", "genome2"):
        assert list(Mdb[col].astype(str)) == list(exp[col].astype(str))
    for col in ("dist", "similarity"):
        assert Mdb[col].dtype == np.float32
        assert np.array_equal(Mdb[col].to_numpy().view(np.uint32), exp[col].to_numpy().view(np.uint32))
    rm = d_cluster.query_vs_MASH_rect(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder)
    kmers = [ln.split("\t")[4] for ln in open(table).read().splitlines()]
    assert ["%d/%d" % (rm.common[q, r], rm.denom[q, r]) for q in range(5) for r in range(5)] == kmers
    forced = d_cluster.query_best_hits(Qdb, str(tmp_path / "wd1"), reference=ref, query_folder=qfolder, top=5)
    assert len(forced) == len(plain) > 5 and list(forced.columns) == list(plain.columns)
    for col in forced.columns:
        a, b = forced[col].to_numpy(), plain[col].to_numpy()
        if a.dtype.kind == "f":
            assert np.array_equal(a.view("u%d" % a.itemsize), b.view("u%d" % b.itemsize)), col
        else:
            assert list(map(str, a)) == list(map(str, b)), col


def test_forced_screen_ran_end_to_end(golden, tmp_path, monkeypatch, capfd):
    """The environment reaches the contexts d_cluster creates: the screened
    plan line is printed, the unscreened one is not."""
    names = _golden_names(golden)
    ref = os.path.join(golden, "MASH_files", "ALL.msh")
    qfolder = str(tmp_path / "queries")
    _query_cache(golden, qfolder, names)
    Qdb = pd.DataFrame({"genome": names, "location": ["/nowhere/" + n for n in names]})
    monkeypatch.setenv("DREPHIP_RECT_SCREEN", "force")
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    capfd.readouterr()
    d_cluster.query_vs_MASH_rect(Qdb, str(tmp_path / "wd"), reference=ref, query_folder=qfolder)
    err = capfd.readouterr().err
    assert _PLAN.search(err) and not _OLD_PLAN.search(err)
