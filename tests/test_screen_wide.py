"""The shared-hash screen (screen.hip) past one marking window and on long and
colliding runs of equal sort keys: sketch sets of tests/edge_cases.py
(wide_screen_sets; their marks are counted on the CPU by
tests/test_edge_helpers.py) with more genomes than the LDS window of
k_screen_mark has row tiles and columns, so that cells are marked through the
window, directly, and both ways by different chunks; with hubs longer than a
wave, twins of a hash that agree with it in the low word and in the entry
fingerprint (runs marked as one hash, which k_screen_light and the LIST
kernels must resolve) or differ in a fingerprint bit (the pairwise path), and
genomes that hold both; and a set with N s > 2^28, where the entry values hold
no usable fingerprint and the marking reads every hash.  Every result is
compared bit for bit, common and denom, with the C oracle's Mash merge
(reference: `mash dist`, drep/d_cluster.py:569-573): the condensed triangle,
row segments, the sparse list on both plans, the sharded screen."""
import numpy as np
import pytest

import oracle
import edge_cases as ec
from drep_amd import _lib
from test_screen import run, sharded_screen

pytestmark = pytest.mark.gpu
S = 16
NAMES = ("A0", "A1", "A31", "B", "C")
_SETS = {}


def wide(name):
    """(H, NH, info, oracle common, oracle denom) of a wide set, made once and shared (read-only)."""
    if not _SETS:
        with _lib.Context(0, 21, S, 42) as ctx:
            R = ctx.screen_geometry()
        for n, (H, NH, info) in ec.wide_screen_sets(R, seed=7).items():
            oc, od = oracle.allpairs(H, NH, S, threads=8)
            for a in (H, NH, oc, od):
                a.setflags(write=False)
            _SETS[n] = (H, NH, info, oc, od)
    return _SETS[name]


def start(i, N):
    return i * N - i * (i + 1) // 2


def assert_pairs(got, exp, what):
    """A sparse list (sorted by (i, j)) against the expected one: no record with i >= j, no pair twice, equal as sets."""
    assert (got[0] < got[1]).all(), ("a record with i >= j", what)
    key = got[0].astype(np.uint64) << np.uint64(32) | got[1].astype(np.uint64)
    assert len(np.unique(key)) == len(key), ("a pair is listed twice", what)
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    for n, g, e in zip(("i", "j", "common", "denom"), got, exp):
        assert np.array_equal(g, e), (what, n)


@pytest.mark.parametrize("name", NAMES)
def test_wide_screen_on_off_and_light(name, monkeypatch):
    """Screen on (with and without the light cells) and off against the
    oracle; the light path writes pairs itself and leaves fewer cells."""
    H, NH, _, oc, od = wide(name)
    with _lib.Context(0, 21, S, 42) as ctx:
        c, d, st = run(ctx, H, NH, ctx.SCREEN_ON)
        assert st["used"] and st["marked"] > 0 and st["entries"] == int(NH.sum())
        assert np.array_equal(c, oc) and np.array_equal(d, od)
        c, d, st = run(ctx, H, NH, ctx.SCREEN_OFF)
        assert not st["used"]
        assert np.array_equal(c, oc) and np.array_equal(d, od)
        monkeypatch.setenv("DREPHIP_SCREEN_LIGHT", "1")
        c, d, st1 = run(ctx, H, NH, ctx.SCREEN_ON)
        assert np.array_equal(c, oc) and np.array_equal(d, od)
        monkeypatch.setenv("DREPHIP_SCREEN_LIGHT", "0")
        c, d, st0 = run(ctx, H, NH, ctx.SCREEN_ON)
        assert np.array_equal(c, oc) and np.array_equal(d, od)
    assert st1["simple"] > st0["simple"] and st1["marked"] < st0["marked"], (st1, st0)


@pytest.mark.parametrize("light", ["0", "1"])
@pytest.mark.parametrize("name", NAMES)
def test_wide_screen_row_segments(name, light, monkeypatch):
    """Row segments off the tile grid: one starts inside the first window's
    rows, past its first genome (the window then starts at the segment's first
    tile), one is the last row alone."""
    H, NH, info, oc, od = wide(name)
    N = len(NH)
    g_lo = info.get("g_lo", 0)
    monkeypatch.setenv("DREPHIP_SCREEN_LIGHT", light)
    with _lib.Context(0, 21, S, 42) as ctx:
        cuts = [0, g_lo + 13, g_lo + ctx.screen_geometry() * ec.MARK_TILES + 3, N - 2, N - 1]
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            n = start(r1, N) - start(r0, N)
            co, do = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
            ctx.allpairs_rows(H, NH, r0, r1, co, do)
            assert ctx.screen_stats()["used"]
            assert np.array_equal(co, oc[start(r0, N):start(r1, N)]), (r0, r1)
            assert np.array_equal(do, od[start(r0, N):start(r1, N)]), (r0, r1)


@pytest.mark.parametrize("name", NAMES)
def test_wide_screen_sparse(name, monkeypatch):
    """The sparse list: the direct plan (with and without light cells, and in
    row blocks with a boundary inside a window) and the fallback."""
    H, NH, _, oc, od = wide(name)
    N = len(NH)
    exp = ec.nonzero_pairs(oc, od, N)
    with _lib.Context(0, 21, S, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        assert_pairs(ctx.allpairs_sparse(H, NH, cap=len(exp[0])), exp, "direct")
        assert ctx.sparse_stats()["direct"] == len(exp[0]) and ctx.sparse_stats()["fallback"] == 0
        monkeypatch.setenv("DREPHIP_SCREEN_LIGHT", "1")
        assert_pairs(ctx.allpairs_sparse(H, NH, cap=len(exp[0])), exp, "direct, light cells")
        assert ctx.sparse_stats()["direct"] == len(exp[0])
        monkeypatch.setenv("DREPHIP_SPARSE_BLOCK_ROWS", "600")       # 8 | 600: blocks cut every window of 1024 rows
        assert_pairs(ctx.allpairs_sparse(H, NH, cap=len(exp[0])), exp, "direct, light cells, row blocks")
        monkeypatch.delenv("DREPHIP_SCREEN_LIGHT")
        assert_pairs(ctx.allpairs_sparse(H, NH, cap=len(exp[0])), exp, "direct, row blocks")
        assert ctx.sparse_stats()["blocks"] >= 6 and ctx.sparse_stats()["fallback"] == 0
        monkeypatch.delenv("DREPHIP_SPARSE_BLOCK_ROWS")
        monkeypatch.setenv("DREPHIP_AP_SCREEN", "2")
        assert_pairs(ctx.allpairs_sparse(H, NH, cap=len(exp[0])), exp, "fallback")
        assert ctx.sparse_stats()["fallback"] == len(exp[0]) and ctx.sparse_stats()["direct"] == 0


@pytest.mark.parametrize("W", [2, 8])
@pytest.mark.parametrize("name", NAMES)
def test_wide_screen_sharded(name, W):
    """The sharded screen: W hash parts, rank boundaries off the tile grid."""
    import torch
    H, NH, _, oc, od = wide(name)
    N = len(NH)
    dH = torch.from_numpy(H.view(np.int64).copy()).cuda()
    dNH = torch.from_numpy(NH.view(np.int32).copy()).cuda()
    cuts = [0] + [N * k // W + 3 for k in range(1, W)] + [N - 1]
    with _lib.Context(0, 21, S, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        ranges = list(zip(cuts[:-1], cuts[1:]))
        segs, checks, _ = sharded_screen(ctx, dH, dNH, N, W, ranges)
        for (r0, r1), (co, do) in zip(ranges, segs):
            assert np.array_equal(co, oc[start(r0, N):start(r1, N)]), (r0, r1)
            assert np.array_equal(do, od[start(r0, N):start(r1, N)]), (r0, r1)
        assert checks > 0


def test_wide_screen_other_tile_size(monkeypatch):
    """Set C at s = 64 with 4 rows per tile (DREPHIP_AP_R=4): the window
    covers 512 rows."""
    s = 64
    monkeypatch.setenv("DREPHIP_AP_R", "4")
    with _lib.Context(0, 21, s, 42) as ctx:
        assert ctx.screen_geometry() == 4
        H, NH, _ = ec.wide_set_c(4, seed=9, s=s)
        N = len(NH)
        oc, od = oracle.allpairs(H, NH, s, threads=8)
        exp = ec.nonzero_pairs(oc, od, N)
        for light in ("0", "1"):
            monkeypatch.setenv("DREPHIP_SCREEN_LIGHT", light)
            c, d, st = run(ctx, H, NH, ctx.SCREEN_ON)
            assert st["used"] and np.array_equal(c, oc) and np.array_equal(d, od), light
            assert_pairs(ctx.allpairs_sparse(H, NH, cap=len(exp[0])), exp, "light " + light)
            assert ctx.sparse_stats()["direct"] == len(exp[0])
        c, d, st = run(ctx, H, NH, ctx.SCREEN_OFF)
        assert not st["used"] and np.array_equal(c, oc) and np.array_equal(d, od)


def test_screen_without_fingerprint():
    """N s > 2^28: the entry values keep fewer than kFpBits bits of the
    hashes' high words, so k_screen_mark tells a run of one hash from a
    collision run by reading every hash, and every reader of an entry masks
    the index.  8200 partial sketches of at most 16 hashes at s = 32767 (the
    band path, light cells on by default; more than 8192 columns: two bitmap
    words per thread in k_screen_lists), built on the device.  The reference
    is the incidence matrix of the short rows (edge_cases.incidence_allpairs,
    checked against the oracle on the CPU).  Every genome is partial, so the
    screen hands every sharing pair's cell to the kernel and -- the hash read
    is exact -- no other: the marked cells are counted too."""
    import torch
    s = ec.SHORT_S
    Hs, NH = ec.short_row_sets(seed=3)
    N = len(NH)
    oc, od, pi, pj = ec.incidence_allpairs(Hs, NH)
    dH = torch.full((N, s), -1, dtype=torch.int64, device="cuda")
    dH[:, :ec.SHORT_MAX] = torch.from_numpy(Hs.view(np.int64)).cuda()
    dNH = torch.from_numpy(NH.view(np.int32)).cuda()
    npairs = N * (N - 1) // 2
    co = torch.zeros(npairs, dtype=torch.int16, device="cuda")
    do = torch.zeros(npairs, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    with _lib.Context(0, 21, s, 42) as ctx:
        R = ctx.screen_geometry()
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        ctx.allpairs_device(dH.data_ptr(), dNH.data_ptr(), N, 0, N, co.data_ptr(), do.data_ptr(), st)
        torch.cuda.synchronize()
        stats = ctx.screen_stats()
        assert stats["used"] and stats["entries"] == int(NH.sum())
        assert np.array_equal(co.cpu().numpy().view(np.uint16), oc)
        assert np.array_equal(do.cpu().numpy().view(np.uint16), od)
        assert stats["marked"] == ec.cell_count(pi, pj, N, R), stats
        buf = torch.zeros((len(pi), 4), dtype=torch.int32, device="cuda")
        rc, n = ctx.allpairs_sparse_device(dH.data_ptr(), dNH.data_ptr(), N, 0, N, buf.data_ptr(), len(pi), st)
        torch.cuda.synchronize()
        assert rc == 0 and n == len(pi)
        rec = buf.cpu().numpy().view(np.uint32)
        rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
        t = ec.cond_index(pi.astype(np.int64), pj.astype(np.int64), N)
        assert_pairs((rec[:, 0], rec[:, 1], rec[:, 2].astype(np.uint16), rec[:, 3].astype(np.uint16)),
                     (pi, pj, oc[t], od[t]), "no fingerprint")
