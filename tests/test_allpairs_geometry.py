"""Every geometry of the whole-row kernel's table (allpairs.hip kQRows: rows
per tile R x chunk class NCH, each with its one launch bound), through every
flavour of k_allpairs_q that exists there: the dense triangle, its screened
LIST form, the sparse list, the dense rectangle, its records, and -- where the
table has them -- the rectangle's screened LIST forms.  Bit for bit against
the C oracle's Mash merge (reference: `mash dist`, drep/d_cluster.py:569-573).
The plan lines of DREPHIP_DEBUG name the R each call ran at, so a geometry
that fell through to another one's kernel fails here.

The geometries allpairs_geometry picks by itself come from s alone; the others
from the A/B override DREPHIP_AP_R.  (8, 16) runs a second time at s = 1000,
by override: a row image of 163072 bytes, near the 160 KiB the override admits."""
import re

import numpy as np
import pytest

import oracle
from drep_amd import _lib

pytestmark = pytest.mark.gpu
UMAX = np.iinfo(np.uint64).max
N, Q = 70, 19                   # neither a multiple of any R (1, 2, 4, 8)
FAM = 5                         # genomes per family: the pairs of one family share hashes, the others none

# (s, DREPHIP_AP_R or None, R, chunk class, the table's RECT LIST flag)
GEOMETRIES = [
    (300, None, 8, 8, True), (300, 4, 4, 8, False), (300, 2, 2, 8, False), (300, 1, 1, 8, False),
    (700, None, 8, 16, True), (1000, None, 4, 16, True), (700, 2, 2, 16, False), (700, 1, 1, 16, False),
    (1500, None, 4, 32, True), (2048, None, 2, 32, True), (1500, 1, 1, 32, False),
    (1000, 8, 8, 16, True),
]
_AP = re.compile(r"\[drephip\] ap plan: R (\d+) C \d+ items \d+ slots \d+ list (\d) ")
_RECT = re.compile(r"\[drephip\] rect plan: R (\d+) ")
_RECT_SCREEN = re.compile(r"\[drephip\] rect screen plan: R (\d+) ")


def sketches(n, s, rng, pools, short):
    """n sorted sketches, genome g drawing s of its family's 2 s pool values
    (g // FAM picks the family); the genomes in `short` keep s // 3 of them."""
    H = np.full((n, s), UMAX, dtype=np.uint64)
    NH = np.zeros(n, dtype=np.uint32)
    for g in range(n):
        k = s // 3 if g in short else s
        H[g, :k] = np.sort(rng.choice(pools[g // FAM], size=s, replace=False))[:k]
        NH[g] = k
    return H, NH


_CASES = {}


def case(s):
    """References, queries and the oracle's counts at sketch size s, computed
    once and shared (read-only): the triangle of the references and the
    query x reference rectangle, both from one run over the stacked set."""
    if s not in _CASES:
        rng = np.random.default_rng(7000 + s)
        pools = [np.unique(rng.integers(0, UMAX - 1, size=2 * s + 64, dtype=np.uint64))[:2 * s]
                 for _ in range(N // FAM)]
        H, NH = sketches(N, s, rng, pools, short=(13, 40))
        QH, QN = sketches(Q, s, rng, pools, short=(5,))
        M = N + Q
        oc, od = oracle.allpairs(np.concatenate([H, QH]), np.concatenate([NH, QN]), s, threads=8)
        i, j = np.triu_indices(M, 1)
        tri = (oc[j < N], od[j < N])
        k = (i < N) & (j >= N)                           # pair (reference i, query j): cell (j - N, i)
        rect = tuple(np.zeros((Q, N), np.uint16) for _ in range(2))
        for out, o in zip(rect, (oc, od)):
            out[j[k] - N, i[k]] = o[k]
        assert (tri[0] > 0).any() and (tri[0] == 0).any() and (rect[0] > 0).any() and (rect[0] == 0).any()
        assert (tri[1] < s).any() and (rect[1] < s).any()              # two short rows: a union below s
        for a in (H, NH, QH, QN) + tri + rect:
            a.setflags(write=False)
        _CASES[s] = (H, NH, QH, QN, tri, rect)
    return _CASES[s]


def records(common, denom, rows, cols):
    """(row, col, common, denom) of the non-zero counts, in (row, col) order."""
    k = common > 0
    return rows[k].astype(np.uint32), cols[k].astype(np.uint32), common[k], denom[k]


def same_records(got, exp):
    assert len(got[0]) == len(exp[0]), (len(got[0]), len(exp[0]))
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)


@pytest.mark.parametrize("s,env_r,R,nch,rect_list", GEOMETRIES)
def test_every_flavour_at_the_geometry(s, env_r, R, nch, rect_list, monkeypatch, capfd):
    assert nch == (8 if s <= 512 else 16 if s <= 1024 else 32)
    H, NH, QH, QN, (tc, td), (rc, rd) = case(s)
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    if env_r is not None:
        monkeypatch.setenv("DREPHIP_AP_R", str(env_r))
    ti, tj = np.triu_indices(N, 1)
    tri_records = records(tc, td, ti, tj)
    qi, ri = np.divmod(np.arange(Q * N), N)
    rect_records = records(rc.reshape(-1), rd.reshape(-1), qi, ri)
    with _lib.Context(0, 21, s, 42) as ctx:
        # the triangle: dense, screened (LIST), and the sparse list
        for mode, lst in ((ctx.SCREEN_OFF, "0"), (ctx.SCREEN_ON, "1")):
            ctx.set_allpairs_screen(mode)
            capfd.readouterr()
            c, d = ctx.allpairs(H, NH)
            ps = _AP.findall(capfd.readouterr().err)
            assert ps and all(p == (str(R), lst) for p in ps), ps
            assert np.array_equal(c, tc), np.nonzero(c != tc)[0][:8]
            assert np.array_equal(d, td), np.nonzero(d != td)[0][:8]
        same_records(ctx.allpairs_sparse(H, NH), tri_records)
        st = ctx.sparse_stats()
        assert (st["direct"], st["fallback"]) == (len(tri_records[0]), 0), st
        # the rectangle: dense and records, unscreened
        ctx.set_rect_screen(ctx.RECT_SCREEN_OFF)
        capfd.readouterr()
        c, d = ctx.dist_rect(QH, QN, H, NH)
        got = ctx.dist_rect_sparse(QH, QN, H, NH)
        err = capfd.readouterr().err
        assert _RECT.findall(err) == [str(R)] * 2 and not _RECT_SCREEN.search(err), err
        assert np.array_equal(c, rc), np.argwhere(c != rc)[:8]
        assert np.array_equal(d, rd), np.argwhere(d != rd)[:8]
        same_records(got, rect_records)
        # the forced two-set screen: the LIST flavours where the table has
        # them, else the unscreened plan again
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE)
        c, d = ctx.dist_rect(QH, QN, H, NH)
        got = ctx.dist_rect_sparse(QH, QN, H, NH)
        err = capfd.readouterr().err
        if rect_list:
            assert _RECT_SCREEN.findall(err) == [str(R)] * 2 and not _RECT.search(err), err
            assert ctx.last_rect_screen_stats()["used"]
        else:
            assert _RECT.findall(err) == [str(R)] * 2 and not _RECT_SCREEN.search(err), err
        assert np.array_equal(c, rc), np.argwhere(c != rc)[:8]
        assert np.array_equal(d, rd), np.argwhere(d != rd)[:8]
        same_records(got, rect_records)
