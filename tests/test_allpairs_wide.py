"""The all-pairs triangle (k_allpairs_q without LIST / RECT, its LIST flavour,
and k_allpairs_band in allpairs.hip) at the column tiles it runs at in
production and at the seams only the triangle has: the diagonal tile, where
each of the R interleaved rows starts at another column; the item count that
shrinks down the triangle; the condensed offsets of the stores; the chunk-mask
chain after the screen's dense verdict; LIST items of up to 512 screened
columns; the failed-table fallback loop's second trip with the `c <= i` skip;
the band kernel past one column tile of 128.

Expected values: the C oracle's literal merge of the whole triangle, computed
once per set; the reversed order of a set (other rows on the diagonal tiles and
in the short last row tile) is cut out of the same arrays.  Every comparison is
bit for bit on common and denom.  Dense results are taken through the device
entry point into device buffers the test poisons, with guards before and after
the segment, so a cell no kernel wrote shows.  The geometry a call ran at is
read from the library's own `ap plan` line (DREPHIP_DEBUG), not restated."""
import re

import numpy as np
import pytest

import edge_cases
import oracle
from drep_amd import _lib
from test_rect import unbuildable_rows

pytestmark = pytest.mark.gpu

POISON = 0xBEEF                 # no count: s <= 32767
FRONT, BACK = 4097, 4096        # guard elements; the odd one leaves the segment 2-byte aligned only

_PLAN = re.compile(r"\[drephip\] ap plan: R (\d+) C (\d+) items (\d+) slots (\d+) list (\d) cmask (\d) cached (\d) cmax (\d+)")
_KEYS = ("R", "C", "items", "slots", "list", "cmask", "cached", "cmax")


def plans(capfd):
    """The `ap plan` lines printed since the last read, as dicts."""
    return [dict(zip(_KEYS, map(int, m))) for m in _PLAN.findall(capfd.readouterr().err)]


def one_plan(capfd, R, C, **more):
    """The single plan line of the last call; it ran at (R, C), with at least
    2048 items where the column loop turns, and with the given fields."""
    ps = plans(capfd)
    assert len(ps) == 1, ps
    p = ps[0]
    assert (p["R"], p["C"]) == (R, C), p
    assert C == 16 or p["items"] >= 2048, p
    assert p["slots"] >= p["items"], p
    for k, v in more.items():
        assert p[k] == v, (k, p)
    return p


def start(i, N):
    return i * N - i * (i + 1) // 2


# ------------------------------------------------------------ the sets
_SETS = {1000: 1025, 100: 3000, 64: 2049, 4096: 257}        # s: N
_CACHE = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def wide(s, n=None, rev=False):
    """(H, NH, common, denom) of the s set: geometry_sketches(N, s) -- dense
    (nearly every pair shares a hash) with zero-key rows, twin rows, partial
    and empty rows -- and the oracle's whole triangle.  n: its first n genomes
    (the counts cut out by index); rev: that set in reversed order, row i the
    genome n - 1 - i (the counts through the square); rev = 7: reversed and
    rotated, row i the genome (n - 1 - i + 7) % n.  Built once, shared
    read-only."""
    N = _SETS[s]
    n = N if n is None else n
    key = (s, n, int(rev))
    if key in _CACHE:
        return _CACHE[key]
    if rev:
        H, NH, oc, od = wide(s, n)
        perm = (n - 1 - np.arange(n) + (0 if rev is True else int(rev))) % n
        pc, pd = edge_cases.permuted_condensed(oc, od, n, perm)
        got = _frozen(np.ascontiguousarray(H[perm]), np.ascontiguousarray(NH[perm]), pc, pd)
    elif n != N:
        H, NH, oc, od = wide(s)
        ii, jj = np.triu_indices(n, 1)
        t = edge_cases.cond_index(ii, jj, N)
        got = _frozen(np.ascontiguousarray(H[:n]), np.ascontiguousarray(NH[:n]), oc[t], od[t])
    else:
        H, NH = edge_cases.geometry_sketches(N, s, seed=7000 + s)
        oc, od = oracle.allpairs(H, NH, s, threads=8)
        got = _frozen(H, NH, oc, od)
    _CACHE[key] = got
    return got


def tile_chains(H, NH, R):
    """The probe chain k_allpairs_q takes for each row tile of the whole
    triangle (rows [0, N - 1) in tiles of R), from the sketches alone: "slow"
    when a row of the tile holds two keys with one low word (k_build_q32 keeps
    it off the fast probe), else "masked" when a row holds the key 0, else
    "fast".  Returns (the chain per tile, the rows of the last tile)."""
    N = len(NH)
    low = H & np.uint64(0xFFFFFFFF)
    twin = np.array([NH[g] > 1 and len(np.unique(low[g, :NH[g]])) < NH[g] for g in range(N)])
    zero = (NH > 0) & (H[:, 0] == 0)
    chains = []
    for i0 in range(0, N - 1, R):
        i1 = min(i0 + R, N - 1)
        chains.append("slow" if twin[i0:i1].any() else "masked" if zero[i0:i1].any() else "fast")
    return chains, (N - 1) - (len(chains) - 1) * R


def holds_its_chains(H, NH, R, kinds=("fast", "masked", "slow")):
    """At least 8 row tiles in each probe chain; the tiles start at row 0 and
    end with the short tile where (N - 1) % R != 0."""
    N = len(NH)
    chains, last_rows = tile_chains(H, NH, R)
    assert len(chains) == -(-(N - 1) // R) and last_rows == ((N - 1) % R or R)
    for k in kinds:
        assert chains.count(k) >= 8, (k, chains.count(k))
    return True


def orders(s, N, R):
    """The data sets of a shape: the set, its reversal and, where the reversal
    cannot hold every probe chain, the rotated reversal as well.  At N = 2049
    and R = 8 a reversed tile [8 k, 8 k + 8) is the genomes 2041 - 8 k ..
    2048 - 8 k, which touch three of the generator's blocks of four genomes,
    and one of any three consecutive blocks holds the key 0: no fast tile
    without it but the few whose zero-key rows are empty.  Rotated by 7 the
    tiles are the generator's own groups of eight again, in reversed order."""
    out = [wide(s, N), wide(s, N, rev=True)]
    assert holds_its_chains(*out[0][:2], R)
    if (N - 1) % 8 == 0 and R == 8:
        assert holds_its_chains(*out[1][:2], R, kinds=("masked", "slow"))
        out.append(wide(s, N, rev=7))
        assert holds_its_chains(*out[2][:2], R)
    else:
        assert holds_its_chains(*out[1][:2], R)
    return out


# ------------------------------------------------------------ how results are taken
def upload(H, NH):
    import torch
    dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    torch.cuda.synchronize()
    return dh, dn, len(NH)


def tri_device(ctx, dev, r0=0, r1=None, want_denom=True):
    """(common, denom or None) of rows [r0, r1) by drephip_allpairs_device into
    poisoned device buffers; asserts that the guards kept their poison."""
    import torch
    dh, dn, N = dev
    r1 = N if r1 is None else r1
    n = start(min(r1, N - 1), N) - start(r0, N)
    bufs = [torch.full((FRONT + n + BACK,), POISON - 0x10000, dtype=torch.int16, device="cuda")
            for _ in range(2 if want_denom else 1)]
    torch.cuda.synchronize()
    ctx.allpairs_device(dh.data_ptr(), dn.data_ptr(), N, r0, r1, bufs[0].data_ptr() + 2 * FRONT,
                        bufs[1].data_ptr() + 2 * FRONT if want_denom else None)
    out = []
    for b in bufs:
        a = b.cpu().numpy().view(np.uint16)
        assert (a[:FRONT] == POISON).all() and (a[FRONT + n:] == POISON).all()
        out.append(a[FRONT:FRONT + n])
    return out[0], (out[1] if want_denom else None)


def same(got, oc, od):
    """Bit for bit; a mismatch names its first cells (offsets in the segment), got and expected."""
    c, d = got
    assert c.shape == oc.shape, (c.shape, oc.shape)
    assert np.array_equal(c, oc), ("common", np.flatnonzero(c != oc)[:8], c[c != oc][:8], oc[c != oc][:8])
    if d is not None:
        assert np.array_equal(d, od), ("denom", np.flatnonzero(d != od)[:8], d[d != od][:8], od[d != od][:8])


def segment(oc, od, N, r0, r1):
    a, b = start(r0, N), start(min(r1, N - 1), N)
    return oc[a:b], od[a:b]


#           s     N     DREPHIP_AP_R  R  C
_SHAPES = [(1000, 1025, 1, 1, 512),             # NCH = 16; N = 2 x 512 + 1: the last column tile is one column
           (1000, 1025, None, 4, 64),
           (100, 3000, 4, 4, 512),              # R x columns per wave = 128
           (64, 2049, None, 8, 128),
           (1000, 1000, None, 4, 64),           # the production shape; sub-triangle
           (1000, 800, 1, 1, 256)]              # sub-triangle


def wide_env(monkeypatch, env_r, **env):
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    if env_r is None:
        monkeypatch.delenv("DREPHIP_AP_R", raising=False)
    else:
        monkeypatch.setenv("DREPHIP_AP_R", str(env_r))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def dense_verdict(ctx, NH):
    """The screen ran, gave way to the dense kernels, and had grouped every entry."""
    st = ctx.screen_stats()
    assert not st["used"] and st["entries"] == int(NH.sum()), st


# ------------------------------------------------------------ 1. every width
@pytest.mark.parametrize("s,N,env_r,R,C", _SHAPES)
def test_triangle_wide_tiles_vs_oracle(s, N, env_r, R, C, monkeypatch, capfd):
    """Screen off: the set and its reversal through the device entry point
    (with and without denominators) and through the host forms."""
    sets = orders(s, N, R)                              # (asserts the probe chains of each)
    fwd, rev = sets[:2]
    for H, NH, oc, od in sets:
        assert len(NH) == N and (oc > 0).mean() > 0.5 and (od < s).any()
    wide_env(monkeypatch, env_r)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_OFF)
        for H, NH, oc, od in sets:
            dev = upload(H, NH)
            capfd.readouterr()
            got = tri_device(ctx, dev)
            one_plan(capfd, R, C, list=0, cmask=0)
            same(got, oc, od)
            got = tri_device(ctx, dev, want_denom=False)
            one_plan(capfd, R, C, list=0, cmask=0)
            same(got, oc, od)
        # the host forms: allpairs with and without denominators, allpairs_rows into the caller's buffers
        H, NH, oc, od = fwd
        same(ctx.allpairs(H, NH, want_denom=True), oc, od)
        one_plan(capfd, R, C, list=0, cmask=0)
        H, NH, oc, od = rev
        c, d = ctx.allpairs(H, NH, want_denom=False)
        one_plan(capfd, R, C, list=0, cmask=0)
        same((c, None), oc, od)
        assert (d == s).all()
        bc = np.full(FRONT + len(oc) + BACK, POISON, dtype=np.uint16)
        bd = np.full(FRONT + len(oc) + BACK, POISON, dtype=np.uint16)
        ctx.allpairs_rows(H, NH, 0, N, bc[FRONT:FRONT + len(oc)], bd[FRONT:FRONT + len(oc)])
        one_plan(capfd, R, C, list=0, cmask=0)
        for b in (bc, bd):
            assert (b[:FRONT] == POISON).all() and (b[FRONT + len(oc):] == POISON).all()
        same((bc[FRONT:FRONT + len(oc)], bd[FRONT:FRONT + len(oc)]), oc, od)


# ------------------------------------------------------------ 2. the other instantiation chain
@pytest.mark.parametrize("shape", [0, 2])
def test_triangle_wide_without_hit_masks(shape, monkeypatch, capfd):
    """DREPHIP_AP_HIT=0: the round-5 probe and scan ends, at C = 512."""
    s, N, env_r, R, C = _SHAPES[shape]
    wide_env(monkeypatch, env_r, DREPHIP_AP_HIT=0)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_OFF)
        for H, NH, oc, od in (wide(s, N), wide(s, N, rev=True)):
            dev = upload(H, NH)
            capfd.readouterr()
            got = tri_device(ctx, dev)
            one_plan(capfd, R, C, list=0, cmask=0)
            same(got, oc, od)


# ------------------------------------------------------------ 3. the chunk-mask chain
@pytest.mark.parametrize("shape", [0, 1, 3])
def test_triangle_wide_dense_verdict_chunk_masks(shape, monkeypatch, capfd):
    """Screen AUTO from two genomes on: these dense sets get the dense verdict
    (the checks outnumber what the screen may cost by far), and the fast tiles
    without the key 0 run probe_rows_v under the chunk masks; then the same
    with DREPHIP_AP_CMASK=0 (no masks: the plain chain after a screen run)."""
    s, N, env_r, R, C = _SHAPES[shape]
    wide_env(monkeypatch, env_r, DREPHIP_SCREEN_MIN_N=2)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_AUTO)
        for H, NH, oc, od in orders(s, N, R)[::-1]:     # (ends with the set itself: fast tiles without the key 0)
            dev = upload(H, NH)
            capfd.readouterr()
            got = tri_device(ctx, dev)
            one_plan(capfd, R, C, list=0, cmask=1)
            dense_verdict(ctx, NH)
            same(got, oc, od)
        got = tri_device(ctx, dev, want_denom=False)
        one_plan(capfd, R, C, list=0, cmask=1)
        same(got, oc, od)
        monkeypatch.setenv("DREPHIP_AP_CMASK", "0")
        got = tri_device(ctx, dev)
        one_plan(capfd, R, C, list=0, cmask=0)
        dense_verdict(ctx, NH)
        same(got, oc, od)


# ------------------------------------------------------------ 4. LIST items of many columns
@pytest.mark.parametrize("shape", [0, 2, 3])
def test_triangle_wide_list_items(shape, monkeypatch, capfd):
    """Screen ON: nearly every column of a row tile is marked, so the LIST
    items hold hundreds of columns; the condensed result, and the records of
    the SPARSE flavour (shape 2: the mid-loop record flush at R x columns per
    wave = 128)."""
    s, N, env_r, R, _ = _SHAPES[shape]
    H, NH, oc, od = wide(s, N)
    wide_env(monkeypatch, env_r)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        for Hx, NHx, ocx, odx in ((H, NH, oc, od), wide(s, N, rev=True)):
            dev = upload(Hx, NHx)
            capfd.readouterr()
            got = tri_device(ctx, dev)
            ps = plans(capfd)
            assert len(ps) == 1 and ps[0]["R"] == R and ps[0]["list"] == 1 and ps[0]["cmask"] == 0, ps
            # (no bound on the item count: the screened items are cut at 512 columns whatever their number --
            # the plan's rule, which halves C below 2048 items, does not apply to them)
            assert ps[0]["cmax"] > 64 and ps[0]["slots"] >= ps[0]["items"] >= (N - 1) // R // 2, ps
            st = ctx.screen_stats()
            assert st["used"] and st["entries"] == int(NHx.sum())
            same(got, ocx, odx)
        exp = edge_cases.nonzero_pairs(oc, od, N)
        got = ctx.allpairs_sparse(H, NH, cap=len(exp[0]))
        st = ctx.sparse_stats()
        assert (got[0] < got[1]).all()                                          # no record with i >= j
        assert len(np.unique(got[0].astype(np.int64) * N + got[1])) == len(got[0])      # none twice
        assert len(got[0]) == len(exp[0])
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
        assert (st["direct"], st["fallback"]) == (len(exp[0]), 0), st


# ------------------------------------------------------------ 5. row segments
@pytest.mark.parametrize("shape", [0, 1])
def test_triangle_wide_row_segments(shape, monkeypatch, capfd):
    """Row ranges whose first row is no multiple of R and whose last tile is
    short, and one-row ranges at both ends of the triangle: each writes its
    condensed segment and nothing else.  Then three balanced row shards on
    three contexts (the in-process multi-device driver)."""
    from drep_amd.d_cluster import condensed_allpairs
    s, N, env_r, R, C = _SHAPES[shape]
    H, NH, oc, od = wide(s, N)
    wide_env(monkeypatch, env_r)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_OFF)
        dev = upload(H, NH)
        capfd.readouterr()
        # the narrowest tile each range may run at.  The lower half at R = 4 is 128 row tiles over at most 512
        # columns: even at C = 32 that is about a thousand items, so the plan's rule leaves it at C = 16
        cmin = (64, 64 if R == 1 else 16, 16, 16)
        for (r0, r1), c in zip(((3, N - 4), (N // 2 + 1, N - 1), (0, 1), (N - 2, N - 1)), cmin):
            got = tri_device(ctx, dev, r0, r1)                  # (asserts the guards)
            ps = plans(capfd)
            assert len(ps) == 1 and ps[0]["R"] == R and ps[0]["list"] == 0, (r0, r1, ps)
            assert ps[0]["C"] >= c and (ps[0]["C"] == 16 or ps[0]["items"] >= 2048), (r0, r1, ps)
            same(got, *segment(oc, od, N, r0, r1))
    c, d = condensed_allpairs(H, NH, s, devices=(0, 0, 0))
    ps = plans(capfd)
    assert len(ps) == 3 and all(p["R"] == R for p in ps), ps
    same((c, d), oc, od)


# ------------------------------------------------------------ 6. the item-list cache
def test_triangle_wide_item_cache_follows_the_data(monkeypatch, capfd):
    """The cached item list depends on the shape alone: other data in the same
    device buffers reuse it and get their own counts; a scratch reallocation
    (a linkage call) drops it."""
    import torch
    s, N, env_r, R, C = _SHAPES[1]
    fwd, rev = wide(s, N), wide(s, N, rev=True)
    wide_env(monkeypatch, env_r)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_OFF)
        dev = upload(*fwd[:2])
        capfd.readouterr()
        for (H, NH, oc, od), cached in ((fwd, 0), (rev, 1), (fwd, 1)):
            dev[0].copy_(torch.from_numpy(H.copy().view(np.int64)))
            dev[1].copy_(torch.from_numpy(NH.copy().view(np.int32)))
            torch.cuda.synchronize()
            got = tri_device(ctx, dev)
            one_plan(capfd, R, C, list=0, cached=cached)
            same(got, oc, od)
        n = 300
        y = np.random.default_rng(6).random(n * (n - 1) // 2)
        ctx.set_linkage_path(ctx.LINK_DENSE)            # the device path: its matrix is new scratch
        assert ctx.linkage(y, "average").shape == (n - 1, 4) and not ctx.linkage_info()["sparse"]
        capfd.readouterr()
        H, NH, oc, od = fwd
        got = tri_device(ctx, dev)
        one_plan(capfd, R, C, list=0, cached=0)
        same(got, oc, od)
        got = tri_device(ctx, dev)
        one_plan(capfd, R, C, list=0, cached=1)
        same(got, oc, od)


# ------------------------------------------------------------ 7. rows without a table
_UNBUILDABLE = {}


def unbuildable_set():
    """The s = 100 set with rows 0, 7, 2047, 2049 and N - 1 replaced by rows of
    three keys with one low word (no cuckoo table holds them: whatever the
    field family, the three share both slots), and their neighbours (1, 8,
    2048, 2050, N - 2) by rows sharing two of those keys; its own oracle."""
    if not _UNBUILDABLE:
        s = 100
        H0, NH0, _, _ = wide(s)
        H, NH = H0.copy(), NH0.copy()
        N = len(NH)
        h, nh = unbuildable_rows(s)
        bad = (0, 7, 2047, 2049, N - 1)
        for k, (g, nb) in enumerate(zip(bad, (1, 8, 2048, 2050, N - 2))):
            src = 0 if k % 2 == 0 else 7
            H[g], NH[g] = h[src], nh[src]
            H[nb], NH[nb] = h[src + 1], nh[src + 1]
        oc, od = oracle.allpairs(H, NH, s, threads=8)
        _UNBUILDABLE["set"] = _frozen(H, NH, oc, od) + (bad,)
    return _UNBUILDABLE["set"]


@pytest.mark.parametrize("mode", ["off", "dense"])
def test_triangle_wide_unbuildable_rows(mode, monkeypatch, capfd):
    """The literal-merge fallback inside k_allpairs_q at R x C = 4 x 512 cells
    per item: its lanes take a second trip, skip the cells at and below the
    diagonal, and store at condensed offsets."""
    s, N, env_r, R, C = _SHAPES[2]
    H, NH, oc, od, bad = unbuildable_set()
    for g in bad:
        lw = H[g, :NH[g]] & np.uint64(0xFFFFFFFF)
        assert (np.unique(lw, return_counts=True)[1] == 3).any()        # three keys, one low word
    t = lambda i, j: edge_cases.cond_index(i, j, N)
    assert oc[t(0, 1)] >= 2 and oc[t(7, 8)] >= 2 and oc[t(0, 7)] >= 3 and oc[t(2047, 2049)] >= 3
    assert oc[t(2047, N - 1)] >= 3 and oc[t(2049, 2050)] >= 2 and oc[t(N - 2, N - 1)] >= 2
    assert R * C > 1024                                 # more cells per item than the workgroup has lanes
    env = {"DREPHIP_SCREEN_MIN_N": 2} if mode == "dense" else {}
    wide_env(monkeypatch, env_r, **env)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_AUTO if mode == "dense" else ctx.SCREEN_OFF)
        dev = upload(H, NH)
        capfd.readouterr()
        got = tri_device(ctx, dev)
        one_plan(capfd, R, C, list=0, cmask=int(mode == "dense"))
        if mode == "dense":
            dense_verdict(ctx, NH)
        same(got, oc, od)
        got = tri_device(ctx, dev, want_denom=False)
        one_plan(capfd, R, C, list=0, cmask=int(mode == "dense"))
        same(got, oc, od)


# ------------------------------------------------------------ 8. the band kernel past one column tile
@pytest.mark.parametrize("variant", ["cap64", "cap300", "cap768", "segments", "round500"])
def test_band_past_one_column_tile(variant, monkeypatch, capfd):
    """s = 4096 (no whole-row table fits), N = 257 = 2 x 128 + 1: three column
    tiles, the last of one column; band caps below, near and at the kernel's
    768; screen off and the dense verdict; row segments; value rounds."""
    s = 4096
    N = _SETS[s]
    H, NH, oc, od = wide(s)
    assert N == 2 * 128 + 1 and (oc > 0).mean() > 0.5 and (od < s).any()
    cap = {"cap64": 64, "cap300": 300, "cap768": 768}.get(variant, 300)
    env = {"DREPHIP_BAND_ROUND": 500} if variant == "round500" else {}
    wide_env(monkeypatch, None, **env)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_path(ctx.AP_BAND, cap)
        dev = upload(H, NH)
        capfd.readouterr()
        if variant == "segments":
            ctx.set_allpairs_screen(ctx.SCREEN_OFF)
            for r0, r1 in ((3, N - 4), (N // 2 + 1, N - 1), (0, 1), (N - 2, N - 1)):
                same(tri_device(ctx, dev, r0, r1), *segment(oc, od, N, r0, r1))
        else:
            for Hx, NHx, ocx, odx in ((H, NH, oc, od), wide(s, rev=True)):
                devx = upload(Hx, NHx)
                ctx.set_allpairs_screen(ctx.SCREEN_OFF)
                same(tri_device(ctx, devx), ocx, odx)
                same(tri_device(ctx, devx, want_denom=False), ocx, odx)
                monkeypatch.setenv("DREPHIP_SCREEN_MIN_N", "2")
                ctx.set_allpairs_screen(ctx.SCREEN_AUTO)
                same(tri_device(ctx, devx), ocx, odx)
                dense_verdict(ctx, NHx)
                monkeypatch.delenv("DREPHIP_SCREEN_MIN_N")
        assert plans(capfd) == []                       # the band path: no whole-row-table plan
