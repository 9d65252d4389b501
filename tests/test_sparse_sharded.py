"""The sharded sparse all-pairs call (drephip_allpairs_sparse_device_marked,
screen.hip): a rank's rows [row0, row1) as records {i, j, common, denom} of the
pairs that share a hash, screened from every hash part's marks
(drephip_screen_part) instead of a grouping of its own -- and the part's bitmap
walked in blocks of row tiles.  One process plays all W ranks, as
tests/test_screen.py::sharded_screen does: one context groups every part and
concatenates their cells and records (a rank receives its own rows' marks; the
call ignores the others).  Every list is compared field by field with the C
oracle's Mash merge (reference: `mash dist`, drep/d_cluster.py:569-573)
restricted to common > 0; assert_list also checks that no pair appears twice."""
import numpy as np
import pytest

import oracle
import edge_cases as ec
from drep_amd import _lib
from drep_amd import parallel
from test_sparse import assert_list, case, expected_list, rows_of

pytestmark = pytest.mark.gpu
UMAX = np.iinfo(np.uint64).max
ERR_NOMEM = -4
EMPTY = tuple(np.zeros(0, t) for t in (np.uint32, np.uint32, np.uint16, np.uint16))


def to_device(H, NH):
    import torch
    return (torch.from_numpy(H.view(np.int64).copy()).cuda(), torch.from_numpy(NH.view(np.int32).copy()).cuda())


def part_marks(ctx, dH, dNH, N, p, W):
    """Part p of W grouped and copied out: (cells [n, 4], records [m, 4], pair checks)."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    c, nc, n = ctx.screen_part(dH.data_ptr(), dNH.data_ptr(), N, p, W, st)
    cl = torch.empty((max(nc, 1), 4), dtype=torch.int32, device="cuda")
    rec = torch.empty((max(n, 1), 4), dtype=torch.int32, device="cuda")
    ctx.screen_part_copy(cl.data_ptr(), rec.data_ptr(), st)
    return cl[:nc], rec[:n], c


def all_marks(ctx, dH, dNH, N, W):
    """Every part's cells and records concatenated, and the records per part."""
    import torch
    parts = [part_marks(ctx, dH, dNH, N, p, W) for p in range(W)]
    return (torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous(),
            [len(p[1]) for p in parts])


def marked_raw(ctx, dH, dNH, N, r0, r1, cells, recs, buf, cap):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    rc, n = ctx.allpairs_sparse_device_marked(dH.data_ptr(), dNH.data_ptr(), N, r0, r1,
                                              cells.data_ptr() if len(cells) else None, len(cells),
                                              recs.data_ptr() if len(recs) else None, len(recs),
                                              buf.data_ptr() if buf is not None else None, cap, st)
    torch.cuda.synchronize()
    return rc, n


def marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, room):
    """The call's list sorted by (i, j), as (i, j, common, denom); `room`
    records past which a guard region must stay untouched."""
    import torch
    SENT = np.uint32(0xDEADBEEF).view(np.int32).item()
    buf = torch.full((room + 16, 4), SENT, dtype=torch.int32, device="cuda")
    rc, n = marked_raw(ctx, dH, dNH, N, r0, r1, cells, recs, buf, room)
    assert rc == 0 and n <= room, (rc, n, room)
    out = buf.cpu().numpy().view(np.uint32)
    assert (out[room:] == np.uint32(0xDEADBEEF)).all()
    rec = out[:n]
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
    return (np.ascontiguousarray(rec[:, 0]), np.ascontiguousarray(rec[:, 1]), rec[:, 2].astype(np.uint16),
            rec[:, 3].astype(np.uint16))


def concat(parts):
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


UNALIGNED = lambda N: [(0, 1), (1, 37), (37, 121), (121, N)]      # noqa: E731


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("s,N", [(64, 300), (1000, 200), (2048, 96)])
def test_marked_equals_oracle(s, N, W):
    """Every range's list equals the oracle's rows; the ranges of a partition
    together give the whole list; all of it on the direct path."""
    H, NH, exp = case(s, N)
    dH, dNH = to_device(H, NH)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
        assert len(cells) > 0
        for ranges in (parallel.row_partition(N, W), UNALIGNED(N)):
            got = []
            for r0, r1 in ranges:
                want = rows_of(exp, r0, r1)
                g = marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, len(want[0]))
                assert_list(g, want, "rows [%d, %d)" % (r0, r1))
                if r0 < min(r1, N - 1):
                    st = ctx.sparse_stats()
                    assert st["direct"] == len(want[0]) and st["fallback"] == 0 and st["blocks"] >= 1, st
                    assert st["scratch_bytes"] > 0
                    assert ctx.screen_stats()["used"]
                got.append(g)
            assert_list(concat(got), exp, "union")


def test_marked_band_takes_the_fallback():
    s, N, W = 4096, 80, 2
    H, NH, exp = case(s, N)
    dH, dNH = to_device(H, NH)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
        got = []
        for r0, r1 in parallel.row_partition(N, W):
            want = rows_of(exp, r0, r1)
            g = marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, len(want[0]))
            assert_list(g, want, "rows [%d, %d)" % (r0, r1))
            st = ctx.sparse_stats()
            assert st["fallback"] == len(want[0]) and st["direct"] == 0, st
            assert ctx.screen_stats()["used"]           # the marked dense call screened the rows
            got.append(g)
        assert_list(concat(got), exp, "union")


@pytest.mark.parametrize("rows", ["R", "3R", "16"])
@pytest.mark.parametrize("s,N", [(1000, 200), (64, 300)])
def test_marked_row_blocks(s, N, rows, monkeypatch):
    W = 3
    H, NH, exp = case(s, N)
    dH, dNH = to_device(H, NH)
    with _lib.Context(0, 21, s, 42) as ctx:
        R = ctx.screen_geometry()
        br = {"R": R, "3R": 3 * R, "16": 16}[rows]
        monkeypatch.setenv("DREPHIP_SPARSE_BLOCK_ROWS", str(br))
        br = max(R, -(-br // R) * R)                       # the call rounds up to whole row tiles
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
        for k, ranges in enumerate((parallel.row_partition(N, W), [(1, 37), (37, 121)])):
            for r0, r1 in ranges:
                want = rows_of(exp, r0, r1)
                g = marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, len(want[0]))
                assert_list(g, want, "rows [%d, %d) in blocks of %s" % (r0, r1, rows))
                st = ctx.sparse_stats()
                nb = -(-(min(r1, N - 1) - r0) // br)
                assert st["blocks"] == nb and (k or nb >= 3) and st["fallback"] == 0, (st, nb)
                assert st["direct"] == len(want[0])


def test_marked_capacity():
    import torch
    s, N, W = 1000, 200, 2
    H, NH, exp = case(s, N)
    r0, r1 = parallel.row_partition(N, W)[0]
    want = rows_of(exp, r0, r1)
    n = len(want[0])
    assert n > 8
    lookup = {(int(a), int(b)): (int(c), int(d)) for a, b, c, d in zip(*want)}
    SENT = np.uint32(0xDEADBEEF).view(np.int32).item()
    dH, dNH = to_device(H, NH)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
        rc, got = marked_raw(ctx, dH, dNH, N, r0, r1, cells, recs, None, 0)      # cap = 0 only counts
        assert rc == ERR_NOMEM and got == n
        assert "records" in _lib.lib().drephip_last_error().decode()
        for cap in (n - 1, n // 2):
            buf = torch.full((cap + 64, 4), SENT, dtype=torch.int32, device="cuda")
            rc, got = marked_raw(ctx, dH, dNH, N, r0, r1, cells, recs, buf, cap)
            assert rc == ERR_NOMEM and got == n
            out = buf.cpu().numpy().view(np.uint32)
            assert (out[cap:] == np.uint32(0xDEADBEEF)).all()                    # the guard records
            assert (out[:cap] != np.uint32(0xDEADBEEF)).any(axis=1).all()        # every slot below cap stored
            seen = set()
            for a, b, c, d in out[:cap]:
                assert lookup[(int(a), int(b))] == (int(c), int(d)) and (int(a), int(b)) not in seen
                seen.add((int(a), int(b)))
        assert_list(marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, got), want, "retry with n")


def cross_part_sketches(s, N=24):
    """Full sketches of distinct random values in [2^40, 2^61) with planted
    hashes: low ones (below 2^30: rank 0.., hash part 0 of 2) and high ones
    (above 2^62: the last ranks, part 1).
      (a) genomes 0, 9    share one low and one high hash (a run of two in each part)
      (b) genomes 2, 11   share a low hash (run of two, part 0); 2, 11 and 13
                          share a high hash (run of three, part 1)
      (c) genomes 5, 17   share one high hash: rank sum >= s
      (d) genomes 7, 20   share one low hash; 20 is partial"""
    rng = np.random.default_rng(s)
    lo = [int(x) for x in rng.choice(np.arange(1 << 20, 1 << 30), 3, replace=False)]
    hi = [(1 << 62) + int(x) for x in rng.choice(np.arange(1, 1 << 30), 3, replace=False)]
    plant = {0: [lo[0], hi[0]], 9: [lo[0], hi[0]], 2: [lo[1], hi[1]], 11: [lo[1], hi[1]], 13: [hi[1]],
             5: [hi[2]], 17: [hi[2]], 7: [lo[2]], 20: [lo[2]]}
    H = np.full((N, s), UMAX, dtype=np.uint64)
    NH = np.full(N, s, dtype=np.uint32)
    NH[20] = s - s // 4
    for g in range(N):
        own = plant.get(g, [])
        base = rng.integers(1 << 40, 1 << 61, size=2 * s, dtype=np.uint64)
        base = np.unique(base)[:int(NH[g]) - len(own)]
        row = np.sort(np.concatenate([base, np.array(own, dtype=np.uint64)]))
        assert len(row) == NH[g] and len(np.unique(row)) == len(row)
        H[g, :len(row)] = row
    return H, NH


@pytest.mark.parametrize("s", [64, 1000])
def test_marked_cross_part_writers(s):
    """Pairs whose evidence is split between two hash parts: each is listed
    exactly once (or not at all) with the oracle's count and denominator."""
    W = 2
    H, NH = cross_part_sketches(s)
    N = len(NH)
    exp = expected_list(H, NH, s)
    pairs = {(int(a), int(b)): (int(c), int(d)) for a, b, c, d in zip(*exp)}
    # the oracle's view of the planted cases
    assert set(pairs) == {(0, 9), (2, 11), (2, 13), (11, 13), (7, 20)} or \
        set(pairs) == {(0, 9), (2, 11), (7, 20)}, pairs                  # (c) is never listed: rank sum >= s
    assert (5, 17) not in pairs and pairs[(0, 9)][0] >= 1
    dH, dNH = to_device(H, NH)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        cells, recs, nrecs = all_marks(ctx, dH, dNH, N, W)
        # (a), (c): runs of two in part 1; (a), (b), (d): runs of two in part 0
        assert nrecs[0] >= 3 and nrecs[1] >= 2, nrecs
        rec = recs.cpu().numpy().view(np.uint32)
        keys = [(int(a), int(b)) for a, b in rec[:, :2]]
        assert keys.count((0, 9)) == 2 and keys.count((2, 11)) == 1 and keys.count((5, 17)) == 1
        assert len(cells) >= 1                                            # (b)'s run of three
        for ranges in ([(0, N)], parallel.row_partition(N, W), [(0, 3), (3, 6), (6, N)]):
            got = []
            for r0, r1 in ranges:
                want = rows_of(exp, r0, r1)
                g = marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, len(want[0]) + 4)
                assert_list(g, want, "rows [%d, %d)" % (r0, r1))
                assert ctx.sparse_stats()["fallback"] == 0
                got.append(g)
            assert_list(concat(got), exp, "union")


_WIDE = {}


def wide_sets():
    if not _WIDE:
        with _lib.Context(0, 21, 16, 42) as ctx:
            R = ctx.screen_geometry()
        for n, (H, NH, _) in ec.wide_screen_sets(R, seed=7).items():
            oc, od = oracle.allpairs(H, NH, 16, threads=8)
            exp = ec.nonzero_pairs(oc, od, len(NH))
            for a in (H, NH) + tuple(exp):
                a.setflags(write=False)
            _WIDE[n] = (H, NH, exp)
    return _WIDE


@pytest.mark.parametrize("W", [2, 8])
@pytest.mark.parametrize("name", ["A0", "A1", "A31", "B", "C"])
def test_marked_wide_sets(name, W):
    """More genomes than the marking window has tiles and columns, twins,
    collision runs, hubs longer than a wave; rank boundaries off the tile grid."""
    s = 16
    H, NH, exp = wide_sets()[name]
    N = len(NH)
    dH, dNH = to_device(H, NH)
    cuts = [0] + [N * k // W + 3 for k in range(1, W)] + [N]
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
        got = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            want = rows_of(exp, r0, r1)
            g = marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, len(want[0]))
            assert_list(g, want, "%s rows [%d, %d)" % (name, r0, r1))
            st = ctx.sparse_stats()
            assert st["direct"] == len(want[0]) and st["fallback"] == 0
            got.append(g)
        assert_list(concat(got), exp, name)


def test_rows_sharded_one_process_retries_once():
    """distributed.allpairs_sparse_rows_sharded outside a process group (the
    sharded screen does not apply: the plain sparse call on the rows): set C
    holds more pairs than the first buffer's 8 per row + 4096, so the call is
    repeated once at the size the library reports; the records come back
    sorted by (i, j)."""
    from drep_amd import distributed as D
    s = 16
    H, NH, exp = wide_sets()["C"]
    N = len(NH)
    assert len(exp[0]) > 8 * N + 4096
    dH, dNH = to_device(H, NH)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        import torch
        rec, n = D.allpairs_sparse_rows_sharded(ctx, dH, dNH, N, 0, N, torch.cuda.current_stream().cuda_stream, "cuda")
        assert n == len(exp[0]) and tuple(rec.shape) == (n, 4) and rec.dtype == torch.int32
        assert ctx.allpairs_screen == ctx.SCREEN_ON
        r = rec.cpu().numpy().view(np.uint32)
        assert_list((np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1]), r[:, 2].astype(np.uint16),
                     r[:, 3].astype(np.uint16)), exp, "set C, sorted on the device")


@pytest.mark.parametrize("W", [2, 8])
def test_marked_short_rows(W):
    """N s > 2^28 (no fingerprint in the entry values), s = 32767: the band
    path, so the fallback, from the parts' marks."""
    import torch
    s = ec.SHORT_S
    Hs, NH = ec.short_row_sets(seed=3)
    N = len(NH)
    oc, od, pi, pj = ec.incidence_allpairs(Hs, NH)
    t = ec.cond_index(pi.astype(np.int64), pj.astype(np.int64), N)
    exp = (pi, pj, oc[t], od[t])
    dH = torch.full((N, s), -1, dtype=torch.int64, device="cuda")
    dH[:, :ec.SHORT_MAX] = torch.from_numpy(Hs.view(np.int64)).cuda()
    dNH = torch.from_numpy(NH.view(np.int32)).cuda()
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
        got = []
        for r0, r1 in parallel.row_partition(N, 2):
            want = rows_of(exp, r0, r1)
            g = marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, len(want[0]))
            assert_list(g, want, "rows [%d, %d)" % (r0, r1))
            assert ctx.sparse_stats()["fallback"] == len(want[0])
            got.append(g)
        assert_list(concat(got), exp, "union")


def test_marked_small_cases():
    import torch
    s = 64
    rng = np.random.default_rng(5)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        for N in (2, 3):
            H = np.sort(rng.integers(1, 1 << 62, size=(N, s), dtype=np.uint64), axis=1)
            H[1, :10] = H[0, :10]                        # genomes 0 and 1 share ten hashes
            H[1] = np.sort(H[1])
            NH = np.full(N, s, dtype=np.uint32)
            exp = expected_list(H, NH, s)
            assert len(exp[0]) >= 1
            dH, dNH = to_device(H, NH)
            for W in (1, 2):
                cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
                assert_list(marked_list(ctx, dH, dNH, N, 0, N, cells, recs, len(exp[0])), exp, "N = %d" % N)
                # a range that starts at the last genome (or past it) holds no pair
                for r0 in (N - 1, N, N + 5):
                    assert_list(marked_list(ctx, dH, dNH, N, r0, N + 7, cells, recs, 4), EMPTY, "row0 = %d" % r0)
                    assert ctx.sparse_stats()["blocks"] == 0
        # every sketch empty; nothing shared
        N = 40
        for H, NH in ((np.full((N, s), UMAX, dtype=np.uint64), np.zeros(N, dtype=np.uint32)),
                      (np.sort(rng.integers(1, 1 << 62, size=(N, s), dtype=np.uint64), axis=1),
                       np.full(N, s, dtype=np.uint32))):
            dH, dNH = to_device(H, NH)
            st = torch.cuda.current_stream().cuda_stream
            for p in range(2):
                _, nc, n = ctx.screen_part(dH.data_ptr(), dNH.data_ptr(), N, p, 2, st)
                assert nc == 0 and n == 0
            e = torch.empty((0, 4), dtype=torch.int32, device="cuda")
            for r0, r1 in ((0, N), (3, 21)):
                assert_list(marked_list(ctx, dH, dNH, N, r0, r1, e, e, 4), EMPTY, "nothing shared")
                st2 = ctx.sparse_stats()
                assert st2["direct"] == 0 and st2["fallback"] == 0 and st2["blocks"] >= 1


@pytest.mark.parametrize("tiles", [1, 5])
@pytest.mark.parametrize("s,N", [(64, 300), (1000, 200)])
def test_screen_part_in_row_tile_blocks(s, N, tiles, monkeypatch):
    """The part's bitmap walked in blocks of row tiles: the same counts, the
    same cells in the same order, the same records, for every part."""
    W = 3
    H, NH, _ = case(s, N)
    dH, dNH = to_device(H, NH)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        assert (N + ctx.screen_geometry() - 1) // ctx.screen_geometry() > 2 * tiles      # several blocks
        base = [part_marks(ctx, dH, dNH, N, p, W) for p in range(W)]
        base = [(c.cpu().numpy().copy(), r.cpu().numpy().copy(), k) for c, r, k in base]
        assert sum(len(c) for c, _, _ in base) > 0 and sum(len(r) for _, r, _ in base) > 0
        monkeypatch.setenv("DREPHIP_SCREEN_PART_BLOCK_TILES", str(tiles))
        for p in range(W):
            c, r, k = part_marks(ctx, dH, dNH, N, p, W)
            c, r = c.cpu().numpy(), r.cpu().numpy()
            assert k == base[p][2] and len(c) == len(base[p][0]) and len(r) == len(base[p][1])
            assert np.array_equal(c, base[p][0]), "cells of part %d" % p
            order = lambda a: a[np.lexsort(a.T[::-1])]                  # noqa: E731
            assert np.array_equal(order(r), order(base[p][1])), "records of part %d" % p


def test_marked_arguments_checked():
    import torch
    s = 1000
    with _lib.Context(0, 21, s, 42) as ctx:
        h = torch.zeros((4, s), dtype=torch.int64, device="cuda")
        n = torch.zeros(4, dtype=torch.int32, device="cuda")
        m = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
        hp, np_, mp = h.data_ptr(), n.data_ptr(), m.data_ptr()
        for args in ((None, np_, 4, 0, 4, None, 0, None, 0, mp, 4),           # no hashes
                     (hp, None, 4, 0, 4, None, 0, None, 0, mp, 4),            # no counts
                     (hp, np_, 4, 0, 4, None, 0, None, 0, None, 4),           # room for records, no buffer
                     (hp, np_, 4, 0, 4, None, 2, None, 0, mp, 4),             # cells counted, none given
                     (hp, np_, 4, 0, 4, None, 0, None, 2, mp, 4)):            # records counted, none given
            with pytest.raises(_lib.DrepHipError, match="null argument"):
                ctx.allpairs_sparse_device_marked(*args)
        cnt = _lib.C.c_uint64(0)
        assert _lib.lib().drephip_allpairs_sparse_device_marked(ctx._h, hp, np_, 4, 0, 4, None, 0, None, 0, mp, 4,
                                                                None, None) != 0             # no n_pairs
        assert "null argument" in _lib.lib().drephip_last_error().decode()
        assert _lib.lib().drephip_allpairs_sparse_device_marked(None, hp, np_, 4, 0, 4, None, 0, None, 0, mp, 4,
                                                                _lib.C.byref(cnt), None) != 0
        ctx.set_allpairs_path(ctx.AP_MERGE)
        with pytest.raises(_lib.DrepHipError, match="marks need the table or band path"):
            ctx.allpairs_sparse_device_marked(hp, np_, 4, 0, 4, None, 0, None, 0, mp, 4)
    with _lib.Context(0, 21, 32767, 42) as ctx:                                # N x s >= 2^32
        with pytest.raises(_lib.DrepHipError, match="the screen needs N x s < 2\\^32"):
            ctx.allpairs_sparse_device_marked(hp, np_, 1 << 18, 0, 4, None, 0, None, 0, mp, 4)
