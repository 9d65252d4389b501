"""The sparse all-pairs call (drephip_allpairs_sparse*, screen.hip /
allpairs.hip SPARSE flavours): only the pairs that share a hash, as records
{i, j, common, denom}, without the condensed vector.  Checked field by field
against the C oracle's Mash merge (reference: `mash dist`,
drep/d_cluster.py:569-573) restricted to common > 0, on the direct path (the
screen and the LIST kernel append their pairs themselves) and on the fallback
(a temporary condensed segment, compacted), in row blocks and row segments,
at and past the buffer's capacity, and end to end through
cluster_mash_sparse / mdb_from_sparse against the condensed pipeline."""
import numpy as np
import pytest

import oracle
from drep_amd import _lib
from drep_amd import d_cluster

pytestmark = pytest.mark.gpu
UMAX = np.iinfo(np.uint64).max
ERR_NOMEM = -4


def planted_sketches(N, s, seed, fam=6, partial_every=7, lo_twins=40, hub=True):
    """tests/test_screen.py's generator: families of `fam` genomes draw from a
    shared pool, every partial_every-th genome is partial, `lo_twins` hashes
    are copied to another genome with only their high word changed (equal sort
    keys, no shared hash), and one hub value sits in a third of all genomes."""
    rng = np.random.default_rng(seed)
    H = np.full((N, s), UMAX, dtype=np.uint64)
    NH = np.zeros(N, dtype=np.uint32)
    hubv = np.uint64(rng.integers(1, UMAX, dtype=np.uint64))
    pools = {}
    for g in range(N):
        f = g // fam
        if f not in pools:
            pools[f] = rng.integers(1, UMAX, size=3 * s, dtype=np.uint64)     # the whole 64-bit range
        own = rng.integers(1, UMAX, size=s, dtype=np.uint64)
        take = rng.random(3 * s) < 0.3
        vals = np.unique(np.concatenate([pools[f][take], own] + ([np.array([hubv])] if hub and g % 3 == 0 else [])))
        n = s if g % partial_every else int(rng.integers(1, s))
        vals = vals[:n]
        H[g, :len(vals)] = vals
        NH[g] = len(vals)
    for _ in range(lo_twins):
        a, b = rng.integers(0, N, 2)
        if a == b or NH[a] == 0 or NH[b] == 0:
            continue
        v = H[a, rng.integers(0, NH[a])]
        twin = (v & np.uint64(0xFFFFFFFF)) | (np.uint64(rng.integers(1, 1 << 32)) << np.uint64(32))
        if twin in H[b, :NH[b]] or twin in H[a, :NH[a]]:
            continue
        row = np.sort(np.concatenate([H[b, :NH[b]], [twin]]))[:s]
        H[b, :] = UMAX
        H[b, :len(row)] = row
        NH[b] = len(row)
    return H, NH


def expected_list(H, NH, s):
    """(i, j, common, denom) of the oracle's pairs with common > 0, in (i, j) order."""
    N = len(NH)
    oc, od = oracle.allpairs(H, NH, s, threads=8)
    ii, jj = np.triu_indices(N, 1)
    k = oc > 0
    return ii[k].astype(np.uint32), jj[k].astype(np.uint32), oc[k], od[k]


_CASES = {}


def case(s, N):
    """The planted sketches of test_screen.py's shapes and seeds and their
    expected list, computed once and shared (read-only)."""
    if (s, N) not in _CASES:
        H, NH = planted_sketches(N, s, seed=s + N)
        exp = expected_list(H, NH, s)
        for a in (H, NH) + exp:
            a.setflags(write=False)
        _CASES[(s, N)] = (H, NH, exp)
    return _CASES[(s, N)]


def rows_of(exp, r0, r1):
    k = (exp[0] >= r0) & (exp[0] < r1)
    return tuple(a[k] for a in exp)


def assert_list(got, exp, what=""):
    names = ("i", "j", "common", "denom")
    for g, dt in zip(got, (np.uint32, np.uint32, np.uint16, np.uint16)):
        assert g.dtype == dt
    key = got[0].astype(np.uint64) << np.uint64(32) | got[1].astype(np.uint64)
    assert len(np.unique(key)) == len(key), "a pair is listed twice " + what
    assert (got[0] < got[1]).all()
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    for n, g, e in zip(names, got, exp):
        assert np.array_equal(g, e), (what, n)


DIRECT = [(64, 300), (1000, 200), (2048, 96)]


@pytest.mark.parametrize("s,N", DIRECT)
def test_sparse_direct_equals_oracle(s, N):
    H, NH, exp = case(s, N)
    assert len(exp[0]) > N                                  # (test_screen.py asserts the same of these inputs)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        got = ctx.allpairs_sparse(H, NH)
        st = ctx.sparse_stats()
        assert_list(got, exp)
        assert st["direct"] == len(exp[0]) and st["fallback"] == 0 and st["blocks"] >= 1 and st["scratch_bytes"] > 0
        sc = ctx.screen_stats()
        assert sc["used"] and sc["entries"] == int(NH.sum()) and sc["marked"] > 0
        ctx.set_timing(True)
        ctx.allpairs_sparse(H, NH)
        assert ctx.kernel_ms(2)[1] >= 1                     # the LIST kernel's launches are still timed


@pytest.mark.parametrize("s,N,how", [(64, 300, "off"), (1000, 200, "off"), (2048, 96, "off"), (4096, 80, "band"),
                                      (64, 300, "merge")])
def test_sparse_fallback_equals_oracle(s, N, how):
    H, NH, exp = case(s, N)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_OFF if how == "off" else ctx.SCREEN_ON)
        if how == "merge":
            ctx.set_allpairs_path(ctx.AP_MERGE)
        got = ctx.allpairs_sparse(H, NH)
        st = ctx.sparse_stats()
        assert_list(got, exp, how)
        assert st["fallback"] == len(exp[0]) and st["direct"] == 0


@pytest.mark.parametrize("s,N", [(1000, 200), (64, 300)])
@pytest.mark.parametrize("mode", ["direct", "fallback"])
def test_sparse_row_blocks(s, N, mode, monkeypatch):
    H, NH, exp = case(s, N)
    monkeypatch.setenv("DREPHIP_SPARSE_BLOCK_ROWS", "16")
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON if mode == "direct" else ctx.SCREEN_OFF)
        got = ctx.allpairs_sparse(H, NH)
        st = ctx.sparse_stats()
        assert_list(got, exp, mode)
        assert st["blocks"] >= 3 and st[mode] == len(exp[0]) and st["direct"] + st["fallback"] == len(exp[0])


@pytest.mark.parametrize("s,N", [(1000, 200), (64, 300)])
@pytest.mark.parametrize("mode", ["direct", "fallback"])
def test_sparse_row_segments(s, N, mode):
    """Cuts that are no multiple of the row tile: a pair of a straddled tile
    still appears exactly once overall."""
    H, NH, exp = case(s, N)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON if mode == "direct" else ctx.SCREEN_OFF)
        parts = []
        for r0, r1 in ((0, 37), (37, 121), (121, N)):
            got = ctx.allpairs_sparse(H, NH, r0, r1)
            assert_list(got, rows_of(exp, r0, r1), "%s rows [%d, %d)" % (mode, r0, r1))
            parts.append(got)
        assert_list(tuple(np.concatenate([p[k] for p in parts]) for k in range(4)), exp, mode)


@pytest.mark.parametrize("mode", ["direct", "fallback"])
def test_sparse_overflow(mode):
    import torch
    s, N = 1000, 200
    H, NH, exp = case(s, N)
    needed = len(exp[0])
    SENT = np.uint32(0xDEADBEEF).view(np.int32).item()
    dh = torch.from_numpy(H.view(np.int64).copy()).cuda()
    dn = torch.from_numpy(NH.view(np.int32).copy()).cuda()
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON if mode == "direct" else ctx.SCREEN_OFF)
        cap = needed - 1
        buf = torch.full((cap + 64, 4), SENT, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        rc, n = ctx.allpairs_sparse_device(dh.data_ptr(), dn.data_ptr(), N, 0, N, buf.data_ptr(), cap, st)
        torch.cuda.synchronize()
        assert rc == ERR_NOMEM and n == needed
        out = buf.cpu().numpy().view(np.uint32)
        assert (out[cap:] == np.uint32(0xDEADBEEF)).all()                 # the 64 guard records
        assert (out[:cap] != np.uint32(0xDEADBEEF)).any(axis=1).all()      # every slot below cap was stored
        # the stored records are distinct pairs of the expected list
        want = {(int(a), int(b)): (int(c), int(d)) for a, b, c, d in zip(*exp)}
        seen = set()
        for a, b, c, d in out[:cap]:
            assert want[(int(a), int(b))] == (int(c), int(d)) and (int(a), int(b)) not in seen
            seen.add((int(a), int(b)))
        # cap = 0 only counts
        rc, n = ctx.allpairs_sparse_device(dh.data_ptr(), dn.data_ptr(), N, 0, N, None, 0, st)
        assert rc == ERR_NOMEM and n == needed
        rc, n = ctx.allpairs_sparse_raw(H, NH, 0, N, None)
        assert rc == ERR_NOMEM and n == needed
        # exactly enough room
        buf2 = torch.full((needed + 64, 4), SENT, dtype=torch.int32, device="cuda")
        rc, n = ctx.allpairs_sparse_device(dh.data_ptr(), dn.data_ptr(), N, 0, N, buf2.data_ptr(), needed, st)
        torch.cuda.synchronize()
        assert rc == 0 and n == needed
        assert (buf2.cpu().numpy().view(np.uint32)[needed:] == np.uint32(0xDEADBEEF)).all()
        # the wrapper's retry: too small a first buffer, then the reported size
        assert_list(ctx.allpairs_sparse(H, NH, cap=needed - 1), exp, mode)
        assert_list(ctx.allpairs_sparse(H, NH, cap=0), exp, mode)


@pytest.mark.parametrize("mode", ["direct", "fallback"])
def test_sparse_nothing_shared_and_all_shared(mode):
    s, N = 200, 150
    rng = np.random.default_rng(11)
    H = np.sort(rng.permutation(np.arange(1, N * s + 1, dtype=np.uint64) * np.uint64(7919)).reshape(N, s), axis=1)
    NH = np.full(N, s, dtype=np.uint32)
    NH[::5] = 37
    H[::5, 37:] = UMAX
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON if mode == "direct" else ctx.SCREEN_OFF)
        rc, n = ctx.allpairs_sparse_raw(H, NH, 0, N, None)
        assert rc == 0 and n == 0
        got = ctx.allpairs_sparse(H, NH)
        assert all(len(g) == 0 for g in got)
        # every genome identical: all N (N - 1) / 2 pairs, common == s
        same = np.tile(np.sort(rng.integers(1, 1 << 60, size=s, dtype=np.uint64)), (N, 1))
        got = ctx.allpairs_sparse(same, np.full(N, s, np.uint32))
        ii, jj = np.triu_indices(N, 1)
        full = np.full(len(ii), s, np.uint16)
        assert_list(got, (ii.astype(np.uint32), jj.astype(np.uint32), full, full), mode)
        assert ctx.sparse_stats()[mode] == N * (N - 1) // 2


def test_sparse_single_shared_hash_pairs():
    """test_screen.py's construction: pairs of otherwise unrelated genomes
    sharing exactly one hash at known positions, on both sides of i + j = s --
    listed with common 1 or absent, by the rank-sum rule; pairs sharing two, or
    with a partial sketch, go to the kernel."""
    s, N = 256, 400
    rng = np.random.default_rng(21)
    H = np.sort(rng.integers(1, 1 << 62, size=(N, s), dtype=np.uint64), axis=1)
    NH = np.full(N, s, dtype=np.uint32)
    for g in range(0, N, 9):
        NH[g] = rng.integers(s // 3, s)
        H[g, NH[g]:] = UMAX
    for _ in range(600):
        a, b = sorted(rng.choice(N, 2, replace=False))
        for _k in range(1 if rng.random() < 0.8 else 2):
            i, j = int(rng.integers(0, NH[a])), int(rng.integers(0, NH[b]))
            v = H[a, i]
            if v in H[b, :NH[b]]:
                continue
            row = np.sort(np.concatenate([np.delete(H[b, :NH[b]], j), [v]]))
            H[b, :NH[b]] = row
    exp = expected_list(H, NH, s)
    oc, _ = oracle.allpairs(H, NH, s, threads=8)
    assert (exp[2] == 1).sum() > 100 and len(exp[0]) < (oc >= 0).sum() - 1000
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        got = ctx.allpairs_sparse(H, NH)
        assert_list(got, exp)
        assert ctx.screen_stats()["simple"] > 100 and ctx.sparse_stats()["fallback"] == 0
        ctx.set_allpairs_screen(ctx.SCREEN_OFF)
        assert_list(ctx.allpairs_sparse(H, NH), exp, "fallback")


@pytest.mark.parametrize("mode", ["direct", "fallback"])
def test_sparse_small_and_empty(mode):
    s = 64
    rng = np.random.default_rng(5)
    row = np.sort(rng.integers(1, 1 << 60, size=s, dtype=np.uint64))
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON if mode == "direct" else ctx.SCREEN_OFF)
        got = ctx.allpairs_sparse(row[None, :], np.array([s], np.uint32))                    # N = 1
        assert all(len(g) == 0 for g in got)
        H2 = np.stack([row, row])                                                           # N = 2, identical
        got = ctx.allpairs_sparse(H2, np.array([s, s], np.uint32))
        assert [g.tolist() for g in got] == [[0], [1], [s], [s]]
        other = np.sort(rng.integers(1, 1 << 60, size=s, dtype=np.uint64))                  # N = 2, unrelated
        got = ctx.allpairs_sparse(np.stack([row, other]), np.array([s, s], np.uint32))
        assert all(len(g) == 0 for g in got)
        # a genome with no hash at all among related ones
        H, NH = planted_sketches(40, s, seed=77)
        H, NH = H.copy(), NH.copy()
        for g in (0, 17, 39):
            H[g, :] = UMAX
            NH[g] = 0
        exp = expected_list(H, NH, s)
        assert len(exp[0]) > 40 and not np.isin(exp[0], (0, 17, 39)).any()
        assert_list(ctx.allpairs_sparse(H, NH), exp, mode)


def test_sparse_light_cells(monkeypatch):
    """DREPHIP_SCREEN_LIGHT=1 (off by default on the whole-row path): cells
    marked by one run of >= 3 entries are appended by k_screen_light itself,
    on tests/test_screen.py's light-cell construction (families of 8 sharing
    30 values; chance values between members of two families, at ranks on both
    sides of i + j = s; hubs; pairs linked twice; partial sketches; low-word
    twins).  Same list, fewer cells left to the LIST kernel, in one block, in
    row blocks and in row segments."""
    s, N, F = 300, 400, 8
    rng = np.random.default_rng(s + N)
    H = np.sort(rng.integers(1, 1 << 62, size=(N, s), dtype=np.uint64), axis=1)
    NH = np.full(N, s, dtype=np.uint32)
    for g in range(5, N, 29):
        NH[g] = rng.integers(s // 3, s)
        H[g, NH[g]:] = UMAX

    def plant(members, v):
        for g in members:
            if v in H[g, :NH[g]]:
                continue
            j = int(rng.integers(0, NH[g]))
            H[g, :NH[g]] = np.sort(np.concatenate([np.delete(H[g, :NH[g]], j), [v]]))

    def fam(f):
        return np.arange(f * F, min(N, f * F + F))
    nf = N // F
    for f in range(nf):
        for _ in range(30):
            plant(fam(f), np.uint64(rng.integers(1, 1 << 62)))
    pairs = rng.permutation([(a, b) for a in range(nf) for b in range(a + 1, nf)])
    for a, b in pairs[:60]:
        ma = rng.choice(fam(a), int(rng.integers(1, F + 1)), replace=False)
        mb = rng.choice(fam(b), int(rng.integers(2, F + 1)), replace=False)
        plant(np.concatenate([ma, mb]), np.uint64(rng.integers(1, 1 << 62)))
    for a, b in pairs[60:70]:
        for _ in range(2):
            plant(np.concatenate([fam(a)[:3], fam(b)[:3]]), np.uint64(rng.integers(1, 1 << 62)))
    for a, b in pairs[:8]:
        plant([fam(a)[0], fam(b)[-1]], np.uint64(rng.integers(1, 1 << 62)))
    for _ in range(3):
        plant(rng.choice(N, 70, replace=False), np.uint64(rng.integers(1, 1 << 62)))
    for _ in range(30):
        a, b = rng.choice(N, 2, replace=False)
        v = H[a, rng.integers(0, NH[a])]
        plant([b], (v & np.uint64(0xFFFFFFFF)) | (np.uint64(rng.integers(1, 1 << 30)) << np.uint64(32)))
    exp = expected_list(H, NH, s)
    assert (exp[2] == 1).sum() > 500
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        assert_list(ctx.allpairs_sparse(H, NH), exp, "no light cells")
        st0 = ctx.screen_stats()
        monkeypatch.setenv("DREPHIP_SCREEN_LIGHT", "1")
        assert_list(ctx.allpairs_sparse(H, NH), exp, "light cells")
        st1 = ctx.screen_stats()
        assert ctx.sparse_stats()["direct"] == len(exp[0])
        assert st1["simple"] > st0["simple"] + 500 and st1["marked"] < st0["marked"] - 200, (st0, st1)
        parts = [ctx.allpairs_sparse(H, NH, r0, r1) for r0, r1 in ((0, 133), (133, 271), (271, N))]
        assert_list(tuple(np.concatenate([p[k] for p in parts]) for k in range(4)), exp, "light cells, row segments")
        monkeypatch.setenv("DREPHIP_SPARSE_BLOCK_ROWS", "48")
        assert_list(ctx.allpairs_sparse(H, NH), exp, "light cells, row blocks")
        assert ctx.sparse_stats()["blocks"] >= 3


@pytest.fixture(scope="module")
def family600():
    """Synthetic genome families (the bench's generator), N = 600, s = 1000:
    the sparse list and the condensed counts of the same sketches, both from
    the GPU through Context."""
    N, s = 600, 1000
    h, nh = oracle.sketch_synth(0, N, 60_000, seed=13, family_size=20, s=s, threads=8)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        i, j, c, d = ctx.allpairs_sparse(h, nh)
        assert ctx.sparse_stats()["direct"] == len(i) > N
        cc, cd = ctx.allpairs(h, nh, want_denom=True)
    ii, jj = np.triu_indices(N, 1)
    k = cc > 0
    assert_list((i, j, c, d), (ii[k].astype(np.uint32), jj[k].astype(np.uint32), cc[k], cd[k]))
    names = ["g%04d.fa" % ((x * 7) % N) for x in range(N)]                # not in sorted order
    ln = np.full(N, 60_000, np.uint64)
    return (d_cluster.SparseMash(names, names, i, j, c, d, nh, ln, s),
            d_cluster.CondensedMash(names, names, cc, cd, nh, ln, s))


@pytest.mark.parametrize("alg", ["single", "average"])
def test_sparse_cluster_end_to_end(family600, alg):
    sm, cm = family600
    Cdb, ret = d_cluster.cluster_mash_condensed(cm, clusterAlg=alg, P_ani=0.9)
    Cdb2, ret2 = d_cluster.cluster_mash_sparse(sm, clusterAlg=alg, P_ani=0.9)
    assert np.array_equal(ret2[0], ret[0]) and ret2[0].tobytes() == ret[0].tobytes()
    assert Cdb2.equals(Cdb)
    assert ret2[2] == ret[2]
    assert 1 < Cdb["primary_cluster"].nunique() < len(sm.names)


def test_sparse_mdb_end_to_end(family600):
    sm, cm = family600
    dense = d_cluster.mdb_from_condensed(cm.names, cm.common, cm.denom, cm.nhash, cm.s)
    want = dense[dense["dist"] < 1]
    got = d_cluster.mdb_from_sparse(sm)
    assert got.equals(want)
    for c in ("dist", "similarity"):
        assert np.array_equal(got[c].to_numpy().view(np.uint32), want[c].to_numpy().view(np.uint32))
