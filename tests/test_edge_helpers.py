"""CPU checks of tests/edge_cases.py: the set-based all-pairs reference
equals the oracle's merge on every generator, the generators produce the
conditions the GPU tests rely on, the plain-Python sketch reference equals
the oracle's sketch on the boundary layouts, and the wide screen sets put marks
inside and outside the marking window and hold the colliding runs they
promise."""
import numpy as np
import pytest

import oracle
import edge_cases as ec

UMAX = ec.UMAX


@pytest.mark.parametrize("s,N", [(64, 60), (100, 48), (1000, 48), (1025, 24), (2048, 24)])
def test_ref_allpairs_equals_oracle_on_geometry_sketches(s, N):
    H, NH = ec.geometry_sketches(N, s, seed=s + N)
    rc, rd = ec.ref_allpairs(H, NH, s)
    oc, od = oracle.allpairs(H, NH, s)
    assert np.array_equal(rc, oc) and np.array_equal(rd, od)
    assert (oc > 0).mean() > 0.5


@pytest.mark.parametrize("how", ["reversed", "random"])
def test_permuted_condensed_equals_reference_of_the_permuted_set(how):
    """The counts of a row permutation cut out of the original condensed
    arrays equal ref_allpairs of the permuted set (the counts are not uniform:
    a permutation that moved nothing, or the wrong way, would show)."""
    s, N = 64, 45
    H, NH = ec.geometry_sketches(N, s, seed=31)
    rc, rd = ec.ref_allpairs(H, NH, s)
    perm = np.arange(N)[::-1] if how == "reversed" else np.random.default_rng(5).permutation(N)
    pc, pd = ec.permuted_condensed(rc, rd, N, perm)
    ec_, ed_ = ec.ref_allpairs(H[perm], NH[perm], s)
    assert pc.dtype == np.uint16 and pd.dtype == np.uint16
    assert np.array_equal(pc, ec_) and np.array_equal(pd, ed_)
    assert not np.array_equal(pc, rc) and not np.array_equal(pd, rd)
    ic, id_ = ec.permuted_condensed(rc, rd, N, np.arange(N))
    assert np.array_equal(ic, rc) and np.array_equal(id_, rd)


def test_ref_pair_tiny_sets():
    """The reference on sets small enough to check by eye."""
    u = lambda *v: np.array(v, dtype=np.uint64)
    assert ec.ref_pair(u(1, 2, 3), u(2, 3, 4), 3) == (2, 3)        # union 1 2 3 4: the 3 smallest hold 2 and 3
    assert ec.ref_pair(u(1, 2, 3), u(2, 3, 4), 2) == (1, 2)
    assert ec.ref_pair(u(0, 5), u(0, int(UMAX) - 1), 4) == (1, 3)
    assert ec.ref_pair(u(), u(7), 4) == (0, 1)
    assert ec.ref_pair(u(), u(), 4) == (0, 0)
    for a, b, s in ((u(1, 2, 3), u(2, 3, 4), 3), (u(0, 5), u(0, int(UMAX) - 1), 4), (u(), u(7), 4)):
        assert ec.ref_pair(a, b, s) == oracle.dist_pair(a, b, s)


def test_geometry_sketches_conditions():
    s, N = 1000, 48
    H, NH = ec.geometry_sketches(N, s, seed=7)
    for g in range(N):
        row = H[g, :NH[g]]
        assert (np.diff(row.astype(object)) > 0).all() and (H[g, NH[g]:] == UMAX).all()
    st = ec.shared_hash_stats(H, NH, s)
    assert st["rank_s_minus_1"] >= 20, st
    assert st["rank_s"] >= 20, st
    assert st["late_counted"] >= 50, st
    assert st["denom_below_s"] > 0, st
    zero_rows = [g for g in range(N) if NH[g] and H[g, 0] == 0]
    assert len(zero_rows) >= 10
    # row tiles (4 consecutive genomes) with and without the key 0, full rows among the zero rows
    assert any(NH[g] == s for g in zero_rows) and any(all(g not in zero_rows for g in range(t, t + 4))
                                                     for t in range(0, N, 4))
    assert sum(1 for g in range(N) if NH[g] == s and H[g, s - 1] == UMAX - 1) >= 2
    assert ((NH > 0) & (NH < s)).sum() >= 2 and (NH == 0).sum() >= 1
    # low-word twins: across genomes everywhere, inside one genome only where planned
    lo = lambda r: (r & np.uint64(0xFFFFFFFF))
    allv = np.unique(H[H != UMAX])
    assert len(allv) - len(np.unique(lo(allv))) >= s // 32       # (a twin nobody drew is not in the set)
    inrow = [g for g in range(N) if len(np.unique(lo(H[g, :NH[g]]))) < NH[g]]
    assert inrow and all(g % 16 == 7 for g in inrow)


@pytest.mark.parametrize("s", [64, 100, 600, 1000, 1025, 2048])
def test_planted_rank_pairs_placement_and_counts(s):
    pp = ec.planted_rank_pairs(s, seed=s)
    P = len(pp["i"])
    exp = ec.rank_pair_expected(pp)
    js = {j for k in range(1, s // 64 + 2) for j in (64 * k - 1, 64 * k, 64 * k + 1) if 0 < j < s}
    assert set(pp["j"].tolist()) == js
    kinds = set()
    for p in range(P):
        A, B, i, j, m, v = pp["A"][p], pp["B"][p], int(pp["i"][p]), int(pp["j"][p]), int(pp["m"][p]), pp["v"][p]
        assert A[i] == v and B[j] == v
        inter, ia, ib = np.intersect1d(A, B, return_indices=True)
        assert len(inter) == m + 1 and ia[:m].tolist() == list(range(m)) and ib[:m].tolist() == list(range(m))
        assert i - (s - j + m) in (-2, -1, 0)
        assert exp[p] == m + (i <= s - 1 - j + m)
        assert ec.ref_pair(A, B, s) == (exp[p], s) == oracle.dist_pair(A, B, s)
        if pp["zero"][p]:                        # the key 0 on A's side only, no match before the probe
            assert A[0] == 0 and B[0] != 0 and m == 0 and not pp["swap"][p]
        else:
            assert A[0] != 0 and B[0] != 0
        t = int(pp["twin"][p])
        if t:
            assert A[i + t] >> np.uint64(32) == v >> np.uint64(32) and A[i + t] != v
        kinds.add((i - (s - j + m), m, bool(pp["swap"][p]), t))
    # every variant with every m, both orders; twins on both sides (s = 64 has the one position j = 63,
    # where rank s - 2 would need i = m - 1, below the m early hashes)
    for d in (-2, -1, 0) if s > 64 else (-1, 0):
        for m in ec.RANK_M:
            assert (d, m, False) in {k[:3] for k in kinds} and (d, m, True) in {k[:3] for k in kinds}
    assert {k[3] for k in kinds} == ({-1, 0, 1} if s > 64 else {k[3] for k in kinds})
    assert set(pp["j"][pp["zero"]].tolist()) == js          # the zero-key block sweeps every position too
    # pairs of different planted pairs share nothing: the matrices' other pairs are all (0, s)
    n = 0
    for H, NH, p0, p1 in ec.rank_pair_matrices(pp, max_pairs=12):
        rc, rd = ec.ref_allpairs(H, NH, s)
        oc, od = oracle.allpairs(H, NH, s)
        assert np.array_equal(rc, oc) and np.array_equal(rd, od)
        N = len(NH)
        idx = ec.cond_index(2 * np.arange(p1 - p0), 2 * np.arange(p1 - p0) + 1, N)
        assert np.array_equal(oc[idx], exp[p0:p1]) and (np.delete(oc, idx) == 0).all() and (od == s).all()
        n += 1
        if n == 3:
            break


def test_planted_rank_pairs_cycled_m():
    pp = ec.planted_rank_pairs(1000, seed=3, cross_m=False)
    full = ec.planted_rank_pairs(1000, seed=3)
    assert 3 * (~pp["zero"]).sum() <= (~full["zero"]).sum() + 6 and set(pp["m"].tolist()) == set(ec.RANK_M)
    assert set(pp["j"].tolist()) == set(full["j"].tolist())
    assert pp["zero"].sum() == full["zero"].sum() > 0


def _rows_ascending(H, NH):
    n = NH.astype(np.int64)[:, None]
    k = np.arange(H.shape[1])[None, :]
    inside = k < n
    assert (H[~inside] == UMAX).all() and (H[inside] != UMAX).all()
    assert ((H[:, 1:] > H[:, :-1]) | ~inside[:, 1:]).all()


@pytest.mark.parametrize("R", [8, 4])
def test_wide_screen_sets_categories(R):
    """The wide sets put marks where tests/test_screen_wide.py needs them, by
    an emulation of the screen's grouping and marking (ec.mark_emulation)."""
    s = 16
    sets = ec.wide_screen_sets(R, seed=7)
    N = ec.wide_n(R)
    assert N % 32 and N > ec.MARK_TILES * R + ec.MARK_COLS + 32
    for name, (H, NH, info) in sets.items():
        assert H.shape == (N, s)
        _rows_ascending(H, NH)
        st = ec.mark_emulation(H, NH, s, R)
        if name[0] == "A":
            assert st["chunks"] == 1 and 3 <= st["runs3"] < ec.MARK_CHUNK, (name, st)
            assert info["g_lo"] % 32 == int(name[1:])
            # every combination of in / out by tile and by column, on the very edges
            for k in ("in_in", "in_out", "out_in", "out_out", "edge_tile_127", "edge_tile_128", "edge_col_2047",
                      "edge_col_2048", "direct_once_same"):
                assert st[k] >= 1, (name, k, st)
            assert (st["direct_twice"] >= 6 and st["window_twice"] >= 1) or name == "A0", (name, st)
            t_in = info["g_lo"] // R + ec.MARK_TILES - 1
            c_lo = info["g_lo"] & ~31
            want = {(t, c) for t in (t_in, t_in + 1) for c in (c_lo + ec.MARK_COLS - 1, c_lo + ec.MARK_COLS, N - 1)}
            assert want <= {(r // R, c) for r, c in info["edges"]}
            assert {r % R for r, _ in info["edges"]} == {0, R - 1}
        if name == "B":
            assert st["chunks"] == 3 and 690 <= st["runs3"] <= 710, st
            for k in ("in_in", "in_out", "out_in", "out_out", "direct_once_same", "direct_twice", "window_twice",
                      "window_and_direct", "window_overhang", "two_on_long_cell", "two_on_long_pair", "rank_below_s",
                      "rank_from_s"):
                assert st[k] >= 1, (name, k, st)
            assert (NH[::11] < s).all() and (np.delete(NH, np.arange(0, N, 11)) == s).all()
        if name == "C":
            for k in ("in_in", "in_out", "out_in", "out_out", "equal_fp_mixed", "equal_fp_mixed_long", "slow_long",
                      "diagonal", "dup_second_shared", "light_other_hash_low_rank", "rank_below_s", "rank_from_s"):
                assert st[k] >= 1, (name, k, st)
            for kind in ("slow", "equal"):
                assert {(p, kind) for p in (0, 63, 64, 127, 128, 199, 699)} <= st["twin_at"], st["twin_at"]
    # the same categories of set C with R = 4 rows per tile at s = 64
    H, NH, _ = ec.wide_set_c(4, 9, s=64)
    _rows_ascending(H, NH)
    st = ec.mark_emulation(H, NH, 64, 4)
    for k in ("equal_fp_mixed_long", "slow_long", "diagonal", "dup_second_shared", "light_other_hash_low_rank"):
        assert st[k] >= 1, (k, st)


_WIDE_REF = [("A0", None), ("A1", None), ("A31", None), ("B", None), ("C", ec.WIDE_HUBS[:-1])]


@pytest.mark.parametrize("name,hubs", _WIDE_REF, ids=[n for n, _ in _WIDE_REF])
def test_ref_allpairs_equals_oracle_on_wide_sets(name, hubs):
    """The oracle, the GPU tests' reference on the wide sets, against the
    set-based reference (set C without its 700-genome hubs: ref_allpairs
    walks every sharing pair in Python)."""
    s, R = 16, 8
    H, NH, _ = ec.wide_set_c(R, 207, s, hubs) if hubs else ec.wide_screen_sets(R, 7)[name]
    oc, od = oracle.allpairs(H, NH, s, threads=8)
    assert (oc > 0).sum() < 200_000
    rc, rd = ec.ref_allpairs(H, NH, s)
    assert np.array_equal(rc, oc) and np.array_equal(rd, od)


def test_short_row_sets_and_incidence_reference():
    """The no-fingerprint case's rows: at most 16 hashes, N s > 2^28 (fewer
    than FP_BITS fingerprint bits), more than 8192 genomes; its reference
    (counts from the incidence matrix) equals the oracle at s = 64, where no
    union of two rows reaches s either."""
    H, NH = ec.short_row_sets(seed=3)
    N = len(NH)
    assert N == ec.SHORT_N > 8192 and N * ec.SHORT_S > 1 << 28 and 32 - ec.entry_bits(N, ec.SHORT_S) < ec.FP_BITS
    assert N * ec.SHORT_S < 1 << 32 and 1 <= NH.min() and NH.max() <= ec.SHORT_MAX and 2 * ec.SHORT_MAX < 64
    _rows_ascending(H, NH)
    H64 = np.full((N, 64), UMAX, dtype=np.uint64)
    H64[:, :ec.SHORT_MAX] = H
    c, d, i, j = ec.incidence_allpairs(H, NH)
    oc, od = oracle.allpairs(H64, NH, 64, threads=8)
    assert np.array_equal(c, oc) and np.array_equal(d, od)
    assert np.array_equal(ec.cond_index(i.astype(np.int64), j.astype(np.int64), N), np.flatnonzero(c))
    # hubs reach the last genome and the columns past 8192; runs longer than a wave whose hashes differ
    assert j.max() == N - 1 and (j > 8192).sum() >= 5 and c.max() >= 2
    st = ec.mark_emulation(H, NH, ec.SHORT_S, 4)
    assert st["slow_long"] == 2 and st["equal_fp_mixed"] == 0 and st["runs3"] >= 300, st
    vals = np.sort(H[H != UMAX])
    lo = vals & np.uint64(0xFFFFFFFF)
    order = np.lexsort((vals, lo))
    twins = (lo[order][1:] == lo[order][:-1]) & (vals[order][1:] != vals[order][:-1])
    # low-word twins that agree in the 3 fingerprint bits the entry values still hold: only the hash read tells them apart
    fp = (vals[order] >> np.uint64(32)) & np.uint64(7)
    assert twins.sum() >= 50 and (twins & (fp[1:] == fp[:-1])).sum() >= 1


def test_boundary_genomes_layout_and_reference():
    genomes, sites = ec.boundary_genomes(seed=5)
    assert len(genomes) == 64
    starts, ends = set(), set()
    multi = 0
    for recs, plan in zip(genomes, sites):
        # absolute position of every base: records lie one separator apart
        span = sum(len(r) for r in recs) + len(recs) - 1
        ok = np.zeros(span + 1, dtype=bool)
        p = 0
        for r in recs:
            ok[p:p + len(r)] = np.isin(r, np.frombuffer(b"ACGT", np.uint8))
            p += len(r) + 1
        multi += len(recs) > 1
        assert 2 * ec.TILE <= ((span + 1 + ec.TILE - 1) // ec.TILE) * ec.TILE <= 3 * ec.TILE
        for q, kind in plan:
            if kind == "start":
                assert ok[q] and not ok[q - 1] and ok[q - 2]
                starts.add(q)
            else:
                assert ok[q] and not ok[q + 1] and ok[q + 2]
                ends.add(q)
        sk, nk = ec.ref_sketch(recs, 1000)
        assert 0 < nk <= 900
        seq, rec_off, _ = ec.flatten([recs])
        assert np.array_equal(sk, oracle.sketch_records(seq, rec_off, 21, 1000, 42))
    assert multi == 32
    for d in range(-24, 25):
        assert ec.TILE + d in starts and 2 * ec.TILE + d in ends
    for d in range(64):
        assert ec.LANE_SITES[0] + d in starts and ec.LANE_SITES[1] + d in ends


def test_genome_end_genomes_and_pack_layout():
    genomes = ec.genome_end_genomes(seed=6)
    spans = [sum(len(r) for r in g) for g in genomes]
    assert spans[0::2] == list(ec.END_SPANS) + [ec.TILE - 1] and set(spans[1::2]) == {500}
    codes, valid, off, pad, nk = ec.pack_layout(genomes, seed=1)
    assert off[0] == ec.TILE and (off % ec.TILE == 0).all() and (pad % ec.TILE == 0).all()
    assert np.array_equal(off[1:], off[:-1] + pad[:-1]) and len(codes) * 16 == len(valid) * 32 == off[-1] + pad[-1]
    assert pad[0] == ec.TILE and pad[2] == ec.TILE and pad[4] == 2 * ec.TILE
    assert nk.tolist() == [80] * len(genomes)
    # the packed words give the sequence back where valid, and valid marks exactly the A/C/G/T bases
    bits = np.unpackbits(valid.view(np.uint8), bitorder="little").astype(bool)
    assert bits.sum() == 100 * len(genomes) and not bits[:ec.TILE].any()
    for g, o in zip(genomes, off):
        r = g[0]
        o = int(o)
        ok = np.isin(r, np.frombuffer(b"ACGT", np.uint8))
        assert np.array_equal(bits[o:o + len(r)], ok) and not bits[o + len(r):o + len(r) + 1].any()
        pos = o + np.flatnonzero(ok)
        c = (codes[pos // 16] >> (2 * (pos % 16)).astype(np.uint32)) & 3
        assert np.array_equal(np.frombuffer(b"ACGT", np.uint8)[c], r[ok])
    # junk under the invalid bits: some invalid position carries each of the four codes
    inv = np.flatnonzero(~bits)[:4096]
    assert set(((codes[inv // 16] >> (2 * (inv % 16)).astype(np.uint32)) & 3).tolist()) == {0, 1, 2, 3}
