"""Generators and references of tests/test_edges.py (GPU) and
tests/test_edge_helpers.py (CPU): a set-based all-pairs reference that shares
no code with the oracle's merge loop, sketch sets built so that the all-pairs
kernels' data-dependent paths are taken (the hash values 0 and UMAX - 1, shared
hashes on both sides of union rank s at every column chunk boundary, shared
hashes late in one sketch and early in the other), sequence layouts that
put a k-mer on every boundary of the sketch kernel's packed layout, and (for
tests/test_screen_wide.py) sketch sets wider than one marking window of the
shared-hash screen, with long and colliding runs of equal sort keys."""
import numpy as np

import oracle

UMAX = np.iinfo(np.uint64).max
HMAX = np.uint64(UMAX - 1)              # the largest hash a sketch can hold (UMAX is the empty slot)
K = 21
TILE = 32768                            # drephip_tile_bases(): asserted by the GPU tests
_U = np.uint64


# ---------------------------------------------------------------- all-pairs reference
def ref_pair(A, B, s):
    """Mash's count of one pair from its definition: denom = min(s, |A u B|),
    common = the shared hashes among the denom smallest of A u B."""
    union = np.union1d(A, B)
    denom = min(s, len(union))
    inter = np.intersect1d(A, B)
    return int(np.isin(inter, union[:denom]).sum()), denom


def ref_allpairs(H, NH, s):
    """(common, denom) of every pair i < j, condensed row-major, uint16.  A
    pair that shares no hash (found from the incidence matrix of the distinct
    values, not by walking the sketches) has common 0 and |A u B| = |A| + |B|;
    every other pair goes through ref_pair."""
    import scipy.sparse as sp
    H = np.asarray(H, dtype=np.uint64)
    NH = np.asarray(NH, dtype=np.int64)
    N = len(NH)
    rows = [H[g, :NH[g]] for g in range(N)]
    for r in rows:
        assert len(np.unique(r)) == len(r) and (r != UMAX).all()
    ii, jj = np.triu_indices(N, 1)
    common = np.zeros(len(ii), dtype=np.uint16)
    denom = np.minimum(s, NH[ii] + NH[jj]).astype(np.uint16)
    if NH.sum() == 0:
        return common, denom
    _, inv = np.unique(np.concatenate(rows), return_inverse=True)
    owner = np.repeat(np.arange(N), NH)
    M = sp.csr_matrix((np.ones(len(inv), np.int32), (owner, inv)), shape=(N, int(inv.max()) + 1))
    S = sp.triu(M @ M.T, 1).tocoo()
    for i, j in zip(S.row, S.col):
        c, d = ref_pair(rows[i], rows[j], s)
        t = i * N - i * (i + 1) // 2 + (j - i - 1)
        common[t], denom[t] = c, d
    return common, denom


def nonzero_pairs(common, denom, N):
    """(i, j, common, denom) of the condensed pairs with common > 0, in (i, j) order."""
    ii, jj = np.triu_indices(N, 1)
    k = common > 0
    return ii[k].astype(np.uint32), jj[k].astype(np.uint32), common[k], denom[k]


def shared_hash_stats(H, NH, s):
    """Where the shared hashes of a sketch set sit: pairs with a shared hash
    at union rank exactly s - 1 (the last one counted) and exactly s (the first
    one not counted), pairs with a counted shared hash at a row or column
    position above 0.7 s, pairs with a denominator below s."""
    N = len(NH)
    st = {"rank_s_minus_1": 0, "rank_s": 0, "late_counted": 0, "denom_below_s": 0}
    for a in range(N):
        A = H[a, :NH[a]]
        for b in range(a + 1, N):
            B = H[b, :NH[b]]
            _, ia, ib = np.intersect1d(A, B, assume_unique=True, return_indices=True)
            rank = ia + ib - np.arange(len(ia))            # position in A u B: i + j - (shared hashes below)
            st["rank_s_minus_1"] += bool((rank == s - 1).any())
            st["rank_s"] += bool((rank == s).any())
            st["late_counted"] += bool(((rank < s) & (np.maximum(ia, ib) > 0.7 * s)).any())
            st["denom_below_s"] += int(NH[a]) + int(NH[b]) - len(ia) < s
    return st


# ---------------------------------------------------------------- sketch sets
def _profile(kind, x):
    """Density of a genome over the universe's rank order x in [0, 1)."""
    if kind == 0:
        return np.ones_like(x)                                     # uniform
    if kind == 1:
        return np.exp(-5.0 * x)                                    # front-heavy
    if kind == 2:
        return np.exp(-5.0 * (1.0 - x))                            # back-heavy
    if kind == 3:
        return np.exp(-0.5 * ((x - 0.5) / 0.12) ** 2) + 0.02       # middle-heavy
    if kind == 4:
        return x + 0.02                                            # rising
    return 1.0 - x + 0.02                                          # falling


def geometry_sketches(N, s, seed):
    """N sketches drawn from one sorted universe of ~3 s values, genome g with
    density profile g % 6 (uniform, front-, back-, middle-heavy, rising,
    falling), so a hash shared by two genomes sits late in one and early in
    the other and the union rank s falls anywhere in either sketch.

    - The universe holds s // 16 low-word twins (equal low 32 bits, different
      high words).  A genome holds at most one member of a twin pair -- the
      lower one in even genomes, the upper one in odd ones -- except genomes
      with g % 16 == 7, which hold both members of the first twin pairs (two
      keys with one low word in one row table).
    - A third of the genomes hold the value 0, in blocks of four consecutive
      genomes ((g // 4) % 3 == 0), so that row tiles with and without the key
      0 both occur at every tile height; every 4th genome holds UMAX - 1,
      which is then a full genome's last element.
    - Genomes with g % 7 == 5 are partial (1 .. s - 1 hashes), those with
      g % 17 == 11 are empty."""
    rng = np.random.default_rng(seed)
    ntw = s // 16
    base = np.unique(rng.integers(1, UMAX - 1, size=3 * s, dtype=np.uint64))
    tw_lo = rng.choice(base, size=ntw, replace=False)
    tw_hi = (tw_lo & _U(0xFFFFFFFF)) | (rng.integers(1, 1 << 32, size=ntw, dtype=np.uint64) << _U(32))
    keep = ~np.isin(tw_hi, base) & (tw_hi != tw_lo) & (tw_hi < HMAX)
    tw_lo, tw_hi = tw_lo[keep], tw_hi[keep]
    uni = np.unique(np.concatenate([base, tw_hi]))
    assert len(uni) == len(base) + len(tw_hi)
    x = np.arange(len(uni)) / len(uni)
    is_lo, is_hi = np.isin(uni, tw_lo), np.isin(uni, tw_hi)
    H = np.full((N, s), UMAX, dtype=np.uint64)
    NH = np.zeros(N, dtype=np.uint32)
    for g in range(N):
        if g % 17 == 11:
            continue
        n = int(rng.integers(1, s)) if g % 7 == 5 else s
        forced = []
        if (g // 4) % 3 == 0:
            forced.append(_U(0))
        if g % 4 == 0:
            forced.append(HMAX)
        w = _profile(g % 6, x)
        w[is_hi if g % 2 == 0 else is_lo] = 0.0                  # at most one member of a twin pair ...
        if g % 16 == 7:                                          # ... or both members of the first few
            both = np.concatenate([tw_lo[:4], tw_hi[:4]])
            forced += list(both)
            w[np.isin(uni, both)] = 0.0
        forced = np.array(forced[:n], dtype=np.uint64)
        own = rng.choice(uni, size=n - len(forced), replace=False, p=w / w.sum())
        vals = np.sort(np.concatenate([forced, own]))
        assert len(np.unique(vals)) == n
        H[g, :n] = vals
        NH[g] = n
    return H, NH


RANK_M = (0, 1, 5)


def planted_rank_pairs(s, seed, cross_m=True):
    """Pairs (A, B) of full sketches that share exactly m + 1 hashes and
    nothing with any other pair: m early shared hashes at positions 0 .. m - 1
    of both, and one probe hash v = A[i] = B[j], whose union rank is
    i + j - m.  For every column position j in {64 k - 1, 64 k, 64 k + 1}
    (0 < j < s; the kernels stream a column in 64-element chunks) three pairs:
    i = s - 1 - j + m (rank s - 1, counted), i = s - j + m (rank s, the first
    hash not counted) and i = s - 2 - j + m, with m in RANK_M (cross_m: every
    m at every position, else m cycles with the position).  In a third of the
    pairs A also holds a value with v's high word and another low word,
    directly below v in A (where rank s puts the element the scan end looks
    at) or directly above it (rank s - 2).  B is j random values below v, v,
    and s - 1 - j values above it; A likewise around position i.  The whole
    sweep comes twice, the second time with A as the later genome (`swap`),
    and a third time with m = 0 and the value 0 as A's first element, which
    B does not hold (`zero`: the row tiles of these pairs hold the key 0, and
    no match precedes the probe; the A sides of this block share the 0 with
    each other).

    Returns a dict of arrays over the pairs: A, B [P, s], i, j, m, swap, zero,
    twin (-1 below, +1 above, 0 none), v."""
    rng = np.random.default_rng(seed)
    js = sorted({j for k in range(1, s // 64 + 2) for j in (64 * k - 1, 64 * k, 64 * k + 1) if 0 < j < s})
    out = {k: [] for k in ("A", "B", "i", "j", "m", "swap", "zero", "twin", "v")}
    lo_floor, hi_ceil = 1 << 40, int(UMAX) - 1

    def side(pos, early, v, twin, zero=False):
        """s sorted values with v at position pos, the early shared values first (after the value 0, if held)."""
        early = np.concatenate([np.zeros(int(zero), np.uint64), early])
        nb, na = pos - len(early), s - 1 - pos
        below = rng.integers(lo_floor, int(v), size=nb, dtype=np.uint64)
        above = rng.integers(int(v) + 1, hi_ceil, size=na, dtype=np.uint64)
        hi = v & ~_U(0xFFFFFFFF)
        if twin < 0:
            below[0] = hi | _U(rng.integers(0, int(v & _U(0xFFFFFFFF))))
        if twin > 0:
            above[0] = hi | _U(rng.integers(int(v & _U(0xFFFFFFFF)) + 1, 1 << 32))
        row = np.sort(np.concatenate([early, below, [v], above]))
        assert len(np.unique(row)) == s and row[pos] == v
        return row

    for swap, zero in ((False, False), (True, False), (False, True)):
        for jx, j in enumerate(js):
            for var, di in enumerate((-1, 0, -2)):
                for mx, m in enumerate(RANK_M):
                    if (m != 0) if zero else (not cross_m and mx != (jx + var) % len(RANK_M)):
                        continue
                    i = s + di - j + m
                    if not (m + zero <= i <= s - 1 and m <= j):
                        continue
                    # v away from both ends of the value range and with a low word that leaves room for a twin
                    v = (_U(rng.integers(1 << 61, 1 << 63)) & ~_U(0xFFFFFFFF)) | _U(rng.integers(1 << 8, (1 << 32) - (1 << 8)))
                    early = np.sort(rng.integers(1, lo_floor, size=m, dtype=np.uint64))
                    assert len(np.unique(early)) == m
                    twin = 0
                    if (jx + var + mx) % 3 == 0:
                        twin = -1 if var == 1 else 1 if var == 2 else (-1 if jx % 2 else 1)
                        if (twin < 0 and i - m - zero < 1) or (twin > 0 and s - 1 - i < 1):
                            twin = 0
                    out["A"].append(side(i, early, v, twin, zero))
                    out["B"].append(side(j, early, v, 0))
                    for k, val in (("i", i), ("j", j), ("m", m), ("swap", swap), ("zero", zero), ("twin", twin),
                                   ("v", v)):
                        out[k].append(val)
    res = {k: np.array(val) for k, val in out.items()}
    res["A"] = res["A"].astype(np.uint64).reshape(-1, s)
    res["B"] = res["B"].astype(np.uint64).reshape(-1, s)
    res["v"] = res["v"].astype(np.uint64)
    return res


def rank_pair_matrices(pp, max_pairs=100):
    """The planted pairs as sketch matrices of at most 2 max_pairs genomes:
    pair p of a matrix is its genomes (2 p, 2 p + 1), A first unless swapped.
    Yields (H, NH, p0, p1): the matrix holds pairs [p0, p1)."""
    P, s = pp["A"].shape
    for p0 in range(0, P, max_pairs):
        p1 = min(P, p0 + max_pairs)
        H = np.empty((2 * (p1 - p0), s), dtype=np.uint64)
        sw = pp["swap"][p0:p1].astype(bool)[:, None]
        H[0::2] = np.where(sw, pp["B"][p0:p1], pp["A"][p0:p1])
        H[1::2] = np.where(sw, pp["A"][p0:p1], pp["B"][p0:p1])
        yield H, np.full(len(H), s, dtype=np.uint32), p0, p1


def rank_pair_expected(pp):
    """common of every planted pair: the m early hashes and, when its union rank is below s, the probe."""
    s = pp["A"].shape[1]
    return pp["m"] + (pp["i"] + pp["j"] - pp["m"] < s)


def cond_index(i, j, N):
    return i * N - i * (i + 1) // 2 + (j - i - 1)


def permuted_condensed(common, denom, N, perm):
    """The condensed (common, denom) of the set (H[perm], NH[perm]) from those
    of (H, NH), through the symmetric N x N square (both counts are symmetric
    in the pair): a second data set per shape without another reference run."""
    perm = np.asarray(perm, dtype=np.int64)
    assert np.array_equal(np.sort(perm), np.arange(N))
    ii, jj = np.triu_indices(N, 1)
    out = []
    for a in (common, denom):
        assert len(a) == N * (N - 1) // 2
        M = np.zeros((N, N), dtype=a.dtype)
        M[ii, jj] = a
        M[jj, ii] = a
        out.append(np.ascontiguousarray(M[perm[:, None], perm[None, :]][ii, jj]))
    return out[0], out[1]


# ---------------------------------------------------------------- sketch references
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def valid_runs(rec):
    """[start, end) of the maximal runs of A/C/G/T in an upper-case record."""
    ok = np.isin(np.asarray(rec, dtype=np.uint8), _ACGT)
    d = np.diff(np.concatenate([[0], ok.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)))


def ref_sketch(records, s, seed=42):
    """(the s smallest distinct hashes, ascending; the number of valid k-mer
    windows) of a genome given as upper-case records, in plain Python: every
    window without an invalid base, min(k-mer, reverse complement) on the
    bytes, Murmur by the oracle's stand-alone function."""
    hashes, nk = set(), 0
    for rec in records:
        b = np.asarray(rec, dtype=np.uint8).tobytes()
        for a, e in valid_runs(rec):
            for p in range(a, e - K + 1):
                w = b[p:p + K]
                rc = w[::-1].translate(_COMP)
                hashes.add(oracle.murmur3_h1(min(w, rc), seed))
                nk += 1
    return np.array(sorted(hashes)[:s], dtype=np.uint64), nk


def flatten(genomes):
    """Genomes (lists of records) as the arguments of sketch_records: seq, rec_off, genome_rec_off."""
    recs = [np.asarray(r, dtype=np.uint8) for g in genomes for r in g]
    seq = np.concatenate(recs) if recs else np.zeros(0, np.uint8)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.uint64)
    return seq, rec_off, gro


RUN_LENGTHS = (20, 21, 22, 41, 85)      # 0, 1, 2, 21 and 65 k-mers
TILE_DELTAS = range(-25, 26)
LANE_DELTAS = range(0, 64)
LANE_SITES = (64 * 100, 64 * 300)       # two interior lane boundaries of a genome's first tile


def boundary_genomes(seed):
    """One genome per offset: genome g places valid runs, in a sea of N, at
    offset dl = g around two interior lane boundaries (64 window ends per lane;
    the 16-base code words and 32-base validity words repeat inside) and, for
    g < len(TILE_DELTAS), at offset dt = g - 25 around the genome's first and
    second tile boundary.  A site at position q = boundary + offset is
    [run P] x [run S] with S starting exactly at q (first site of a kind) or
    [run E] x [run Q] with E's last base exactly at q (second site); x is the
    one invalid base between the two runs: an N in odd genomes, which are one
    record, and a record break in even genomes, which are several records.
    Run lengths are drawn from RUN_LENGTHS.  Returns (genomes, sites): lists
    of upper-case records, and per genome its sites' (q, kind) for the CPU
    check."""
    rng = np.random.default_rng(seed)
    genomes, sites = [], []
    for g in LANE_DELTAS:
        dl = g
        plan = [(LANE_SITES[0] + dl, "start"), (LANE_SITES[1] + dl, "end")]
        span = TILE + 300 + int(rng.integers(0, 5000))
        if g < len(TILE_DELTAS):
            dt = TILE_DELTAS[g]
            plan += [(TILE + dt, "start"), (2 * TILE + dt, "end")]
            span = 2 * TILE + 300 + int(rng.integers(0, 5000))
        buf = np.full(span, ord("N"), dtype=np.uint8)
        breaks = []
        for q, kind in plan:
            l1, l2 = (int(x) for x in rng.choice(RUN_LENGTHS, 2))
            x = q - 1 if kind == "start" else q + 1            # the invalid base between the runs
            buf[x - l1:x] = _ACGT[rng.integers(0, 4, l1)]
            buf[x + 1:x + 1 + l2] = _ACGT[rng.integers(0, 4, l2)]
            breaks.append(x)
        if g % 2 == 0:
            # the same positions with a record break for every x: the separator takes x's place
            recs, a = [], 0
            for x in sorted(breaks):
                recs.append(buf[a:x].copy())
                a = x + 1
            recs.append(buf[a:].copy())
        else:
            recs = [buf]
        genomes.append(recs)
        sites.append(plan)
    return genomes, sites


END_SPANS = (TILE - 2, TILE - 1, TILE, TILE + 1, TILE + 20, TILE + 21)


def genome_end_genomes(seed):
    """Genomes whose only valid bases are their last 100, with spans around one
    tile (TILE - 1: one pad base before the next genome; TILE: a tile of
    padding), each followed by a genome whose first 100 bases are valid; one
    more of them (span TILE - 1) ends the call."""
    rng = np.random.default_rng(seed)
    genomes = []
    for span in END_SPANS + (TILE - 1,):
        e = np.full(span, ord("N"), dtype=np.uint8)
        e[-100:] = _ACGT[rng.integers(0, 4, 100)]
        genomes.append([e])
        if len(genomes) < 2 * len(END_SPANS):
            f = np.full(500, ord("N"), dtype=np.uint8)
            f[:100] = _ACGT[rng.integers(0, 4, 100)]
            genomes.append([f])
    return genomes


def pack_layout(genomes, seed):
    """The packed device layout (include/drephip.h) of genomes given as
    records, by hand: 2-bit codes A0 C1 G2 T3, 16 bases per uint32 (base p at
    bits 2 (p % 16)), validity 32 bases per uint32; genome g at base_off[g]
    (a multiple of the tile, the first at one tile), records one invalid base
    apart.  Every invalid position -- the first tile, separators, N, padding --
    carries a random code.  Returns codes, valid, base_off, padded, nkmers."""
    rng = np.random.default_rng(seed)
    off, pad, nk = [], [], []
    cur = TILE
    for recs in genomes:
        span = sum(len(r) for r in recs) + max(len(recs) - 1, 0)
        off.append(cur)
        pad.append((span + 1 + TILE - 1) // TILE * TILE)
        cur += pad[-1]
    code = rng.integers(0, 4, cur, dtype=np.uint8)
    val = np.zeros(cur, dtype=bool)
    lut = np.full(256, 4, dtype=np.uint8)
    lut[_ACGT] = np.arange(4)
    for recs, o in zip(genomes, off):
        p, n = o, 0
        for r in recs:
            c = lut[np.asarray(r, dtype=np.uint8)]
            ok = c < 4
            code[p:p + len(r)][ok] = c[ok]
            val[p:p + len(r)] = ok
            n += sum(max(0, e - a - K + 1) for a, e in valid_runs(r))
            p += len(r) + 1
        nk.append(n)
    codes = (code.reshape(-1, 16).astype(np.uint32) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64)
    valid = np.packbits(val.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
    return (codes.astype(np.uint32), np.ascontiguousarray(valid), np.array(off, np.uint64), np.array(pad, np.uint64),
            np.array(nk, np.uint64))


# ---------------------------------------------------------------- the shared-hash screen past one marking window
# k_screen_mark of drep_amd/csrc/screen.hip: a workgroup ORs a chunk of kMarkChunk runs (of >= 3 entries, in
# first-genome order) into an LDS window of kMarkTiles row tiles x kMarkCols columns anchored at the first genome
# g_lo of the chunk's first run (tiles from g_lo // R, columns from g_lo & ~31); marks outside it go to the bitmap
# directly.  A run whose entry fingerprints (the low 32 - vbits bits of the hashes' high words, used from kFpBits
# bits on) all agree is marked as one hash.
MARK_CHUNK, MARK_TILES, MARK_COLS, FP_BITS = 256, 128, 2048, 4
WIDE_HUBS = (65, 128, 129, 200, 700)


def entry_bits(N, s):
    """vbits of screen_front: the bits an entry index g s + k needs."""
    return max(1, int(N * s - 1).bit_length())


class _Plants:
    """Sorted rows of random distinct 62-bit values; plant() puts a value into
    genomes by replacing one entry that was not planted itself and sorting the
    row again (as tests/test_screen.py::test_screen_light_cells does)."""

    def __init__(self, N, s, rng, partial_every=0):
        self.rng, self.s = rng, s
        self.H = np.sort(rng.integers(1, 1 << 62, size=(N, s), dtype=np.uint64), axis=1)
        assert len(np.unique(self.H)) == N * s
        self.NH = np.full(N, s, dtype=np.uint32)
        for g in range(0, N, partial_every) if partial_every else ():
            self.NH[g] = rng.integers(s // 2, s)
            self.H[g, self.NH[g]:] = UMAX
        self.used = set()

    def value(self):
        while True:
            v = int(self.rng.integers(1 << 48, 1 << 62))
            if v not in self.used:
                return v

    def plant(self, genomes, v):
        for g in genomes:
            n = int(self.NH[g])
            row = self.H[g, :n]
            assert _U(v) not in row
            free = [k for k in range(n) if int(row[k]) not in self.used]
            j = free[int(self.rng.integers(len(free)))]
            self.H[g, :n] = np.sort(np.concatenate([np.delete(row, j), [_U(v)]]))
        self.used.add(int(v))


def wide_n(R):
    """Genomes of the wide sets: past the window in tiles and in columns, no multiple of 32."""
    return MARK_TILES * R + MARK_COLS + 1100


def wide_set_a(R, seed, anchor, s=16):
    """One chunk, so one window, anchored at g_lo = 32 + anchor (c_lo = 32).
    For the window's last row tile (g_lo // R + 127) and the first tile past
    it, a run of three {r, col, z} per edge: the tile's first row r with the
    columns c_lo + 2047 (the window's last), c_lo + 2048 and N - 1, its last
    row with their neighbours c_lo + 2046, c_lo + 2049, N - 2 -- each of
    these cells is marked once (a light cell) -- and, for anchor != 0, the
    last row with the first row's columns as well: those cells are marked by
    two runs.  Returns H, NH and {g_lo, edges: [(r, col)]}."""
    rng = np.random.default_rng(seed)
    N = wide_n(R)
    p = _Plants(N, s, rng)
    g_lo = 32 + anchor
    c_lo = g_lo & ~31
    p.plant([g_lo, g_lo + 1, g_lo + 2], p.value())
    edges, k = [], 0
    for T in (g_lo // R + MARK_TILES - 1, g_lo // R + MARK_TILES):
        for r, d in ((T * R, 0), (T * R + R - 1, 1)):
            cols = [c_lo + MARK_COLS - 1 - d, c_lo + MARK_COLS + d, N - 1 - d]
            if d and anchor:
                cols += [c_lo + MARK_COLS - 1, c_lo + MARK_COLS, N - 1]
            for col in cols:
                z = col + 7 + k if col + 60 < N else c_lo + MARK_COLS + 300 + k
                p.plant(sorted([r, col, z]), p.value())
                edges.append((r, col))
                k += 1
    return p.H, p.NH, {"g_lo": g_lo, "edges": edges}


def wide_set_b(R, seed, s=16):
    """Many chunks: 700 runs of 3 to 5 genomes whose first genomes lie about 5
    apart (a chunk of 256 runs spans ~1280 rows: its later runs start past its
    128 row tiles), the other members anywhere above; 40 runs of the first
    chunk extended by a row of a later chunk's run and one of its columns (a
    cell marked directly by the one and through the window of the other);
    runs of two on cells and on pairs of longer runs; partial sketches every
    11th genome."""
    rng = np.random.default_rng(seed)
    N = wide_n(R)
    p = _Plants(N, s, rng, partial_every=11)
    runs = []
    for i in range(700):
        f = 5 * i + int(rng.integers(0, 3))
        runs.append([f] + sorted(int(x) for x in rng.choice(np.arange(f + 1, N), int(rng.integers(2, 5)), replace=False)))
    for j in range(40):
        y = 300 + 8 * j
        fy = runs[y][0]
        col = fy + 100 + j
        runs[y] = sorted(set(runs[y]) | {col})
        row = fy + 1 if (fy + 1) % R else fy                 # a row of fy's tile
        x = 3 + 6 * j
        runs[x] = sorted(set(runs[x]) | {row, col})
    for r in runs:
        p.plant(r, p.value())
    for i in range(0, 700, 7):                              # runs of two
        a, c = runs[i][0], runs[i][-1]
        if i % 2:
            p.plant([a, c], p.value())                      # a second hash of a pair of the run
        else:
            a2 = [g for g in range(a // R * R, a // R * R + R) if g not in runs[i]][0]
            p.plant(sorted([a2, c]), p.value())             # another row of the cell
    return p.H, p.NH, {}


def wide_set_c(R, seed, s=16, hubs=WIDE_HUBS):
    """Long and colliding runs.  A twin of v has v's low word (one sort key,
    one run): the slow twin v ^ (1 << 33) differs in a fingerprint bit, the
    equal twin v ^ (1 << 63) -- or another bit from 47 up in the small mixes,
    so that its rank varies -- has v's fingerprint.
    - per hub length m: a clean hub, and per twin kind a hub whose entries 0,
      63, 64 and m - 1 hold the twin;
    - m = 129 with the single twin at 63, at 64; m = 65 with it at 0, at 64;
      m = 129 with every other entry holding the twin; each per twin kind;
    - equal-fingerprint mixes, 8 of each, half on neighbouring genomes (one
      row tile), half spread: {v, v, v'} with v' in the first, second, third
      genome; {v, v, v', v'} in three orders; a genome holding v and v' with
      two others holding v, or holding v', the double genome first, second,
      third."""
    rng = np.random.default_rng(seed)
    N = wide_n(R)
    p = _Plants(N, s, rng)

    def hub(m, twin_at, bit):
        g = np.sort(rng.choice(N, m, replace=False))
        v = p.value()
        tw = np.zeros(m, dtype=bool)
        tw[list(twin_at)] = True
        p.plant(g[~tw], v)
        if tw.any():
            p.plant(g[tw], v ^ (1 << bit))

    for m in hubs:
        hub(m, (), 0)
        for bit in (33, 63):
            hub(m, (0, 63, 64, m - 1), bit)
    for bit in (33, 63):
        for m, at in ((129, 63), (129, 64), (65, 0), (65, 64)):
            hub(m, (at,), bit)
        hub(129, range(1, 129, 2), bit)
    for rep in range(8):
        def genomes(n):
            if rep % 2:
                return np.sort(rng.choice(N, n, replace=False))
            g0 = int(rng.integers(0, N - 2 * n))
            return np.arange(g0, g0 + n)
        bit = 63 if rep < 2 else int(rng.integers(47, 62))
        for n, who in ((3, (0,)), (3, (1,)), (3, (2,)), (4, (2, 3)), (4, (1, 3)), (4, (0, 3))):
            g = genomes(n)
            v = p.value()
            p.plant(np.delete(g, who), v)
            p.plant(g[list(who)], v ^ (1 << bit))
        for both in (0, 1, 2):
            for others_twin in (False, True):
                g = genomes(3)
                v = p.value()
                p.plant([g[both]], v)
                p.plant([g[both]], v ^ (1 << bit))
                p.plant(np.delete(g, both), v ^ (1 << bit) if others_twin else v)
    return p.H, p.NH, {}


def wide_screen_sets(R, seed):
    """The sketch sets of tests/test_screen_wide.py at s = 16, by name: A0, A1,
    A31 (wide_set_a with that anchor), B, C (wide_set_b, wide_set_c) as (H, NH,
    info).  R: rows per row tile (Context.screen_geometry())."""
    sets = {"A%d" % a: wide_set_a(R, seed + a, a) for a in (0, 1, 31)}
    sets["B"] = wide_set_b(R, seed + 100)
    sets["C"] = wide_set_c(R, seed + 200)
    return sets


def mark_emulation(H, NH, s, R):
    """What k_screen_mark does with a sketch set, counted: the entries grouped
    by low word, the runs of >= 3 ordered by (first genome, key) and cut into
    chunks of MARK_CHUNK, each run's cells (row tile of the smaller genome,
    larger genome) -- every entry pair of a run whose fingerprints agree (all
    hashes, below FP_BITS fingerprint bits), else the pairs of equal hashes --
    sorted into window and direct marks by its chunk's window.  Returns a dict
    of counts (see the keys below)."""
    N = len(NH)
    fbits = 32 - entry_bits(N, s)
    g = np.repeat(np.arange(N), NH)
    k = np.concatenate([np.arange(n) for n in NH])
    h = H[g, k]
    key = (h & _U(0xFFFFFFFF)).astype(np.int64)
    o = np.argsort(key, kind="stable")
    g, k, h, key = g[o], k[o], h[o], key[o]
    heads = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    ends = np.concatenate([heads[1:], [len(key)]])
    full = NH == s
    st = dict.fromkeys(("runs3", "chunks", "in_in", "in_out", "out_in", "out_out", "edge_tile_127", "edge_tile_128",
                        "edge_col_2047", "edge_col_2048", "direct_once_same", "direct_twice", "window_twice",
                        "window_and_direct", "window_overhang", "two_on_long_cell", "two_on_long_pair",
                        "equal_fp_mixed", "equal_fp_mixed_long", "slow_long", "diagonal", "dup_second_shared",
                        "light_other_hash_low_rank", "rank_below_s", "rank_from_s"), 0)
    st["twin_at"] = set()
    long_runs = [(int(g[a]), int(key[a]), a, e) for a, e in zip(heads, ends) if e - a >= 3]
    long_runs.sort()
    st["runs3"] = len(long_runs)
    st["chunks"] = (len(long_runs) + MARK_CHUNK - 1) // MARK_CHUNK
    cells, chunk_of, inwin, same_of = [], [], [], []
    other_hash = []                                          # cells of pairs a light cell must not count
    for q, (_, _, a, e) in enumerate(long_runs):
        if q % MARK_CHUNK == 0:
            g_lo = long_runs[q][0]
            t_lo, c_lo = g_lo // R, g_lo & ~31
            st["window_overhang"] += (t_lo + MARK_TILES) * R > N or c_lo + MARK_COLS > N
        gs, hs, ks = g[a:e], h[a:e], k[a:e]
        m = e - a
        if fbits >= FP_BITS:
            fp = (hs >> _U(32)) & _U((1 << fbits) - 1)
            same = bool((fp == fp[0]).all())
        else:
            same = bool((hs == hs[0]).all())
        mixed = not (hs == hs[0]).all()
        xi, yi = np.triu_indices(m, 1)
        share = (hs[xi] == hs[yi]) & (gs[xi] != gs[yi])
        if same:
            st["equal_fp_mixed"] += mixed
            st["equal_fp_mixed_long"] += mixed and m > 64
            st["diagonal"] += bool((gs[1:] == gs[:-1]).any())
            dup = np.flatnonzero(gs[1:] == gs[:-1]) + 1     # second entries of genomes that hold two
            st["dup_second_shared"] += int(sum(((hs == hs[d]) & (gs != gs[d])).any() and hs[d] != hs[d - 1] for d in dup))
            wrong = ~share & (gs[xi] != gs[yi]) & full[gs[xi]] & full[gs[yi]] & (ks[xi] + ks[yi] < s)
            other_hash.append((gs[xi][wrong] // R) * N + gs[yi][wrong])
            keep = np.ones(len(xi), dtype=bool)
        else:
            st["slow_long"] += m > 64
            keep = share
        if mixed and m > 64:
            vals, cnt = np.unique(hs, return_counts=True)
            st["twin_at"] |= {(int(p), "equal" if same else "slow") for p in np.flatnonzero(hs == vals[np.argmin(cnt)])
                              if cnt.min() <= 4}
        one = share & full[gs[xi]] & full[gs[yi]]
        st["rank_below_s"] += int((one & (ks[xi] + ks[yi] < s)).sum())
        st["rank_from_s"] += int((one & (ks[xi] + ks[yi] >= s)).sum())
        c = np.unique((gs[xi][keep] // R) * N + gs[yi][keep])
        t, col = c // N, c % N
        w = (t - t_lo < MARK_TILES) & (col - c_lo < MARK_COLS)
        st["in_in"] += int(w.sum())
        st["in_out"] += int(((t - t_lo < MARK_TILES) & ~(col - c_lo < MARK_COLS)).sum())
        st["out_in"] += int((~(t - t_lo < MARK_TILES) & (col - c_lo < MARK_COLS)).sum())
        st["out_out"] += int((~(t - t_lo < MARK_TILES) & ~(col - c_lo < MARK_COLS)).sum())
        st["edge_tile_127"] += int((t - t_lo == MARK_TILES - 1).sum())
        st["edge_tile_128"] += int((t - t_lo == MARK_TILES).sum())
        st["edge_col_2047"] += int((col - c_lo == MARK_COLS - 1).sum())
        st["edge_col_2048"] += int((col - c_lo == MARK_COLS).sum())
        cells.append(c)
        chunk_of.append(np.full(len(c), q // MARK_CHUNK))
        inwin.append(w)
        same_of.append(np.full(len(c), same))
    if not cells:
        return st
    cells, chunk_of, inwin, same_of = (np.concatenate(x) for x in (cells, chunk_of, inwin, same_of))
    uc, inv, cnt = np.unique(cells, return_inverse=True, return_counts=True)
    once = cnt[inv] == 1
    st["direct_once_same"] = int((once & ~inwin & same_of).sum())
    nwin = np.bincount(inv, weights=inwin, minlength=len(uc))
    ndir = cnt - nwin
    st["direct_twice"] = int((ndir >= 2).sum())
    st["window_twice"] = int((nwin >= 2).sum())
    for u in np.flatnonzero((nwin >= 1) & (ndir >= 1)):
        sel = inv == u
        st["window_and_direct"] += len(set(chunk_of[sel][inwin[sel]]) ^ set(chunk_of[sel][~inwin[sel]])) > 0
    if other_hash:
        oh = np.unique(np.concatenate(other_hash))
        at = np.searchsorted(uc, oh)
        st["light_other_hash_low_rank"] = int((cnt[at] == 1).sum())
    for a, e in zip(heads, ends):                            # runs of two that hold one hash in two genomes
        if e - a == 2 and h[a] == h[a + 1] and g[a] != g[a + 1]:
            c = (g[a] // R) * N + g[a + 1]
            at = np.searchsorted(uc, c)
            st["two_on_long_cell"] += bool(at < len(uc) and uc[at] == c)
    pairs = {}                                               # (short runs only: the sets plant these on runs of <= 6)
    for a, e in zip(heads, ends):
        if 2 <= e - a <= 6:
            for x in range(a, e):
                for y in range(x + 1, e):
                    if h[x] == h[y] and g[x] != g[y]:
                        pairs.setdefault((int(g[x]), int(g[y])), []).append(e - a)
    st["two_on_long_pair"] = sum(1 for v in pairs.values() if 2 in v and max(v) >= 3)
    return st


# ---------------------------------------------------------------- no fingerprint: N s > 2^28
SHORT_N, SHORT_S, SHORT_MAX = 8200, 32767, 16


def short_row_sets(seed, N=SHORT_N, nmax=SHORT_MAX):
    """N partial sketches of at most nmax hashes (rows [N, nmax], UMAX past
    NH): hubs of 70 and 200 genomes over the whole of 0 .. N - 1 (the last
    genome among them), a collision run of 100 genomes that hold v and
    v ^ (1 << 63) in turn, one of 90 with v and v ^ (1 << 33), 300 triples, 300
    runs of two, low-word twins."""
    rng = np.random.default_rng(seed)
    rows = [set(int(x) for x in rng.integers(1, 1 << 62, size=int(rng.integers(2, 9)))) for _ in range(N)]

    def plant(gs, v):
        for x in gs:
            if len(rows[x]) < nmax:
                rows[x].add(int(v))

    def some(m, last=False):
        gs = rng.choice(N - 1, m, replace=False)
        return np.concatenate([gs[1:], [N - 1]]) if last else gs
    plant(some(70), rng.integers(1, 1 << 62))
    plant(some(200, last=True), rng.integers(1, 1 << 62))
    for m, bit in ((100, 63), (90, 33)):
        gs, v = np.sort(some(m)), int(rng.integers(1 << 48, 1 << 62))
        plant(gs[0::2], v)
        plant(gs[1::2], v ^ (1 << bit))
    for _ in range(300):
        plant(some(3), rng.integers(1, 1 << 62))
        plant(some(2), rng.integers(1, 1 << 62))
    for _ in range(50):
        a, b = some(2)
        v = int(rng.integers(1 << 48, 1 << 62))
        plant([a], v)
        plant([b], v ^ (1 << int(rng.integers(32, 64))))
    H = np.full((N, nmax), UMAX, dtype=np.uint64)
    NH = np.zeros(N, dtype=np.uint32)
    for x, r in enumerate(rows):
        H[x, :len(r)] = np.sort(np.array(sorted(r), dtype=np.uint64))
        NH[x] = len(r)
    return H, NH


def incidence_allpairs(H, NH):
    """(common, denom) condensed of sketches so short that no pair's union
    reaches s (|A u B| <= |A| + |B| < s): common = |A n B|, denom = |A| + |B| -
    |A n B|, from the incidence matrix of the distinct values."""
    import scipy.sparse as sp
    N = len(NH)
    n = NH.astype(np.int64)
    vals = np.concatenate([H[x, :n[x]] for x in range(N)])
    _, inv = np.unique(vals, return_inverse=True)
    M = sp.csr_matrix((np.ones(len(inv), np.int32), (np.repeat(np.arange(N), n), inv)), shape=(N, int(inv.max()) + 1))
    S = sp.triu(M @ M.T, 1).tocsr()
    S.sort_indices()
    S = S.tocoo()                                            # in (i, j) order
    common = np.zeros(N * (N - 1) // 2, dtype=np.uint16)
    denom = np.empty(N * (N - 1) // 2, dtype=np.uint16)
    for i in range(N - 1):
        o = cond_index(i, i + 1, N)
        denom[o:o + N - 1 - i] = n[i] + n[i + 1:]
    t = cond_index(S.row.astype(np.int64), S.col.astype(np.int64), N)
    common[t] = S.data
    denom[t] -= S.data.astype(np.uint16)
    return common, denom, S.row.astype(np.uint32), S.col.astype(np.uint32)


def cell_count(i, j, N, R):
    """Distinct cells (row tile of i, column j) of the pairs (i, j)."""
    return len(np.unique((i // R).astype(np.int64) * N + j))
