"""Generators and references of tests/test_edges.py (GPU) and
tests/test_edge_helpers.py (CPU): a set-based all-pairs reference that shares
no code with the oracle's merge loop, sketch sets built so that the all-pairs
kernels' data-dependent paths are taken (the hash values 0 and UMAX - 1, shared
hashes on both sides of union rank s at every column chunk boundary, shared
hashes late in one sketch and early in the other), and sequence layouts that
put a k-mer on every boundary of the sketch kernel's packed layout."""
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
