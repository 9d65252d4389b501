"""The data-dependent paths of the all-pairs kernels and the layout boundaries
of the sketch kernel, on inputs built to reach them (tests/edge_cases.py).

All-pairs (reference: `mash dist`, drep/d_cluster.py:569-573): every case is
compared bit for bit with the set-based reference (edge_cases.ref_allpairs)
and with the C oracle's merge.  The geometry sets hold the hash values 0 (the
whole-row kernel's MASKED instantiation) and UMAX - 1, low-word twins inside
and across rows, partial and empty sketches, and shared hashes late in one
sketch and early in the other; the planted rank pairs put a shared hash on
both sides of union rank s at every 64-element chunk boundary of the column
(the union-rank scan ends of ap_columns: past, past_v).  The matrix runs them
through the table, band and merge paths, every screen mode, the probe of
DREPHIP_AP_HIT=0, the row-tile heights of DREPHIP_AP_R, row segments and the
sparse output.

Sketch (reference: `mash sketch`, drep/d_cluster.py:543-544): with fewer
valid k-mers than the sketch size every valid k-mer's hash must be in the
sketch and nothing else, so one k-mer lost or invented at a tile, lane, word
or genome edge fails exactly; checked against a plain-Python enumeration and
the oracle."""
import numpy as np
import pytest

import oracle
import edge_cases as ec
from drep_amd import _lib

pytestmark = pytest.mark.gpu
UMAX = ec.UMAX

# ---------------------------------------------------------------- all-pairs inputs, built once
GEOM_N = {64: 200, 100: 150, 600: 64, 1000: 48, 1025: 40, 2048: 24, 4096: 24}
_CACHE = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _with_refs(H, NH, s):
    rc, rd = ec.ref_allpairs(H, NH, s)
    oc, od = oracle.allpairs(H, NH, s, threads=8)
    assert np.array_equal(rc, oc) and np.array_equal(rd, od), "the two references disagree"
    return _frozen(H, NH, rc, rd, oc, od)


def sets_of(gen, s):
    """The sketch matrices of a generator at sketch size s with both
    references: geometry -- one matrix; rank -- the planted pairs, 100 to a
    matrix (every m at every position up to s = 1000, above it m cycles)."""
    if (gen, s) not in _CACHE:
        if gen == "geom":
            H, NH = ec.geometry_sketches(GEOM_N[s], s, seed=s)
            _CACHE[(gen, s)] = [_with_refs(H, NH, s)]
        else:
            pp = ec.planted_rank_pairs(s, seed=s, cross_m=s <= 1000)
            exp = ec.rank_pair_expected(pp)
            mats = []
            for H, NH, p0, p1 in ec.rank_pair_matrices(pp):
                m = _with_refs(H, NH, s)
                idx = ec.cond_index(2 * np.arange(p1 - p0), 2 * np.arange(p1 - p0) + 1, len(NH))
                assert np.array_equal(m[4][idx], exp[p0:p1])
                mats.append(m)
            _CACHE[(gen, s)] = mats
    return _CACHE[(gen, s)]


def _start(i, N):
    return i * N - i * (i + 1) // 2


def _condensed(ctx, H, NH):
    return ctx.allpairs(H, NH, want_denom=True)


def _merge(ctx, H, NH):
    import torch
    N = len(NH)
    dh = torch.from_numpy(H.view(np.int64).copy()).cuda()
    dn = torch.from_numpy(NH.view(np.int32).copy()).cuda()
    c = torch.zeros(N * (N - 1) // 2, dtype=torch.int16, device="cuda")
    d = torch.zeros(N * (N - 1) // 2, dtype=torch.int16, device="cuda")
    ctx.allpairs_device(dh.data_ptr(), dn.data_ptr(), N, 0, N, c.data_ptr(), d.data_ptr(),
                        torch.cuda.current_stream().cuda_stream, merge=True)
    torch.cuda.synchronize()
    return c.cpu().numpy().view(np.uint16), d.cpu().numpy().view(np.uint16)


def _rows(ctx, H, NH):
    """The triangle from row segments whose first rows (3, 10, N // 2 + 1) are no multiple of a tile height > 1."""
    N = len(NH)
    c = np.zeros(N * (N - 1) // 2, np.uint16)
    d = np.zeros(N * (N - 1) // 2, np.uint16)
    bounds = sorted({min(b, N - 1) for b in (0, 3, 10, N // 2 + 1, N - 1)})
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        a, b = _start(r0, N), _start(r1, N)
        ctx.allpairs_rows(H, NH, r0, r1, c[a:b], d[a:b])
    return c, d


# ---------------------------------------------------------------- the matrix
# (generator, s, path, screen, DREPHIP_AP_HIT, DREPHIP_AP_R, output)
#   path:   "table" | ("band", cap) | "merge"
#   screen: "off" | "on" (the LIST kernels) | "dense" (auto mode from 2 genomes, the screen's dense verdict:
#           chunk masks) | "dense0" (the same with DREPHIP_AP_CMASK=0)
#   output: "condensed" | "rows" | "sparse"
SIZES = (64, 100, 600, 1000, 1025, 2048)
CASES = []
for _gen in ("geom", "rank"):
    for _s in SIZES:
        for _scr in ("off", "on", "dense"):
            CASES.append((_gen, _s, "table", _scr, None, None, "condensed"))
    for _s in (64, 1000):
        CASES.append((_gen, _s, "table", "dense0", None, None, "condensed"))
    for _s in (64, 600, 1000, 2048):                                # the probe and scan ends of DREPHIP_AP_HIT=0
        for _scr in ("off", "on", "dense"):
            CASES.append((_gen, _s, "table", _scr, "0", None, "condensed"))
    for _s, _scr in ((64, "dense"), (1000, "off"), (1000, "on"), (2048, "off")):    # rows per tile
        for _r in (1, 2, 4, 8):
            CASES.append((_gen, _s, "table", _scr, None, _r, "condensed"))
    CASES.append((_gen, 1000, "table", "off", "0", 2, "condensed"))
    CASES.append((_gen, 1000, "table", "off", "0", 8, "rows"))
    for _scr in ("off", "on", "dense"):
        CASES.append((_gen, 1000, "table", _scr, None, None, "rows"))
    CASES.append((_gen, 100, "table", "on", None, 2, "rows"))
    for _s in (64, 1000, 2048):
        CASES.append((_gen, _s, "table", "on", None, None, "sparse"))       # direct: the SPARSE LIST kernel
    CASES.append((_gen, 1000, "table", "off", None, None, "sparse"))        # fallback: from the condensed counts
    CASES.append((_gen, 1000, "table", "on", "0", None, "sparse"))
    CASES.append((_gen, 1000, "table", "on", None, 8, "sparse"))
    for _cap in (64, 300, 768):
        CASES.append((_gen, 1000, ("band", _cap), "off", None, None, "condensed"))
        CASES.append((_gen, 4096, ("band", _cap), "off" if _cap != 300 else "on", None, None, "condensed"))
    CASES.append((_gen, 1000, ("band", 300), "on", None, None, "condensed"))
    CASES.append((_gen, 1000, ("band", 64), "off", None, None, "rows"))
    CASES.append((_gen, 4096, ("band", 768), "on", None, None, "sparse"))
    for _s in (64, 1000):
        CASES.append((_gen, _s, "merge", "off", None, None, "condensed"))


def _case_id(c):
    gen, s, path, scr, hit, r, out = c
    p = path if isinstance(path, str) else "band%d" % path[1]
    return "-".join([gen, "s%d" % s, p, scr] + (["hit" + hit] if hit else []) + (["R%d" % r] if r else []) + [out])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_allpairs_matrix(case, monkeypatch):
    gen, s, path, scr, hit, R, out = case
    if hit is not None:
        monkeypatch.setenv("DREPHIP_AP_HIT", hit)
    if R is not None:
        monkeypatch.setenv("DREPHIP_AP_R", str(R))
    if scr.startswith("dense"):
        monkeypatch.setenv("DREPHIP_SCREEN_MIN_N", "2")
        if gen == "rank":
            # unrelated genomes: the screen would pay; a ratio that makes any check too many gives its dense verdict
            monkeypatch.setenv("DREPHIP_SCREEN_RATIO", "1e15")
        if scr == "dense0":
            monkeypatch.setenv("DREPHIP_AP_CMASK", "0")
    with _lib.Context(0, 21, s, 42) as ctx:
        if R is not None:
            if ctx.screen_geometry() != R:
                pytest.skip("R = %d rows of s = %d do not fit the LDS: the override is not taken" % (R, s))
        ctx.set_allpairs_screen({"off": ctx.SCREEN_OFF, "on": ctx.SCREEN_ON}.get(scr, ctx.SCREEN_AUTO))
        if path != "table" and path != "merge":
            ctx.set_allpairs_path(ctx.AP_BAND, path[1])
        for H, NH, rc, rd, oc, od in sets_of(gen, s):
            N = len(NH)
            if out == "sparse":
                got = ctx.allpairs_sparse(H, NH)
                st = ctx.sparse_stats()
                for refc, refd in ((rc, rd), (oc, od)):
                    exp = ec.nonzero_pairs(refc, refd, N)
                    assert len(got[0]) == len(exp[0])
                    for g, e in zip(got, exp):
                        assert np.array_equal(g, e)
                direct = scr == "on" and path == "table"
                assert (st["direct"], st["fallback"]) == ((len(got[0]), 0) if direct else (0, len(got[0])))
                continue
            c, d = (_merge if path == "merge" else _rows if out == "rows" else _condensed)(ctx, H, NH)
            bad = np.flatnonzero((c != rc) | (d != rd))
            ii, jj = np.triu_indices(N, 1)
            assert len(bad) == 0, [(int(ii[t]), int(jj[t]), int(c[t]), int(rc[t]), int(d[t]), int(rd[t])) for t in bad[:8]]
            assert np.array_equal(c, oc) and np.array_equal(d, od)
            if path != "merge":
                sst = ctx.screen_stats()
                if scr == "on":
                    assert sst["used"] and sst["entries"] == int(NH.sum())
                elif scr == "off":
                    assert not sst["used"] and sst["entries"] == 0
                else:
                    assert not sst["used"] and sst["entries"] == int(NH.sum())     # the screen ran and gave way
    if gen == "geom":
        # the key 0 in full and partial rows, UMAX - 1 ending a full row
        assert ((H[:, 0] == 0) & (NH == s)).any() and ((H[:, 0] == 0) & (NH < s) & (NH > 0)).any()
        assert ((NH == s) & (H[:, s - 1] == UMAX - 1)).any()


def test_allpairs_override_is_taken():
    """DREPHIP_AP_R is honoured where the tiles fit (the matrix above skips
    the values that are not): every height at s = 64 and 1000, up to 4 at 2048."""
    import os
    taken = {}
    try:
        for s in (64, 1000, 2048):
            with _lib.Context(0, 21, s, 42) as ctx:
                taken[s] = []
                for r in (1, 2, 4, 8):
                    os.environ["DREPHIP_AP_R"] = str(r)
                    if ctx.screen_geometry() == r:
                        taken[s].append(r)
    finally:
        os.environ.pop("DREPHIP_AP_R", None)
    assert taken == {64: [1, 2, 4, 8], 1000: [1, 2, 4, 8], 2048: [1, 2, 4]}


# ---------------------------------------------------------------- sketch
S = 1000


def _upper(recs):
    return [np.where((r >= 97) & (r <= 122), r - 32, r).astype(np.uint8) for r in recs]


def _check_every_kmer(genomes, h, nh, ln, s=S, seed=42):
    for g, recs in enumerate(genomes):
        want, nk = ec.ref_sketch(recs, s, seed)
        assert nh[g] == len(want), (g, int(nh[g]), len(want))
        assert np.array_equal(h[g, :nh[g]], want), g
        assert (h[g, nh[g]:] == UMAX).all(), g
        assert int(ln[g]) == sum(len(r) for r in recs)
        seq, rec_off, _ = ec.flatten([recs])
        assert np.array_equal(want, oracle.sketch_records(seq, rec_off, 21, s, seed)), g


@pytest.fixture(scope="module")
def boundary_run(ctx1000):
    """The boundary genomes sketched in one call (shared, read-only)."""
    assert _lib.tile_bases() == ec.TILE
    genomes, _ = ec.boundary_genomes(seed=5)
    h, nh, ln = ctx1000.sketch_records(*ec.flatten(genomes))
    return genomes, h, nh, ln


def test_sketch_every_kmer_at_tile_and_lane_boundaries(boundary_run):
    """Valid runs of 20-85 bases that start and end at every offset -25..+25
    around a tile boundary and 0..63 around a lane boundary, N-delimited and
    as separate records, genomes of 2-3 tiles in one call: with at most 900
    valid k-mers and s = 1000 the threshold admits every hash, so the sketch
    is exactly the set of valid k-mers' hashes."""
    genomes, h, nh, ln = boundary_run
    for recs in genomes:
        assert ec.ref_sketch(recs, S)[1] <= 900
    _check_every_kmer(genomes, h, nh, ln)
    assert (nh > 0).all() and (nh < S).all()


def test_sketch_every_kmer_at_genome_ends(ctx1000):
    """Genomes valid only in their last 100 bases, spanning one tile give or
    take (one pad base; a whole tile of padding; the valid stretch across the
    tile edge), each followed by a genome valid in its first 100 bases, and
    one as the call's last genome."""
    genomes = ec.genome_end_genomes(seed=6)
    h, nh, ln = ctx1000.sketch_records(*ec.flatten(genomes))
    _check_every_kmer(genomes, h, nh, ln)
    assert (nh == 80).all()


def test_sketch_junk_under_invalid_bits(ctx1000, boundary_run):
    """The device entry point on a hand-packed layout whose invalid positions
    (first tile, N, separators, padding) carry random codes: the sketches of
    the host path, which packs code 0 there."""
    import torch
    genomes, h, nh, _ = boundary_run
    more = ec.genome_end_genomes(seed=6)
    codes, valid, off, pad, nk = ec.pack_layout(genomes + more, seed=9)
    n = len(off)
    d_codes = torch.from_numpy(codes.view(np.int32)).cuda()
    d_valid = torch.from_numpy(valid.view(np.int32)).cuda()
    d_h = torch.zeros((n, S), dtype=torch.int64, device="cuda")
    d_nh = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx1000.sketch_device(d_codes.data_ptr(), d_valid.data_ptr(), off, pad, nk, n, d_h.data_ptr(), d_nh.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gh, gnh = d_h.cpu().numpy().view(np.uint64), d_nh.cpu().numpy().view(np.uint32)
    assert np.array_equal(gnh[:len(genomes)], nh) and np.array_equal(gh[:len(genomes)], h)
    for g, recs in enumerate(more):
        want, _ = ec.ref_sketch(recs, S)
        assert gnh[len(genomes) + g] == len(want) and np.array_equal(gh[len(genomes) + g, :len(want)], want)


def test_sketch_exact_sizes():
    """s one below, at and one above the number D of distinct canonical k-mers
    (~3000), and every-k-mer sketches of ~0.95 s k-mers at s = 12000 (the LDS
    finalize) and 32767 (the global one)."""
    rng = np.random.default_rng(31)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    rec = A[rng.integers(0, 4, 3020)]
    allk, nk = ec.ref_sketch([rec], 1 << 20)
    D = len(allk)
    assert nk == 3000 and 2990 <= D <= 3000
    arg = ec.flatten([[rec]])
    for s in (D - 1, D, D + 1):
        with _lib.Context(0, 21, s, 42) as ctx:
            h, nh, _ = ctx.sketch_records(*arg)
        want = allk[:s]
        assert nh[0] == len(want) == min(s, D) and np.array_equal(h[0, :nh[0]], want) and (h[0, nh[0]:] == UMAX).all()
        assert np.array_equal(want, oracle.sketch_records(rec, arg[1], 21, s, 42))
    for s in (12000, 32767):
        L = int(0.95 * s) + 20
        recs = [A[rng.integers(0, 4, L // 2)], A[rng.integers(0, 4, L - L // 2 + 20)]]
        with _lib.Context(0, 21, s, 42) as ctx:
            h, nh, ln = ctx.sketch_records(*ec.flatten([recs]))
        _check_every_kmer([recs], h, nh, ln, s=s)
        assert 0.94 * s < nh[0] < s


@pytest.mark.parametrize("seed", [0, 1, 0x80000000, 0xFFFFFFFF])
def test_sketch_seeds_vs_oracle(seed):
    """Murmur seeds other than Mash's 42 (drephip_create takes any 32-bit
    seed; the hash kernel folds it in as ^ seed and 5 seed + c): the input of
    test_sketch_mixed_case_nruns_vs_oracle against the oracle's seed argument."""
    rng = np.random.default_rng(3)
    A = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    recs = [A[rng.choice(9, 300_000, p=[.24, .24, .24, .24, .01, .01, .01, .01, 0])],
            A[rng.choice(9, 50_000, p=[.2, .2, .2, .2, 0, 0, 0, 0, .2])],
            A[rng.integers(0, 4, 700)]]
    genomes = [recs[:2], recs[2:]]
    with _lib.Context(0, 21, S, seed) as ctx:
        h, nh, _ = ctx.sketch_records(*ec.flatten(genomes))
    for g, rs in enumerate(genomes):
        seq, rec_off, _ = ec.flatten([_upper(rs)])                  # the oracle takes upper case
        want = oracle.sketch_records(seq, rec_off, 21, S, seed)
        assert nh[g] == len(want) and np.array_equal(h[g, :nh[g]], want)
    assert nh[0] == S and nh[1] < S
    # the partial genome holds every k-mer: the plain-Python reference with this seed
    want, _ = ec.ref_sketch(_upper(genomes[1]), S, seed)
    assert np.array_equal(h[1, :nh[1]], want)
    if seed != 42:
        assert not np.array_equal(want, ec.ref_sketch(_upper(genomes[1]), S, 42)[0])
