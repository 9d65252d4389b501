"""Parity of the HIP path (libdrephip.so via its C ABI) with the oracle and the
reference fixtures.  Integer outputs are compared bit-exactly."""
import glob
import os
import shutil

import numpy as np
import pandas as pd
import pytest

import oracle
from drep_amd import _lib
from drep_amd.mash_io import read_msh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 1000
UMAX = np.iinfo(np.uint64).max


def _pad(h, s):
    out = np.full(s, UMAX, dtype=np.uint64)
    out[:len(h)] = h
    return out


# ------------------------------------------------------------------ sketch
def test_sketch_reference_genomes_bitexact(golden, ctx1000):
    fas = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))
    h, nh, ln = ctx1000.sketch_files(fas, threads=4)
    for i, fa in enumerate(fas):
        ref = read_msh(os.path.join(golden, "MASH_files", "sketches",
                                    os.path.basename(fa)[:-3] + ".msh")).references[0]
        assert nh[i] == len(ref.hashes) == S
        assert np.array_equal(h[i], ref.hashes)
        assert int(ln[i]) == ref.length


def test_sketch_files_many_batches(golden, tmp_path, monkeypatch):
    """The overlapped ingest pipeline (producer thread + two pinned buffers) with
    a batch size forced down to ~1 genome: 12 files (the 4 reference genomes,
    plain and gzip, repeated) in many batches give the reference's sketches in
    order, and the ingest stats add up."""
    import gzip
    fas = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))
    files = []
    for rep in range(3):
        for fa in fas:
            if rep == 1:
                files.append(fa)                                  # gzip
            else:
                p = tmp_path / ("r%d_" % rep + os.path.basename(fa)[:-3])
                p.write_bytes(gzip.open(fa).read())
                files.append(str(p))
    monkeypatch.setenv("DREPHIP_INGEST_BATCH_BASES", "3000000")
    with _lib.Context(0, 21, S, 42) as ctx:
        h, nh, ln = ctx.sketch_files(files, threads=3)
        st = ctx.ingest_stats()
    assert st["batches"] >= 4          # 3 files (~10 Mbp) per batch
    assert st["wall_s"] >= max(st["produce_s"], st["gpu_s"]) * 0.5
    for i, f in enumerate(files):
        ref = read_msh(os.path.join(golden, "MASH_files", "sketches",
                                    os.path.basename(f).split("_", 1)[-1].replace(".gz", "") + ".msh")).references[0] \
            if not f.endswith(".gz") else \
            read_msh(os.path.join(golden, "MASH_files", "sketches", os.path.basename(f)[:-3] + ".msh")).references[0]
        assert nh[i] == S and np.array_equal(h[i], ref.hashes) and int(ln[i]) == ref.length, f


def test_sketch_files_estimate_overflow(golden, tmp_path, monkeypatch):
    """The ingest places each genome in a region sized from its file (plain
    size, or a gzip trailer's ISIZE -- the LAST member's size).  A two-member
    gzip file whose last member is large enough to pass for the whole file
    underestimates its bases: that genome is repacked at the end of the batch.
    Sketches equal the oracle's, in order, with neighbours in the same batch."""
    import gzip
    import zlib
    fas = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))
    txt = [gzip.open(fa).read() for fa in fas]
    multi = tmp_path / "two_members.fa.gz"
    half = len(txt[0]) // 2
    cut = txt[0].index(b"\n", half) + 1                     # split at a line end
    with open(multi, "wb") as fh:
        for part in (txt[0][:cut], txt[0][cut:]):
            co = zlib.compressobj(6, zlib.DEFLATED, 31)       # one gzip member each
            fh.write(co.compress(part) + co.flush())
    assert len(gzip.open(multi).read()) == len(txt[0])
    plain = tmp_path / "plain.fa"
    plain.write_bytes(txt[1])
    files = [str(plain), str(multi), fas[2], str(multi), fas[3]]
    want = [fas[1], fas[0], fas[2], fas[0], fas[3]]
    for bb in (None, "4000000"):
        if bb:
            monkeypatch.setenv("DREPHIP_INGEST_BATCH_BASES", bb)
        with _lib.Context(0, 21, S, 42) as ctx:
            h, nh, ln = ctx.sketch_files(files, threads=3)
        for i, fa in enumerate(want):
            ref = read_msh(os.path.join(golden, "MASH_files", "sketches",
                                        os.path.basename(fa)[:-3] + ".msh")).references[0]
            assert nh[i] == S and np.array_equal(h[i], ref.hashes) and int(ln[i]) == ref.length, (bb, i)


def _records_case(rng, kind):
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    if kind == "nruns_lower_multirecord":
        recs = []
        for L in rng.integers(1, 60000, 9):
            b = A[rng.integers(0, 4, int(L))].copy()
            b[rng.random(int(L)) < 0.002] = ord("N")
            low = rng.random(int(L)) < 0.3
            b[low] += 32
            recs.append(b)
        recs += [A[rng.integers(0, 4, 20)], A[rng.integers(0, 4, 21)], np.zeros(0, np.uint8)]
        return recs
    if kind == "iupac_and_junk":
        b = A[rng.integers(0, 4, 50000)].copy()
        junk = np.frombuffer(b"RYKMSWBDHVN-*xU u", dtype=np.uint8)
        pos = rng.integers(0, 50000, 300)
        b[pos] = junk[rng.integers(0, len(junk), 300)]
        return [b]
    if kind == "tiny":               # fewer than s distinct k-mers: partial sketch
        return [A[rng.integers(0, 4, 400)]]
    if kind == "empty":
        return [np.zeros(0, np.uint8)]
    if kind == "all_n":
        return [np.full(5000, ord("N"), np.uint8)]
    if kind == "repeats_up":         # heavy repeats: threshold must be raised
        unit = A[rng.integers(0, 4, 3000)]
        return [np.tile(unit, 300)]
    if kind == "repeats_bisect":     # first raise overshoots the LDS sort -> bisection
        unit = A[rng.integers(0, 4, 300_000)]
        return [np.concatenate([unit, unit, unit, unit[:100_000]])]
    if kind == "tandem":
        return [np.tile(np.frombuffer(b"AT", np.uint8), 40000), A[rng.integers(0, 4, 100000)]]
    raise KeyError(kind)


CASES = ["nruns_lower_multirecord", "iupac_and_junk", "tiny", "empty", "all_n", "repeats_up",
         "repeats_bisect", "tandem"]


def test_sketch_edge_cases_vs_oracle(ctx1000):
    rng = np.random.default_rng(11)
    genomes = [_records_case(rng, k) for k in CASES]
    recs = [r for g in genomes for r in g]
    seq = np.concatenate(recs).astype(np.uint8) if recs else np.zeros(0, np.uint8)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.uint64)
    h, nh, ln = ctx1000.sketch_records(seq, rec_off, gro)
    upper = np.where((seq >= 97) & (seq <= 122), seq - 32, seq).astype(np.uint8)
    for gi, kind in enumerate(CASES):
        r0, r1 = int(gro[gi]), int(gro[gi + 1])
        sub = upper[int(rec_off[r0]):int(rec_off[r1])]
        off = (rec_off[r0:r1 + 1] - rec_off[r0]).astype(np.uint64)
        want = oracle.sketch_records(sub, off, 21, S, 42)
        assert nh[gi] == len(want), kind
        assert np.array_equal(h[gi, :nh[gi]], want), kind
        assert (h[gi, nh[gi]:] == UMAX).all(), kind
        assert int(ln[gi]) == int(off[-1]), kind


@pytest.mark.parametrize("s", [1, 64, 4096, 12000, 12001, 20000, 32767])
def test_sketch_sizes_vs_oracle(s):
    """Sketch sizes up to kMaxSketch = 32767 (dRep's -ms is unbounded,
    drep/argumentParser.py:103): above 12000 the finalize sorts its
    candidates in a global buffer instead of LDS."""
    rng = np.random.default_rng(s)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = [A[rng.integers(0, 4, 250_000)], A[rng.integers(0, 4, 3000)], A[rng.integers(0, 4, 900_000)]]
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.arange(len(recs) + 1, dtype=np.uint64)
    with _lib.Context(0, 21, s, 42) as ctx:
        h, nh, _ = ctx.sketch_records(seq, rec_off, gro)
    for g in range(len(recs)):
        want = oracle.sketch_records(recs[g], np.array([0, len(recs[g])], np.uint64), 21, s, 42)
        assert np.array_equal(h[g, :nh[g]], want)


@pytest.mark.parametrize("seed", [3, 4, 5, 9])
def test_sketch_mixed_case_nruns_vs_oracle(seed):
    """The hash kernel gives the oracle's sketches on lower case, N runs,
    multi-record genomes and a partial sketch."""
    rng = np.random.default_rng(seed)
    A = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    recs = [A[rng.choice(9, 300_000, p=[.24, .24, .24, .24, .01, .01, .01, .01, 0])],
            A[rng.choice(9, 50_000, p=[.2, .2, .2, .2, 0, 0, 0, 0, .2])],
            A[rng.integers(0, 4, 700)]]
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.array([0, 2, 3], dtype=np.uint64)           # genome 0 = records 0-1, genome 1 = record 2
    with _lib.Context(0, 21, S, 42) as ctx:
        h, nh, _ = ctx.sketch_records(seq, rec_off, gro)
    for g, (a, b) in enumerate([(0, 2), (2, 3)]):
        sub = np.concatenate(recs[a:b])
        sub = np.where((sub >= 97) & (sub <= 122), sub - 32, sub).astype(np.uint8)   # the oracle takes upper case
        off = np.concatenate([[0], np.cumsum([len(r) for r in recs[a:b]])]).astype(np.uint64)
        want = oracle.sketch_records(sub, off, 21, S, 42)
        assert nh[g] == len(want) and np.array_equal(h[g, :nh[g]], want)
    assert nh[1] < S


@pytest.mark.parametrize("s", [1, 1000, 12000, 24000])
def test_sketch_finalize_vs_oracle(s):
    """The bucket-sort finalize gives the oracle's sketches: full and partial
    sketches, its 4096- and 16384-candidate LDS instantiations and the
    global-buffer one (s > 12000), and a low-complexity genome whose
    candidates crowd few buckets."""
    rng = np.random.default_rng(100 + s)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    motif = A[rng.integers(0, 4, 40)]
    recs = [A[rng.integers(0, 4, 400_000)], A[rng.integers(0, 4, 5000)],
            np.tile(motif, 2000) if s > 1 else A[rng.integers(0, 4, 30)]]
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.arange(len(recs) + 1, dtype=np.uint64)
    with _lib.Context(0, 21, s, 42) as ctx:
        h, nh, _ = ctx.sketch_records(seq, rec_off, gro)
    for g in range(len(recs)):
        want = oracle.sketch_records(recs[g], np.array([0, len(recs[g])], np.uint64), 21, s, 42)
        assert nh[g] == len(want) and np.array_equal(h[g, :nh[g]], want), g


def test_sketch_every_kmer_hash_vs_oracle():
    """With s above the number of distinct k-mers every canonical k-mer's hash
    is in the sketch: the table-driven Murmur of every k-mer of a 9000-base
    genome (each of the 256 + 256 + 1024 table entries used) equals the
    oracle's."""
    rng = np.random.default_rng(77)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    rec = A[rng.integers(0, 4, 9000)]
    with _lib.Context(0, 21, 12000, 42) as ctx:
        h, nh, _ = ctx.sketch_records(rec, np.array([0, len(rec)], np.uint64), np.array([0, 1], np.uint64))
    want = oracle.sketch_records(rec, np.array([0, len(rec)], np.uint64), 21, 12000, 42)
    assert len(want) > 8900 and nh[0] == len(want) and np.array_equal(h[0, :nh[0]], want)


def test_synth_device_matches_oracle_generator(ctx1000):
    """The bench's on-device generator + device sketch == oracle generator +
    oracle sketch (5 Mbp genomes, the BASELINE genome size)."""
    import torch
    n, L, fam, seed = 6, 5_000_000, 3, 9
    tile = _lib.tile_bases()
    P = _lib.padded_bases([L])
    total = tile + n * P
    codes = torch.zeros(total // 16, dtype=torch.int32, device="cuda")
    valid = torch.zeros(total // 32, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream    # order after torch's fills
    ctx1000.synth_device(seed, 0, n, fam, L, codes.data_ptr(), valid.data_ptr(), st)
    hashes = torch.zeros((n, S), dtype=torch.int64, device="cuda")
    nhash = torch.zeros(n, dtype=torch.int32, device="cuda")
    off = np.array([tile + i * P for i in range(n)], np.uint64)
    ctx1000.sketch_device(codes.data_ptr(), valid.data_ptr(), off, np.full(n, P, np.uint64),
                          np.full(n, L - 20, np.uint64), n, hashes.data_ptr(), nhash.data_ptr(), st)
    torch.cuda.synchronize()
    h = hashes.cpu().numpy().view(np.uint64)
    nh = nhash.cpu().numpy().view(np.uint32)
    oh, onh = oracle.sketch_synth(0, n, L, seed=seed, family_size=fam, threads=6)
    assert np.array_equal(nh, onh)
    assert np.array_equal(h, oh)
    # the packed bases themselves
    asc = oracle.synth_ascii(4, L, seed=seed, family_size=fam)
    code = np.frombuffer(bytes(256), np.uint8).copy()
    code[[65, 67, 71, 84]] = [0, 1, 2, 3]
    c = code[asc]
    words = codes[(tile + 4 * P) // 16:(tile + 4 * P) // 16 + L // 16].cpu().numpy().view(np.uint32)
    unpacked = ((words[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)
    assert np.array_equal(unpacked, c[:len(unpacked)])


# --------------------------------------------------------------- all-pairs
def _ref_sketches(golden):
    refs = read_msh(os.path.join(golden, "MASH_files", "ALL.msh")).references
    H = np.stack([_pad(r.hashes, S) for r in refs])
    NH = np.array([len(r.hashes) for r in refs], np.uint32)
    return refs, H, NH


def test_allpairs_reference_table(golden, ctx1000):
    """Shared-hash counts of the 5 reference genomes == MASH_table.tsv."""
    refs, H, NH = _ref_sketches(golden)
    c, d = ctx1000.allpairs(H, NH)
    rows = [l.split("\t") for l in open(os.path.join(golden, "MASH_files", "MASH_table.tsv"))]
    names = [r.name for r in refs]
    N = len(refs)
    for row in rows:
        i, j = names.index(row[0]), names.index(row[1])
        if i == j:
            continue
        a, b = min(i, j), max(i, j)
        k = a * N - a * (a + 1) // 2 + (b - a - 1)
        cc, dd = row[4].strip().split("/")
        assert (int(c[k]), int(d[k])) == (int(cc), int(dd))


def _family_sketches(n, L, fam, seed):
    return oracle.sketch_synth(0, n, L, seed=seed, family_size=fam, threads=8)


@pytest.fixture(scope="module")
def family():
    return _family_sketches(160, 400_000, 20, 5)


def test_allpairs_family_vs_oracle(family, ctx1000):
    h, nh = family
    c, d = ctx1000.allpairs(h, nh)
    oc, od = oracle.allpairs(h, nh, S, threads=8)
    assert np.array_equal(c, oc) and np.array_equal(d, od)
    assert c.max() > 500          # similar pairs are exercised


@pytest.mark.parametrize("path", ["table", "band"])
@pytest.mark.parametrize("partial", [False, True])
def test_allpairs_unbuildable_table_falls_back_to_merge(path, partial):
    """Three hashes of one row sharing their low 32 bits land in the same two
    slots under every field family, so no cuckoo table exists for that row:
    the table kernel merges that row's pairs literally (the band path reruns
    the segment with the merge kernel) -- counts and denominators still exact,
    also when some sketches are partial."""
    h, nh = _unbuildable_rows()
    if partial:                       # partial sketches: denominators below s
        for i in (1, 7, 12):          # unions below s: denominators < s
            nh[i] = 300 + i
            h[i, nh[i]:] = UMAX
    N = len(nh)
    oc, od = oracle.allpairs(h, nh, S, threads=4)
    good = h.copy()
    for i in (0, 7, 1, 8):
        good[i] = h[i + 2]
        good[i, nh[i]:] = UMAX
    ogc, ogd = oracle.allpairs(good, nh, S, threads=4)
    with _lib.Context(0, 21, S, 42) as ctx:
        if path == "band":
            ctx.set_allpairs_path(ctx.AP_BAND, 256)
        c, d = ctx.allpairs(h, nh)
        # a clean call, then a failing one again, on the same context
        c2, d2 = ctx.allpairs(good, nh)
        c3, d3 = ctx.allpairs(h, nh)
        # one row range at a time (row segments through the same path)
        cs = np.zeros_like(c)
        ds = np.zeros_like(d)
        for r0, r1 in ((0, 3), (3, 8), (8, N)):
            a = r0 * N - r0 * (r0 + 1) // 2
            b = r1 * N - r1 * (r1 + 1) // 2 if r1 < N else len(c)
            ctx.allpairs_rows(h, nh, r0, r1, cs[a:b], ds[a:b] if partial else None)
    assert np.array_equal(c, oc) and np.array_equal(c3, oc) and np.array_equal(cs, oc)
    assert np.array_equal(c2, ogc)
    if partial:
        assert np.array_equal(d, od) and np.array_equal(d2, ogd) and np.array_equal(ds, od)
        assert (od < S).any()
    assert c.max() >= 2


@pytest.mark.parametrize("path", ["table", "band"])
@pytest.mark.parametrize("seed", [0, 1])
def test_allpairs_twin_low_words_vs_oracle(seed, path):
    """Rows holding two hashes with one low 32-bit word (twins) fill both of
    those keys' slots, so a lookup can match a slot whose high word differs and
    must try the other: such rows leave the fast probe (k_build_q32 flags them).
    Columns hold the first twin only, the second only, both, or neither.  Keys
    whose rotated quotient is all ones (they "match" an empty slot word) are
    spread over rows and columns too."""
    rng = np.random.default_rng(seed)
    N = 16
    pool = rng.choice(2 ** 62, size=400 + N * S, replace=False).astype(np.uint64)
    shared, fresh = pool[:400], pool[400:].reshape(N, S)  # a common block, so counts are non-trivial
    lo = np.uint64(0x2468ACE1)
    tw = np.array([(np.uint64(k) << np.uint64(44)) | lo for k in (5, 9)], dtype=np.uint64)
    h = np.zeros((N, S), np.uint64)
    for i in range(N):
        pick = {0: tw, 1: tw, 2: tw, 3: tw[:1], 4: tw[:1], 5: tw[1:], 6: tw[1:], 7: tw, 8: tw}.get(i, tw[:0])
        em = np.array([(np.uint64(k) << np.uint64(44)) | np.uint64(w) for k, w in
                       ((3, 0xAECFFFFF), (4, 0xFFFFABCF), (6, 0x8F0FFFFF))], dtype=np.uint64)[i % 4:]
        base = np.concatenate([pick, em, shared[: 200 + 10 * i]])
        h[i] = np.sort(np.concatenate([base, fresh[i][: S - len(base)]]))
    assert all(len(np.unique(r)) == S for r in h)
    nh = np.full(N, S, np.uint32)
    oc, od = oracle.allpairs(h, nh, S, threads=4)
    with _lib.Context(0, 21, S, 42) as ctx:
        if path == "band":                    # band tables of 256 elements: twins in the first band
            ctx.set_allpairs_path(ctx.AP_BAND, 256)
        c, d = ctx.allpairs(h, nh)
    assert np.array_equal(c, oc) and np.array_equal(d, od)
    assert oc.max() >= 150


def _unbuildable_rows():
    """Rows 0 and 7 hold three hashes with one low word (no cuckoo table can
    hold them); rows 1 and 8 share two of them."""
    rng = np.random.default_rng(3)
    N = 24
    base = np.sort(rng.choice(2 ** 62, size=(N, 2000), replace=False).astype(np.uint64), axis=1)
    h = np.full((N, S), UMAX, dtype=np.uint64)
    for i in range(N):                                   # families: shared prefixes
        pool = base[i // 6]
        keep = np.sort(rng.choice(len(pool), S, replace=False))
        h[i] = pool[keep]
    lo = np.uint64(0x12345678)
    bad = np.array([(np.uint64(k) << np.uint64(40)) | lo for k in (1, 2, 3)], dtype=np.uint64)
    for i in (0, 7):
        row = np.unique(np.concatenate([h[i][:S - 3], bad]))
        h[i] = row[:S]
        h[i + 1] = np.unique(np.concatenate([h[i + 1][:S - 2], bad[:2]]))[:S]
    nh = np.full(N, S, np.uint32)
    return h, nh


def test_allpairs_device_async_wait():
    """drephip_allpairs_device_async returns once the kernels are queued; rows
    whose table cannot be built are merged literally inside the kernel, so the
    counts are exact however the call is completed (drephip_allpairs_wait or
    the next all-pairs call), and a clean call between two failing ones is not
    affected."""
    import torch
    h, nh = _unbuildable_rows()
    N = len(nh)
    good = h.copy()
    for i in (0, 7, 1, 8):
        good[i] = h[i + 2]
    oc, _ = oracle.allpairs(h, nh, S, threads=4)
    ogc, _ = oracle.allpairs(good, nh, S, threads=4)
    st = torch.cuda.current_stream().cuda_stream
    dn = torch.from_numpy(nh.view(np.int32)).cuda()
    with _lib.Context(0, 21, S, 42) as ctx:
        outs = []
        for rows, how in ((h, "wait"), (good, "wait"), (h, "next_call"), (good, "wait"), (h, "wait")):
            dh = torch.from_numpy(rows.view(np.int64)).cuda()
            c = torch.zeros(N * (N - 1) // 2, dtype=torch.int16, device="cuda")
            for _ in range(2):          # the second call reuses the item list: the deferred form
                ctx.allpairs_device_async(dh.data_ptr(), dn.data_ptr(), N, 0, N, c.data_ptr(), None, st)
                if how == "wait":
                    ctx.allpairs_wait()
                else:                   # completed by the next all-pairs call (a synchronous one)
                    ctx.allpairs_device(dh.data_ptr(), dn.data_ptr(), N, N, N, c.data_ptr(), None, st)
            torch.cuda.synchronize()
            outs.append(c.cpu().numpy().view(np.uint16))
    for c, want in zip(outs, (oc, ogc, oc, ogc, oc)):
        assert np.array_equal(c, want)


def test_allpairs_rejects_unpadded_rows(ctx1000):
    """Rows past nhash must be UINT64_MAX (the kernels read whole rows): the
    host entry point checks and reports instead of miscounting."""
    h = np.full((3, S), UMAX, dtype=np.uint64)
    h[:, :10] = np.arange(10, dtype=np.uint64) + 1
    nh = np.array([10, 10, 10], np.uint32)
    c, _ = ctx1000.allpairs(h, nh)
    assert list(c) == [10, 10, 10]
    h[1, 20] = 5
    with pytest.raises(_lib.DrepHipError, match="UINT64_MAX"):
        ctx1000.allpairs(h, nh)


def test_allpairs_partial_sketches_vs_oracle(ctx1000):
    rng = np.random.default_rng(3)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = A[rng.integers(0, 4, 600_000)]
    recs = []
    for i in range(40):
        L = int(rng.choice([60, 300, 700, 1200, 5000, 600_000]))
        x = base[:L].copy()
        m = rng.random(L) < rng.choice([0.0, 0.01, 0.05])
        x[m] = A[rng.integers(0, 4, int(m.sum()))]
        recs.append(x)
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.arange(len(recs) + 1, dtype=np.uint64)
    h, nh, _ = ctx1000.sketch_records(seq, rec_off, gro)
    assert (nh < S).any() and (nh == S).any()
    c, d = ctx1000.allpairs(h, nh)
    oc, od = oracle.allpairs(h, nh, S)
    assert np.array_equal(c, oc) and np.array_equal(d, od)


@pytest.mark.parametrize("s", [1, 16, 100, 513, 1024, 1025, 2048, 2049, 4096, 10000, 12000, 20000, 32767])
def test_allpairs_sketch_sizes(s):
    h, nh = oracle.sketch_synth(0, 48, 120_000, seed=s, family_size=12, s=s, threads=8)
    with _lib.Context(0, 21, s, 42) as ctx:
        c, d = ctx.allpairs(h, nh)
    oc, od = oracle.allpairs(h, nh, s, threads=8)
    assert np.array_equal(c, oc) and np.array_equal(d, od)


@pytest.mark.parametrize("s,cap", [(1, 1), (100, 7), (1000, 64), (1000, 1024), (4096, 300),
                                   (10000, 1024), (12000, 1000), (20000, 768)])
def test_allpairs_band_kernel_vs_oracle(s, cap):
    """Value-banded kernel (production path for s > 2048): many bands per row
    tile at small caps, bit-exact counts and denominators."""
    h, nh = oracle.sketch_synth(0, 40, 150_000, seed=s + cap, family_size=10, s=s, threads=8)
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_path(ctx.AP_BAND, cap)
        c, d = ctx.allpairs(h, nh, want_denom=True)
    oc, od = oracle.allpairs(h, nh, s, threads=8)
    assert np.array_equal(c, oc) and np.array_equal(d, od)
    if s >= 1000:
        assert c.max() > s // 2


@pytest.mark.parametrize("screen", ["on", "off"])
@pytest.mark.parametrize("per,cap,chunk", [(0, 768, 0), (1, 768, 0), (37, 300, 8), (300, 300, 0), (640, 768, 16),
                                           (640, 200, 0), (5000, 768, 0)])
def test_allpairs_band_value_rounds(per, cap, chunk, screen, monkeypatch):
    """The band kernel's value rounds (one launch per global value range,
    item state parked in HBM between launches): any round size -- none, one
    element, rounds narrower and wider than the band cap, a single round --
    and item chunks of 8-16 (every chunk runs all rounds before the next)
    give the oracle's counts and denominators, screened (LIST) and dense."""
    s = 4096
    h, nh = oracle.sketch_synth(0, 72, 150_000, seed=per + cap, family_size=9, s=s, threads=8)
    nh = nh.copy()
    h = h.copy()
    h[5, 1000:] = UMAX; nh[5] = 1000                  # a partial row and an empty one
    h[17, :] = UMAX; nh[17] = 0
    monkeypatch.setenv("DREPHIP_BAND_ROUND", str(per))
    if chunk:
        monkeypatch.setenv("DREPHIP_BAND_CHUNK", str(chunk))
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_path(ctx.AP_BAND, cap)
        ctx.set_allpairs_screen(ctx.SCREEN_ON if screen == "on" else ctx.SCREEN_OFF)
        c, d = ctx.allpairs(h, nh, want_denom=True)
    oc, od = oracle.allpairs(h, nh, s, threads=8)
    assert np.array_equal(c, oc) and np.array_equal(d, od)
    assert c.max() > s // 2


def test_allpairs_band_partial_and_segments(family, ctx1000):
    """Band kernel on partial sketches (denominator from the full intersection)
    and on row-range segments."""
    import torch
    rng = np.random.default_rng(11)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = A[rng.integers(0, 4, 300_000)]
    recs = []
    for i in range(36):
        L = int(rng.choice([0, 60, 300, 700, 1200, 5000, 300_000]))
        x = base[:L].copy()
        m = rng.random(L) < rng.choice([0.0, 0.01, 0.05])
        x[m] = A[rng.integers(0, 4, int(m.sum()))]
        recs.append(x)
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.arange(len(recs) + 1, dtype=np.uint64)
    with _lib.Context(0, 21, S, 42) as ctx:
        h, nh, _ = ctx.sketch_records(seq, rec_off, gro)
        assert (nh < S).any() and (nh == S).any() and (nh == 0).any()
        ctx.set_allpairs_path(ctx.AP_BAND, 50)
        c, d = ctx.allpairs(h, nh, want_denom=True)
        oc, od = oracle.allpairs(h, nh, S)
        assert np.array_equal(c, oc) and np.array_equal(d, od)
        # row segments of the family set, band path
        h, nh = family
        N = len(nh)
        dh = torch.from_numpy(h.view(np.int64)).cuda()
        dn = torch.from_numpy(nh.view(np.int32)).cuda()
        oc, _ = oracle.allpairs(h, nh, S, threads=8)
        full = np.zeros(N * (N - 1) // 2, np.uint16)

        def start(i):
            return i * N - i * (i + 1) // 2

        ctx.set_allpairs_path(ctx.AP_BAND, 200)
        for r0, r1 in zip([0, 3, 61, N - 2], [3, 61, N - 2, N]):
            n = start(min(r1, N - 1)) - start(r0)
            out = torch.zeros(n, dtype=torch.int16, device="cuda")
            ctx.allpairs_device(dh.data_ptr(), dn.data_ptr(), N, r0, r1, out.data_ptr(), None,
                                torch.cuda.current_stream().cuda_stream)
            full[start(r0):start(r0) + n] = out.cpu().numpy().view(np.uint16)
        assert np.array_equal(full, oc)


def test_allpairs_row_segments_and_merge_kernel(family, ctx1000):
    """Row-range sharding (the multi-GPU split) and the literal-merge kernel
    agree with the full triangle."""
    import torch
    h, nh = family
    N = len(nh)
    dh = torch.from_numpy(h.view(np.int64)).cuda()
    dn = torch.from_numpy(nh.view(np.int32)).cuda()
    full = np.zeros(N * (N - 1) // 2, np.uint16)
    oc, _ = oracle.allpairs(h, nh, S, threads=8)

    def start(i):
        return i * N - i * (i + 1) // 2

    bounds = [0, 1, 17, 64, 100, N - 2, N]
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        n = start(min(r1, N - 1)) - start(r0) if r0 < N - 1 else 0
        if n <= 0:
            continue
        out = torch.zeros(n, dtype=torch.int16, device="cuda")
        ctx1000.allpairs_device(dh.data_ptr(), dn.data_ptr(), N, r0, r1, out.data_ptr(), None,
                                torch.cuda.current_stream().cuda_stream)
        full[start(r0):start(r0) + n] = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(full, oc)
    out = torch.zeros(N * (N - 1) // 2, dtype=torch.int16, device="cuda")
    ctx1000.allpairs_device(dh.data_ptr(), dn.data_ptr(), N, 0, N, out.data_ptr(), None,
                            torch.cuda.current_stream().cuda_stream, merge=True)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), oc)


@pytest.mark.parametrize("screen", ["2", "1"])
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0, 0, 0]])
def test_condensed_allpairs_multi_device(family, devices, screen, monkeypatch):
    """In-process multi-device all-pairs (drephip_allpairs_rows per device on
    balanced row ranges, threads) assembles the same triangle, with partial
    sketches (denominators) too -- with the shared-hash screen off and forced
    on (each device screens its own row range)."""
    from drep_amd.d_cluster import condensed_allpairs
    monkeypatch.setenv("DREPHIP_AP_SCREEN", screen)
    h, nh = family
    oc, od = oracle.allpairs(h, nh, S, threads=8)
    c, d = condensed_allpairs(h, nh, S, devices)
    assert np.array_equal(c, oc) and (d == S).all()
    h2, nh2 = h.copy(), nh.copy()
    nh2[::7] = 500
    for i in range(0, len(nh2), 7):
        h2[i, 500:] = UMAX
    oc, od = oracle.allpairs(h2, nh2, S, threads=8)
    c, d = condensed_allpairs(h2, nh2, S, devices)
    assert np.array_equal(c, oc) and np.array_equal(d, od)


def test_split_launches_match_oracle(family, monkeypatch):
    """Every N-scaled launch is issued in pieces of < 2^32 work-items
    (kMaxLaunchItems; at N = 10^5 the all-pairs grid needs 5).  A tiny cap
    (DREPHIP_MAX_LAUNCH_ITEMS) forces dozens of pieces at test sizes: table,
    band and merge all-pairs, the sketch hash kernel and the synthetic
    generator must still match the oracle exactly."""
    import torch
    monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", "8192")
    h, nh = family
    N = len(nh)
    oc, _ = oracle.allpairs(h, nh, S, threads=8)
    with _lib.Context(0, 21, S, 42) as ctx:
        c, _ = ctx.allpairs(h, nh)                                   # table path
        assert np.array_equal(c, oc)
        ctx.set_allpairs_path(ctx.AP_BAND, 64)
        c, _ = ctx.allpairs(h, nh)
        assert np.array_equal(c, oc)
        dh = torch.from_numpy(h.view(np.int64)).cuda()
        dn = torch.from_numpy(nh.view(np.int32)).cuda()
        out = torch.zeros(N * (N - 1) // 2, dtype=torch.int16, device="cuda")
        ctx.allpairs_device(dh.data_ptr(), dn.data_ptr(), N, 0, N, out.data_ptr(), None,
                            torch.cuda.current_stream().cuda_stream, merge=True)
        assert np.array_equal(out.cpu().numpy().view(np.uint16), oc)
        # sketch + synth: 3 genomes of 300 kbp = ~30 tiles, 16 per piece
        n, L, seed, fam = 3, 300_000, 11, 2
        tile = _lib.tile_bases()
        P = _lib.padded_bases([L])
        codes = torch.zeros((tile + n * P) // 16, dtype=torch.int32, device="cuda")
        valid = torch.zeros((tile + n * P) // 32, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        ctx.synth_device(seed, 0, n, fam, L, codes.data_ptr(), valid.data_ptr(), st)
        hh = torch.zeros((n, S), dtype=torch.int64, device="cuda")
        nn = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx.sketch_device(codes.data_ptr(), valid.data_ptr(), np.array([tile + i * P for i in range(n)], np.uint64),
                          np.full(n, P, np.uint64), np.full(n, L - 20, np.uint64), n, hh.data_ptr(), nn.data_ptr(), st)
        torch.cuda.synchronize()
    oh, onh = oracle.sketch_synth(0, n, L, seed=seed, family_size=fam, threads=3)
    assert np.array_equal(hh.cpu().numpy().view(np.uint64), oh)
    assert np.array_equal(nn.cpu().numpy().view(np.uint32), onh)


# ---------------------------------------------------------------- drop-in
@pytest.mark.parametrize("gpus", [None, "0,0,0"])
def test_all_vs_all_MASH_dropin_reproduces_reference(golden, tmp_path, gpus):
    """all_vs_all_MASH on the reference's test genomes (Sakai from its cached
    .msh, as the reference's own sketch cache would) -> Mdb bit-identical to
    the reference's parse of its fixture MASH_table.tsv, then primary
    clustering identical to the reference's Cdb / linkage.  gpus="0,0,0" runs
    the multi-device path (sketch shards and all-pairs row ranges on three
    contexts, one host thread each) on the one device of the test box."""
    import json
    from drep_amd import d_cluster
    fas = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))
    gdir = tmp_path / "genomes"
    gdir.mkdir()
    locs = []
    for fa in fas:
        dst = gdir / os.path.basename(fa)[:-3]
        import gzip
        dst.write_bytes(gzip.open(fa).read())
        locs.append(str(dst))
    sakai = str(gdir / "Escherichia_coli_Sakai.fna")
    locs.append(sakai)
    Bdb = pd.DataFrame({"genome": [os.path.basename(x) for x in locs], "location": locs})
    wd = tmp_path / "wd"
    chunk = wd / "MASH_files" / "sketches" / "chunk_0"
    chunk.mkdir(parents=True)
    shutil.copy(os.path.join(golden, "MASH_files", "sketches", "Escherichia_coli_Sakai.fna.msh"),
                chunk / "Escherichia_coli_Sakai.fna.msh")
    Mdb = d_cluster.all_vs_all_MASH(Bdb, str(wd), processors=4, **({"gpus": gpus} if gpus else {}))
    meta = json.load(open(os.path.join(golden, "ref", "mdb_parsed_dtypes.json")))
    exp = pd.read_csv(os.path.join(golden, "ref", "mdb_parsed.csv"))
    assert len(Mdb) == 25
    assert {c: str(t) for c, t in Mdb.dtypes.items()} == meta["dtypes"]
    for g in ("genome1", "genome2"):
        assert list(Mdb[g].cat.categories) == meta["categories"][g]
        assert Mdb[g].cat.ordered
        assert list(Mdb[g].astype(str)) == list(exp[g])
    assert list(Mdb["dist"].to_numpy().view(np.uint32)) == meta["dist_bits"]
    assert list(Mdb["similarity"].to_numpy().view(np.uint32)) == meta["similarity_bits"]
    # reference layout: one chunk dir with 5 .msh + chunk_all.msh
    assert len(glob.glob(str(wd / "MASH_files" / "sketches" / "*"))) == 1
    assert len(glob.glob(str(wd / "MASH_files" / "sketches" / "*" / "*"))) == 6
    for alg in ("average", "single"):
        mdb = Mdb.copy()
        Cdb, ret = d_cluster.cluster_mash_database(mdb, clusterAlg=alg, P_ani=0.9)      # GPU linkage
        exp_c = pd.read_csv(os.path.join(golden, "ref", "cdb_%s.csv" % alg))
        assert Cdb.to_dict("list") == exp_c.to_dict("list")
        ref = Mdb.copy()
        ref["dist"] = 1 - ref["similarity"]
        pd.testing.assert_frame_equal(ret[1], ref.pivot(index="genome1", columns="genome2", values="dist"),
                                      check_exact=True)
        assert list(mdb["dist"].to_numpy().view(np.uint32)) == link_bits_after(golden, alg)
        link = json.load(open(os.path.join(golden, "ref", "linkage_%s.json" % alg)))
        got = [[float(v).hex() for v in row] for row in ret[0]]
        assert got == link["linkage"]


def link_bits_after(golden, alg):
    import json
    return json.load(open(os.path.join(golden, "ref", "linkage_%s.json" % alg)))["dist_bits_after"]


def _device_synth_sketches(N, L, fam, seed, s=S):
    """Sketches of the bench's synthetic genomes (on-device generator + the
    product sketch kernel; the generator and kernel are oracle-pinned above)."""
    import torch
    tile = _lib.tile_bases()
    P = _lib.padded_bases([L])
    with _lib.Context(0, 21, s, 42) as ctx:
        st = torch.cuda.current_stream().cuda_stream
        codes = torch.zeros((tile + N * P) // 16, dtype=torch.int32, device="cuda")
        valid = torch.zeros((tile + N * P) // 32, dtype=torch.int32, device="cuda")
        ctx.synth_device(seed, 0, N, fam, L, codes.data_ptr(), valid.data_ptr(), st)
        hh = torch.zeros((N, s), dtype=torch.int64, device="cuda")
        nn = torch.zeros(N, dtype=torch.int32, device="cuda")
        ctx.sketch_device(codes.data_ptr(), valid.data_ptr(), np.array([tile + i * P for i in range(N)], np.uint64),
                          np.full(N, P, np.uint64), np.full(N, L - 20, np.uint64), N, hh.data_ptr(), nn.data_ptr(), st)
        torch.cuda.synchronize()
    return hh.cpu().numpy().view(np.uint64), nn.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("method", ["average", "single", "complete", "weighted"])
def test_cluster_mash_database_gpu_equals_reference_steps(method):
    """dRep's own entry point on the GPU: cluster_mash_database (native pivot,
    drephip_linkage_square) on the Mdb all_vs_all_MASH builds for 10^3
    synthetic genomes (shuffled names) equals the reference's steps run
    literally -- in-place dist update, pandas pivot, squareform, scipy linkage,
    fcluster (d_cluster.py:445-459, 619-623): linkage_db, Z, Cdb and the
    updated dist column bit for bit."""
    import scipy.cluster.hierarchy as sch
    import scipy.spatial.distance as ssd
    from drep_amd import d_cluster
    N = 1000
    h, nh = _device_synth_sketches(N, 200_000, 25, 0xD2E9 + 3)
    with _lib.Context(0, 21, S, 42) as ctx:
        c, d = ctx.allpairs(h, nh)
    names = ["g%05d.fna" % i for i in np.random.default_rng(4).permutation(N)]
    Mdb = d_cluster.mdb_from_condensed(names, c, d, nh, S)
    ref = Mdb.copy()
    ref["dist"] = 1 - ref["similarity"]
    lp = ref.pivot(index="genome1", columns="genome2", values="dist")
    Z = sch.linkage(ssd.squareform(np.asarray(lp)), method=method)
    fcl = sch.fcluster(Z, 1 - 0.95, criterion="distance")
    Cdb, (Zg, ldb, args) = d_cluster.cluster_mash_database(Mdb, clusterAlg=method, P_ani=0.95)
    pd.testing.assert_frame_equal(ldb, lp, check_exact=True)
    assert type(ldb.index) is type(lp.index) and ldb.index.dtype == lp.index.dtype
    assert np.array_equal(Zg, Z), np.argwhere(Zg != Z)[:5]
    assert list(Cdb["primary_cluster"]) == list(fcl) and list(Cdb["genome"]) == list(lp.columns)
    assert np.array_equal(Mdb["dist"].to_numpy().view(np.uint32), ref["dist"].to_numpy().view(np.uint32))
    assert 1 < Cdb["primary_cluster"].nunique() < N
    assert args == {"linkage_method": method, "linkage_cutoff": 1 - 0.95, "comparison_algorithm": "MASH"}


def test_linkage_square_checks_like_scipy():
    """drephip_linkage_square raises squareform's / linkage's ValueErrors
    (asymmetric, nonzero diagonal, NaN, inf) with scipy's messages, and a
    -0.0 / +0.0 mirror pair or a float64 pivot still gives scipy's Z."""
    import scipy.cluster.hierarchy as sch
    import scipy.spatial.distance as ssd
    from drep_amd import d_cluster
    rng = np.random.default_rng(8)
    n = 300
    y = np.round(rng.random(n * (n - 1) // 2), 2).astype(np.float32)
    M = ssd.squareform(y)
    for method in ("average", "single"):
        want = sch.linkage(ssd.squareform(M), method=method)
        assert np.array_equal(d_cluster._square_linkage(M, method, 0), want)
        assert np.array_equal(d_cluster._square_linkage(M.astype(np.float64), method, 0),
                              sch.linkage(ssd.squareform(M.astype(np.float64)), method=method))
    M0 = M.copy()
    M0[3, 9] = np.float32(0.0)
    M0[9, 3] = np.float32(-0.0)
    assert np.array_equal(d_cluster._square_linkage(M0, "average", 0),
                          sch.linkage(ssd.squareform(M0), method="average"))
    cases = []
    A = M.copy(); A[4, 7] = np.float32(0.5); A[7, 4] = np.float32(0.25); cases.append(A)
    B = M.copy(); B[5, 5] = np.float32(0.1); cases.append(B)
    Cn = M.copy(); Cn[2, 6] = Cn[6, 2] = np.nan; cases.append(Cn)
    Ci = M.copy(); Ci[2, 6] = Ci[6, 2] = np.inf; cases.append(Ci)
    for X in cases:
        with pytest.raises(ValueError) as want:
            sch.linkage(ssd.squareform(X), method="average")
        with pytest.raises(ValueError) as got:
            d_cluster._square_linkage(X, "average", 0)
        assert str(got.value) == str(want.value)


def _dropin_bdb(golden, tmp_path):
    import gzip
    fas = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))
    gdir = tmp_path / "genomes"
    gdir.mkdir(exist_ok=True)
    locs = []
    for fa in fas:
        dst = gdir / os.path.basename(fa)[:-3]
        dst.write_bytes(gzip.open(fa).read())
        locs.append(str(dst))
    locs.append(str(gdir / "Escherichia_coli_Sakai.fna"))     # FASTA absent: its cached sketch is used
    return pd.DataFrame({"genome": [os.path.basename(x) for x in locs], "location": locs})


def test_all_vs_all_MASH_groupsize_and_no_kwargs_call(golden, tmp_path):
    """The reference's own checks of the boundary (tests/test_suite.py:635-666):
    25 rows, 0.01 < dist(YI6-1, TX0104) < 0.02, one chunk dir with 6 files by
    default and, with groupSize=2, 3 chunk dirs with 8 files; plus the
    no-kwargs call shape of compare_winners (drep/d_evaluate.py:67), which
    reuses the cached sketches and must return the same Mdb."""
    from drep_amd import d_cluster
    Bdb = _dropin_bdb(golden, tmp_path)
    sakai = os.path.join(golden, "MASH_files", "sketches", "Escherichia_coli_Sakai.fna.msh")

    def check(Mdb):
        assert len(Mdb) == 25
        db = Mdb[(Mdb['genome1'] == 'Enterococcus_faecalis_YI6-1.fna') &
                 (Mdb['genome2'] == 'Enterococcus_faecalis_TX0104.fa')]
        d = float(db['dist'].tolist()[0])
        assert 0.01 < d < 0.02

    wd = tmp_path / "wd_groups"
    (wd / "MASH_files" / "sketches" / "chunk_2").mkdir(parents=True)
    shutil.copy(sakai, wd / "MASH_files" / "sketches" / "chunk_2" / "Escherichia_coli_Sakai.fna.msh")
    Mdb2 = d_cluster.all_vs_all_MASH(Bdb, str(wd), groupSize=2)
    check(Mdb2)
    assert len(glob.glob(str(wd / "MASH_files" / "sketches" / "*"))) == 3
    assert len(glob.glob(str(wd / "MASH_files" / "sketches" / "*" / "*"))) == 8

    wd = tmp_path / "wd_default"
    (wd / "MASH_files" / "sketches" / "chunk_0").mkdir(parents=True)
    shutil.copy(sakai, wd / "MASH_files" / "sketches" / "chunk_0" / "Escherichia_coli_Sakai.fna.msh")
    Mdb1 = d_cluster.all_vs_all_MASH(Bdb, str(wd), MASH_sketch="1000", processors=2)     # CLI passes a str
    check(Mdb1)
    assert len(glob.glob(str(wd / "MASH_files" / "sketches" / "*"))) == 1
    assert len(glob.glob(str(wd / "MASH_files" / "sketches" / "*" / "*"))) == 6
    again = d_cluster.all_vs_all_MASH(Bdb, str(wd))          # compare_winners' call: no kwargs, cached sketches
    assert again.equals(Mdb1) and Mdb2.equals(Mdb1)


def test_errors_are_reported_not_hidden(ctx1000, tmp_path):
    """The reference ignores Mash's exit codes (drep/__init__.py:44-48); the
    C ABI returns them: unreadable inputs, bad sizes and bad devices raise with
    a message instead of producing missing or wrong rows."""
    with pytest.raises(_lib.DrepHipError, match="nonexistent"):
        ctx1000.sketch_files([str(tmp_path / "nonexistent.fna")])
    bad = tmp_path / "broken.fa.gz"
    bad.write_bytes(b"\x1f\x8b\x08\x00not really gzip")
    with pytest.raises(_lib.DrepHipError):
        ctx1000.sketch_files([str(bad)])
    with pytest.raises(_lib.DrepHipError):
        _lib.Context(device=0, k=21, s=0, seed=42)
    assert _lib.max_sketch() == 32767          # uint16 counts; 0xFFFF stays an impossible count
    with pytest.raises(_lib.DrepHipError, match=r"sketch size must be in 1\.\.32767"):
        _lib.Context(device=0, k=21, s=_lib.max_sketch() + 1, seed=42)
    with pytest.raises(_lib.DrepHipError):
        _lib.Context(device=1 << 20, k=21, s=1000, seed=42)
    h = np.full((2, S), UMAX, dtype=np.uint64)
    with pytest.raises(_lib.DrepHipError):
        ctx1000.allpairs(h, np.array([S + 1, 0], np.uint32))


def test_device_calls_follow_callers_stream(ctx1000):
    """Device-pointer calls run on the caller's stream: a synth issued right
    after torch's (asynchronous) zero-fill of a multi-GB buffer on torch's
    default stream (handle 0) must not be overwritten by that fill."""
    import torch
    n, L = 1200, 5_000_000               # ~2.3 GB packed: the fill outlasts a launch
    tile = _lib.tile_bases()
    P = _lib.padded_bases([L])
    total = tile + n * P
    st = torch.cuda.current_stream().cuda_stream
    codes = torch.zeros(total // 16, dtype=torch.int32, device="cuda")
    valid = torch.zeros(total // 32, dtype=torch.int32, device="cuda")
    ctx1000.synth_device(1, 0, n, 100, L, codes.data_ptr(), valid.data_ptr(), st)
    torch.cuda.synchronize()
    for g in (0, n // 2, n - 1):
        w0 = (tile + g * P) // 32
        assert int((valid[w0:w0 + L // 32] != -1).sum()) == 0, g
    del codes, valid
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_sketch_layout_cache_follows_layout_changes(ctx1000):
    """The tile table is cached on the context between calls with the same
    layout; a call with a different layout (same genome count) must not reuse
    it.  Sketch A B C, then the same genomes listed as C A B, then A B C again."""
    import torch
    n, L, seed = 3, 300_000, 21
    tile = _lib.tile_bases()
    P = _lib.padded_bases([L])
    total = tile + n * P
    st = torch.cuda.current_stream().cuda_stream
    codes = torch.zeros(total // 16, dtype=torch.int32, device="cuda")
    valid = torch.zeros(total // 32, dtype=torch.int32, device="cuda")
    ctx1000.synth_device(seed, 0, n, 1, L, codes.data_ptr(), valid.data_ptr(), st)
    oh, onh = oracle.sketch_synth(0, n, L, seed=seed, family_size=1, threads=3)

    def run(order):
        off = np.array([tile + i * P for i in order], np.uint64)
        h = torch.zeros((n, S), dtype=torch.int64, device="cuda")
        nh = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx1000.sketch_device(codes.data_ptr(), valid.data_ptr(), off, np.full(n, P, np.uint64),
                              np.full(n, L - 20, np.uint64), n, h.data_ptr(), nh.data_ptr(), st)
        torch.cuda.synchronize()
        return h.cpu().numpy().view(np.uint64), nh.cpu().numpy().view(np.uint32)

    for order in ([0, 1, 2], [2, 0, 1], [2, 0, 1], [0, 1, 2]):
        h, nh = run(order)
        assert np.array_equal(h, oh[order]) and np.array_equal(nh, onh[order]), order


# ------------------------------------------------------ primary clustering
@pytest.mark.parametrize("method", ["single", "complete", "average", "weighted"])
@pytest.mark.parametrize("n,kind", [(2, "ties"), (3, "ties"), (17, "ties"), (257, "ties"), (300, "cont"),
                                    (64, "equal"), (400, "fewvals"), (1500, "mash"), (4500, "mash"),
                                    (2100, "ties"), (700, "above1"), (300, "negative")])
def test_gpu_linkage_matches_scipy(method, n, kind):
    """drephip_linkage == scipy.cluster.hierarchy.linkage bit for bit, with
    Mash-like ties (a few distinct distances, many 1.0), continuous values,
    all-equal distances, a few values whose Lance-Williams averages round
    (fewvals), family structure with 1.0 between families (mash), values
    above 1.0 and negative values (no sparse form; scipy accepts both): the dense GPU path at three grid densities of
    the chain-step kernel (16 entries per lane: several passes), and the
    automatic choice (the sparse path wherever no value exceeds 1.0)."""
    import scipy.cluster.hierarchy as sch
    rng = np.random.default_rng(n * 31 + len(method))
    m = n * (n - 1) // 2
    if kind == "ties":
        vals = np.array([0.0, 0.00243596, 0.0157245, 0.0157245, 0.05, 0.1, 0.243761, 1.0, 1.0, 1.0])
        y = vals[rng.integers(0, len(vals), m)]
    elif kind == "cont":
        y = rng.random(m)
    elif kind == "fewvals":
        y = np.array([0.1, 0.3, 0.7])[rng.integers(0, 3, m)]
    elif kind == "mash":
        fam = rng.integers(0, max(1, n // 40), n)
        iu = np.triu_indices(n, 1)
        same = fam[iu[0]] == fam[iu[1]]
        y = np.ones(m)
        y[same] = np.round(rng.random(int(same.sum())) * 0.2, 3)
    elif kind == "above1":
        y = rng.random(m) * 1.5
    elif kind == "negative":
        y = rng.random(m) - 0.3
    else:
        y = np.full(m, 0.5)
    Zs = sch.linkage(y, method=method)
    # grid densities of the chain-step kernel: the default (one-wave
    # workgroups up to n = 16384), 128/256-lane workgroups at 1, 4 and 16
    # entries per lane, one-wave workgroups with several entries per lane
    variants = [(None, {}), ("4", {})]
    if n <= 2000:
        variants += [("1", {}), ("16", {}), ("2", {"DREPHIP_LINK_WG": "64"}), ("8", {"DREPHIP_LINK_WG": "64"})]
    # the matrix compacted as clusters retire, at many chain states: short
    # graph batches, the merge count read after each, down to 4 active clusters
    variants += [(None, {"DREPHIP_LINK_COMPACT_MIN": "4", "DREPHIP_LINK_BATCH": "16", "DREPHIP_LINK_POLL": "1"}),
                 (None, {"DREPHIP_LINK_COMPACT_MIN": "4", "DREPHIP_LINK_BATCH": "6", "DREPHIP_LINK_POLL": "1"})]
    if n <= 2000:
        variants += [("2", {"DREPHIP_LINK_COMPACT_MIN": "4", "DREPHIP_LINK_BATCH": "10", "DREPHIP_LINK_POLL": "1"})]

    for per_lane, env in variants:
        if per_lane is not None:
            os.environ["DREPHIP_LINK_PER_LANE"] = per_lane
        os.environ.update(env)
        try:
            with _lib.Context(0, 21, S, 42) as ctx:
                ctx.set_linkage_path(ctx.LINK_DENSE)
                Z = ctx.linkage(y, method)
                assert not ctx.linkage_info()["sparse"]
        finally:
            for k in ["DREPHIP_LINK_PER_LANE"] + list(env):
                os.environ.pop(k, None)
        assert Z.shape == Zs.shape
        assert np.array_equal(Z, Zs), (per_lane, env, np.argwhere(Z != Zs)[:5])
    with _lib.Context(0, 21, S, 42) as ctx:
        Z = ctx.linkage(y, method)
        if kind in ("mash", "above1", "negative"):      # small components / no sparse form
            assert ctx.linkage_info()["sparse"] == (kind == "mash")
        assert np.array_equal(Z, Zs), ("auto", np.argwhere(Z != Zs)[:5])
        ctx.set_linkage_path(ctx.LINK_SPARSE)
        if kind in ("above1", "negative"):
            with pytest.raises(_lib.DrepHipError, match="above 1.0, below 0"):
                ctx.linkage(y, method)
        else:
            Z = ctx.linkage(y, method)
            assert ctx.linkage_info()["sparse"]
            assert np.array_equal(Z, Zs), ("sparse", np.argwhere(Z != Zs)[:5])


@pytest.mark.parametrize("method", ["complete", "average", "weighted"])
def test_gpu_linkage_compaction_runs(method, capfd, monkeypatch):
    """The compaction (linkage.hip, k_lk_cmp_rank) happens where it should --
    each time at most half the matrix's rows are active, not below
    DREPHIP_LINK_COMPACT_MIN -- and Z stays scipy's; off with
    DREPHIP_LINK_COMPACT=0."""
    import re
    import scipy.cluster.hierarchy as sch
    n = 3000
    rng = np.random.default_rng(7)
    fam = rng.integers(0, 60, n)
    iu = np.triu_indices(n, 1)
    y = np.where(fam[iu[0]] == fam[iu[1]], np.round(rng.random(len(iu[0])) * 0.2, 3), 1.0)
    Zs = sch.linkage(y, method=method)
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    monkeypatch.setenv("DREPHIP_LINK_BATCH", "32")
    monkeypatch.setenv("DREPHIP_LINK_POLL", "1")
    for cmin, want in (("100", range(4, 6)), ("2", range(6, 13))):
        monkeypatch.setenv("DREPHIP_LINK_COMPACT_MIN", cmin)
        capfd.readouterr()
        with _lib.Context(0, 21, S, 42) as ctx:
            ctx.set_linkage_path(ctx.LINK_DENSE)
            Z = ctx.linkage(y, method)
        err = capfd.readouterr().err
        got = int(re.search(r"compactions (\d+)", err).group(1))
        assert got in want, (cmin, got, err[-500:])
        assert np.array_equal(Z, Zs), (cmin, np.argwhere(Z != Zs)[:5])
    monkeypatch.setenv("DREPHIP_LINK_COMPACT", "0")
    capfd.readouterr()
    with _lib.Context(0, 21, S, 42) as ctx:
        ctx.set_linkage_path(ctx.LINK_DENSE)
        Z = ctx.linkage(y, method)
    assert "compactions 0" in capfd.readouterr().err
    assert np.array_equal(Z, Zs)


@pytest.mark.parametrize("path", ["auto", "dense", "sparse"])
@pytest.mark.parametrize("method", ["average", "single", "complete", "weighted"])
def test_cluster_mash_condensed_gpu_equals_reference_path(family, ctx1000, method, path, monkeypatch):
    """Primary clustering from device-resident all-pairs counts (GPU linkage:
    the pairs below 1.0 extracted on the device and replayed on the host --
    the automatic choice here -- or the dense n x n chain) gives the reference
    path's linkage matrix and Cdb (scipy on the float32 Mdb distances), with
    names in a shuffled order."""
    from drep_amd.d_cluster import CondensedMash, cluster_mash_condensed
    monkeypatch.setenv("DREPHIP_LINK_PATH", path)
    h, nh = family
    N = len(nh)
    c, d = ctx1000.allpairs(h, nh)
    rng = np.random.default_rng(5)
    names = ["g%04d.fna" % i for i in rng.permutation(N)]
    cm = CondensedMash(names, names, c, d, nh, np.full(N, 400_000, np.uint64), S)
    cdb_cpu, (z_cpu, _, _) = cluster_mash_condensed(cm, clusterAlg=method, P_ani=0.95, gpu=None)
    cdb_gpu, (z_gpu, _, _) = cluster_mash_condensed(cm, clusterAlg=method, P_ani=0.95, gpu=0)
    assert np.array_equal(z_gpu, z_cpu)
    assert cdb_gpu.equals(cdb_cpu)
    assert cdb_gpu['primary_cluster'].nunique() > 1


@pytest.mark.parametrize("partial", [False, True])
def test_linkage_counts_device_sparse_vs_dense(ctx1000, partial):
    """The two linkage paths on device counts agree bit for bit with each other
    and with scipy: families of 1-60 genomes (pairs below 1.0 only inside a
    family), count ties, shuffled rows (perm), partial sketches (a denominator
    per pair), and the pair list reported by drephip_last_linkage_info."""
    import torch
    import scipy.cluster.hierarchy as sch
    from drep_amd.d_cluster import linkage_tables, _linkage_values
    rng = np.random.default_rng(11 + partial)
    n = 1500
    fam = np.repeat(np.arange(200), rng.integers(1, 60, 200))[:n]
    rng.shuffle(fam)
    iu = np.triu_indices(n, 1)
    same = fam[iu[0]] == fam[iu[1]]
    common = np.zeros(len(same), np.uint16)
    common[same] = rng.integers(1, 40, int(same.sum())) * 20          # many equal counts
    denom = np.full(len(same), S, np.uint16)
    if partial:
        denom = rng.choice(np.array([600, 800, S], np.uint16), len(same))
        common = np.minimum(common, denom)
    perm = rng.permutation(n).astype(np.uint32)
    lut, off = linkage_tables(np.unique(denom), S)
    st = torch.cuda.current_stream().cuda_stream
    d_c = torch.from_numpy(common.view(np.int16)).cuda()
    d_d = torch.from_numpy(denom.view(np.int16)).cuda() if partial else None
    # scipy on the same matrix, rows in perm order
    D = np.zeros((n, n))
    v = _linkage_values(common, denom)
    D[perm[iu[0]], perm[iu[1]]] = v
    D = D + D.T
    from scipy.spatial.distance import squareform
    y = squareform(D, checks=False)
    for method in ("average", "single", "complete", "weighted"):
        Zs = sch.linkage(y, method=method)
        got = {}
        for path in (ctx1000.LINK_SPARSE, ctx1000.LINK_DENSE):
            ctx1000.set_linkage_path(path)
            got[path] = ctx1000.linkage_counts_device(d_c.data_ptr(), None if d_d is None else d_d.data_ptr(), n,
                                                      perm, lut, off, method, st)
            info = ctx1000.linkage_info()
            assert info["sparse"] == (path == ctx1000.LINK_SPARSE)
            if info["sparse"]:
                assert info["pairs"] == int((common > 0).sum())
        ctx1000.set_linkage_path(ctx1000.LINK_AUTO)
        assert np.array_equal(got[ctx1000.LINK_SPARSE], Zs), method
        assert np.array_equal(got[ctx1000.LINK_DENSE], Zs), method


def test_sketch_device_async_wait(ctx1000):
    """drephip_sketch_device_async queues the sketch without reading its
    threshold status back; all-pairs queued behind it on the same stream sees
    the final sketches, and drephip_sketch_wait reruns the call when a genome
    needs another threshold round (forced here by overstating its k-mer count,
    which seeds the threshold ~1000x too low)."""
    import torch
    n, L, fam, seed = 4, 300_000, 2, 5
    tile = _lib.tile_bases()
    P = _lib.padded_bases([L])
    codes = torch.zeros((tile + n * P) // 16, dtype=torch.int32, device="cuda")
    valid = torch.zeros((tile + n * P) // 32, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx1000.synth_device(seed, 0, n, fam, L, codes.data_ptr(), valid.data_ptr(), st)
    off = np.array([tile + i * P for i in range(n)], np.uint64)
    pad = np.full(n, P, np.uint64)
    oh, onh = oracle.sketch_synth(0, n, L, seed=seed, family_size=fam)
    oc, _ = oracle.allpairs(oh, onh, S)

    def run(nk, wait=True, sync_after=False):
        hashes = torch.zeros((n, S), dtype=torch.int64, device="cuda")
        nhash = torch.zeros(n, dtype=torch.int32, device="cuda")
        common = torch.zeros(n * (n - 1) // 2, dtype=torch.int16, device="cuda")
        ctx1000.sketch_device_async(codes.data_ptr(), valid.data_ptr(), off, pad, nk, n,
                                    hashes.data_ptr(), nhash.data_ptr(), st)
        if sync_after:       # a sketch call before the wait is refused; the pending check is kept
            with pytest.raises(_lib.DrepHipError, match="pending"):
                ctx1000.sketch_device(codes.data_ptr(), valid.data_ptr(), off, pad, nk, n,
                                      hashes.data_ptr(), nhash.data_ptr(), st)
            with pytest.raises(_lib.DrepHipError, match="pending"):
                ctx1000.sketch_device_async(codes.data_ptr(), valid.data_ptr(), off, pad, nk, n,
                                            hashes.data_ptr(), nhash.data_ptr(), st)
        ctx1000.allpairs_device(hashes.data_ptr(), nhash.data_ptr(), n, 0, n, common.data_ptr(), None, st)
        redone = ctx1000.sketch_wait() if wait else None
        if redone:
            ctx1000.allpairs_device(hashes.data_ptr(), nhash.data_ptr(), n, 0, n, common.data_ptr(), None, st)
        torch.cuda.synchronize()
        return (hashes.cpu().numpy().view(np.uint64), nhash.cpu().numpy().view(np.uint32),
                common.cpu().numpy().view(np.uint16), redone)

    good = np.full(n, L - 20, np.uint64)
    h, nh, c, redone = run(good)
    assert redone is False
    assert np.array_equal(nh, onh) and np.array_equal(h, oh) and np.array_equal(c, oc)
    bad = good.copy()
    bad[1] *= 1000
    h, nh, c, redone = run(bad)
    assert redone is True
    assert np.array_equal(nh, onh) and np.array_equal(h, oh) and np.array_equal(c, oc)
    h, nh, c, redone = run(bad, sync_after=True)
    assert redone is True
    assert np.array_equal(h, oh) and np.array_equal(c, oc)
    assert ctx1000.sketch_wait() is False          # nothing pending


def test_linkage_counts_device_rejects_missing_tables(ctx1000):
    """drephip_linkage_counts_device refuses a denominator with no distance
    table and a count above its denominator instead of reading outside the
    table (device-side check)."""
    import torch
    from drep_amd.d_cluster import linkage_tables
    n = 6
    c = torch.from_numpy(np.arange(n * (n - 1) // 2, dtype=np.int16) * 10).cuda()
    d_full = torch.full((n * (n - 1) // 2,), S, dtype=torch.int16, device="cuda")
    perm = np.arange(n, dtype=np.uint32)
    lut, off = linkage_tables(np.array([S]), S)
    st = torch.cuda.current_stream().cuda_stream
    Z = ctx1000.linkage_counts_device(c.data_ptr(), None, n, perm, lut, off, "average", st)
    Z2 = ctx1000.linkage_counts_device(c.data_ptr(), d_full.data_ptr(), n, perm, lut, off, "average", st)
    assert np.array_equal(Z, Z2) and Z.shape == (n - 1, 4)
    lut7, off7 = linkage_tables(np.array([700]), S)          # no table for s
    with pytest.raises(_lib.DrepHipError, match="lut_off"):
        ctx1000.linkage_counts_device(c.data_ptr(), None, n, perm, lut7, off7, "average", st)
    d_bad = d_full.clone()
    d_bad[3] = 700                                           # denominator without a table
    with pytest.raises(_lib.DrepHipError, match="denominator"):
        ctx1000.linkage_counts_device(c.data_ptr(), d_bad.data_ptr(), n, perm, lut, off, "average", st)
    d_small = torch.full_like(d_full, 700)
    c_big = c.clone()
    c_big[2] = 701                                           # count above its denominator
    with pytest.raises(_lib.DrepHipError, match="exceeds"):
        ctx1000.linkage_counts_device(c_big.data_ptr(), d_small.data_ptr(), n, perm, lut7, off7, "average", st)


_ADVERSE_SCRIPT = r"""
import json, os, sys
import numpy as np
import scipy.cluster.hierarchy as sch
sys.path.insert(0, os.getcwd())
from drep_amd import _lib
out = {"build": _lib.build_id(), "cases": []}
rng = np.random.default_rng(17)
for n, fams in ((300, 12), (3000, 60)):
    fam = rng.integers(0, fams, n)
    iu = np.triu_indices(n, 1)
    y = np.where(fam[iu[0]] == fam[iu[1]], np.round(rng.random(len(iu[0])) * 0.2, 3), 1.0)
    for method in ("single", "complete", "average", "weighted"):
        Zs = sch.linkage(y, method=method)
        for wg in ("64", "256"):
            if method == "single" and wg == "64":
                continue
            os.environ["DREPHIP_LINK_WG"] = wg
            with _lib.Context(0, 21, 1000, 42) as ctx:
                ctx.set_linkage_path(ctx.LINK_DENSE)
                Z = ctx.linkage(y, method)
            out["cases"].append({"n": n, "method": method, "wg": wg, "equal": bool(np.array_equal(Z, Zs))})
print(json.dumps(out))
"""


@pytest.mark.parametrize("order", ["even", "odd"])
def test_linkage_adverse_workgroup_order(order):
    """The chain step, MST step and compaction kernels rest on "no workgroup
    reads what another workgroup of the same launch writes" (DESIGN 4.4,
    producer/consumer table).  Under a debug build whose even (odd) workgroups
    sleep ~14 us before their loads -- every other workgroup of the launch has
    stored by then -- Z must still be scipy's, for all four methods, one-wave
    and 256-lane step workgroups, with compactions at many chain states.  The
    variant libraries are built by __graft_entry__.build() (tools/build_ab.sh,
    EXTRA=-DDREPHIP_LK_ADVERSE=1/2) and run in a child process."""
    import json
    import subprocess
    import sys
    lib = os.path.join(ROOT, "drep_amd", "lib_ab", "adverse_" + order, "libdrephip.so")
    if not os.path.exists(lib):
        pytest.skip("adverse-order build missing (run __graft_entry__.build())")
    env = dict(os.environ, DREPHIP_LIB=lib, DREPHIP_LINK_BATCH="32", DREPHIP_LINK_POLL="1",
               DREPHIP_LINK_COMPACT_MIN="100")
    r = subprocess.run([sys.executable, "-c", _ADVERSE_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "DREPHIP_LK_ADVERSE=%d" % (1 if order == "even" else 2) in res["build"].get("extra", "")
    assert len(res["cases"]) == 14
    bad = [c for c in res["cases"] if not c["equal"]]
    assert not bad, bad
