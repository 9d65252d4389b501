"""Device FASTA ingest (drep_amd/csrc/ingest_device.hip) where its small tests
do not reach: k_fasta_tile_scan once a lane of its one 512-lane workgroup walks
more than one text tile (calls of 512, 513, 1024 and 1025 tiles, with file
starts, empty files, all four entry states and the '+' flag placed on purpose
relative to the lanes' chunks), the three tiled kernels issued in pieces
(DREPHIP_MAX_LAUNCH_ITEMS), and k_valid_kmers on bitmaps designed around its
word, lane and chunk edges for k from 1 to 32.  Every case goes through
ingest_cases._check_all (the oracle's kseq plus the numpy layout, the host
packer, and a k-mer count taken from the bitmap's run lengths) and asserts
first, from the sizes of its own inputs, that it has the shape it is there for."""
import re

import numpy as np
import pytest

import oracle
from drep_amd import _lib
from ingest_cases import K, S, _check_all, _device_pack, _rand_seq, _wrap

pytestmark = pytest.mark.gpu
SCAN_WG = 512                           # kScanWG: lanes of the scan kernel's one workgroup
CAP_ITEMS = "2048"                      # DREPHIP_MAX_LAUNCH_ITEMS: 8 workgroups of 256 lanes per dispatch
ALL_ONES = 0xFFFFFFFF


def _ntiles(text, T):
    return (len(text) + T - 1) // T


def _per(ntiles):
    """Tiles a lane of the scan kernel walks in a call of `ntiles` tiles."""
    return (ntiles + SCAN_WG - 1) // SCAN_WG


def _sized(rng, n, name=b"exact"):
    """A FASTA file of exactly n >= 16 bytes: wrapped lines of ACGT with some N."""
    assert n >= 16
    t = b">" + name + b"\n" + _wrap(_rand_seq(rng, n, b"ACGTACGTN"), 80)
    t = t[:n - 1] + b"\n"
    assert len(t) == n
    return t


def _genome(rng, n, T):
    """A wrapped multi-record genome with some N, of exactly n text tiles."""
    parts, size, i = [], 0, 0
    while size < n * T:
        parts.append(b">contig_%d some description\n" % i + _wrap(_rand_seq(rng, 60000 + 997 * i, b"ACGTACGTACGTACGTN"), 70))
        size += len(parts[-1])
        i += 1
    t = b"".join(parts)[:n * T - 41]
    assert _ntiles(t, T) == n and t.count(b">") >= 1
    return t


class _Call:
    """The files of one pack call in order, with each one's first tile and tile
    count, its expected status and (where not the default) its region size."""

    def __init__(self, T, per, seed):
        self.T, self.per, self.rng = T, per, np.random.default_rng(seed)
        self.texts, self.status, self.caps, self.first, self.tiles, self.at = [], [], {}, [], [], 0

    def add(self, text, status=0):
        self.texts.append(text)
        self.status.append(status)
        self.first.append(self.at)
        self.tiles.append(_ntiles(text, self.T))
        self.at += self.tiles[-1]
        return len(self.texts) - 1

    def plain(self, n):
        """A spacer: a plain FASTA file of n tiles."""
        return self.add(_sized(self.rng, n * self.T - 100 - 7 * n))

    def align(self, pos):
        """Spacer so that the next file's first tile is tile `pos` of a lane's chunk."""
        n = (pos - self.at) % self.per
        if n:
            self.plain(n)
        assert self.at % self.per == pos

    def pos(self, f):
        return self.first[f] % self.per

    def chunk(self, f):
        return self.first[f] // self.per

    def starts_in_chunk(self, l):
        return sum(1 for f in range(len(self.texts)) if self.tiles[f] and self.first[f] // self.per == l)

    def inner_chunks(self, f):
        """Byte offsets in file f of the lane chunks that lie wholly inside it,
        are full of its text and do not hold its first tile: chunks entered
        mid-file and left mid-file."""
        T, p = self.T, self.per
        a, b = self.first[f], self.first[f] + self.tiles[f]
        offs = [(l * p - a) * T for l in range(a // p + 1, b // p)]
        return [o for o in offs if o + p * T <= len(self.texts[f])]

    def region_caps(self):
        return [self.caps.get(f, _lib.padded_bases([len(t)])) for f, t in enumerate(self.texts)]


def _edge_set(c):
    """Section (b): the files that put each branch of the scan kernel at a known
    place relative to the lanes' chunks [l * per, (l + 1) * per), appended to
    call `c`; every placement is asserted here.  Sizes depend on c.per and on
    c.at % c.per alone."""
    T, p, rng = c.T, c.per, c.rng
    tile = _lib.tile_bases()
    q = lambda n: _rand_seq(rng, n, b"ACGTACGTN")                     # noqa: E731
    long = 3 * p * T

    # ---- a chunk wholly inside one entry state
    t = b"x" * (long + T // 2) + b">h\n" + q(50) + b"\n"
    f = c.add(t)                                                      # HUNT
    assert [o for o in c.inner_chunks(f) if t[o:o + p * T] == b"x" * (p * T)]
    t = b">" + b"h" * (long + 5) + b"\n" + q(90) + b"\n>b\nGG\n"
    f = c.add(t)                                                      # HDR
    assert t.index(b"\n") > long and [o for o in c.inner_chunks(f) if o + p * T <= t.index(b"\n")]
    t = b">a\n" + q(long + 5) + b"\n"
    f = c.add(t)                                                      # SEQ
    assert [o for o in c.inner_chunks(f) if o > 3 and b"\n" not in t[o:o + p * T]]
    t = b">" + b"s" * 62 + b"\n" + b"".join(q(63) + b"\n" for _ in range((long + T // 2) // 64))
    f = c.add(t)                                                      # START: every tile begins a line
    assert T % 64 == 0 and c.inner_chunks(f)
    assert all(t[o - 1:o] == b"\n" for o in c.inner_chunks(f))
    assert all(t[j * T - 1:j * T] == b"\n" for j in range(1, c.tiles[f]))

    # ---- file starts
    c.align(0)
    f = c.plain(2)
    assert c.pos(f) == 0                                              # first tile of a chunk
    c.align(p - 1)
    f = c.plain(2)
    assert c.pos(f) == p - 1 and c.tiles[f] == 2                      # last tile of a chunk, and on into the next
    if p >= 3:
        c.align(1)
        f = c.plain(3)
        assert 0 < c.pos(f) < p - 1                                   # a middle tile
        c.align(0)
        fs = [c.add(_sized(rng, T)), c.add(b">one\nACGTTGCAACGTTGCAACGTTGCAAC\n"), c.add(_sized(rng, T - 1))]
        assert [c.tiles[f] for f in fs] == [1, 1, 1] and c.starts_in_chunk(c.chunk(fs[0])) == 3
    c.align(0)
    f0 = c.plain(2 * p - 2)                                           # ends so that two tiles of a chunk are left
    fs = [c.add(_sized(rng, T - 17)), c.add(_sized(rng, 4000))]
    assert c.tiles[f0] == 2 * p - 2 and c.pos(fs[0]) == p - 2 and c.chunk(fs[0]) == c.chunk(fs[1])
    assert c.starts_in_chunk(c.chunk(fs[0])) == 2
    # an empty file between two files that start in one chunk
    c.align(0)
    fs = [c.add(_sized(rng, T - 7)), c.add(b""), c.add(_sized(rng, 300))]
    assert c.chunk(fs[0]) == c.chunk(fs[2]) and c.tiles[fs[1]] == 0 and c.first[fs[1]] == c.first[fs[2]]
    # a file that ends inside a header, then one that starts with no header:
    # the boundary inside a chunk, then at a chunk edge
    ends_in_hdr = b">a\n" + q(40) + b"\n>a header that the file ends in"
    no_hdr = q(30) + b"\n>b\n" + q(60) + b"\n"
    c.align(0)
    fa, fb = c.add(ends_in_hdr), c.add(no_hdr)
    assert c.chunk(fa) == c.chunk(fb) and c.first[fb] == c.first[fa] + 1
    c.align(p - 1)
    fa, fb = c.add(ends_in_hdr), c.add(no_hdr)
    assert c.pos(fb) == 0 and c.first[fb] == c.first[fa] + 1 and c.chunk(fb) == c.chunk(fa) + 1

    # ---- the '+' bit across chunks
    # '+' in the first tile, 3 per more tiles at the least, and the next file starts mid-chunk
    n = 3 * p + 1
    while (c.at + n) % p != 1:
        n += 1
    t = (b">f\nACGT\n+\nIIII\n>g\n" + _wrap(q(n * T), 70))[:n * T - 50] + b"\n"
    f = c.add(t, status=1)
    assert t.index(b"\n+") < T and t.count(b"\n+") == 1 and c.tiles[f] == n >= 3 * p + 1
    g = c.add(_sized(rng, T - 100))
    assert c.pos(g) != 0 and c.first[g] == c.first[f] + n             # g shares its chunk with f's last tile
    # the only '+' line in the last tile, 3 per tiles or more after the start
    t = (b">f\n" + _wrap(q(long + 2 * T), 70))[:long + T + 99] + b"\n" + b"+\n" + b"I" * 30 + b"\n"
    f = c.add(t, status=1)
    assert t.count(b"\n+") == 1 and (t.index(b"\n+") + 1) // T == c.tiles[f] - 1 >= 3 * p
    # '+' inside header lines and in the middle of sequence lines only
    t = b">h + plus +\n" + b"".join((b">r+ +x\n" if i % 9 == 8 else b"") + q(30) + b"+" + q(29) + b"\n"
                                    for i in range(2 * p * T // 61))
    f = c.add(t)
    assert b"\n+" not in t and t.count(b"+") > 2 * p * T // 61 and c.tiles[f] >= 2 * p - 1
    # a region one tile too small (status 2) between two packed files in the same chunks
    c.align(0)
    fl = c.add(_sized(rng, T - 33))
    body = _wrap(_rand_seq(rng, tile + 5000), 70)
    n = _ntiles(b">big \n" + body, T)
    while (c.at + n) % p == 0:
        n += 1
    t = b">big " + b"h" * ((n - _ntiles(b">big \n" + body, T)) * T) + b"\n" + body
    f = c.add(t, status=2)
    c.caps[f] = tile                                                  # its padded span is two tiles
    fr = c.add(_sized(rng, 2000))
    assert c.tiles[f] == n and c.chunk(fl) == c.chunk(f) and c.pos(fr) != 0 and c.first[fr] == c.first[f] + n


def _scan_call(T, ntiles, filler_first, seed=21):
    """Section (a): the edge set and a filler genome in a call of exactly
    `ntiles` tiles, an empty file first and last.  At 512 tiles (one tile per
    lane) the edge set is laid out for chunks of two."""
    per = _per(ntiles)
    layout = max(per, 2)
    probe = _Call(T, layout, seed)
    _edge_set(probe)
    E = probe.at
    c = _Call(T, layout, seed)
    c.add(b"")
    rng = np.random.default_rng(seed + 1)
    if filler_first:
        tail = (ntiles - E) % layout
        c.add(_genome(rng, ntiles - E - tail, T))
        assert c.at % layout == 0
        _edge_set(c)
        if tail:
            c.plain(tail)
    else:
        _edge_set(c)
        c.add(_genome(rng, ntiles - E, T))
    c.add(b"")
    assert c.at == ntiles == sum(_ntiles(t, T) for t in c.texts)
    assert c.tiles[0] == 0 and c.tiles[-1] == 0
    return c


# ------------------------------------------------------------------ 1a, 1b
@pytest.mark.parametrize("filler_first", [True, False], ids=["filler_first", "filler_last"])
@pytest.mark.parametrize("ntiles,per,busy", [(512, 1, 512), (513, 2, 257), (1024, 2, 512), (1025, 3, 342)])
def test_scan_chunk_boundaries(ctx1000, tmp_path, ntiles, per, busy, filler_first):
    T = _lib.text_tile_bytes()
    c = _scan_call(T, ntiles, filler_first)
    assert _per(c.at) == per and (c.at + per - 1) // per == busy      # lanes that have a tile
    assert c.per == max(per, 2)                                       # the edge set's placements hold for this per
    if ntiles == 513:
        assert c.at - 256 * per == 1                                  # lane 256 has one tile, lanes 257-511 none
    if filler_first:
        assert c.first[2] >= c.at - c.first[2]                        # the edge set sits at the high lanes
    else:
        assert c.first[-2] < 0.3 * c.at                               # ... at the low lanes
    _check_all(ctx1000, c.texts, tmp_path, "scan", want_status=c.status, caps=c.region_caps())


# ------------------------------------------------------------------ 1c
def _many_texts(T):
    """About 1100 files of one tile each, lengths from 1 to T and a few of one
    byte, and every 7th file of the call empty; most hold 21 to 900 bases in one to three
    records, behind junk before the first header and a long header line."""
    rng = np.random.default_rng(33)
    q = lambda n: _rand_seq(rng, n, b"ACGTACGTACGTN")                 # noqa: E731
    texts = []
    for i in range(1288):
        if i % 7 == 6:
            texts.append(b"")
            continue
        if i % 97 == 5:
            texts.append((b">", b"\n", b"A")[i % 3])
            continue
        n = T if i % 50 == 0 else int(rng.integers(1, T + 1))
        nb = int(rng.integers(21, 901))
        w = int(rng.integers(20, 120))
        cuts = np.sort(rng.integers(0, nb + 1, int(rng.integers(0, 3))))
        lens = np.diff(np.concatenate([[0], cuts, [nb]]))
        body = b"".join(b">r%d\n" % j + _wrap(q(int(m)), w) for j, m in enumerate(lens))
        room = n - len(body)
        if room < 0:
            t = body[:n]
        else:
            junk = (b"junk before any header\n" * (room // 40 + 1))[:room // 2]
            hdr = room - len(junk)
            t = junk + (b">" + b"h" * (hdr - 2) + b"\n" if hdr >= 2 else b"j" * hdr) + body
        assert len(t) == n
        texts.append(t)
    return texts


@pytest.fixture(scope="module")
def many_texts():
    return _many_texts(_lib.text_tile_bytes())


def test_scan_many_files_per_chunk(ctx1000, tmp_path, many_texts):
    T = _lib.text_tile_bytes()
    tiles = [_ntiles(t, T) for t in many_texts]
    assert max(tiles) == 1 and T in [len(t) for t in many_texts] and 1 in [len(t) for t in many_texts]
    ntiles = sum(tiles)
    per = _per(ntiles)
    assert per == 3 and ntiles > 2 * SCAN_WG
    # every tile starts a file: per file starts in every full chunk, with the
    # empty files among them
    assert sum(1 for t in many_texts if not t) > 150
    _check_all(ctx1000, many_texts, tmp_path, "many")


# ------------------------------------------------------------------ 1d
def test_record_dense_and_sequence_dense_tiles(ctx1000, tmp_path):
    T = _lib.text_tile_bytes()
    rng = np.random.default_rng(34)
    q = lambda n: _rand_seq(rng, n, b"ACGTACGTN")                     # noqa: E731
    one = b">\nA\n" * (T // 4)                                        # one tile of one-base records
    texts = [
        b">\n" * (T // 2) + _wrap(q(3000), 60),                       # T/2 records started in one tile, no base in it
        b">\nA\n" * (3 * T // 4),                                     # separator, base, separator, ... over three tiles
        b">\nC\n" * (3 * T // 4) + b">\n",                            # the same, ending in an empty record
        one + q(T) + b"\n" + one,                                     # a tile of T sequence bytes between two such
    ]
    assert len(texts[0]) > T and texts[0][:T] == b">\n" * (T // 2) and texts[0][T:T + 1] in b"ACGTN"
    assert len(texts[1]) == 3 * T
    assert len(one) == T and b"\n" not in texts[3][T:2 * T] and b">" not in texts[3][T:2 * T]
    assert texts[3][2 * T:2 * T + 3] == b"\n>\n"
    _check_all(ctx1000, texts, tmp_path, "dense")


# ------------------------------------------------------------------ 1e
def test_many_small_files_end_to_end(tmp_path, monkeypatch, many_texts):
    """Files shorter than the sketch size: a sketch holds the hash of every
    k-mer of its file, so one mispacked base anywhere changes it."""
    monkeypatch.delenv("DREPHIP_INGEST_BATCH_BASES", raising=False)
    T = _lib.text_tile_bytes()
    files, want = [], []
    for i, t in enumerate(many_texts):
        if len(t) < K:
            continue
        p = tmp_path / ("small_%04d.fa" % i)
        p.write_bytes(t)
        seq, off, ln = oracle.read_fasta(str(p))
        if not 21 <= ln <= 900:
            continue
        files.append(str(p))
        want.append((oracle.sketch_records(seq, off, K, S), ln))
    assert len(files) > SCAN_WG and _per(len(files)) >= 2              # one tile each: more than 512 tiles in the call
    assert max(len(t) for t in many_texts) <= T
    with _lib.Context(0, K, S, 42) as ctx:
        ctx.set_ingest_path("device")
        dev = ctx.sketch_files(files, threads=4)
        paths, st = ctx.ingest_paths(), ctx.ingest_stats()
    with _lib.Context(0, K, S, 42) as ctx:
        host = ctx.sketch_files(files, threads=4)
    assert paths["device_files"] == len(files) and paths["host_files"] == 0
    assert st["batches"] == 1
    assert sum(len(h) > 0 for h, _ in want) > SCAN_WG                  # more than 512 of them have a k-mer
    for got in (dev, host):
        for i, (h, ln) in enumerate(want):
            assert len(h) < S and got[1][i] == len(h) and int(got[2][i]) == ln, files[i]
            assert np.array_equal(got[0][i][:len(h)], h), files[i]


# ------------------------------------------------------------------ 2
def _same_call(a, b):
    ra, ca, va, *_ = a
    rb, cb, vb, *_ = b
    assert all(np.array_equal(ra[key], rb[key]) for key in ra)
    assert np.array_equal(ca, cb) and np.array_equal(va, vb)


def test_split_launches_summary_and_pack(ctx1000, tmp_path, monkeypatch):
    T = _lib.text_tile_bytes()
    c = _scan_call(T, 513, True)
    caps = c.region_caps()
    monkeypatch.delenv("DREPHIP_MAX_LAUNCH_ITEMS", raising=False)
    whole = _device_pack(ctx1000, c.texts, caps=caps)
    monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", CAP_ITEMS)
    per_dispatch = int(CAP_ITEMS) // 256
    assert per_dispatch == 8 and c.at > per_dispatch and (c.at + per_dispatch - 1) // per_dispatch == 65
    _check_all(ctx1000, c.texts, tmp_path, "splitscan", want_status=c.status, caps=caps)
    _same_call(_device_pack(ctx1000, c.texts, caps=caps), whole)


def test_split_launches_kmer_count(ctx1000, tmp_path, monkeypatch):
    tile = _lib.tile_bases()
    rng = np.random.default_rng(35)
    texts, caps = [], []
    for g, L in enumerate((40_000, 300_000, 301_234)):
        lens = [L // 3, L // 3 + 11, L - 2 * (L // 3) - 11]
        texts.append(b"".join(b">g%d_%d\n" % (g, j) + _wrap(_rand_seq(rng, m, b"ACGTACGTACGTACGTACGTN"), 80)
                              for j, m in enumerate(lens)))
        caps.append(_lib.padded_bases(lens) + 2 * tile)
    chunk_first = np.concatenate([[0], np.cumsum(caps) // tile])
    per_dispatch = int(CAP_ITEMS) // 256
    assert per_dispatch == 8 and chunk_first[-1] > 2 * per_dispatch   # three dispatches at the least
    assert chunk_first[1] < per_dispatch < chunk_first[2]             # the second genome straddles a dispatch edge
    assert chunk_first[2] < 3 * per_dispatch < chunk_first[3]         # and the third a later one
    monkeypatch.delenv("DREPHIP_MAX_LAUNCH_ITEMS", raising=False)
    whole = _device_pack(ctx1000, texts, caps=caps)
    monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", CAP_ITEMS)
    _check_all(ctx1000, texts, tmp_path, "splitkmer", caps=caps)
    _same_call(_device_pack(ctx1000, texts, caps=caps), whole)


# ------------------------------------------------------------------ 3
KMER_EDGES = (32, 128, 32768, 65536)    # a bitmap word, a lane's 128 bases, the count chunks


def _designed_runs(k, tile):
    """(start, length) of the valid runs of section 3: for every edge E, runs of
    length k-1, k, k+1, 31, 32, 33 and 64 whose last base is at E-1, E or E+1,
    and that begin k-1 bases before E; one run over a whole chunk."""
    runs = {(tile, tile)}
    for E in KMER_EDGES:
        for r in {k - 1, k, k + 1, 31, 32, 33, 64}:
            if r < 1:
                continue
            for s in (E - r, E - r + 1, E - r + 2, E - (k - 1)):
                if s >= 0:
                    runs.add((s, r))
    return sorted(runs)


def _designed_genomes(k, tile, rng):
    """The runs spread over genomes (first fit; runs in one genome keep an
    invalid base between them).  Genome lengths alternate between 3 tile - 1
    (padded to three chunks, all used) and 3 tile (a fourth, all invalid); each
    also ends in a run of k + 1.  Returns per genome (length, runs)."""
    genomes = []
    for s, r in _designed_runs(k, tile):
        for runs in genomes:
            if all(s + r < a or a + b < s for a, b in runs):
                runs.append((s, r))
                break
        else:
            genomes.append([(s, r)])
    out = []
    for i, runs in enumerate(genomes):
        L = 3 * tile - 1 + i % 2
        runs.append((L - (k + 1), k + 1))
        assert max(a + b for a, b in runs[:-1]) < L - (k + 1) - 1
        out.append((L, sorted(runs)))
    return out


def _designed_texts(L, runs, rng, g):
    """One genome as a single record (N at every invalid position) and as
    several records (the invalid position behind each run is a record
    separator instead): (single text, multi text, records of the multi form)."""
    seq = np.full(L, ord("N"), np.uint8)
    for s, r in runs:
        seq[s:s + r] = np.frombuffer(_rand_seq(rng, r), np.uint8)
    single = b">single_%d\n" % g + seq.tobytes() + b"\n"
    breaks = [s + r for s, r in runs if s + r < L]
    recs, a = [], 0
    for b in breaks:
        recs.append(seq[a:b].tobytes())
        a = b + 1
    recs.append(seq[a:].tobytes())
    multi = b"".join(b">multi_%d_%d\n" % (g, j) + rec + b"\n" for j, rec in enumerate(recs))
    return single, multi, recs


def _windows(recs, k):
    """Windows of k valid bases inside a record: the definition of a k-mer."""
    return sum(max(0, len(m) - k + 1) for rec in recs for m in re.findall(rb"[ACGTacgt]+", rec))


@pytest.mark.parametrize("k", [1, 2, 20, 21, 31, 32])
def test_valid_kmers_at_word_lane_and_chunk_edges(tmp_path, k):
    tile = _lib.tile_bases()
    assert tile == 32768 == 256 * 128
    rng = np.random.default_rng(100 + k)
    texts, caps, direct = [], [], []
    designed = _designed_genomes(k, tile, rng)
    all_runs = {run for _, runs in designed for run in runs}
    assert (tile, tile) in all_runs and (0, 32) in all_runs           # a whole chunk; a run from the genome's position 0
    assert {(E - k, k) for E in KMER_EDGES} <= all_runs and {(E - k + 1, k + 1) for E in KMER_EDGES} <= all_runs
    for g, (L, runs) in enumerate(designed):
        single, multi, recs = _designed_texts(L, runs, rng, g)
        n = sum(max(0, r - k + 1) for _, r in runs)
        assert _windows([single.split(b"\n")[1]], k) == n == _windows(recs, k)
        padded = _lib.padded_bases([L])
        assert padded == (3 + g % 2) * tile and _lib.padded_bases([len(r) for r in recs]) == padded
        for t in (single, multi):
            texts.append(t)
            caps.append(padded + 2 * tile)                            # two count chunks past the genome: the early exit
            direct.append(n)
    assert len(designed) >= 10
    with _lib.Context(0, k, S, 42) as ctx:
        # the tile before every region is all ones: a run from position 0 is
        # kept from joining it by the rule for a genome's first word alone
        r = _check_all(ctx, texts, tmp_path, "k%d" % k, caps=caps, gap_tiles=1, fill=ALL_ONES, k=k)
    assert [int(x) for x in r["n_kmers"]] == direct
