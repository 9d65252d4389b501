"""Device FASTA ingest (drep_amd/csrc/ingest_device.hip): FASTA text in device
memory parsed and 2-bit packed by kernels, against two independent sources
that must both agree with it: the oracle's byte-level kseq (oracle.read_fasta
+ a numpy restatement of the layout) and the host packer (drephip_fasta_pack /
drephip_fasta_info); then the whole drephip_sketch_files and drop-in on the
device path against the host path and the committed sketches."""
import glob
import gzip
import os

import numpy as np
import pandas as pd
import pytest

import oracle
from drep_amd import _lib, d_cluster
from drep_amd.mash_io import read_msh
from ingest_cases import FILL, K, S, _check_all, _device_pack, _expected, _rand_seq, _wrap

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1
def test_kseq_corner_cases_fasta_side(ctx1000, tmp_path):
    rng = np.random.default_rng(11)
    long_mixed = b">mixed case and IUPAC\n" + _wrap(_rand_seq(rng, 5000, b"ACGTACGTACGTacgtacgtNRYKMSWBDHV"), 61)
    texts = [
        b"junk >hdr one\nACGT\nacgtN\n>two\nGGGG\n",                 # header hunt mid-line
        b"some text\nmore @h1 x\nACGTACGTACGTACGTACGTACGTAC\n@h2\nTTTTGGGGCCCCAAAATTTTGGGGCC\n",   # '@' headers
        b">f\nACGT\n>",                                               # '>' as the last byte
        b">f\nACGT\n>g",                                              # header at EOF without newline
        b">a\n>b\n>c\nACGT\n>d\n",                                    # empty records: consecutive and trailing
        b">a\nAC\n\n\nGT\n\nTTAA\n",                                  # empty lines inside a record
        b">a\r\nACG\r\n\r\nTTA\r\n\n>b\r\nAC\r\n",                    # CRLF, a line of only '\r'
        b">a\nACGT\r\r\nGG\n",                                        # a line ending '\r\r\n'
        b">a\nACGT\nGGTT\r",                                          # final line without '\n', ending in '\r'
        b"",                                                          # an empty file
        b"no header at all\nACGTACGT\n",                              # no header
        b">lower\nacgtacgtacgtacgtacgtacgtacgt\nACGTacgt\n",          # lower case
        b">junk\nAC GT\x00N-*RYKM\tacgu\x7f\xffACGT\nNNNN\n",         # IUPAC, spaces, NUL, high bytes
        b">",                                                         # only a header character
        b"\n\n\n",                                                    # only newlines
        long_mixed,
    ]
    _check_all(ctx1000, texts, tmp_path, "corner")


# ------------------------------------------------------------------ 2
FASTQ_CASES = {
    "fastq_quality_lookalikes": b"@r1\nACGTACGT\n+\n@>+!\n@@II\n@r2 x\nTTTT\n+r2\n>>>>\n",
    "fastq_long_quality": b"@a\nACGT\n+\nIIII\n@b\nCCCC\n+\nIIIIII\n@c\nGGGG\n+\nIIII\n",
    "fastq_short_quality": b">f\nAAAACCCC\n@q\nACGTACGT\n+\nIII\n",
    "fastq_plus_eof": b">f\nAAAA\n@q\nACGT\n+",
    "fastq_empty_record": b">f\nACGT\n@e\n+\n",
    "after_fastq_hunt": b"@a\nAC\n+\nII\nnoise x@b\nGGTT\n",
    "crlf": b">a\r\nACG\r\n\r\nTTA\r\n\n@b\r\nAC\r\n+\r\nII\r\n",
}


def test_fastq_flagged_never_mispacked(ctx1000, tmp_path):
    names = sorted(FASTQ_CASES)
    # longer records around the same shapes, so that the sketches are not empty
    rng = np.random.default_rng(5)
    s1, s2 = _rand_seq(rng, 3000), _rand_seq(rng, 2000)
    big = b">plain\n" + _wrap(s1, 70) + b"@fq\n" + s2 + b"\n+\n" + b"I" * len(s2) + b"\n>after\n" + _wrap(s1[::-1], 70)
    texts = [FASTQ_CASES[n] for n in names] + [big]
    r, *_ = _device_pack(ctx1000, texts)
    assert (r["status"] == 1).all(), dict(zip(names + ["big"], r["status"]))
    files = []
    for i, t in enumerate(texts):
        p = tmp_path / ("q%02d.fq" % i)
        p.write_bytes(t)
        files.append(str(p))
    with _lib.Context(0, K, S, 42) as ctx:
        assert ctx.ingest_paths()["path"] == "host"
        want = ctx.sketch_files(files, threads=2)
        assert ctx.ingest_paths() == {"path": "host", "device_files": 0, "host_files": len(files), "text_bytes": 0}
        ctx.set_ingest_path("device")
        got = ctx.sketch_files(files, threads=2)
        paths = ctx.ingest_paths()
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert want[1][-1] > 0                                            # the long file has a sketch
    assert paths["device_files"] == 0 and paths["host_files"] == len(files)
    assert paths["text_bytes"] == sum(len(t) for t in texts)


# ------------------------------------------------------------------ 3
def test_tile_edges(ctx1000, tmp_path):
    T = _lib.text_tile_bytes()
    rng = np.random.default_rng(3)
    q = lambda n: _rand_seq(rng, n, b"ACGTACGTN")                     # noqa: E731

    def sized(n):                                                      # a file of exactly n bytes
        t = b">exact\n" + _wrap(q(n), 80)
        t = t[:n - 1] + b"\n"
        assert len(t) == n
        return t
    texts = [
        b">a\n" + q(T - 4) + b"\n" + b"CGTCGT\n",                     # '\n' is the last byte of a tile
        b">a\n" + q(T - 3) + b"\nCGTCGT\n",                           # '\n' is the first byte of the next
        b">a\n" + q(T - 4) + b"\r\nCGTCGT\n",                         # '\r' last in a tile, '\n' first in the next
        b"x" * (T - 1) + b">hdr\n" + q(100) + b"\n",                  # the first '>' is the last byte of a tile
        b">" + b"h" * (2 * T + 10) + b"\n" + q(90) + b"\n>b\nGG\n",   # a header line over three tiles
        b">a\n" + q(3 * T + 5) + b"\n",                               # one unwrapped line of 3T + 5 bytes
        b">a\n" + q(T - 4) + b"\n" + b">b\n" + q(50) + b"\n",         # a record starts exactly at a tile boundary
        sized(T), sized(T - 1), sized(T + 1),
        b">a\n" + q(40) + b"\n>a header that the file ends in",       # ends inside a header ...
        q(30) + b"\n>b\n" + q(60) + b"\n",                            # ... and the next file starts with no header
        b">a\n" + q(T - 5) + b"\n\n" + q(7) + b"\n",                  # an empty line astride the boundary
        b">a\n" + q(T - 4) + b">" + q(9) + b"\n",                     # a '>' inside a sequence line at the boundary
    ]
    assert texts[0][T - 1:T] == b"\n" and texts[1][T:T + 1] == b"\n" and texts[2][T - 1:T + 1] == b"\r\n"
    assert texts[3][T - 1:T] == b">" and texts[6][T:T + 1] == b">" and texts[13][T - 1:T] == b">"
    _check_all(ctx1000, texts, tmp_path, "edge")


# ------------------------------------------------------------------ 4
def test_word_and_separator_alignment(ctx1000, tmp_path):
    rng = np.random.default_rng(4)
    every = b"".join(b">r%d\n" % n + (_rand_seq(rng, n) + b"\n" if n else b"") for n in range(71))
    many = b"".join(b">x\n" + (_rand_seq(rng, n) + b"\n" if n else b"") for n in rng.integers(0, 13, 3000))
    tail = b">t\n" + _wrap(_rand_seq(rng, 40000), 60)                # two output tiles
    assert len(many) > 3 * _lib.text_tile_bytes()
    # regions are adjacent (no gap): a file's last word and the next file's
    # first word are neighbours written by different tiles
    _check_all(ctx1000, [every, tail, many, every[::-1].replace(b"\n", b"", 1)], tmp_path, "align")


# ------------------------------------------------------------------ 5
def test_region_too_small(ctx1000, tmp_path):
    tile = _lib.tile_bases()
    rng = np.random.default_rng(6)
    texts = [b">a\n" + _wrap(_rand_seq(rng, 20000), 70),
             b">big\n" + _wrap(_rand_seq(rng, tile + 5000), 70),      # needs two tiles
             b">c\n" + _wrap(_rand_seq(rng, 9000), 70)]
    need = []
    for f, t in enumerate(texts):
        p = tmp_path / ("small_%d.fa" % f)
        p.write_bytes(t)
        need.append(_expected(p, tile))
    assert need[1][0] == 2 * tile
    caps = [need[0][0], need[1][0] - tile, need[2][0]]
    r, codes, valid, base, caps = _device_pack(ctx1000, texts, caps=caps, gap_tiles=1)
    assert list(r["status"]) == [0, 2, 0]
    keep_c = np.ones(len(codes), bool)
    keep_v = np.ones(len(valid), bool)
    for f in range(3):
        b, cap = int(base[f]), int(caps[f])
        keep_c[b // 16:(b + cap) // 16] = False
        keep_v[b // 32:(b + cap) // 32] = False
        if f == 1:
            continue
        P, want_c, want_v, ln, nrec, nk = need[f]
        assert np.array_equal(codes[b // 16:(b + P) // 16], want_c) and np.array_equal(valid[b // 32:(b + P) // 32], want_v)
        assert (r["length"][f], r["n_records"][f], r["padded"][f], r["n_kmers"][f]) == (ln, nrec, P, nk)
    # the first tile, the gaps around the small region and the tail keep the fill
    assert (codes[keep_c] == FILL).all() and (valid[keep_v] == FILL).all()
    # the file reports its true size, so that a caller can make room
    assert r["length"][1] == need[1][3] and r["padded"][1] == need[1][0]


# ------------------------------------------------------------------ 6
def test_argument_errors(ctx1000):
    import torch
    L = _lib.lib()
    tile = _lib.tile_bases()
    text = torch.zeros(64, dtype=torch.uint8, device="cuda")
    codes = torch.zeros(2 * tile // 16, dtype=torch.int32, device="cuda")
    valid = torch.zeros(2 * tile // 32, dtype=torch.int32, device="cuda")
    base, cap = np.array([tile], np.uint64), np.array([tile], np.uint64)

    def call(d_text, off):
        return L.drephip_fasta_pack_device(ctx1000.handle, d_text, np.array(off, np.uint64), 1, base, cap,
                                           codes.data_ptr(), valid.data_ptr(), None, None, None, None, None, None)
    assert call(text.data_ptr(), [0, 40]) == 0
    assert call(None, [0, 40]) == -1 and L.drephip_last_error()
    assert call(text.data_ptr(), [8, 40]) == -1 and b"aligned" in L.drephip_last_error()
    assert call(text.data_ptr() + 4, [0, 40]) == -1 and b"aligned" in L.drephip_last_error()
    with pytest.raises(ValueError):
        ctx1000.set_ingest_path("gpu")


# ------------------------------------------------------------------ 7, 8
@pytest.fixture(scope="module")
def real_files(golden, tmp_path_factory):
    """The four reference genomes inflated to plain files, plus one left gzip."""
    td = tmp_path_factory.mktemp("ingest_real")
    src = sorted(glob.glob(os.path.join(golden, "genomes", "*.gz")))
    assert len(src) == 4
    files = []
    for f in src:
        p = td / os.path.basename(f)[:-3]
        p.write_bytes(gzip.open(f).read())
        files.append(str(p))
    z = td / ("z_" + os.path.basename(src[1]))
    z.write_bytes(open(src[1], "rb").read())
    files.insert(2, str(z))
    return files


def _msh_of(golden, path):
    name = os.path.basename(path)
    name = name[2:-3] if name.startswith("z_") else name
    return read_msh(os.path.join(golden, "MASH_files", "sketches", name + ".msh")).references[0]


@pytest.mark.parametrize("batch_bases", [None, "3000000"])
def test_whole_path_on_real_genomes(golden, real_files, monkeypatch, batch_bases):
    if batch_bases:
        monkeypatch.setenv("DREPHIP_INGEST_BATCH_BASES", batch_bases)
    else:
        monkeypatch.delenv("DREPHIP_INGEST_BATCH_BASES", raising=False)
    # the device path first and on a context of its own: nothing the host path
    # left in the device scratch can help it
    with _lib.Context(0, K, S, 42) as ctx:
        ctx.set_ingest_path("device")
        got = ctx.sketch_files(real_files, threads=3)
        paths, st = ctx.ingest_paths(), ctx.ingest_stats()
    with _lib.Context(0, K, S, 42) as ctx:
        want = ctx.sketch_files(real_files, threads=3)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    for i, f in enumerate(real_files):
        ref = _msh_of(golden, f)
        assert got[1][i] == S and np.array_equal(got[0][i], ref.hashes) and int(got[2][i]) == ref.length, f
    plain = [f for f in real_files if not f.endswith(".gz")]
    assert paths == {"path": "device", "device_files": 4, "host_files": 1,
                     "text_bytes": sum(os.path.getsize(f) for f in plain)}
    assert st["batches"] >= (3 if batch_bases else 1)


def test_host_packed_regions_over_stale_scratch(golden, real_files, tmp_path, monkeypatch):
    """A gzip file (packed by the host reader, copied over its region) before a
    plain file in one batch, on a context whose device scratch an earlier
    device-path call with another layout left full of valid bases: the slack
    between the gzip genome's padded span and its region must be zero, or
    k-mers spanning stale bases and the next genome's first bases are hashed.
    The next genome is shorter than the sketch size, so every one of its
    k-mers is in its sketch and a single stray one shows."""
    monkeypatch.delenv("DREPHIP_INGEST_BATCH_BASES", raising=False)
    rng = np.random.default_rng(8)
    filler = tmp_path / "filler.fa"
    filler.write_bytes(b">filler\n" + _rand_seq(rng, 6_000_000) + b"\n")          # one record over every later region
    tiny = tmp_path / "tiny.fa"
    tiny.write_bytes(b">tiny\n" + _wrap(_rand_seq(rng, 700), 60))
    gz = [f for f in real_files if f.endswith(".gz")]
    plain = [f for f in real_files if not f.endswith(".gz")]
    files = [gz[0], str(tiny), gz[0], plain[0], str(tiny)]
    with _lib.Context(0, K, S, 42) as ctx:
        want = ctx.sketch_files(files, threads=2)
    with _lib.Context(0, K, S, 42) as ctx:
        ctx.set_ingest_path("device")
        ctx.sketch_files([str(filler)], threads=2)
        got = ctx.sketch_files(files, threads=2)
        paths, st = ctx.ingest_paths(), ctx.ingest_stats()
    assert st["batches"] == 1 and paths["device_files"] == 3 and paths["host_files"] == 2
    oh, oln = oracle.sketch_fasta(str(tiny), K, S)
    assert len(oh) == 700 - K + 1 < S
    for i in (1, 4):
        assert got[1][i] == len(oh) and np.array_equal(got[0][i][:len(oh)], oh) and int(got[2][i]) == oln
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    for i in (0, 2, 3):
        ref = _msh_of(golden, files[i])
        assert got[1][i] == S and np.array_equal(got[0][i], ref.hashes) and int(got[2][i]) == ref.length


def test_dropin_ingest_kwarg(real_files, tmp_path):
    Bdb = pd.DataFrame({"genome": [os.path.basename(f) for f in real_files], "location": real_files})
    host = d_cluster.all_vs_all_MASH(Bdb, str(tmp_path / "host"), processors=3, ingest="host")
    dev = d_cluster.all_vs_all_MASH(Bdb, str(tmp_path / "dev"), processors=3, ingest="device")

    def bits(df):
        df = df.copy()
        for c in df.columns:
            if df[c].dtype == np.float32:
                df[c] = df[c].to_numpy().view(np.uint32)
        return df
    assert len(dev) == len(real_files) ** 2
    assert bits(dev).equals(bits(host))
    with pytest.raises(ValueError):
        d_cluster.all_vs_all_MASH(Bdb, str(tmp_path / "x"), ingest="x")
