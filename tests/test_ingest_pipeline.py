"""The batch pipeline behind drephip_sketch_files (drep_amd/csrc/ingest_pipeline.h
and .cpp) on both ingest paths: small files in many batches, so that both of
its slots are reused, every kind of file among them, and an error in a later
batch.  Expected sketches and lengths are the oracle's; the batch count is a
restatement of the take-until-target rule from the files' sizes and gzip
trailers."""
import gzip
import os
import zlib

import numpy as np
import pytest

import oracle
from drep_amd import _lib

pytestmark = pytest.mark.gpu
K = 21
S = 200                     # every file with sequence fills it
TARGET = 100000             # DREPHIP_INGEST_BATCH_BASES: two or three files per batch
PATHS = ("host", "device")


def _fasta(rng, bases, name=b"g", wrap=70):
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, bases)].tobytes()
    return b">" + name + b"\n" + b"".join(seq[i:i + wrap] + b"\n" for i in range(0, bases, wrap))


def _estimate(path):
    """Upper bound on a file's bases: its size; a gzip file's last ISIZE where
    that is at least the file's size, else four times the size; 0 if missing."""
    if not os.path.exists(path):
        return 0
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b" and len(raw) >= 18:
        isize = int.from_bytes(raw[-4:], "little")
        return isize if isize >= len(raw) else 4 * len(raw)
    return len(raw)


def _batches(files, target=TARGET):
    """Files are taken until their estimates reach the target, at least one."""
    out, cur, total = [], [], 0
    for i, f in enumerate(files):
        if cur and total >= target:
            out.append(cur)
            cur, total = [], 0
        cur.append(i)
        total += _estimate(f)
    return out + [cur] if cur else out


def _padded(bases):
    tile = _lib.tile_bases()
    return (bases + 1 + tile - 1) // tile * tile


@pytest.fixture(scope="module")
def nine(tmp_path_factory):
    """Nine files of 1 to 3 tiles: {files, bases (single records), kind, want
    (the oracle's sketch and length)}."""
    td = tmp_path_factory.mktemp("ingest_pipeline")
    rng = np.random.default_rng(29)
    spec = [("plain", 40000), ("plain", 70000), ("gz", 50000), ("fastq", 33000), ("gz2", 90000), ("header", 0),
            ("plain", 60000), ("plain", 98000), ("plain", 33000)]
    files = []
    for i, (kind, bases) in enumerate(spec):
        text = _fasta(rng, bases)
        p = td / ("f%d_%s.fa" % (i, kind))
        if kind == "gz":
            p = td / (p.name + ".gz")
            p.write_bytes(gzip.compress(text))
        elif kind == "gz2":
            # two members; the last one's ISIZE passes for the whole file's and
            # underestimates it: the genome outgrows its region
            p = td / (p.name + ".gz")
            cut = text.index(b"\n", len(text) // 2) + 1
            with open(p, "wb") as fh:
                for part in (text[:cut], text[cut:]):
                    co = zlib.compressobj(6, zlib.DEFLATED, 31)
                    fh.write(co.compress(part) + co.flush())
            assert gzip.open(p).read() == text and _padded(_estimate(str(p))) < _padded(bases)
        elif kind == "fastq":
            seq = text.split(b"\n", 1)[1].replace(b"\n", b"")
            p.write_bytes(b"@r\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
        else:
            p.write_bytes(text)
        files.append(str(p))
    want = [oracle.sketch_fasta(f, K, S) for f in files]
    for (kind, bases), (h, ln) in zip(spec, want):
        assert ln == bases and len(h) == (S if bases else 0)
    return {"files": files, "bases": [b for _, b in spec], "kind": [k for k, _ in spec], "want": want}


def _check(got, want, idx):
    h, nh, ln = got
    assert len(nh) == len(idx)
    for row, i in enumerate(idx):
        oh, oln = want[i]
        assert nh[row] == len(oh) and np.array_equal(h[row, :len(oh)], oh) and int(ln[row]) == oln, (row, i)


@pytest.fixture()
def small_batches(monkeypatch):
    monkeypatch.setenv("DREPHIP_INGEST_BATCH_BASES", str(TARGET))


@pytest.mark.parametrize("path", PATHS)
def test_nine_files_in_four_batches(nine, small_batches, path):
    files, kind = nine["files"], nine["kind"]
    batches = _batches(files)
    assert len(batches) >= 4 and all(2 <= len(b) <= 3 for b in batches)
    overflowing = sum(_padded(b) > _padded(_estimate(f)) for f, b in zip(files, nine["bases"]))
    assert overflowing == 1
    with _lib.Context(0, K, S, 42) as ctx:
        ctx.set_ingest_path(path)
        got = ctx.sketch_files(files, threads=3)
        st, who = ctx.ingest_stats(), ctx.ingest_paths()
    _check(got, nine["want"], range(len(files)))
    assert st["batches"] == len(batches)
    assert st["overflow_genomes"] == overflowing
    if path == "host":
        assert who == {"path": "host", "device_files": 0, "host_files": len(files), "text_bytes": 0}
    else:
        plain = [f for f, k in zip(files, kind) if k not in ("gz", "gz2")]         # their text is copied ...
        on_device = sum(k in ("plain", "header") for k in kind)                    # ... and the FASTQ file handed back
        assert who == {"path": "device", "device_files": on_device, "host_files": len(files) - on_device,
                       "text_bytes": sum(os.path.getsize(f) for f in plain)}


@pytest.mark.parametrize("first", PATHS)
@pytest.mark.parametrize("where", ["third_batch", "file_0"])
def test_missing_file_in_a_later_batch(nine, small_batches, tmp_path, first, where):
    files = nine["files"]
    at = _batches(files)[2][0] if where == "third_batch" else 0
    missing = str(tmp_path / "not_there.fa")
    bad = files[:at] + [missing] + files[at:]
    assert _batches(bad)[2 if at else 0][0] == at
    other = PATHS[1 - PATHS.index(first)]
    with _lib.Context(0, K, S, 42) as ctx:
        for path in (first, other):
            ctx.set_ingest_path(path)
            with pytest.raises(_lib.DrepHipError, match="not_there.fa"):
                ctx.sketch_files(bad, threads=3)
            got = ctx.sketch_files(files, threads=3)
            _check(got, nine["want"], range(len(files)))
            assert ctx.ingest_stats()["batches"] == len(_batches(files))


@pytest.mark.parametrize("path", PATHS)
def test_empty_and_one_file_lists(nine, small_batches, path):
    files = nine["files"]
    with _lib.Context(0, K, S, 42) as ctx:
        ctx.set_ingest_path(path)
        for i in (1, 4):                                   # a plain file, and the one that overflows its region
            _check(ctx.sketch_files([files[i]], threads=3), nine["want"], [i])
            assert ctx.ingest_stats()["batches"] == 1
        h, nh, ln = ctx.sketch_files([])
        assert h.shape == (0, S) and len(nh) == 0 and len(ln) == 0
        # the entry point itself with no files: nothing to do, and the last call's figures are reset
        one64, one32 = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
        assert _lib.lib().drephip_sketch_files(ctx.handle, None, 0, 3, one64, one32, one64) == 0
        assert ctx.ingest_stats()["batches"] == 0 and ctx.ingest_paths()["host_files"] == 0
        assert ctx.ingest_path == path
