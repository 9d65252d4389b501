"""Helpers and references of tests/test_ingest_device.py and
tests/test_ingest_device_scan.py (GPU): a numpy restatement of the packed
layout, a count of valid k-mers taken from the validity bitmap by run lengths
(no code shared with either C++ run_k_mask), one drephip_fasta_pack_device call
over in-memory texts with every word outside the regions pre-filled, and the
comparison of such a call with the oracle's kseq and the host packer."""
import ctypes as C

import numpy as np

import oracle
from drep_amd import _lib

S = 1000
K = 21
FILL = 0x5A5A5A5A


def _np_pack(recs, tile):
    """numpy restatement of the packed layout (include/drephip.h) for one genome."""
    span = sum(len(r) for r in recs) + max(len(recs) - 1, 0)
    P = ((span + 1 + tile - 1) // tile) * tile
    bases = np.full(P, 255, np.uint8)
    pos = 0
    for r in recs:
        bases[pos:pos + len(r)] = r
        pos += len(r) + 1
    lut = np.full(256, 4, np.uint8)
    for ch, c in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
        lut[ch] = c
    code = lut[bases]
    ok = code < 4
    c2 = np.where(ok, code, 0).astype(np.uint32).reshape(-1, 16)
    codes = (c2 << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    v = ok.astype(np.uint32).reshape(-1, 32)
    valid = (v << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return P, codes, valid


def np_valid_kmers(valid_words, k):
    """Bit positions of one genome's validity bitmap (uint32 words, bit b of
    word w is position 32 w + b) that end a run of at least k set bits, counted
    from run lengths: position i's run length is i minus the last clear
    position at or before it."""
    words = np.ascontiguousarray(valid_words, dtype="<u4")
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    if len(bits) == 0:
        return 0
    idx = np.arange(len(bits), dtype=np.int64)
    last_clear = np.maximum.accumulate(np.where(bits == 0, idx, -1))
    return int(np.count_nonzero(idx - last_clear >= k))


def _expected(path, tile, k=K):
    """(P, codes, valid, length, n_records, n_kmers) of one file, from the oracle
    and from the host packer, which must agree with each other; the k-mer count
    must also be what the bitmap alone gives (np_valid_kmers)."""
    seq, off, ln = oracle.read_fasta(str(path))
    recs = [seq[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    P, want_c, want_v = _np_pack(recs, tile)
    info = _lib.fasta_info(str(path), k)
    codes = np.zeros((tile + P) // 16, np.uint32)
    valid = np.zeros((tile + P) // 32, np.uint32)
    length, nk = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().drephip_fasta_pack(str(path).encode(), k, codes, valid, tile, tile + P, C.byref(length),
                                         C.byref(nk)) == 0
    assert np.array_equal(codes[tile // 16:], want_c) and np.array_equal(valid[tile // 32:], want_v), path
    assert info["length"] == ln == length.value and info["n_records"] == len(recs) and info["padded"] == P, path
    assert info["n_kmers"] == nk.value, path
    assert nk.value == np_valid_kmers(want_v, k), path
    return P, want_c, want_v, ln, len(recs), nk.value


def _device_pack(ctx, texts, caps=None, gap_tiles=0, fill=FILL):
    """One drephip_fasta_pack_device call over `texts` (bytes each): regions in
    file order, `gap_tiles` untouched tiles between them, every word of the
    buffers pre-filled with `fill`; the bytes between files are '>' characters,
    which belong to no file.  Returns (results, codes, valid, base_off, caps)."""
    import torch
    tile = _lib.tile_bases()
    sizes = [len(t) for t in texts]
    starts, off = _lib.text_layout(sizes)
    host = np.full(max(int(off[-1]), 16), ord(">"), np.uint8)
    for t, st in zip(texts, starts):
        host[int(st):int(st) + len(t)] = np.frombuffer(t, np.uint8)
    text = torch.from_numpy(host).cuda()
    if caps is None:
        caps = [_lib.padded_bases([sz]) for sz in sizes]
    caps = np.asarray(caps, np.uint64)
    base = np.zeros(len(texts), np.uint64)
    at = tile
    for f in range(len(texts)):
        base[f] = at
        at += int(caps[f]) + gap_tiles * tile
    at += tile
    word = int(np.array(fill, np.uint32).view(np.int32))
    codes = torch.full((at // 16,), word, dtype=torch.int32, device="cuda")
    valid = torch.full((at // 32,), word, dtype=torch.int32, device="cuda")
    r = ctx.fasta_pack_device(text, off, base, caps, codes, valid)
    torch.cuda.synchronize()
    return r, codes.cpu().numpy().view(np.uint32), valid.cpu().numpy().view(np.uint32), base, caps


def _check_all(ctx, texts, tmp_path, tag, want_status=None, caps=None, gap_tiles=0, fill=FILL, k=K):
    """Pack `texts` in one call and hold every file's region and per-file
    results against the oracle and the host packer; everything outside the
    regions keeps its fill.  `want_status` (one entry per file, default all 0):
    a file expected with status 1 (it needs the host reader) or 2 (its region,
    given in `caps`, is too small) is held to that status and to a region left
    all zero, a status 2 file also to its true length, record count and padded
    size.  `k` is the context's k-mer length."""
    tile = _lib.tile_bases()
    if want_status is None:
        want_status = [0] * len(texts)
    assert len(want_status) == len(texts)
    r, codes, valid, base, caps = _device_pack(ctx, texts, caps=caps, gap_tiles=gap_tiles, fill=fill)
    touched_c = np.zeros(len(codes), bool)
    touched_v = np.zeros(len(valid), bool)
    for f, t in enumerate(texts):
        what = (tag, f, t[:60])
        b, cap = int(base[f]), int(caps[f])
        got_c, got_v = codes[b // 16:(b + cap) // 16], valid[b // 32:(b + cap) // 32]
        touched_c[b // 16:(b + cap) // 16] = True
        touched_v[b // 32:(b + cap) // 32] = True
        assert r["status"][f] == want_status[f], what
        if want_status[f] == 1:
            assert not got_c.any() and not got_v.any(), what
            continue
        p = tmp_path / ("%s_%02d.fa" % (tag, f))
        p.write_bytes(t)
        P, want_c, want_v, ln, nrec, nk = _expected(p, tile, k)
        if want_status[f] == 2:
            assert P > cap, what
            assert (r["length"][f], r["n_records"][f], r["padded"][f]) == (ln, nrec, P), what
            assert not got_c.any() and not got_v.any(), what
            continue
        assert (r["length"][f], r["n_records"][f], r["padded"][f], r["n_kmers"][f]) == (ln, nrec, P, nk), what
        assert P <= cap, what
        assert np.array_equal(got_v[:P // 32], want_v), what
        assert np.array_equal(got_c[:P // 16], want_c), what
        assert not got_c[P // 16:].any() and not got_v[P // 32:].any(), what       # the slack up to cap
    assert (codes[~touched_c] == fill).all() and (valid[~touched_v] == fill).all(), tag
    return r


def _rand_seq(rng, n, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def _wrap(seq, w):
    return b"".join(seq[i:i + w] + b"\n" for i in range(0, len(seq), w))
