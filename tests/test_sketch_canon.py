"""The sketch hash kernel's canonical-strand choice (drep_amd/csrc/canon.h) and
its staged admit path.

The kernel picks the strand on the high words of the two top-aligned k-mers
(k is odd, so base 10 always differs between the strands and lies in the high
word), takes min(fhi, chi) as the canonical high word and cuts the tail index
(bases 16-20) of either strand straight from the code words.

CPU part: the cut through the host entry (the kernel's own inline functions)
against a reference that works from ASCII -- the smaller of the k-mer and its
reverse complement in memcmp order, re-encoded -- for every residue r of the
window end, on random words, on k-mers whose strands differ only at base 10,
on k-mers that differ at base 0, and with every tail value on either strand.
GPU part: sketches against the C oracle where the strand is decided late on
every residue, with N runs at chunk, lane and tile boundaries, and with the
admit stage overflowing at kMaxThr and at a real threshold.  Every comparison
is exact."""
import numpy as np
import pytest

import oracle
from drep_amd import _lib

ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.zeros(256, np.uint32)
CODE[ASCII] = np.arange(4, dtype=np.uint32)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
K = 21
TILE, LANE, CHUNK = 32768, 64, 16


def _pack(bases):
    """n x 48 base codes -> n x 3 code words (base i of a word at bits 2i)."""
    b = bases.astype(np.uint32).reshape(len(bases), 3, 16)
    return (b << (2 * np.arange(16, dtype=np.uint32))).sum(axis=2, dtype=np.uint64).astype(np.uint32)


def _reference(bases, r):
    """(high word, tail index, forward chosen) of the canonical 21-mer ending
    at base 32 + r of each row, from the ASCII strings."""
    q = 32 + r
    hi = np.zeros(len(bases), np.uint32)
    tail = np.zeros(len(bases), np.uint32)
    fwd = np.zeros(len(bases), bool)
    for i, row in enumerate(ASCII[bases[:, q - 20:q + 1]]):
        kmer = row.tobytes()
        rc = kmer.translate(COMP)[::-1]
        c = CODE[np.frombuffer(min(kmer, rc), dtype=np.uint8)]      # bytes order is memcmp order
        fwd[i] = kmer < rc
        hi[i] = (c[:16].astype(np.uint64) << (30 - 2 * np.arange(16, dtype=np.uint64))).sum()
        tail[i] = (c[16:] << (8 - 2 * np.arange(5, dtype=np.uint32))).sum()
    return hi, tail, fwd


def _check(bases, r):
    hi, tail = _lib.canon_eval(_pack(bases), r)
    whi, wtail, fwd = _reference(bases, r)
    assert np.array_equal(hi, whi), (r, np.flatnonzero(hi != whi)[:4])
    assert np.array_equal(tail, wtail), (r, np.flatnonzero(tail != wtail)[:4])
    return wtail, fwd


def _revcomp(x):
    return 3 - x[:, ::-1]


@pytest.mark.parametrize("r", range(16))
def test_canon_random_words(r):
    rng = np.random.default_rng(800 + r)
    bases = rng.integers(0, 4, (1500, 48))
    # extreme words around the random ones
    bases[:4] = np.array([0, 3, 0, 3])[:, None]
    bases[4, ::2], bases[4, 1::2] = 0, 3
    _, fwd = _check(bases, r)
    assert fwd.any() and not fwd.all()


@pytest.mark.parametrize("r", range(16))
def test_canon_strands_differ_only_at_base_10(r):
    """k-mers X m revcomp(X), |X| = 10: the reverse complement is
    X comp(m) revcomp(X), so the strands agree on the first ten bases and on
    the last ten, and base 10 alone decides -- forward for m in {A, C}."""
    rng = np.random.default_rng(900 + r)
    q = 32 + r
    for m in range(4):
        bases = rng.integers(0, 4, (300, 48))
        X = rng.integers(0, 4, (300, 10))
        bases[:, q - 20:q - 10] = X
        bases[:, q - 10] = m
        bases[:, q - 9:q + 1] = _revcomp(X)
        _, fwd = _check(bases, r)
        assert fwd.all() if m < 2 else not fwd.any(), (r, m)


@pytest.mark.parametrize("r", range(16))
def test_canon_strands_differ_at_base_0(r):
    """Base 0 of the forward strand is the base at q - 20, base 0 of the reverse
    strand the complement of the base at q: every pair with the two different."""
    rng = np.random.default_rng(1000 + r)
    q = 32 + r
    for first in range(4):
        for last in range(4):
            if first == 3 - last:
                continue
            bases = rng.integers(0, 4, (60, 48))
            bases[:, q - 20] = first
            bases[:, q] = last
            _, fwd = _check(bases, r)
            assert fwd.all() if first < 3 - last else not fwd.any(), (r, first, last)


@pytest.mark.parametrize("r", range(16))
def test_canon_every_tail_value_on_either_strand(r):
    """All 1024 tail values on the strand that wins; r < 4 are the residues at
    which the tail field straddles two code words, on both strands."""
    rng = np.random.default_rng(1100 + r)
    q = 32 + r
    every = (np.arange(1024)[:, None] >> (8 - 2 * np.arange(5))) & 3      # base 16 on top
    # forward wins: it starts with AAAAA, its last five bases run through every value
    bases = rng.integers(0, 4, (1024, 48))
    bases[:, q - 20:q - 15] = 0
    bases[:, q - 4:q + 1] = every
    tail, fwd = _check(bases, r)
    assert len(np.unique(tail[fwd])) >= 1000
    assert np.array_equal(tail[fwd], np.arange(1024)[fwd])
    # reverse wins: the k-mer ends with TTTTT, the reverse strand's last five
    # bases (the complements of the k-mer's first five, reversed) run through every value
    bases = rng.integers(0, 4, (1024, 48))
    bases[:, q - 4:q + 1] = 3
    bases[:, q - 20:q - 15] = _revcomp(every)
    tail, fwd = _check(bases, r)
    assert len(np.unique(tail[~fwd])) >= 1000
    assert np.array_equal(tail[~fwd], np.arange(1024)[~fwd])


def test_canon_eval_rejects_bad_residue():
    with pytest.raises(_lib.DrepHipError):
        _lib.canon_eval(np.zeros((1, 3), np.uint32), 16)


# ----------------------------------------------------------------------- GPU
def _sketch_vs_oracle(recs, s):
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(x) for x in recs])]).astype(np.uint64)
    gro = np.arange(len(recs) + 1, dtype=np.uint64)
    with _lib.Context(0, K, s, 42) as ctx:
        h, nh, ln = ctx.sketch_records(seq, rec_off, gro)
    for g, rec in enumerate(recs):
        want = oracle.sketch_records(rec, np.array([0, len(rec)], np.uint64), K, s, 42)
        assert nh[g] == len(want), (s, g, int(nh[g]), len(want))
        assert np.array_equal(h[g, :nh[g]], want), (s, g)
        assert (h[g, nh[g]:] == np.iinfo(np.uint64).max).all()
        assert int(ln[g]) == len(rec)


@pytest.fixture(scope="module")
def late_genome():
    """96 k-mers X m revcomp(X) back to back (2016 bases): 21 is odd, so their
    window ends fall on every residue mod 16, six times each, with m cycling
    through the four bases."""
    rng = np.random.default_rng(1200)
    X = rng.integers(0, 4, (96, 10))
    m = (np.arange(96) // 16 + np.arange(96)) % 4
    codes = np.concatenate([X, m[:, None], _revcomp(X)], axis=1).reshape(-1)
    ends = 20 + 21 * np.arange(96)
    for res in range(16):
        assert len(set(m[ends % 16 == res])) == 4, res
    return ASCII[codes]


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2000, 1])
def test_sketch_late_deciding_kmers_vs_oracle(late_genome, s):
    """s = 2000 >= the 1996 k-mers: T = kMaxThr, every k-mer is admitted and the
    admit stage overflows into the in-place path; s = 1: a real threshold."""
    _sketch_vs_oracle([late_genome], s)


def _n_run_genome(run, rng):
    """70,000 bases (two tiles and a partial third) with N runs of `run` bases
    ending at and starting at a chunk, a lane and a tile boundary (ending at
    32768, starting at 65536; the other boundaries 256 bases apart)."""
    g = ASCII[rng.integers(0, 4, 70_000)].copy()
    chunk_b = [5 * CHUNK + 4096, 5 * CHUNK + 4096 + 256]          # multiples of 16, not of 64
    lane_b = [9 * LANE + 8192, 9 * LANE + 8192 + 256]             # multiples of 64, not of the tile
    assert all(b % CHUNK == 0 and b % LANE for b in chunk_b) and all(b % LANE == 0 and b % TILE for b in lane_b)
    for before, after in (chunk_b, lane_b, (TILE, 2 * TILE)):
        g[before - run:before] = ord("N")
        g[after:after + run] = ord("N")
    return g


@pytest.mark.gpu
def test_sketch_n_runs_at_boundaries_vs_oracle():
    """The normal threshold path with staged admits; one genome per run length
    (1, 20, 21), since a tile boundary takes one run on each side."""
    rng = np.random.default_rng(1300)
    _sketch_vs_oracle([_n_run_genome(run, rng) for run in (1, 20, 21)], 1000)


@pytest.mark.gpu
def test_sketch_stage_overflow_at_real_threshold_vs_oracle():
    """65,536 bases at s = 4096: T is about 2^64 / 8, some 4,000 admits per tile
    against a stage of 128 -- the overflow path below kMaxThr."""
    rng = np.random.default_rng(1400)
    _sketch_vs_oracle([ASCII[rng.integers(0, 4, 65_536)]], 4096)
