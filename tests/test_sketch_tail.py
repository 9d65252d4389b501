"""The sketch hash kernel's tail index, taken from the other strand's high word
(drep_amd/csrc/canon.h).

The canonical 21-mer's bases 16-20 are the reversed complement of bases 0-4
of the strand that lost, so the kernel indexes its tail table -- stored
permuted by tail_index_of_head -- with the top 10 bits u of max(fhi, chi).
drephip_canon_eval returns the natural tail index through the same function.

CPU part: every u on either strand at every residue against a reference that
works from ASCII; the map is an involution and a bijection; strands decided
only at base 10, where max and min share their first ten bases.
GPU part: two genomes whose canonical tails run through all 1024 values, on
the forward and on the reverse strand, against the C oracle at a sketch size
that keeps every k-mer and at a real threshold.  Every comparison is exact."""
import numpy as np
import pytest

import oracle
from drep_amd import _lib

ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.zeros(256, np.uint32)
CODE[ASCII] = np.arange(4, dtype=np.uint32)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
K = 21
FIELDS = (np.arange(1024)[:, None] >> (8 - 2 * np.arange(5))) & 3      # field 0 (the top two bits) first


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
    return tail, fwd


def _revcomp(x):
    return 3 - x[:, ::-1]


def _loser_starts_with_every_u(r, forward_wins, rng):
    """1024 rows, row u: the 21-mer ending at base 32 + r whose losing strand
    starts with the five fields of u.  The winner starts with A and the loser's
    base 0 is u's top field, so base 0 fixes the winner for every u whose top
    field is not A; for the other 256 the winner goes on AAAAA A against a
    loser with T at base 5, fixed there at the latest."""
    q = 32 + r
    bases = rng.integers(0, 4, (1024, 48))
    kmer = bases[:, q - 20:q + 1]                      # a view: writes land in bases
    if forward_wins:
        kmer[:, 16:] = _revcomp(FIELDS)                # reverse strand's bases 0-4 = u
        kmer[:, :6] = 0                                # forward: AAAAA A
        kmer[:, 15] = 0                                # reverse strand's base 5 = T
    else:
        kmer[:, :5] = FIELDS                           # forward strand's bases 0-4 = u
        kmer[:, 15:] = 3                               # reverse: AAAAA A
        kmer[:, 5] = 3                                 # forward strand's base 5 = T
    return bases


def _rev5_not(u):
    f = 3 - ((u[:, None] >> (8 - 2 * np.arange(5))) & 3)
    return (f[:, ::-1] << (8 - 2 * np.arange(5))).sum(axis=1)


@pytest.mark.parametrize("r", range(16))
def test_tail_from_every_losing_head(r):
    """Every u in 0..1023 as the losing strand's first five bases, with the
    forward and with the reverse strand winning: the returned tail is the
    ASCII reference's, and is rev5(~u)."""
    rng = np.random.default_rng(1500 + r)
    u = np.arange(1024)
    for forward_wins in (True, False):
        bases = _loser_starts_with_every_u(r, forward_wins, rng)
        tail, fwd = _check(bases, r)
        assert fwd.all() if forward_wins else not fwd.any(), (r, forward_wins)
        assert np.array_equal(tail, _rev5_not(u)), (r, forward_wins)


@pytest.mark.parametrize("r", [0, 3, 4, 15])
def test_tail_map_is_an_involution_and_a_bijection(r):
    """u -> tail through the host entry (the function the kernel's table is
    stored by): onto 0..1023, and applying it twice gives u back."""
    rng = np.random.default_rng(1600 + r)
    for forward_wins in (True, False):
        y, _ = _check(_loser_starts_with_every_u(r, forward_wins, rng), r)
        assert np.array_equal(np.sort(y), np.arange(1024))
        assert np.array_equal(y[y], np.arange(1024))


@pytest.mark.parametrize("r", range(16))
def test_tail_strands_differ_only_at_base_10(r):
    """k-mers X m revcomp(X), |X| = 10: the strands share their first ten bases
    and their last ten, so max and min of the high words differ only from base
    10 on, and the top 10 bits of either give the tail."""
    rng = np.random.default_rng(1700 + r)
    q = 32 + r
    for m in range(4):
        bases = rng.integers(0, 4, (320, 48))
        X = rng.integers(0, 4, (320, 10))
        X[:256, :4] = (np.arange(256)[:, None] >> (6 - 2 * np.arange(4))) & 3
        bases[:, q - 20:q - 10] = X
        bases[:, q - 10] = m
        bases[:, q - 9:q + 1] = _revcomp(X)
        tail, fwd = _check(bases, r)
        assert fwd.all() if m < 2 else not fwd.any(), (r, m)
        # both strands end with revcomp(X[:5])
        want = (_revcomp(X[:, :5]) << (8 - 2 * np.arange(5))).sum(axis=1)
        assert np.array_equal(tail, want), (r, m)


# ----------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def tail_genomes():
    """1024 back-to-back 21-mers AAAAA + 11 random bases + tail, the tail running
    through all 1024 values (21,504 bases; 21 is odd, so the window ends fall on
    every residue mod 16): each starts with AAAAA, so its forward strand wins
    unless it ends with TTTTT.  The second genome is the reverse complement of
    the first: there the same k-mers win as the reverse strand.  With them the
    oracle's sketches at both sizes, computed once."""
    rng = np.random.default_rng(1800)
    codes = np.concatenate([np.zeros((1024, 5), np.int64), rng.integers(0, 4, (1024, 11)), FIELDS], axis=1)
    assert len({e % 16 for e in 20 + 21 * np.arange(1024)}) == 16
    fwd = codes.reshape(-1)
    recs = [ASCII[fwd], ASCII[3 - fwd[::-1]]]
    assert len(recs[0]) - K + 1 <= 32767
    want = {s: [oracle.sketch_records(rec, np.array([0, len(rec)], np.uint64), K, s, 42) for rec in recs]
            for s in (32767, 16)}
    return recs, want


@pytest.mark.gpu
@pytest.mark.parametrize("s", [32767, 16])
def test_sketch_every_tail_on_either_strand_vs_oracle(tail_genomes, s):
    """s = 32767 >= the 21,484 k-mers: T = kMaxThr, every distinct k-mer's hash
    is in the sketch, so a wrong table entry for any u changes the output.
    s = 16: a real threshold, the staged admits and the permuted table behind
    the prefilter."""
    recs, want = tail_genomes
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(x) for x in recs])]).astype(np.uint64)
    gro = np.arange(len(recs) + 1, dtype=np.uint64)
    with _lib.Context(0, K, s, 42) as ctx:
        h, nh, ln = ctx.sketch_records(seq, rec_off, gro)
    for g, rec in enumerate(recs):
        w = want[s][g]
        assert nh[g] == len(w), (s, g, int(nh[g]), len(w))
        assert np.array_equal(h[g, :nh[g]], w), (s, g)
        assert (h[g, nh[g]:] == np.iinfo(np.uint64).max).all()
        assert int(ln[g]) == len(rec)
    # the two genomes hold the same canonical k-mers
    assert np.array_equal(h[0], h[1])
