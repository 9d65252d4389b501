"""The sketch hash kernel's reject-early test (drep_amd/csrc/prefilter.h).

A k-mer reaches the test as the two fmix64 states before their last multiply,
(q1, q2); its hash is h1 = fin(q1 C2) + fin(q2 C2), fin(p) = p ^ (p >> 33).
The prefilter tests v = hi((q1 + q2) C2) + 1 <= Tp, Tp = hi(T) + 2 (all ones
from hi(T) = 0xFFFFFFFE on), a necessary condition for h1 <= T: hi(P) and
hi(h1) differ by the carries of two low-word sums, -1, 0 or +1.

CPU part: the predicate through the host entry (the kernel's own inline
functions) on crafted (q1, q2, T) families -- pairs with a chosen h1 are built
by choosing the two fin values and mapping back through fin (an involution)
and the inverse of C2.
GPU part: sketches against the C oracle at the smallest shapes where the bound
can go wrong."""
import numpy as np
import pytest

import oracle
from drep_amd import _lib

C2 = 0xc4ceb9fe1a85ec53
C2_INV = pow(C2, -1, 1 << 64)
M64 = (1 << 64) - 1
U = np.uint64

HI_T = [0, 1, 2, 5, 1 << 21, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFC, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF]
PER_TARGET = 400


def _fin(p):
    return p ^ (p >> U(33))


def _pairs_with_h1(h1, rng):
    """(q1, q2) with fin(q1 C2) + fin(q2 C2) = h1, one pair per entry of h1: the
    first fin value is random with its low word drawn from {0, 1, all ones,
    random} so that both low-word carries take both values."""
    n = len(h1)
    lo = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    kind = rng.integers(0, 4, n)
    lo = np.where(kind == 0, U(0), np.where(kind == 1, U(1), np.where(kind == 2, U(0xFFFFFFFF), lo)))
    f1 = (rng.integers(0, 1 << 32, n, dtype=np.uint64) << U(32)) | lo
    f2 = h1 - f1
    return _fin(f1) * U(C2_INV), _fin(f2) * U(C2_INV)


def _family(hi_t, rng):
    """Thresholds with high word hi_t and the (q1, q2) cases held against each:
    h1 at T, T - 1, 0 and hi(T) << 32, h1 just above T, random h1 below T, the
    two window values hi(T) + 1 and hi(T) + 2, and the rejected range
    hi(T) + 3 .. 0xFFFFFFFD at both ends and inside."""
    out = []
    for lo_t in (0, 1, int(rng.integers(2, 0xFFFFFFFF)), 0xFFFFFFFF):
        T = (hi_t << 32) | lo_t
        targets = [T, (T - 1) & M64, 0, hi_t << 32, (T + 1) & M64]
        his = [hi_t + d for d in (1, 2, 3, 4) if hi_t + d <= 0xFFFFFFFF] + [0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF]
        if hi_t + 3 < 0xFFFFFFFD:
            his += [int(x) for x in rng.integers(hi_t + 3, 0xFFFFFFFD, 3)]
        for h in his:
            for l in (0, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))):
                targets.append((h << 32) | l)
        h1 = np.repeat(np.array(targets, dtype=np.uint64), PER_TARGET)
        below = rng.integers(0, T + 1, PER_TARGET, dtype=np.uint64, endpoint=False) if T else np.zeros(1, np.uint64)
        h1 = np.concatenate([h1, below])
        q1, q2 = _pairs_with_h1(h1, rng)
        out.append((T, h1, q1, q2))
    return out


@pytest.fixture(scope="module")
def families():
    rng = np.random.default_rng(2107)
    return {hi_t: _family(hi_t, rng) for hi_t in HI_T}


def _carries(q1, q2):
    p1, p2 = q1 * U(C2), q2 * U(C2)
    m = U(0xFFFFFFFF)
    cp = ((p1 & m) + (p2 & m)) >> U(32)
    cf = ((_fin(p1) & m) + (_fin(p2) & m)) >> U(32)
    return cf.astype(int), cp.astype(int)


def test_prefilter_no_false_reject(families):
    """exact (h1 <= T) implies pass, for every family; the library's exact bit
    is the one computed here from Python-side h1; every carry combination
    occurs among the admitted cases of every hi(T)."""
    total = 0
    with np.errstate(over="ignore"):
        for hi_t, fam in families.items():
            combos = set()
            for T, h1, q1, q2 in fam:
                p1, p2 = q1 * U(C2), q2 * U(C2)
                assert np.array_equal(_fin(p1) + _fin(p2), h1)          # the construction gives the chosen h1
                ok, exact = _lib.prefilter_eval(q1, q2, T)
                assert np.array_equal(exact, h1 <= U(T)), hex(T)
                bad = exact & ~ok
                assert not bad.any(), (hex(T), [hex(int(x)) for x in h1[bad][:4]])
                assert exact.sum() >= 3 * PER_TARGET // 2
                cf, cp = _carries(q1[exact], q2[exact])
                combos |= set(zip(cf.tolist(), cp.tolist()))
                if hi_t >= 0xFFFFFFFE:                                   # saturated bound: nothing is rejected
                    assert ok.all(), hex(T)
                total += len(h1)
            assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}, (hex(hi_t), combos)
    assert total >= 100_000, total


def test_prefilter_window_is_three_values(families):
    """For hi(T) <= 0xFFFFFFFD every case with hi(T) + 3 <= hi(h1) <= 0xFFFFFFFD
    is rejected: the window holds hi(T) + 3 values of hi(h1), no more."""
    checked = 0
    for hi_t, fam in families.items():
        if hi_t > 0xFFFFFFFD:
            continue
        for T, h1, q1, q2 in fam:
            hh = (h1 >> U(32)).astype(np.int64)
            sel = (hh >= hi_t + 3) & (hh <= 0xFFFFFFFD)
            ok, _ = _lib.prefilter_eval(q1[sel], q2[sel], T)
            assert not ok.any(), (hex(T), [hex(int(x)) for x in h1[sel][ok][:4]])
            if hi_t + 3 <= 0xFFFFFFFD:
                assert sel.sum() >= 2 * PER_TARGET
            checked += int(sel.sum())
    assert checked >= 50_000, checked


# ----------------------------------------------------------------------- GPU
LENGTHS = [21, 2021, 40_000, 100_000]      # one k-mer; nk = 2001 (first T below kMaxThr at s = 1000); past one
                                           # 32768-base tile; at s = 1 the smallest reachable hi(T), ~8.6e4


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [5, 6])
@pytest.mark.parametrize("s", [1000, 1])
def test_sketch_small_thresholds_vs_oracle(s, seed):
    rng = np.random.default_rng(seed)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = [A[rng.integers(0, 4, n)] for n in LENGTHS]
    seq = np.concatenate(recs)
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    gro = np.arange(len(recs) + 1, dtype=np.uint64)
    with _lib.Context(0, 21, s, 42) as ctx:
        h, nh, ln = ctx.sketch_records(seq, rec_off, gro)
    for g, r in enumerate(recs):
        want = oracle.sketch_records(r, np.array([0, len(r)], np.uint64), 21, s, 42)
        assert nh[g] == len(want) == min(s, len(want)), (s, len(r))
        assert np.array_equal(h[g, :nh[g]], want), (s, len(r))
        assert (h[g, nh[g]:] == np.iinfo(np.uint64).max).all()
        assert int(ln[g]) == len(r)
