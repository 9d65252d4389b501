#!/usr/bin/env python3
"""Writes tests/golden/pvalue_grid.json: seeded rows (common, len_a, len_b, s,
exact) for the Mash p-value, `exact` being the regularized incomplete beta
I_r(common, n - common + 1) = P(X >= common), X ~ Binomial(n, r), evaluated
with mpmath at 80 digits and stored as a 30-digit decimal string.  r and n
follow d_cluster.mash_pvalue (k = 21).  Not run by the tests; needs mpmath.

Conditions checked here (the run fails when one does not hold):
  - rows whose exact value lies within a factor 4 of 2^-1022 are dropped;
  - a row whose '%g' text from mash_pvalue (scipy) differs from the exact
    value's is dropped, and at most 1 row in 1000 may go that way;
  - at least 300 rows remain in the normal range and at least 100 below it;
  - at most 1000 rows are written.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 21
SKETCH_SIZES = (1, 16, 400, 1000, 2048, 10000, 32767)
LEN_MIN, LEN_MAX = 25, 2 * 10 ** 11


def r_and_n(len_a, len_b, s, k=K):
    """r and n as mash_pvalue forms them (float64, this order)."""
    kspace = 4.0 ** k
    px = 1.0 / (1.0 + kspace / np.float64(len_a))
    py = 1.0 / (1.0 + kspace / np.float64(len_b))
    r = px * py / (px + py - px * py)
    M = kspace * (px + py) / (1.0 + r)
    return float(r), int(np.floor(np.minimum(M, s)))


def exact_tail(mp, c, n, r):
    """P(X >= c) for X ~ Binomial(n, r); r is the float64 value, taken exactly."""
    if c == 0:
        return mp.mpf(1)
    if c > n:
        return mp.mpf(0)
    return mp.betainc(c, n - c + 1, 0, mp.mpf(r), regularized=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=960)
    ap.add_argument("--seed", type=int, default=20240521)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pvalue_grid.json"))
    a = ap.parse_args()
    import mpmath as mp
    from drep_amd.d_cluster import mash_pvalue
    mp.mp.dps = 80
    rng = np.random.default_rng(a.seed)
    tiny = mp.mpf(2) ** -1022
    rows, dropped_edge, dropped_text, seen = [], 0, 0, 0
    while len(rows) < a.rows:
        s = int(SKETCH_SIZES[rng.integers(len(SKETCH_SIZES))])
        # log-uniform lengths; one draw in four keeps the two within a factor 4
        la = int(round(float(np.exp(rng.uniform(np.log(LEN_MIN), np.log(LEN_MAX))))))
        if rng.integers(4) == 0:
            lb = int(np.clip(round(la * float(np.exp(rng.uniform(-1.4, 1.4)))), LEN_MIN, LEN_MAX))
        else:
            lb = int(round(float(np.exp(rng.uniform(np.log(LEN_MIN), np.log(LEN_MAX))))))
        r, n = r_and_n(la, lb, s)
        how = int(rng.integers(4))
        if how == 0:
            c = int(rng.integers(1, 41))
        elif how == 1:
            c = int(rng.integers(1, n + 2))
        elif how == 2:
            mean, sd = n * r, max(1.0, (n * r * (1.0 - r)) ** 0.5)
            c = int(np.clip(round(mean + float(rng.uniform(-6, 12)) * sd), 1, n + 1))
        else:
            c = int(rng.integers(1, 201))
        if c > s:
            continue
        seen += 1
        ex = exact_tail(mp, c, n, r)
        if ex != 0 and tiny / 4 <= ex <= tiny * 4:
            dropped_edge += 1
            continue
        if ex >= tiny:
            host = float(mash_pvalue(np.array([c]), np.array([la]), np.array([lb]), s)[0])
            if "%g" % host != "%g" % float(ex):
                dropped_text += 1
                continue
        rows.append({"common": c, "len_a": la, "len_b": lb, "s": s, "exact": mp.nstr(ex, 30)})
    normal = sum(1 for q in rows if mp.mpf(q["exact"]) >= tiny)
    below = len(rows) - normal
    print("rows %d (normal %d, below 2^-1022 %d); drawn %d, dropped near 2^-1022 %d, dropped on text %d"
          % (len(rows), normal, below, seen, dropped_edge, dropped_text))
    assert len(rows) <= 1000
    assert dropped_text * 1000 <= seen, "more than 1 row in 1000 dropped on its text"
    assert normal >= 300 and below >= 100, (normal, below)
    with open(a.out, "w") as f:
        json.dump({"k": K, "seed": a.seed, "mpmath_dps": 80, "rows": rows}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
