"""The four routes through the shared-hash screen's row-block driver
(screen.hip, screen_block: own grouping or every hash part's marks, into the
condensed segment or the pair list) still take the paths they took: equal
outputs do not show that -- a silent fallback, or light cells switched on, give
the same pairs -- so after every call the screen's and the sparse call's stats
are compared with tests/golden/screen_route_stats.json, recorded from the
library of the commit named in that file (never from the code under test):

    DREPHIP_LIB=<that commit's libdrephip.so> python tests/test_screen_routes.py <commit> > tests/golden/screen_route_stats.json

Every result is also compared with the C oracle's Mash merge (reference:
`mash dist`, drep/d_cluster.py:569-573), as tests/test_screen.py and
tests/test_sparse_sharded.py do.  The condensed routes' `simple` is not
pinned: there k_screen_simple reads cells that other lanes of the same launch
may still be marking, so its count is not a fixed number."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                   # run as a script (the recorder)
    sys.path.insert(0, ROOT)

import oracle                                              # noqa: E402
from drep_amd import _lib                                  # noqa: E402
from test_sparse import assert_list, case, rows_of         # noqa: E402
from test_sparse_sharded import all_marks, marked_list, to_device    # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "screen_route_stats.json")
CASES = [(64, 300), (1000, 200)]
W = 3                                                      # hash parts of the marked routes
SCREEN_KEYS = ("used", "entries", "runs", "checks", "marked")
SPARSE_KEYS = ("blocks", "direct", "fallback")
_DENSE = {}


def dense_oracle(s, N):
    """The oracle's whole condensed vectors of case(s, N), computed once."""
    if (s, N) not in _DENSE:
        H, NH, exp = case(s, N)
        oc, od = oracle.allpairs(H, NH, s, threads=8)
        assert int((oc > 0).sum()) == len(exp[0])
        oc.setflags(write=False)
        od.setflags(write=False)
        _DENSE[(s, N)] = (oc, od)
    return _DENSE[(s, N)]


def condensed(ctx, dH, dNH, N, r0, r1, marks=None):
    """Rows [r0, r1) into a condensed segment (from the marks, if given)."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    start = lambda i: i * N - i * (i + 1) // 2             # noqa: E731
    n = start(min(r1, N - 1)) - start(r0)
    co = torch.zeros(n, dtype=torch.int16, device="cuda")
    do = torch.zeros(n, dtype=torch.int16, device="cuda")
    if marks is None:
        ctx.allpairs_device(dH.data_ptr(), dNH.data_ptr(), N, r0, r1, co.data_ptr(), do.data_ptr(), st)
    else:
        cells, recs = marks
        ctx.allpairs_device_marked(dH.data_ptr(), dNH.data_ptr(), N, r0, r1, co.data_ptr(), do.data_ptr(),
                                   cells.data_ptr(), len(cells), recs.data_ptr(), len(recs), st)
    torch.cuda.synchronize()
    return co.cpu().numpy().view(np.uint16), do.cpu().numpy().view(np.uint16), start(r0), n


def sparse_list(ctx, dH, dNH, N, r0, r1, room):
    """allpairs_sparse_device's list sorted by (i, j); a guard region past `room` stays untouched."""
    import torch
    SENT = np.uint32(0xDEADBEEF).view(np.int32).item()
    buf = torch.full((room + 16, 4), SENT, dtype=torch.int32, device="cuda")
    rc, n = ctx.allpairs_sparse_device(dH.data_ptr(), dNH.data_ptr(), N, r0, r1, buf.data_ptr(), room,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and n <= room, (rc, n, room)
    out = buf.cpu().numpy().view(np.uint32)
    assert (out[room:] == np.uint32(0xDEADBEEF)).all()
    rec = out[:n]
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
    return (np.ascontiguousarray(rec[:, 0]), np.ascontiguousarray(rec[:, 1]), rec[:, 2].astype(np.uint16),
            rec[:, 3].astype(np.uint16))


def route_stats(s, N, env):
    """Every route over rows (37, 121) and (0, N), each result checked against
    the oracle: {route: its pinned stats}.  `env`: a pytest MonkeyPatch."""
    H, NH, exp = case(s, N)
    oc, od = dense_oracle(s, N)
    dH, dNH = to_device(H, NH)
    got = {}
    with _lib.Context(0, 21, s, 42) as ctx:
        ctx.set_allpairs_screen(ctx.SCREEN_ON)
        env.setenv("DREPHIP_SPARSE_BLOCK_ROWS", str(3 * ctx.screen_geometry()))
        cells, recs, _ = all_marks(ctx, dH, dNH, N, W)
        assert len(cells) > 0 and len(recs) > 0

        def pinned(sparse):
            st = ctx.screen_stats()
            d = {k: st[k] for k in SCREEN_KEYS + (("simple",) if sparse else ())}
            if sparse:
                sp = ctx.sparse_stats()
                d.update({k: sp[k] for k in SPARSE_KEYS})
            return d

        def run_condensed(name, r0, r1, marks):
            c, d, o, n = condensed(ctx, dH, dNH, N, r0, r1, marks)
            what = "%s rows [%d, %d)" % (name, r0, r1)
            assert np.array_equal(c, oc[o:o + n]), what
            assert np.array_equal(d, od[o:o + n]), what
            got["%s[%d,%d)" % (name, r0, r1)] = pinned(False)

        def run_sparse(name, r0, r1, marked):
            want = rows_of(exp, r0, r1)
            g = marked_list(ctx, dH, dNH, N, r0, r1, cells, recs, len(want[0])) if marked else \
                sparse_list(ctx, dH, dNH, N, r0, r1, len(want[0]))
            assert_list(g, want, "%s rows [%d, %d)" % (name, r0, r1))
            got["%s[%d,%d)" % (name, r0, r1)] = pinned(True)

        for r0, r1 in ((37, 121), (0, N)):
            run_condensed("device", r0, r1, None)
            run_condensed("device_marked", r0, r1, (cells, recs))
            run_sparse("sparse", r0, r1, False)
            run_sparse("sparse_marked", r0, r1, True)
        env.setenv("DREPHIP_SCREEN_LIGHT", "1")
        run_sparse("light_sparse", 0, N, False)
        run_condensed("light_device", 0, N, None)
        env.delenv("DREPHIP_SCREEN_LIGHT")
    return got


@pytest.mark.parametrize("s,N", CASES)
def test_routes_keep_their_paths(s, N, monkeypatch):
    gold = json.load(open(GOLDEN))["stats"]["s%d_N%d" % (s, N)]
    got = route_stats(s, N, monkeypatch)
    assert sorted(got) == sorted(gold)
    for name in sorted(got):
        print(name, got[name])
    for name in sorted(got):
        assert got[name] == gold[name], (name, got[name], gold[name])
        assert got[name]["used"]
        if "fallback" in got[name]:
            assert got[name]["fallback"] == 0 and got[name]["blocks"] >= 1


if __name__ == "__main__":
    # the recorder: every route's stats, twice (they are fixed numbers), as JSON
    with pytest.MonkeyPatch.context() as mp:
        stats = {"s%d_N%d" % c: route_stats(*c, mp) for c in CASES}
        again = {"s%d_N%d" % c: route_stats(*c, mp) for c in CASES}
    assert stats == again
    print(json.dumps({"recorded_from": sys.argv[1], "hash_parts": W, "block_rows": "3R", "stats": stats}, indent=1,
                     sort_keys=True))
