"""The three forms of the query-against-reference call (the dense rectangle,
records, best hits) crossed with its three kernels (table, band, merge), the
two-set screen off and forced, and one block or several: every route of the
host side's block driver.  Expected values: the C oracle's Mash
merge of every (query, reference) pair, exactly.

The sets are tests/test_rect_screen.py's case(64): 41 queries x 97 references
with empty, partial and twin rows and the largest admitted hash; 97 is odd and a
multiple of no column tile.  Rows [3, 38): a first row above 0, rows of the
41 on either side that must stay untouched, and 35 rows in blocks of 5 (the
scratch rectangle's bound) or 7 (the screen's), the smaller bound winning where
both apply."""
import numpy as np
import pytest

from drep_amd import _lib
from test_rect_screen import AP_BAND, AP_MERGE, AP_TABLE, NREF, POISON, case, did_not_run, expected_top, ran

pytestmark = pytest.mark.gpu
S, Q0, Q1, TOP = 64, 3, 38, 3
KNOBS = {"DREPHIP_RECT_BLOCK_ROWS": "5", "DREPHIP_RECT_TOP_BLOCK_ROWS": "5", "DREPHIP_RECT_SCREEN_BLOCK_ROWS": "7"}


def screened_blocks(form, kernel, small):
    """The screen's block count of a forced call over the 35 rows: the scratch
    rectangle's 5-row bound applies to best hits and to records by the band
    kernel (the smaller of the two bounds wins: 7 blocks), the screen's own
    7-row bound alone to the dense form and to records by the table kernel,
    which appends by itself (5 blocks)."""
    if not small:
        return 1
    return 7 if form == "top" or (form == "records" and kernel == AP_BAND) else 5


def dense(ctx, H, NH, nq, ec, ed):
    import torch
    dh = torch.from_numpy(H.copy().view(np.int64)).cuda()
    dn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
    bc = torch.full((nq, NREF), POISON, dtype=torch.int16, device="cuda")
    bd = torch.full((nq, NREF), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.dist_rect_device(dh.data_ptr(), dn.data_ptr(), nq, dh.data_ptr(), dn.data_ptr(), NREF, Q0, Q1,
                         bc[Q0].data_ptr(), bd[Q0].data_ptr())
    for got, exp in ((bc, ec), (bd, ed)):
        g = got.cpu().numpy().view(np.uint16)
        assert np.array_equal(g[Q0:Q1], exp[Q0:Q1]), np.argwhere(g[Q0:Q1] != exp[Q0:Q1])[:8]
        assert (g[:Q0] == POISON).all() and (g[Q1:] == POISON).all()        # rows outside the range: untouched


def records(ctx, H, NH, nq, ec, ed):
    q, r, c, d = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, Q0, Q1)
    k = ec[Q0:Q1] > 0
    assert np.array_equal(q, np.nonzero(k)[0] + Q0) and np.array_equal(r, np.nonzero(k)[1])
    assert np.array_equal(c, ec[Q0:Q1][k]) and np.array_equal(d, ed[Q0:Q1][k])


def best_hits(ctx, H, NH, nq, ec, ed):
    got = ctx.dist_rect_top(H[:nq], NH[:nq], H, NH, TOP, Q0, Q1)
    for a, b in zip(got, expected_top(ec[Q0:Q1], ed[Q0:Q1], TOP)):
        assert np.array_equal(a, b)


FORMS = {"dense": dense, "records": records, "top": best_hits}


@pytest.mark.parametrize("small", [False, True], ids=["one_block", "small_blocks"])
@pytest.mark.parametrize("force", [False, True], ids=["screen_off", "screen_force"])
@pytest.mark.parametrize("kernel", [AP_TABLE, AP_BAND, AP_MERGE], ids=["table", "band", "merge"])
@pytest.mark.parametrize("form", ["dense", "records", "top"])
def test_form_kernel_screen_blocks(form, kernel, force, small, monkeypatch):
    H, NH, nq, (ec, ed) = case(S)
    for knob, rows in KNOBS.items():
        if small:
            monkeypatch.setenv(knob, rows)
        else:
            monkeypatch.delenv(knob, raising=False)
    with _lib.Context(0, 21, S, 42) as ctx:
        if kernel == AP_BAND:
            ctx.set_rect_band(ctx.RECT_BAND_FORCE, 64)
        elif kernel == AP_MERGE:
            ctx.set_allpairs_path(ctx.AP_MERGE)
        ctx.set_rect_screen(ctx.RECT_SCREEN_FORCE if force else ctx.RECT_SCREEN_OFF)
        FORMS[form](ctx, H, NH, nq, ec, ed)
        assert ctx.last_rect_info() == (kernel, 0)
        if force and kernel != AP_MERGE:
            ran(ctx, screened_blocks(form, kernel, small))
        else:
            did_not_run(ctx)                                                # (the merge kernel is never screened)
