"""The query rectangle (drephip_dist_rect*, the RECT flavour of k_allpairs_q /
ap_columns, k_rect_merge, k_rect_compact, k_rect_top in allpairs.hip) at the
geometry it was built for and at its seams: column tiles wide enough for a
wave's column loop to turn (several columns per wave, the mid-loop record
flush of RECT, SPARSE, item groups of more than one item, a second trip of the
failed-table fallback loop), launches split at max_blocks, k_rect_top's grid
stride over long rows that start mid-vector, and the row blocks of the record
form's merge route.

Expected values: the C oracle's literal merge over the stack (queries, then
references), rows [0, Q) only; best hits by test_rect_top.expected_top.  Every
comparison is bit for bit on common and denom.  The geometry a test ran at is
read from the library's own `rect plan` line (DREPHIP_DEBUG), not restated."""
import re
from fractions import Fraction

import numpy as np
import pytest

import edge_cases
import oracle
from drep_amd import _lib
from test_rect import ERR_NOMEM, case, unbuildable_rows
from test_rect_top import EMPTY, POISON, expected_top, sets

pytestmark = pytest.mark.gpu

_PLAN = re.compile(r"\[drephip\] rect plan: R (\d+) C (\d+) items (\d+) slots (\d+) gmax (\d+) pieces (\d+)")


def plans(capfd):
    """The `rect plan` lines printed since the last read, as dicts."""
    keys = ("R", "C", "items", "slots", "gmax", "pieces")
    return [dict(zip(keys, map(int, m))) for m in _PLAN.findall(capfd.readouterr().err)]


def oracle_rows(QH, QN, RH, RN, s):
    """(common, denom) [Q, N] by the oracle's merge: rows [0, Q) of the stack
    (queries, then references), so only Q x (Q + N) pairs are merged."""
    Q, N = len(QN), len(RN)
    M = Q + N
    oc, od = oracle.allpairs(np.concatenate([QH, RH]), np.concatenate([QN, RN]).astype(np.uint32), s, r0=0, r1=Q,
                             threads=8)
    q = np.arange(Q, dtype=np.int64)[:, None]
    r = np.arange(N, dtype=np.int64)[None, :] + Q
    t = q * M - q * (q + 1) // 2 + (r - q - 1)
    return oc[t], od[t]


def records_of(ec, ed):
    """(q, r, common, denom) of the non-zero cells, sorted by (q, r): what
    Context.dist_rect_sparse returns."""
    k = ec > 0
    qq, rr = np.nonzero(k)
    return qq, rr, ec[k], ed[k]


def same_records(got, exp):
    return all(np.array_equal(g, e) for g, e in zip(got, exp))


# The dense results are taken through the device entry points into device
# buffers poisoned by the test, a guard row before and after: the host forms
# copy a scratch buffer of the context out whole, and freshly allocated device
# memory may still hold an earlier call's (correct) results, so through them a
# cell or a row that a kernel never wrote need not show.
def upload(QH, QN, RH, RN):
    import torch
    t = [torch.from_numpy(a.copy().view(v)).cuda() for a, v in ((QH, np.int64), (QN, np.int32), (RH, np.int64), (RN, np.int32))]
    torch.cuda.synchronize()
    return t, (t[0].data_ptr(), t[1].data_ptr(), len(QN), t[2].data_ptr(), t[3].data_ptr(), len(RN))


def rect_device(ctx, dev, q0=0, q1=None, merge=False):
    """(common, denom) of rows [q0, q1) by drephip_dist_rect[_merge]_device;
    asserts that the guard rows kept their poison."""
    import torch
    _, args = dev
    Q, N = args[2], args[5]
    q1 = Q if q1 is None else q1
    rows = q1 - q0
    out = [torch.full((rows + 2, N), 0xBEEF - 0x10000, dtype=torch.int16, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    ctx.dist_rect_device(*args, q0, q1, out[0][1].data_ptr(), out[1][1].data_ptr(), merge=merge)
    c, d = (o.cpu().numpy().view(np.uint16) for o in out)
    for a in (c, d):
        assert (a[0] == 0xBEEF).all() and (a[-1] == 0xBEEF).all()
    return c[1:-1], d[1:-1]


def check_rect(got, ec, ed):
    c, d = got
    assert c.shape == ec.shape and d.shape == ed.shape
    assert np.array_equal(c, ec), np.argwhere(c != ec)[:8]
    assert np.array_equal(d, ed), np.argwhere(d != ed)[:8]


# ------------------------------------------------------------ the wide sets
# geometry_sketches(N, s) as references, its first rows as queries: dense sets
# (nearly every cell non-zero) with zero-key rows, twin rows (g % 16 == 7),
# partial rows and empty rows; every query is also a reference.
_WIDE_SETS = {1000: (1025, 700), 100: (3000, 1368), 64: (2049, 1824)}      # s: (N, the most queries used)
_WIDE = {}


def wide(s, Q):
    """(H, NH, common, denom) of the s set with its first Q rows as queries.
    The set and the oracle's rectangle of its largest Q are computed once and
    shared read-only; a smaller Q is the first rows of that rectangle."""
    if s not in _WIDE:
        N, qmax = _WIDE_SETS[s]
        H, NH = edge_cases.geometry_sketches(N, s, seed=7000 + s)
        ec, ed = oracle_rows(H[:qmax], NH[:qmax], H, NH, s)
        for a in (H, NH, ec, ed):
            a.setflags(write=False)
        _WIDE[s] = (H, NH, ec, ed)
    H, NH, ec, ed = _WIDE[s]
    assert Q <= len(ec)
    return H, NH, ec[:Q], ed[:Q]


def holds_what_it_is_for(H, NH, Q, ed, s):
    """Among the queries: a row with the key 0, a row with two keys of one low
    word, a partial row, an empty row; and denominators below s."""
    qn = NH[:Q]
    twin = any(len(np.unique(H[g, :qn[g]] & np.uint64(0xFFFFFFFF))) < qn[g] for g in range(7, Q, 16))
    return bool(((H[:Q, 0] == 0) & (qn > 0)).any() and twin and ((qn > 0) & (qn < s)).any() and (qn == 0).any()
                and (ed < s).any())


#           s     Q     N     DREPHIP_AP_R  R  C
_SHAPES = [(1000, 700, 1025, 1, 1, 512),           # the production tile, NCH 16; a last tile of one column
           (1000, 300, 1025, 1, 1, 128),           # an intermediate tile
           (1000, 520, 1025, None, 4, 64),         # interleaved rows with a real column loop
           (100, 1368, 3000, 4, 4, 512),           # R x columns per wave = 128: the mid-loop record flush
           (64, 1824, 2049, None, 8, 256)]         # R = 8, NCH 8, R x columns per wave = 128


def wide_env(monkeypatch, env_r, hit=None):
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    if env_r is None:
        monkeypatch.delenv("DREPHIP_AP_R", raising=False)
    else:
        monkeypatch.setenv("DREPHIP_AP_R", str(env_r))
    if hit is not None:
        monkeypatch.setenv("DREPHIP_AP_HIT", str(hit))


def is_wide(p, R, C):
    """The plan line of a call that reached the geometry the test is for."""
    return p["R"] == R and p["C"] == C and p["gmax"] > 1 and p["slots"] > p["items"] and p["items"] >= 2048


def check_wide(ctx, capfd, QH, QN, H, NH, ec, ed, R, C):
    """dist_rect (device and host form) and dist_rect_sparse against the
    oracle, every call at (R, C)."""
    dev = upload(QH, QN, H, NH)
    capfd.readouterr()
    got = rect_device(ctx, dev)
    ps = plans(capfd)
    assert len(ps) == 1 and is_wide(ps[0], R, C), ps
    check_rect(got, ec, ed)
    check_rect(ctx.dist_rect(QH, QN, H, NH), ec, ed)    # the host form
    ps = plans(capfd)
    assert len(ps) == 1 and is_wide(ps[0], R, C), ps
    exp = records_of(ec, ed)
    got = ctx.dist_rect_sparse(QH, QN, H, NH, cap=len(exp[0]))
    ps = plans(capfd)
    assert len(ps) == 1 and is_wide(ps[0], R, C), ps
    assert len(got[0]) == len(exp[0]) and same_records(got, exp)


@pytest.mark.parametrize("s,Q,N,env_r,R,C", _SHAPES)
def test_wide_tiles_vs_oracle(s, Q, N, env_r, R, C, monkeypatch, capfd):
    H, NH, ec, ed = wide(s, Q)
    assert len(NH) == N and holds_what_it_is_for(H, NH, Q, ed, s)
    assert (ec > 0).mean() > 0.5                        # dense: the records fill a wave's 64 slots
    wide_env(monkeypatch, env_r)
    with _lib.Context(0, 21, s, 42) as ctx:
        check_wide(ctx, capfd, H[:Q], NH[:Q], H, NH, ec, ed, R, C)


def test_wide_tile_without_hit_masks(monkeypatch, capfd):
    """DREPHIP_AP_HIT=0: the other ap_columns instantiation chain, at C = 512."""
    s, Q, N, env_r, R, C = _SHAPES[0]
    H, NH, ec, ed = wide(s, Q)
    wide_env(monkeypatch, env_r, hit=0)
    with _lib.Context(0, 21, s, 42) as ctx:
        check_wide(ctx, capfd, H[:Q], NH[:Q], H, NH, ec, ed, R, C)


def test_wide_tile_row_range_writes_only_its_cells(monkeypatch, capfd):
    """Rows [3, 518) of 520 at R = 4: the first row is no multiple of R, the
    last row tile is short, and the rows before and after stay untouched."""
    s, Q, N, env_r, R, C = _SHAPES[2]
    H, NH, ec, ed = wide(s, Q)
    q0, q1 = 3, 518
    wide_env(monkeypatch, env_r)
    with _lib.Context(0, 21, s, 42) as ctx:
        dev = upload(H[:Q], NH[:Q], H, NH)
        capfd.readouterr()
        got = rect_device(ctx, dev, q0, q1)             # (asserts the guard rows)
        ps = plans(capfd)
        assert len(ps) == 1 and is_wide(ps[0], R, C), ps
        check_rect(got, ec[q0:q1], ed[q0:q1])
        # the host form into the caller's buffers
        bc = np.full((q1 - q0 + 2, N), 0xBEEF, dtype=np.uint16)        # a guard row before and after
        bd = np.full((q1 - q0 + 2, N), 0xBEEF, dtype=np.uint16)
        ctx.dist_rect(H[:Q], NH[:Q], H, NH, q0, q1, bc[1:-1], bd[1:-1])
        assert (bc[0] == 0xBEEF).all() and (bc[-1] == 0xBEEF).all()
        assert (bd[0] == 0xBEEF).all() and (bd[-1] == 0xBEEF).all()
        check_rect((bc[1:-1], bd[1:-1]), ec[q0:q1], ed[q0:q1])
        capfd.readouterr()
        exp = records_of(ec[q0:q1], ed[q0:q1])
        got = ctx.dist_rect_sparse(H[:Q], NH[:Q], H, NH, q0, q1, cap=len(exp[0]))
        assert np.array_equal(got[0], exp[0] + q0) and same_records(got[1:], exp[1:])


def test_wide_tile_failed_tables(monkeypatch, capfd):
    """Query rows 0 and 7 (and the same reference rows) hold three hashes with
    one low word, rows 1 and 8 share two of them: inside a tile of R x C =
    8 x 256 cells the literal-merge fallback's lanes take a second trip."""
    s, Q, N, env_r, R, C = _SHAPES[4]
    H0, NH0, _, _ = wide(s, Q)
    H, NH = H0.copy(), NH0.copy()
    h, nh = unbuildable_rows(s)
    for i in (0, 1, 7, 8):
        H[i], NH[i] = h[i], nh[i]
    low = [h[i] & np.uint64(0xFFFFFFFF) for i in (0, 7)]
    assert all((np.unique(x, return_counts=True)[1] == 3).any() for x in low)      # three keys, one low word
    QH, QN = H[:Q].copy(), NH[:Q].copy()
    ec, ed = oracle_rows(QH, QN, H, NH, s)
    assert ec[0, 0] == s and ec[7, 7] == s and ec[0, 1] >= 2 and ec[8, 7] >= 2 and ec[0, 7] >= 3
    wide_env(monkeypatch, env_r)
    with _lib.Context(0, 21, s, 42) as ctx:
        check_wide(ctx, capfd, QH, QN, H, NH, ec, ed, R, C)
    assert R * C > 1024                                 # more cells per tile than the workgroup has lanes


# ------------------------------------------------------------ 2. split launches
CAP_ITEMS = "2048"           # DREPHIP_MAX_LAUNCH_ITEMS: 8 workgroups per dispatch, of 1024 or of 256 lanes


@pytest.mark.parametrize("s", [64, 1000])
def test_split_rect_launches_match_oracle(s, monkeypatch, capfd):
    """launch_q in pieces of 8 items: the rectangle and the records."""
    H, NH, nq, (ec, ed) = case(s)
    monkeypatch.setenv("DREPHIP_DEBUG", "1")
    monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", CAP_ITEMS)
    exp = records_of(ec, ed)
    with _lib.Context(0, 21, s, 42) as ctx:
        dev = upload(H[:nq], NH[:nq], H, NH)
        capfd.readouterr()
        got = rect_device(ctx, dev)
        ps = plans(capfd)
        assert len(ps) == 1 and ps[0]["pieces"] > 1 and ps[0]["slots"] > 8, ps
        check_rect(got, ec, ed)
        got = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, cap=len(exp[0]))
        ps = plans(capfd)
        assert len(ps) == 1 and ps[0]["pieces"] > 1, ps
        assert len(got[0]) == len(exp[0]) and same_records(got, exp)


def test_split_merge_launches_match_oracle(monkeypatch):
    """k_rect_merge in pieces of 2048 cells (41 x 97 = 3977: the second one
    partial), and the k_rect_compact pieces of the record form's merge route."""
    s = 64
    H, NH, nq, (ec, ed) = case(s)
    assert 2048 < ec.size < 2 * 2048
    monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", CAP_ITEMS)
    exp = records_of(ec, ed)
    with _lib.Context(0, 21, s, 42) as ctx:
        dev = upload(H[:nq], NH[:nq], H, NH)
        check_rect(rect_device(ctx, dev, merge=True), ec, ed)
        check_rect(rect_device(ctx, dev, 3, 38, merge=True), ec[3:38], ed[3:38])
        ctx.set_allpairs_path(ctx.AP_MERGE)
        got = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, cap=len(exp[0]))
        assert len(got[0]) == len(exp[0]) and same_records(got, exp)
        check_rect(rect_device(ctx, dev), ec, ed)


def top_raw(ctx, QH, QN, RH, RN, top, exp):
    """drephip_dist_rect_top_device of every row into poisoned device buffers
    with a guard row before and after, compared with expected_top's (ref,
    common, denom, count): a row the kernel skipped keeps its poison."""
    import torch
    Q = len(QN)
    ref, common, denom, count = exp
    keep, args = upload(QH, QN, RH, RN)                # (`keep` holds the device matrices until the call is done)
    d_hits = torch.full(((Q + 2) * top * 4,), POISON - (1 << 32), dtype=torch.int32, device="cuda")
    d_cnt = torch.full((Q + 2,), POISON - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.dist_rect_top_device(*args, 0, Q, top, d_hits.data_ptr() + top * 16, d_cnt.data_ptr() + 4)
    hits = d_hits.cpu().numpy().view(np.uint32).reshape(Q + 2, top, 4)
    cnt = d_cnt.cpu().numpy().view(np.uint32)
    assert (hits[0] == POISON).all() and (hits[-1] == POISON).all() and cnt[0] == POISON and cnt[-1] == POISON
    assert np.array_equal(cnt[1:-1], count), np.nonzero(cnt[1:-1] != count)[0][:8]
    got = hits[1:-1]
    r = got[:, :, 0].astype(np.int64)
    r[r == EMPTY] = -1
    assert np.array_equal(r, ref), np.nonzero((r != ref).any(axis=1))[0][:8]
    assert np.array_equal(got[:, :, 1], common) and np.array_equal(got[:, :, 2], denom) and (got[:, :, 3] == 0).all()


@pytest.mark.parametrize("top", [3, 64])
@pytest.mark.parametrize("s", [64, 1000])
def test_split_top_launch_strides_the_rows(s, top, monkeypatch):
    """41 rows on the 8 workgroups the cap leaves: up to six rows each."""
    QH, QN, RH, RN, n, ec, ed = sets(s)
    assert len(QN) > 5 * 8
    monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", CAP_ITEMS)
    with _lib.Context(0, 21, s, 42) as ctx:
        top_raw(ctx, QH, QN, RH, RN, top, expected_top(ec, ed, top))


# ------------------------------------------------------------ 3. long, unaligned, strided rows
_LONG = {}


def long_rows(top=None):
    """24 queries against 6149 references at s = 64 (geometry_sketches, the
    queries its first rows): N is odd, so the rows start at all eight offsets
    within a 16-byte vector, and most rows hold more hits than k_rect_top's
    4096-key list.  With `top`: and the expected hits, computed once per top."""
    if "set" not in _LONG:
        s, N, Q = 64, 6149, 24
        H, NH = edge_cases.geometry_sketches(N, s, seed=6149)
        ec, ed = oracle_rows(H[:Q], NH[:Q], H, NH, s)
        for a in (H, NH, ec, ed):
            a.setflags(write=False)
        _LONG["set"] = (s, H[:Q], NH[:Q], H, NH, ec, ed)
    if top is None:
        return _LONG["set"]
    if top not in _LONG:
        _LONG[top] = expected_top(*_LONG["set"][5:], top)
    return _LONG["set"] + (_LONG[top],)


def test_long_rows_set_holds_what_it_is_for():
    s, QH, QN, RH, RN, ec, ed = long_rows()
    N = len(RN)
    nz = (ec > 0).sum(axis=1)
    assert (nz > 4096).any() and (nz == 0).any() and QN[11] == 0
    assert len({(q * N) % 8 for q in range(len(QN))}) == 8 and N > 2 * 2048
    assert len(np.unique(ed[ec > 0])) > 1
    # ratios tie at the cut: hit 64 and the one left out
    exp = long_rows(64)[-1]
    tied = 0
    for q in np.nonzero(nz > 64)[0]:
        last = Fraction(int(exp[1][q, 63]), int(exp[2][q, 63]))
        listed = set(exp[0][q])
        tied += any(Fraction(int(ec[q, r]), int(ed[q, r])) == last for r in np.nonzero(ec[q])[0] if r not in listed)
    assert tied > 0


@pytest.mark.parametrize("setting", ["default", "capped", "capped_blocks"])
@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("top", [1, 64])
def test_top_long_unaligned_rows(top, merge, setting, monkeypatch):
    """default: one workgroup per row; capped: 8 workgroups, three rows each;
    capped_blocks: blocks of 5 rows, whose block-local rows start at other
    offsets within a vector than the same rows of the whole call."""
    s, QH, QN, RH, RN, ec, ed, exp = long_rows(top)
    if setting != "default":
        monkeypatch.setenv("DREPHIP_MAX_LAUNCH_ITEMS", CAP_ITEMS)
    if setting == "capped_blocks":
        monkeypatch.setenv("DREPHIP_RECT_TOP_BLOCK_ROWS", "5")
    with _lib.Context(0, 21, s, 42) as ctx:
        if merge:
            ctx.set_allpairs_path(ctx.AP_MERGE)
        top_raw(ctx, QH, QN, RH, RN, top, exp)


# ------------------------------------------------------------ 4. record-form row blocks
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("s", [64, 4096])
def test_record_row_blocks(s, rows, monkeypatch):
    """DREPHIP_RECT_BLOCK_ROWS: the merge route's block loop runs several
    times (s = 4096 under AUTO, s = 64 under AP_MERGE) and lists the same
    records; the cap / n_pairs contract holds across the blocks."""
    import torch
    H, NH, nq, (ec, ed) = case(s)
    nref = len(NH)
    exp = records_of(ec, ed)
    need = len(exp[0])
    assert need > nq
    monkeypatch.setenv("DREPHIP_RECT_BLOCK_ROWS", str(rows))
    with _lib.Context(0, 21, s, 42) as ctx:
        if s <= 2048:
            ctx.set_allpairs_path(ctx.AP_MERGE)
        ctx.set_timing(True, kernels=[2])
        got = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, cap=need)
        assert ctx.kernel_ms(2)[1] == -(-nq // rows)            # one k_rect_merge span per block
        assert len(got[0]) == need and same_records(got, exp)
        # a row range: the blocks start at q0
        q0, q1 = 3, 17
        k = (exp[0] >= q0) & (exp[0] < q1)
        got = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, q0, q1, cap=need)
        assert ctx.kernel_ms(2)[1] == -(-(q1 - q0) // rows)
        assert same_records(got, [a[k] for a in exp])
        # values <= 0 are ignored: one block
        monkeypatch.setenv("DREPHIP_RECT_BLOCK_ROWS", "0")
        got = ctx.dist_rect_sparse(H[:nq], NH[:nq], H, NH, cap=need)
        assert ctx.kernel_ms(2)[1] == 1 and same_records(got, exp)
        monkeypatch.setenv("DREPHIP_RECT_BLOCK_ROWS", str(rows))
        # cap = 0 counts; cap = need - 1: NOMEM, the size needed, nothing past cap
        dqh = torch.from_numpy(H[:nq].copy().view(np.int64)).cuda()
        dqn = torch.from_numpy(NH[:nq].copy().view(np.int32)).cuda()
        drh = torch.from_numpy(H.copy().view(np.int64)).cuda()
        drn = torch.from_numpy(NH.copy().view(np.int32)).cuda()
        args = (dqh.data_ptr(), dqn.data_ptr(), nq, drh.data_ptr(), drn.data_ptr(), nref, 0, nq)
        torch.cuda.synchronize()
        assert ctx.dist_rect_sparse_device(*args, None, 0) == (ERR_NOMEM, need)
        buf = torch.full((need + 8, 4), 0x7EADBEEF, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ctx.dist_rect_sparse_device(*args, buf.data_ptr(), need - 1) == (ERR_NOMEM, need)
        got = buf.cpu().numpy()
        assert (got[need - 1:] == 0x7EADBEEF).all()
        rec = got[:need - 1].view(np.uint32)
        assert len(set(map(tuple, rec[:, :2]))) == need - 1                 # each pair at most once
        assert all(a < nq and b < nref and ec[a, b] == cc and ed[a, b] == dd and cc > 0 for a, b, cc, dd in rec)
        buf.fill_(0x7EADBEEF)
        torch.cuda.synchronize()
        assert ctx.dist_rect_sparse_device(*args, buf.data_ptr(), need) == (0, need)
        rec = buf.cpu().numpy()[:need].view(np.uint32)
        rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
        assert np.array_equal(rec[:, 0], exp[0]) and np.array_equal(rec[:, 1], exp[1])
        assert np.array_equal(rec[:, 2], exp[2]) and np.array_equal(rec[:, 3], exp[3])
