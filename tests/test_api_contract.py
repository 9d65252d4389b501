"""The argument contract of the C API (include/drephip.h), pinned call by call:
return codes, drephip_last_error texts, the order the checks fire in, what an
empty or a refused call leaves in its outputs, the cap / n_pairs /
DREPHIP_ERR_NOMEM protocol of the record forms, and what a refused call does to
the timing figures.  Nothing here can go wrong at a particular size: the inputs
are tiny (s = 64, N = 12, Q = 5) and every test is an argument or staging test.

The calls go to the library through a second ctypes handle whose pointer
arguments are all void* (`raw`): _lib's ndpointer types refuse None, and NULL
is half of what is tested.  Null contexts and the host-only entries need no
device; the rest is marked gpu.

Three things the library does that a reader of the header might not expect,
pinned as they are:
  * the dense host forms drephip_allpairs and drephip_allpairs_rows test
    nhash[i] <= s and the UINT64_MAX padding, but accept an unordered row;
  * the sparse triangle host forms check the rows (and the _sig form the
    lengths) before they tell an empty row range apart, so an empty call with a
    bad matrix is refused; the dense triangle forms and every rectangle form
    return 0 for an empty call whatever the matrices hold;
  * a count-only call (cap 0, pairs NULL) returns DREPHIP_ERR_NOMEM, not 0,
    when the rows hold any record: n_pairs is the answer."""
import ctypes as C

import numpy as np
import pytest

import oracle
from drep_amd import _lib
from test_sparse_host import family_sketches

S, N, Q = 64, 12, 5
QROWS = [0, 1, 2, 7, 8]                # the queries: copies of these reference rows
OK, ARG, NOMEM, UNSUPPORTED = 0, -1, -4, -5
FILL16, FILL32 = 0xABCD, 0xABCDABCD
PAIR_CAP = 128                         # room for every record of the triangle (66 pairs) or the rectangle (60)

_RAW = None


def raw(name):
    """`name` of libdrephip.so with every array argument typed void*."""
    global _RAW
    if _RAW is None:
        _lib.lib()
        _RAW = C.CDLL(_lib.LIB_PATH)
    fn = getattr(_RAW, name)
    res, args = _lib.SIGNATURES[name]
    fn.restype = res
    fn.argtypes = [C.c_void_p if hasattr(a, "_dtype_") else a for a in args]
    return fn


def p(a):
    return None if a is None else a.ctypes.data


def last():
    return _lib.lib().drephip_last_error().decode()


def refused(rc, code, text):
    assert rc == code and text in last(), (rc, last())


# ------------------------------------------------------------------ no device
GUARDED = """drephip_sketch drephip_sketch_files drephip_fasta_pack_device drephip_sketch_device
    drephip_sketch_device_async drephip_sketch_wait drephip_synth_device drephip_allpairs_device
    drephip_allpairs_device_async drephip_allpairs_wait drephip_screen_part drephip_screen_part_copy
    drephip_allpairs_device_marked drephip_allpairs_merge_device drephip_allpairs drephip_allpairs_rows
    drephip_allpairs_sparse_device drephip_allpairs_sparse_device_marked drephip_allpairs_sparse
    drephip_dist_rect_device drephip_dist_rect_merge_device drephip_dist_rect drephip_dist_rect_sparse_device
    drephip_dist_rect_sparse drephip_allpairs_sparse_sig drephip_dist_rect_sparse_sig drephip_dist_rect_top_device
    drephip_dist_rect_top drephip_pvalue_records_device drephip_pvalue_records drephip_pvalue_hits_device
    drephip_records_filter_device drephip_set_linkage_path drephip_linkage drephip_linkage_square
    drephip_linkage_counts_device drephip_linkage_reserve drephip_set_timing drephip_set_allpairs_path
    drephip_set_rect_band drephip_set_rect_screen drephip_set_allpairs_screen drephip_last_sparse_stats
    drephip_last_linkage_info drephip_last_linkage_stats""".split()


def _zero(t):
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return None
    return 0.0 if t is C.c_double else 0


@pytest.mark.parametrize("name", GUARDED)
def test_null_context(name):
    fn = raw(name)
    refused(fn(*[_zero(t) for t in fn.argtypes]), ARG, "null context")


def test_null_context_of_the_entries_that_name_no_context():
    refused(raw("drephip_screen_geometry")(None, None), ARG, "null argument")
    refused(raw("drephip_screen_worth")(None, 4, 0, None, None), ARG, "null argument")
    refused(raw("drephip_last_kernel_ms")(None, 0, None, None), ARG, "bad argument")
    refused(raw("drephip_last_linkage_launches")(None, None), ARG, "null argument")
    assert raw("drephip_destroy")(None) == OK


def test_host_only_entries():
    Z = np.full(8, 7.0)
    i, j, v = np.zeros(1, np.uint32), np.ones(1, np.uint32), np.full(1, 0.5)
    ls = raw("drephip_linkage_sparse")
    for n in (0, 1):                                                  # nothing to link: Z is not touched (nor read)
        assert ls(n, 0, None, None, None, 0, None) == OK
        assert ls(n, 1, p(i), p(j), p(v), 0, p(Z)) == OK and (Z == 7.0).all()
    refused(ls(3, 1, p(i), p(j), p(v), 0, None), ARG, "null argument")
    for a in ((None, p(j), p(v)), (p(i), None, p(v)), (p(i), p(j), None)):
        refused(ls(3, 1, *a, 0, p(Z)), ARG, "null argument")
    assert ls(3, 0, None, None, None, 0, p(Z)) == OK                  # no pair listed: no pair arrays needed
    lut = np.zeros(4)
    refused(raw("drephip_distance_lut")(21, 3, None), ARG, "bad argument")
    refused(raw("drephip_distance_lut")(0, 3, p(lut)), ARG, "bad argument")
    refused(raw("drephip_distance_lut")(21, 0, p(lut)), ARG, "bad argument")
    refused(raw("drephip_rect_screen_mode_of")(None, None), ARG, "null argument")
    refused(raw("drephip_device_count")(None), ARG, "null pointer")
    refused(raw("drephip_create")(0, 21, 1000, 42, None), ARG, "null out")


# --------------------------------------------------------------------- device
class Env:
    pass


@pytest.fixture(scope="module")
def env():
    import torch
    e = Env()
    e.H, e.NH = family_sketches(N, S, seed=1)
    e.QH, e.QN = e.H[QROWS].copy(), e.NH[QROWS].copy()
    e.LEN, e.QLEN = np.full(N, 10 ** 6, np.uint64), np.full(Q, 10 ** 6, np.uint64)
    assert e.NH[0] < S and e.NH[2] == e.NH[3] == e.NH[4] == S        # a partial row and full rows, on both sides

    def up(a, view):
        return torch.from_numpy(a.view(view).copy()).cuda()
    e.dH, e.dNH, e.dQH, e.dQN = up(e.H, np.int64), up(e.NH, np.int32), up(e.QH, np.int64), up(e.QN, np.int32)
    e.dC = torch.zeros(Q * N + N * N, dtype=torch.int16, device="cuda")      # room for either dense output
    e.dD = torch.zeros(Q * N + N * N, dtype=torch.int16, device="cuda")
    e.dP = torch.zeros((PAIR_CAP, 4), dtype=torch.int32, device="cuda")      # records, hits, counts
    e.tri = (p(e.H), p(e.NH), N, 0, N)
    e.rect = (p(e.QH), p(e.QN), Q, p(e.H), p(e.NH), N, 0, Q)
    e.dtri = (e.dH.data_ptr(), e.dNH.data_ptr(), N, 0, N)
    e.drect = (e.dQH.data_ptr(), e.dQN.data_ptr(), Q, e.dH.data_ptr(), e.dNH.data_ptr(), N, 0, Q)
    # the records each side holds: the pairs with a nonzero count (the C oracle's Mash merge)
    oc, _ = oracle.allpairs(e.H, e.NH, S)
    e.tri_true = int((oc > 0).sum())
    oc, _ = oracle.allpairs(np.vstack([e.QH, e.H]), np.concatenate([e.QN, e.NH]), S)
    ii, jj = np.triu_indices(Q + N, 1)
    e.rect_true = int((oc[(ii < Q) & (jj >= Q)] > 0).sum())
    assert 2 < e.tri_true < PAIR_CAP and 2 < e.rect_true < PAIR_CAP
    torch.cuda.synchronize()
    e.ctx = _lib.Context(0, 21, S, 42)
    e.h = e.ctx.handle
    yield e
    e.ctx.close()


def nulls(e, name, args, must, nullable=()):
    """`name`(ctx, *args): NULL at each index of `must` is refused, NULL at each of `nullable` is not."""
    fn = raw(name)
    for i in must:
        a = list(args)
        a[i] = None
        refused(fn(e.h, *a), ARG, "null argument")
    for i in nullable:
        a = list(args)
        a[i] = None
        assert fn(e.h, *a) == OK, (name, i, last())
    assert fn(e.h, *args) == OK, (name, last())


@pytest.mark.gpu
def test_null_arguments_of_the_triangle(env):
    e = env
    n = C.c_uint64(0)
    dC, dD, dP = e.dC.data_ptr(), e.dD.data_ptr(), e.dP.data_ptr()
    for name in ("drephip_allpairs_device", "drephip_allpairs_merge_device"):
        nulls(e, name, [*e.dtri, dC, dD, None], must=(0, 1, 5), nullable=(6,))
    nulls(e, "drephip_allpairs_device_async", [*e.dtri, dC, dD, None], must=(0, 1, 5), nullable=(6,))
    assert raw("drephip_allpairs_wait")(e.h) == OK
    # the marks forms: only their refusals (test_sparse_sharded.py runs them)
    marked = raw("drephip_allpairs_device_marked")
    for a in ([None, e.dtri[1], N, 0, N, dC, dD, None, 0, None, 0, None], [e.dtri[0], None, N, 0, N, dC, dD, None, 0, None, 0, None],
              [*e.dtri, None, dD, None, 0, None, 0, None], [*e.dtri, dC, dD, None, 2, None, 0, None],
              [*e.dtri, dC, dD, None, 0, None, 2, None]):
        refused(marked(e.h, *a), ARG, "null argument")
    smarked = raw("drephip_allpairs_sparse_device_marked")
    for a in ([*e.dtri, None, 0, None, 0, dP, 4, None, None], [*e.dtri, None, 0, None, 0, None, 4, C.byref(n), None],
              [*e.dtri, None, 2, None, 0, dP, 4, C.byref(n), None], [*e.dtri, None, 0, None, 2, dP, 4, C.byref(n), None]):
        refused(smarked(e.h, *a), ARG, "null argument")
    nulls(e, "drephip_allpairs_sparse_device", [*e.dtri, dP, PAIR_CAP, C.byref(n), None], must=(0, 1, 5, 7))
    part = raw("drephip_screen_part")
    c, nc, nr = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    good = [e.dtri[0], e.dtri[1], N, 0, 1, C.byref(c), C.byref(nc), C.byref(nr), None]
    for i in (0, 1, 5, 6, 7):
        a = list(good)
        a[i] = None
        refused(part(e.h, *a), ARG, "null argument")
    refused(part(e.h, *good[:3], 1, 1, *good[5:]), ARG, "part must be below nparts")
    refused(part(e.h, *good[:3], 0, 0, *good[5:]), ARG, "part must be below nparts")
    refused(part(e.h, good[0], good[1], 1, *good[3:]), ARG, "the screen needs N >= 2")
    refused(raw("drephip_screen_part_copy")(e.h, None, None, None), ARG, "no screen part to copy")
    # the host forms
    co, do, pairs = np.zeros(N * N, np.uint16), np.zeros(N * N, np.uint16), np.zeros((PAIR_CAP, 4), np.uint32)
    nulls(e, "drephip_allpairs", [p(e.H), p(e.NH), N, p(co), p(do)], must=(0, 1, 3), nullable=(4,))
    nulls(e, "drephip_allpairs_rows", [*e.tri, p(co), p(do)], must=(0, 1, 5), nullable=(6,))
    nulls(e, "drephip_allpairs_sparse", [*e.tri, p(pairs), PAIR_CAP, C.byref(n)], must=(0, 1, 5, 7))
    listed = C.c_uint64(0)
    pv = np.zeros(PAIR_CAP)
    nulls(e, "drephip_allpairs_sparse_sig", [*e.tri, p(e.LEN), 1.0, None, p(pairs), PAIR_CAP, p(pv), C.byref(n), C.byref(listed)],
          must=(0, 1, 5, 8, 11), nullable=(10, 12))


@pytest.mark.gpu
def test_null_arguments_of_the_rectangle(env):
    e = env
    n, listed = C.c_uint64(0), C.c_uint64(0)
    dC, dD, dP = e.dC.data_ptr(), e.dD.data_ptr(), e.dP.data_ptr()
    for name in ("drephip_dist_rect_device", "drephip_dist_rect_merge_device"):
        nulls(e, name, [*e.drect, dC, dD, None], must=(0, 1, 3, 4, 8), nullable=(9,))
        assert raw(name)(e.h, *e.drect[:6], 3, 3, None, None, None) == OK         # no row: no output needed
        assert raw(name)(e.h, None, None, 0, *e.drect[3:], None, None, None) == OK   # no query: no query matrix needed
    nulls(e, "drephip_dist_rect_sparse_device", [*e.drect, dP, PAIR_CAP, C.byref(n), None], must=(0, 1, 3, 4, 8, 10))
    nulls(e, "drephip_dist_rect_top_device", [*e.drect, 2, dP, dD, None], must=(0, 1, 3, 4, 9, 10))
    assert raw("drephip_dist_rect_top_device")(e.h, *e.drect[:6], 3, 3, 2, None, None, None) == OK
    co, do, pairs = np.zeros(Q * N, np.uint16), np.zeros(Q * N, np.uint16), np.zeros((PAIR_CAP, 4), np.uint32)
    hits, count, pv = np.zeros((Q, 2, 4), np.uint32), np.zeros(Q, np.uint32), np.zeros(PAIR_CAP)
    nulls(e, "drephip_dist_rect", [*e.rect, p(co), p(do)], must=(0, 1, 3, 4, 8), nullable=(9,))
    nulls(e, "drephip_dist_rect_sparse", [*e.rect, p(pairs), PAIR_CAP, C.byref(n)], must=(0, 1, 3, 4, 8, 10))
    nulls(e, "drephip_dist_rect_top", [*e.rect, 2, p(hits), p(count)], must=(0, 1, 3, 4, 9, 10))
    nulls(e, "drephip_dist_rect_sparse_sig",
          [*e.rect, p(e.QLEN), p(e.LEN), 1.0, None, p(pairs), PAIR_CAP, p(pv), C.byref(n), C.byref(listed)],
          must=(0, 1, 3, 4, 8, 9, 12, 15), nullable=(14, 16))


@pytest.mark.gpu
def test_null_arguments_of_sketch_and_synth(env):
    e = env
    d = e.dP.data_ptr()                                               # stands for every device buffer: never read
    off = np.zeros(2, np.uint64)
    for name in ("drephip_sketch_device", "drephip_sketch_device_async"):
        fn = raw(name)
        assert fn(e.h, None, None, None, None, None, 0, None, None, None) == OK          # no genome: nothing needed
        good = [d, d, p(off), p(off), p(off), 1, d, d, None]
        for i in (0, 1, 2, 3, 4, 6, 7):
            a = list(good)
            a[i] = None
            refused(fn(e.h, *a), ARG, "null argument")
    redone = C.c_int(5)
    assert raw("drephip_sketch_wait")(e.h, C.byref(redone)) == OK and redone.value == 0   # nothing pending
    synth = raw("drephip_synth_device")
    refused(synth(e.h, 1, 0, 1, 1, 1000, None, d, None), ARG, "null argument")
    refused(synth(e.h, 1, 0, 1, 1, 1000, d, None, None), ARG, "null argument")


# ------------------------------------------------------------- the host forms
TRI_HOST = ("drephip_allpairs_rows", "drephip_allpairs_sparse", "drephip_allpairs_sparse_sig")
RECT_HOST = ("drephip_dist_rect", "drephip_dist_rect_sparse", "drephip_dist_rect_sparse_sig", "drephip_dist_rect_top")


def host_form(e, name, a, b, H=None, NH=None, QH=None, QN=None, n_ref=N, n_query=Q, LEN=None):
    """One host-form call over rows [a, b) with sentinel-filled outputs: (rc, n_pairs or None, outputs)."""
    H, NH = e.H if H is None else H, e.NH if NH is None else NH
    QH, QN = e.QH if QH is None else QH, e.QN if QN is None else QN
    LEN = e.LEN if LEN is None else LEN
    n, listed = C.c_uint64(77), C.c_uint64(77)
    o16 = [np.full(N * N, FILL16, np.uint16) for _ in range(2)]
    o32 = [np.full((PAIR_CAP, 4), FILL32, np.uint32), np.full(PAIR_CAP, FILL32, np.uint32)]
    pv = np.full(PAIR_CAP, -3.0)
    tri = (p(H), p(NH), n_ref, a, b)
    rect = (p(QH), p(QN), n_query, p(H), p(NH), n_ref, a, b)
    fn = raw(name)
    if name == "drephip_allpairs":
        return fn(e.h, p(H), p(NH), n_ref, p(o16[0]), p(o16[1])), None, o16
    if name == "drephip_allpairs_rows":
        return fn(e.h, *tri, p(o16[0]), p(o16[1])), None, o16
    if name == "drephip_allpairs_sparse":
        return fn(e.h, *tri, p(o32[0]), PAIR_CAP, C.byref(n)), n.value, o32[:1]
    if name == "drephip_allpairs_sparse_sig":
        rc = fn(e.h, *tri, p(LEN), 1.0, None, p(o32[0]), PAIR_CAP, p(pv), C.byref(n), C.byref(listed))
        return rc, n.value, [o32[0], pv, listed]
    if name == "drephip_dist_rect":
        return fn(e.h, *rect, p(o16[0]), p(o16[1])), None, o16
    if name == "drephip_dist_rect_sparse":
        return fn(e.h, *rect, p(o32[0]), PAIR_CAP, C.byref(n)), n.value, o32[:1]
    if name == "drephip_dist_rect_sparse_sig":
        rc = fn(e.h, *rect, p(e.QLEN), p(LEN), 1.0, None, p(o32[0]), PAIR_CAP, p(pv), C.byref(n), C.byref(listed))
        return rc, n.value, [o32[0], pv, listed]
    assert name == "drephip_dist_rect_top"
    return fn(e.h, *rect, 2, p(o32[0]), p(o32[1])), None, o32


def untouched(outs):
    for o in outs:
        if isinstance(o, C.c_uint64):
            assert o.value in (0, 77)                  # n_listed: zeroed or left alone, never a count
        else:
            assert (o == {np.dtype(np.uint16): FILL16, np.dtype(np.uint32): FILL32, np.dtype(np.float64): -3.0}[o.dtype]).all()


def violations(hashes, nhash, full, partial):
    """(what, hashes, nhash, message): the matrix with one row check violated."""
    big = nhash.copy()
    big[full] = S + 1
    swap = hashes.copy()
    swap[full, [4, 9]] = swap[full, [9, 4]]
    dup = hashes.copy()
    dup[full, 7] = dup[full, 6]
    pad = hashes.copy()
    pad[partial, nhash[partial]] = 5
    return (("big", hashes, big, "nhash[i] > s"), ("unordered", swap, nhash, "ascending and distinct"),
            ("duplicate", dup, nhash, "ascending and distinct"), ("padding", pad, nhash, "UINT64_MAX past"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("drephip_allpairs_sparse", "drephip_allpairs_sparse_sig") + RECT_HOST)
def test_row_checks_of_the_ordered_host_forms(env, name):
    e = env
    rows = (0, N) if name in TRI_HOST else (0, Q)
    for what, h, nh, msg in violations(e.H, e.NH, 3, 0):
        rc, n, outs = host_form(e, name, *rows, H=h, NH=nh)
        refused(rc, ARG, msg)
        assert n in (None, 0), what
        untouched(outs)
    if name in RECT_HOST:
        for what, h, nh, msg in violations(e.QH, e.QN, 2, 0):
            rc, n, outs = host_form(e, name, *rows, QH=h, QN=nh)
            refused(rc, ARG, msg)
            assert n in (None, 0), what
            untouched(outs)
    rc, n, outs = host_form(e, name, *rows)                           # and the matrices as they are pass
    assert rc == OK and n in (None, e.tri_true if name in TRI_HOST else e.rect_true), last()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("drephip_allpairs", "drephip_allpairs_rows"))
def test_row_checks_of_the_dense_triangle_host_forms(env, name):
    """drephip_allpairs and drephip_allpairs_rows test nhash[i] <= s and the
    padding only: an unordered row is accepted (its counts mean nothing)."""
    e = env
    for what, h, nh, msg in violations(e.H, e.NH, 3, 0):
        if what == "duplicate":
            continue
        rc, _, outs = host_form(e, name, 0, N, H=h, NH=nh)
        if what == "unordered":
            assert rc == OK, last()
        else:
            refused(rc, ARG, msg)
            untouched(outs)
    rc, _, outs = host_form(e, name, 0, N)
    want, _ = oracle.allpairs(e.H, e.NH, S)
    assert rc == OK and np.array_equal(outs[0][:len(want)], want) and (outs[0][len(want):] == FILL16).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", TRI_HOST)
def test_empty_row_ranges_of_the_triangle(env, name):
    e = env
    for a, b in ((5, 5), (7, 3), (N - 1, N), (N, N + 4)):
        rc, n, outs = host_form(e, name, a, b)
        assert rc == OK and n in (None, 0), (a, b, last())
        untouched(outs)
    for few in (0, 1):                                                # fewer than two genomes: no pair
        rc, n, outs = host_form(e, name, 0, few, n_ref=few)
        assert rc == OK and n in (None, 0)
        untouched(outs)
    # an empty call with a bad matrix: the dense form returns before its row
    # check, the sparse forms check first (the module docstring)
    big = e.NH.copy()
    big[3] = S + 1
    rc, n, outs = host_form(e, name, 5, 5, NH=big)
    if name == "drephip_allpairs_rows":
        assert rc == OK
    else:
        refused(rc, ARG, "nhash[i] > s")
    assert n in (None, 0)
    untouched(outs)


@pytest.mark.gpu
def test_allpairs_of_fewer_than_two_genomes(env):
    for few in (0, 1):
        rc, _, outs = host_form(env, "drephip_allpairs", 0, 0, n_ref=few)
        assert rc == OK
        untouched(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RECT_HOST)
def test_empty_ranges_of_the_rectangle(env, name):
    e = env
    big = e.NH.copy()
    big[3] = S + 1
    for kw in (dict(a=0, b=Q, n_query=0), dict(a=0, b=Q, n_ref=0), dict(a=3, b=3), dict(a=4, b=2), dict(a=Q, b=Q + 3),
               dict(a=3, b=3, NH=big)):                               # (an empty call does not look at the rows)
        rc, n, outs = host_form(e, name, **kw)
        assert rc == OK and n in (None, 0), (kw, last())
        untouched(outs)


# ----------------------------------------------------------- the record forms
RECORD_FORMS = ("drephip_allpairs_sparse", "drephip_allpairs_sparse_device", "drephip_dist_rect_sparse",
                "drephip_dist_rect_sparse_device", "drephip_allpairs_sparse_sig", "drephip_dist_rect_sparse_sig")


def records(e, name, cap, max_p=1.0, lengths=None):
    """(rc, n_pairs, the first min(n_pairs, cap) records, n_listed or None)"""
    import torch
    n, listed = C.c_uint64(77), C.c_uint64(77)
    buf = np.full((max(cap, 1), 4), FILL32, np.uint32)
    pp = p(buf) if cap else None
    fn = raw(name)
    tri = "allpairs" in name
    nl = None
    if name.endswith("_device"):
        d = torch.full((max(cap, 1), 4), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = fn(e.h, *(e.dtri if tri else e.drect), d.data_ptr() if cap else None, cap, C.byref(n), None)
        torch.cuda.synchronize()
        buf = d.cpu().numpy().view(np.uint32)
    elif name.endswith("_sig"):
        ln = lengths or ((e.LEN,) if tri else (e.QLEN, e.LEN))
        rc = fn(e.h, *(e.tri if tri else e.rect), *[p(x) for x in ln], max_p, None, pp, cap, None, C.byref(n), C.byref(listed))
        nl = listed.value
    else:
        rc = fn(e.h, *(e.tri if tri else e.rect), pp, cap, C.byref(n))
    return rc, n.value, buf[:min(n.value, cap)], nl


@pytest.mark.gpu
@pytest.mark.parametrize("name", RECORD_FORMS)
def test_nomem_protocol(env, name):
    e = env
    true = e.tri_true if "allpairs" in name else e.rect_true
    text = "more records than cap" if name.endswith("_sig") else "the pair list holds"
    rc, n, _, nl = records(e, name, 0)                                # cap 0, pairs NULL: the count
    refused(rc, NOMEM, text)
    assert n == true and nl in (None, true)
    rc, n, full, nl = records(e, name, true)                          # room for exactly that many
    assert rc == OK and n == true and nl in (None, true), last()
    everything = set(map(tuple, full.tolist()))
    assert len(everything) == true and all(c > 0 and 0 < d <= S for _, _, c, d in everything)
    rc, n, part, nl = records(e, name, true - 1)                      # one too few: the count, and cap records
    refused(rc, NOMEM, text)
    assert n == true and nl in (None, true) and len(part) == true - 1
    got = set(map(tuple, part.tolist()))
    assert len(got) == true - 1 and got < everything


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("drephip_allpairs_sparse_sig", "drephip_dist_rect_sparse_sig"))
def test_sig_arguments(env, name):
    e = env
    tri = "allpairs" in name
    true = e.tri_true if tri else e.rect_true
    for bad in (-0.1, 1.1, float("nan")):
        rc, n, _, nl = records(e, name, PAIR_CAP, max_p=bad)
        refused(rc, ARG, "max_p must lie in [0, 1]")
        assert (n, nl) == (77, 77)                                    # refused before the outputs are zeroed
    for side in range(1 if tri else 2):
        ln = [e.LEN.copy()] if tri else [e.QLEN.copy(), e.LEN.copy()]
        ln[side][1] = 0                                               # row 1 holds hashes
        rc, n, _, nl = records(e, name, PAIR_CAP, lengths=tuple(ln))
        refused(rc, ARG, "a genome with a non-empty sketch has length 0")
        assert (n, nl) == (0, 0)
    ln = [e.LEN.copy()] if tri else [e.QLEN.copy(), e.LEN.copy()]
    ln[-1][5] = 0                                                     # reference row 5 is empty: no length needed
    rc, n, _, nl = records(e, name, PAIR_CAP, lengths=tuple(ln))
    assert rc == OK and n == nl == true, last()
    for max_p in (1.0, 1e-30, 0.0):
        rc, n, rec, nl = records(e, name, PAIR_CAP, max_p=max_p)
        assert rc == OK and nl == true and n <= nl and len(rec) == n, last()


@pytest.mark.gpu
def test_rect_top_bounds(env):
    e = env
    hits, count = np.full((Q, 65, 4), FILL32, np.uint32), np.full(Q, FILL32, np.uint32)
    for top in (0, 65):
        refused(raw("drephip_dist_rect_top")(e.h, *e.rect, top, p(hits), p(count)), ARG, "top must be in 1..64")
        refused(raw("drephip_dist_rect_top_device")(e.h, *e.drect, top, e.dP.data_ptr(), e.dD.data_ptr(), None), ARG,
                "top must be in 1..64")
        # refused even where nothing would run, and after the null test
        refused(raw("drephip_dist_rect_top")(e.h, *e.rect[:6], 3, 3, top, p(hits), p(count)), ARG, "top must be in 1..64")
        refused(raw("drephip_dist_rect_top")(e.h, None, *e.rect[1:], top, p(hits), p(count)), ARG, "null argument")
    assert (hits == FILL32).all() and (count == FILL32).all()
    most = np.zeros((Q, 64, 4), np.uint32)
    assert raw("drephip_dist_rect_top")(e.h, *e.rect, 64, p(most), p(count)) == OK


# -------------------------------------------------------------------- linkage
@pytest.mark.gpu
def test_linkage_arguments(env):
    e = env
    Z = np.full(16, 7.0)
    y, M = np.full(3, 0.5), np.zeros((3, 3), np.float32)
    perm, lut = np.arange(3, dtype=np.uint32), np.linspace(1.0, 0.0, S + 1)
    lut_off = np.full(S + 1, -1, np.int32)
    lut_off[S] = 0
    d = e.dC.data_ptr()
    link, square = raw("drephip_linkage"), raw("drephip_linkage_square")
    counts, reserve = raw("drephip_linkage_counts_device"), raw("drephip_linkage_reserve")
    for n in (0, 1):                                                  # nothing to link: OK, Z not touched
        assert link(e.h, None, n, 0, None) == OK and link(e.h, p(y), n, 0, p(Z)) == OK
        assert square(e.h, None, n, 99, None) == OK and square(e.h, p(M), n, 0, p(Z)) == OK
        assert counts(e.h, None, None, n, None, None, 0, None, 0, None, None) == OK
        assert counts(e.h, d, None, n, p(perm), p(lut), len(lut), p(lut_off), 0, p(Z), None) == OK
        assert reserve(e.h, n) == OK
    assert (Z == 7.0).all()
    big = "linkage supports n <= 200000"
    refused(link(e.h, p(y), 200001, 0, p(Z)), UNSUPPORTED, big)
    refused(square(e.h, p(M), 200001, 0, p(Z)), UNSUPPORTED, big)
    refused(counts(e.h, d, None, 200001, p(perm), p(lut), len(lut), p(lut_off), 0, p(Z), None), UNSUPPORTED, big)
    refused(reserve(e.h, 200001), UNSUPPORTED, big)
    refused(link(e.h, None, 200001, 0, p(Z)), ARG, "null argument")   # the null test comes first
    refused(link(e.h, None, 3, 0, p(Z)), ARG, "null argument")
    refused(link(e.h, p(y), 3, 0, None), ARG, "null argument")
    refused(square(e.h, None, 3, 0, p(Z)), ARG, "null argument")
    refused(square(e.h, p(M), 3, 0, None), ARG, "null argument")
    for method in (3, -1, 7):
        refused(square(e.h, p(M), 3, method, p(Z)), UNSUPPORTED, "linkage method must be single, complete, average or weighted")
    good = [d, None, 3, p(perm), p(lut), len(lut), p(lut_off), 0, p(Z), None]
    for i in (0, 3, 4, 6, 8):
        a = list(good)
        a[i] = None
        refused(counts(e.h, *a), ARG, "null argument")
    for bad in ([0, 1, 1], [0, 1, 3], [2, 2, 2]):                     # a repeat, an entry out of range
        a = list(good)
        bp = np.array(bad, np.uint32)
        a[3] = p(bp)
        refused(counts(e.h, *a), ARG, "perm is not a permutation of 0..n-1")
    a = list(good)
    a[5] = S                                                          # lut_off[S] = 0 needs S + 1 entries
    refused(counts(e.h, *a), ARG, "lut_off/lut_len mismatch")
    off2 = lut_off.copy()
    off2[3] = len(lut) - 3                                            # denominator 3 needs 4 entries from there
    a = list(good)
    a[6] = p(off2)
    refused(counts(e.h, *a), ARG, "lut_off/lut_len mismatch")
    none = np.full(S + 1, -1, np.int32)
    a = list(good)
    a[6] = p(none)
    refused(counts(e.h, *a), ARG, "d_denom is NULL")
    assert (Z == 7.0).all()
    refused(raw("drephip_set_linkage_path")(e.h, 3), ARG, "bad linkage path")


# ---------------------------------------------------------------------- marks
@pytest.mark.gpu
def test_marks_forms_refuse_what_the_screen_cannot_index(env):
    e = env
    n = C.c_uint64(77)
    dC, dP = e.dC.data_ptr(), e.dP.data_ptr()
    huge = (1 << 32) // S                                             # N x s = 2^32: an argument check, nothing is read
    marked, smarked = raw("drephip_allpairs_device_marked"), raw("drephip_allpairs_sparse_device_marked")
    refused(marked(e.h, e.dtri[0], e.dtri[1], huge, 0, 4, dC, None, None, 0, None, 0, None), UNSUPPORTED,
            "the screen needs N x s < 2^32")
    refused(smarked(e.h, e.dtri[0], e.dtri[1], huge, 0, 4, None, 0, None, 0, dP, 4, C.byref(n), None), UNSUPPORTED,
            "the screen needs N x s < 2^32")
    assert n.value == 0
    e.ctx.set_allpairs_path(e.ctx.AP_MERGE)
    try:
        n.value = 77
        refused(marked(e.h, *e.dtri, dC, None, None, 0, None, 0, None), ARG, "marks need the table or band path")
        refused(smarked(e.h, *e.dtri, None, 0, None, 0, dP, 4, C.byref(n), None), ARG, "marks need the table or band path")
        assert n.value == 0
    finally:
        e.ctx.set_allpairs_path(e.ctx.AP_AUTO)
    refused(raw("drephip_set_allpairs_path")(e.h, 4, 1024), ARG, "unknown all-pairs path")
    refused(raw("drephip_set_allpairs_path")(e.h, 0, 0), ARG, "band_cap must be in 1..1024")


# --------------------------------------------------------------------- timing
@pytest.mark.gpu
def test_timing_survives_a_refused_call(env):
    e = env
    dC = e.dC.data_ptr()
    e.ctx.set_timing(True)
    try:
        assert raw("drephip_allpairs_device")(e.h, *e.dtri, dC, None, None) == OK
        ms, launches = e.ctx.kernel_ms(2)                             # the all-pairs kernel
        assert launches > 0 and ms > 0
        refused(raw("drephip_allpairs_device")(e.h, None, e.dtri[1], N, 0, N, dC, None, None), ARG, "null argument")
        assert e.ctx.kernel_ms(2) == (ms, launches)
        n = C.c_uint64(0)
        refused(raw("drephip_allpairs_sparse")(e.h, *e.tri, None, 4, C.byref(n)), ARG, "null argument")
        refused(raw("drephip_dist_rect_top")(e.h, *e.rect, 2, None, None), ARG, "null argument")
        refused(raw("drephip_linkage_reserve")(e.h, 200001), UNSUPPORTED, "n <= 200000")
        assert e.ctx.kernel_ms(2) == (ms, launches)
        # a record call that ends in DREPHIP_ERR_NOMEM is timed like one that succeeds
        rc, cnt, _, _ = records(e, "drephip_allpairs_sparse_device", 1)
        assert rc == NOMEM and cnt == e.tri_true and sum(e.ctx.kernel_ms(w)[1] for w in (2, 3, 4)) > 0
    finally:
        e.ctx.set_timing(False)


# ------------------------------------------------------- the Python layer's checks
@pytest.mark.gpu
def test_python_layer_value_errors(env):
    e = env
    ctx = e.ctx
    short = e.H[:, :S - 1]
    co = np.zeros(N * N, np.uint16)
    for call in (lambda: ctx.allpairs(short, e.NH), lambda: ctx.allpairs_rows(short, e.NH, 0, N, co),
                 lambda: ctx.allpairs_sparse_raw(short, e.NH, 0, N, None), lambda: ctx.allpairs_sparse(short, e.NH)):
        with pytest.raises(ValueError, match=r"hashes must be \[N, s\] = \[12, 64\], got \(12, 63\)"):
            call()
    for call in (lambda: ctx.allpairs_sparse_sig(short, e.NH, e.LEN), lambda: ctx.allpairs_sparse_sig(e.H, e.NH, e.LEN[:-1]),
                 lambda: ctx.allpairs_sparse_sig_raw(short, e.NH, e.LEN, 0, N, 1.0, None, None, None),
                 lambda: ctx.allpairs_sparse_sig_raw(e.H, e.NH, e.LEN[:-1], 0, N, 1.0, None, None, None)):
        with pytest.raises(ValueError, match=r"hashes must be \[N, s\] and length \[N\]"):
            call()
    for bad in (np.zeros((8, 4), np.int32), np.zeros((8, 3), np.uint32), np.zeros(32, np.uint32),
                np.zeros((8, 8), np.uint32)[:, :4]):
        for call in (lambda: ctx.allpairs_sparse_raw(e.H, e.NH, 0, N, bad),
                     lambda: ctx.dist_rect_sparse_raw(e.QH, e.QN, e.H, e.NH, 0, Q, bad)):
            with pytest.raises(ValueError, match=r"pairs must be a contiguous uint32 \[cap, 4\] array"):
                call()
    # the retry of the record calls: a first buffer that is too small is invisible
    want = ctx.allpairs_sparse(e.H, e.NH)
    assert len(want[0]) == e.tri_true
    for cap in (0, 1, e.tri_true - 1, e.tri_true):
        got = ctx.allpairs_sparse(e.H, e.NH, cap=cap)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    want = ctx.dist_rect_sparse(e.QH, e.QN, e.H, e.NH)
    assert len(want[0]) == e.rect_true
    for cap in (0, 1, e.rect_true):
        got = ctx.dist_rect_sparse(e.QH, e.QN, e.H, e.NH, cap=cap)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    rc, cnt = ctx.allpairs_sparse_raw(e.H, e.NH, 0, N, np.zeros((1, 4), np.uint32))
    assert (rc, cnt) == (NOMEM, e.tri_true)
    rc, cnt = ctx.dist_rect_sparse_raw(e.QH, e.QN, e.H, e.NH, 0, Q, np.zeros((1, 4), np.uint32))
    assert (rc, cnt) == (NOMEM, e.rect_true)
