"""GPU: every loop or launch of the feature kernels whose SECOND iteration starts only above a size, crossed once each
("Size steps": the table of those loops, their thresholds and the test of this module that crosses each).

  A  the exact scan's launcher cuts a batch into chunks of queries (exact_run in ann_host.hip): q0 > 0
  B  the tag sort's scan carries across chunks of 1 024 histogram words, its init kernel and the allow-list pack take a
     second grid stride above 4096 x 256 rows
  C  the sorted scan ranks a batch through LDS tiles of 256 queries, one block per 256 queries
  D  the hashed tail's CSR scan carries across chunks of 1 024 buckets, its count and place kernels take a second grid
     stride above 4096 x 256 (row, try) items
  F  rows appended behind the tag order: the mask fill takes a second grid stride above 1024 x 256 queries

Every test first asserts that its threshold is crossed, from the host's constants restated below (the way _scan_tile and
_tile_rows restate exact_shape): a later change of a constant fails the precondition, not the crossing.  Every comparison
is on ids and distance bytes, with no tolerance.  A's reference is numpy (tests/test_gpu_exact_knn.py: np_exact, np_dists);
B's is numpy for the order, the runs and the id sets, and Index.exact_query(where=) -- the scan A ties to numpy -- for the
distance bytes; C's and F's is Index.exact_query(where=); D's is the twin index, the library's hash codes, numpy's hit test
and A.exact_knn (tests/test_gpu_tail_hash.py: Expect).  Large row counts are appended rows on one small index.

What fails if a second iteration is wrong:
  A  without the q0 * k output offset the second chunk's rows are never written and the first chunk's are overwritten: the
     numpy comparison fails for nearly every query; without A.q0 the second chunk answers the first chunk's queries.
  B  without the carry the digits of the second chunk land on the first chunk's places: the keys are not sorted and the
     runs differ from searchsorted (the first assertion, before any scan).  Without the second stride of tsort_init_kernel
     or filter_pack_kernel the rows from 1 048 576 on are missing from the order / keep stale bits: the id sets (their
     union covers every position) and filter_count differ.
  C  without the cross-tile tie-break two queries of the shared run get one list slot: one of them is never answered, and
     its row differs from exact_query's.
  D  without the carry the buckets from 1 024 on start at the wrong offsets: the expected hashed rows that hit ONLY there
     (asserted to exist) are not found.  Without the second stride the last tail rows are never filed: the planted copies
     of the queries, each its query's nearest at distance 0, are missing.
  F  without the second stride the mask words of the last queries are not written: their fresh rows -- copies of exactly
     those queries -- fail the tag test."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd.sharded import HipEngine
from oracle import oracle_py as O
from tests.test_gpu_exact_knn import gpu_exact, normal, np_dists, np_exact, ranges, same
from tests.test_gpu_query_k import _codes_of, _np, _same_bits
from tests.test_gpu_sorted import FULL, _intervals, _runs_numpy, _triple, _u32, _values
from tests.test_gpu_sorted import _eq as sorted_eq
from tests.test_gpu_tail import SHAPES, _rows, _twins
from tests.test_gpu_tail_hash import Expect, _nonvacuous, _valid, _want
from tests.test_gpu_tail_hash import _eq as hash_eq

pytestmark = pytest.mark.gpu

# ---- the host's constants, restated (ann_host.hip, ann_sorted_kernels.h, ann_tail_hash_kernels.h, ann_filter_kernels.h)
EX_WS_BYTES = 256 << 20       # ANN_EX_WS_BYTES: the exact scan's workspace cap
EX_RANGES_MAX = 16384         # ranges <= 16384 / k
KEY_BYTES = {"f32": 8, "f64": 16}
SORT_ITEMS = 2048             # ANN_SORT_ITEMS: pairs per block of the tag sort; 256 histogram words per block
SCAN_CHUNK = 1024             # words tsort_scan_kernel / thash_scan_kernel scan per turn, then carry
ORDER_TILE = 256              # queries per LDS tile and per block of sorted_order_kernel
GRID_CAP = 4096 * 256         # grid_for(work, 256, 4096): threads of one grid stride (tsort_init, thash_count, thash_place)
PACK_ROWS = 4096 * 4 * 64     # grid_for((n + 63) / 64, 4, 4096): rows of one grid stride of filter_pack_kernel (one wave: 64)
FILL_CAP = 1024 * 256         # grid_for(work, 256, 1024): sorted_fill_kernel, exact_tail_kernel

SUB = 0x0000FFF0              # a field in two bytes of the tag word: two passes of the sort, the second must be stable
_built = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _query_chunk(prec, n, k, forced):
    """exact_run restated for a forced range count: (the most queries one launch takes, the ranges).  The launcher rounds
    the chunk DOWN to whole query groups, so a batch larger than this is cut in every case."""
    r = max(1, min(forced, n, max(1, EX_RANGES_MAX // k)))
    rr = -(-n // r)
    r = -(-n // rr)
    return EX_WS_BYTES // (r * k * KEY_BYTES[prec]), r


def _np_select(dist, valid, k):
    """The k smallest (distance, id) among the valid rows of every query, then pads (n, +inf): dist, valid [Q, n]."""
    Qn, n = dist.shape
    ids = np.arange(n)
    wi = np.full((Qn, k), n, dtype=np.int64)
    wd = np.full((Qn, k), np.inf, dtype=dist.dtype)
    for q in range(Qn):
        order = np.lexsort((ids, dist[q]))
        order = order[valid[q, order]][:k]
        wi[q, :order.size], wd[q, :order.size] = order, dist[q, order]
    return wi, wd


def _small():
    """One f32 index of 2 000 rows, d = 16, fixed mode on, handed out without tail, filter, tags or order."""
    if "small" not in _built:
        tp = _cuda(_rows("f32", 2000, 16, 8100))
        A._lib.load("f32")
        torch.cuda.synchronize()
        O.srandom(8101)
        ix = A.Index.precomp(tp, 6, 2)
        ix.set_fixed(True)
        _built["small"] = (tp, ix)
    tp, ix = _built["small"]
    ix.drop_tail()
    ix.set_filter(None)
    ix.set_tags(None)
    assert ix.tag_order is None and ix.n_total == ix.n == 2000 and ix.d == 16
    return tp, ix


# ------------------------------------------------------------------------------------------ A: the exact scan's query chunks
A_N, A_D, A_K, A_R = 1100, 8, 1024, 16
A_CASES = [("f32", 2101), ("f64", 1101)]  # one chunk is 2 048 (f32) / 1 024 (f64) queries at 16 ranges and k = 1024


def _a_crossed(prec, n, Qn):
    chunk, r = _query_chunk(prec, n, A_K, A_R)
    assert r == A_R and A_R * A_K == EX_RANGES_MAX  # the most ranges the launcher allows: the smallest chunk
    assert chunk < Qn < 2 * chunk and Qn % 4  # a second launch with q0 > 0, a short one, its last query group ragged
    return chunk


@pytest.mark.parametrize("prec,Qn", A_CASES, ids=["%s-Q%d" % c for c in A_CASES])
def test_exact_scan_in_two_query_chunks(prec, Qn):
    _a_crossed(prec, A_N, Qn)
    pts, y = normal(prec, A_N, A_D, Qn, 4100 + Qn)
    with ranges(A_R):
        same(gpu_exact(pts, y, A_K), np_exact(pts, y, A_K), "%s Q=%d" % (prec, Qn))


@pytest.mark.parametrize("prec,Qn", A_CASES, ids=["%s-Q%d" % c for c in A_CASES])
def test_exact_scan_self_exclude_in_two_query_chunks(prec, Qn):
    n = Qn + 7  # y = points[:Q]: query q of the second chunk leaves out row q0 + (q - q0), not row q - q0
    _a_crossed(prec, n, Qn)
    pts, _ = normal(prec, n, A_D, 1, 4200 + Qn)
    y = np.ascontiguousarray(pts[:Qn])
    with ranges(A_R):
        got = gpu_exact(pts, y, A_K, self_exclude=True)
    same(got, np_exact(pts, y, A_K, self_exclude=True), "%s Q=%d self" % (prec, Qn))
    assert not (got[0] == np.arange(Qn)[:, None]).any()


@pytest.mark.parametrize("prec,Qn", A_CASES, ids=["%s-Q%d" % c for c in A_CASES])
def test_exact_scan_pads_in_the_second_query_chunk(prec, Qn):
    chunk = _a_crossed(prec, A_N, Qn)
    assert min(chunk, Qn) * A_K > FILL_CAP  # exact_tail_kernel's second grid stride as well
    pts, y = normal(prec, A_N, A_D, Qn, 4300 + Qn)
    dist = np_dists(pts, y)
    rng = np.random.default_rng(4400 + Qn)
    tp, ty = _cuda(pts), _cuda(y)
    # an allow list of fewer than k rows: every query ends in pads, those of the second chunk written at q0 > 0
    allow = rng.random(A_N) < 0.6
    assert 0 < allow.sum() < A_K
    with ranges(A_R):
        got = _np(A.exact_knn(tp, ty, A_K, allow=_cuda(allow)))
    want = _np_select(dist, np.broadcast_to(allow, dist.shape), A_K)
    same(got, want, "%s Q=%d allow" % (prec, Qn))
    assert (got[0][chunk:, allow.sum():] == A_N).all() and np.isinf(got[1][chunk:, allow.sum():]).all()
    # tags and an allow list: every third query admits every allowed row (k of them exist: no pad), the others a quarter
    tags = rng.integers(0, 4, size=A_N).astype(np.uint32)
    allow = np.ones(A_N, dtype=bool)
    allow[rng.choice(A_N, 40, replace=False)] = False
    q = np.arange(Qn)
    qmask = np.where(q % 3 == 0, 0, 3).astype(np.uint32)
    qval = np.where(q % 3 == 0, 0, q % 4).astype(np.uint32)
    valid = ((tags[None, :] & qmask[:, None]) == qval[:, None]) & allow[None, :]
    few = valid.sum(axis=1) < A_K
    assert few[chunk:].any() and (~few)[chunk:].any() and few[:chunk].any() and (~few)[:chunk].any()
    with ranges(A_R):
        got = _np(A.exact_knn(tp, ty, A_K, allow=_cuda(allow), tags=tags, where=(qmask, qval)))
    same(got, _np_select(dist, valid, A_K), "%s Q=%d tags and allow" % (prec, Qn))


def test_index_exact_query_in_two_query_chunks():
    """Index.exact_query(k=1024, where=) on the launcher's chunks, without and with a tail; the reference is
    A.exact_knn(tags=, where=, allow=) over all rows, which the tests above tie to numpy at these sizes."""
    tp, ix = _small()
    n, Qn, m = ix.n, 2101, 50
    for rows in (n, n + m):
        chunk, r = _query_chunk("f32", rows, A_K, A_R)
        assert r == A_R and chunk < Qn < 2 * chunk and Qn % 4
    rng = np.random.default_rng(4500)
    ty = _cuda(_rows("f32", Qn, ix.d, 4501))
    tail = _cuda(_rows("f32", m, ix.d, 4502))
    tags = rng.integers(0, 4, size=n + m).astype(np.uint32)
    allow = rng.random(n + m) < 0.9
    q = np.arange(Qn)
    where = (np.where(q % 3 == 0, 0, 3).astype(np.uint32), np.where(q % 3 == 0, 0, q % 4).astype(np.uint32))
    with ranges(A_R):
        ix.set_tags(tags[:n])
        ix.set_filter(allow[:n])
        got = _np(ix.exact_query(ty, k=A_K, where=where))
        want = _np(A.exact_knn(tp, ty, A_K, allow=_cuda(allow[:n]), tags=tags[:n], where=where))
        assert _same_bits(got, want), "built rows"
        assert (got[0][chunk:] == n).any() and (got[0][chunk:, -1] < n).any()  # pads and full rows in the second chunk
        ix.append(tail, tags=tags[n:])
        ix.set_filter(allow)
        got = _np(ix.exact_query(ty, k=A_K, where=where))
        want = _np(A.exact_knn(torch.cat([tp, tail]), ty, A_K, allow=_cuda(allow), tags=tags, where=where))
        assert _same_bits(got, want), "built rows and tail"
        assert ((got[0][chunk:] >= n) & (got[0][chunk:] < n + m)).any() and (got[0][chunk:] == n + m).any()


# ------------------------------------------------------------------------------------------ B: the tag order
def _tag_column(rows, seed):
    """(uint32 [rows], the values): a value in bits 4..15, at most 1 000 rows per value, scattered over the ids; junk in every
    other bit."""
    rng = np.random.default_rng(seed)
    nvals = -(-rows // 1000)
    assert nvals < 4096
    vals = ((np.arange(nvals) * 7 + 13) % 4096).astype(np.uint32)  # distinct; every low nibble occurs from nine values on
    val = np.empty(rows, dtype=np.uint32)
    val[rng.permutation(rows)] = vals[np.arange(rows) % nvals]
    junk = rng.integers(0, 1 << 32, size=rows, dtype=np.uint64).astype(np.uint32) & np.uint32(~SUB & FULL)
    assert np.unique(vals).size == nvals and np.bincount(val).max() <= 1000
    return (val << np.uint32(4)) | junk, vals


def _digits_behind_the_first_chunk(tags, mask):
    """Does a pass of the sort file some digit wholly behind the first 1 024 histogram words (word = digit * nblk + block)?
    Only then does the scan's carry decide where a pair goes."""
    nblk = -(-tags.shape[0] // SORT_ITEMS)
    keys = tags & np.uint32(mask)
    return any((((keys >> np.uint32(s)) & np.uint32(255)).astype(np.int64) * nblk >= SCAN_CHUNK).any()
               for s in (0, 8, 16, 24) if (mask >> s) & 255)


def _grow(ix, rows, seed):
    ix.append(_rows("f32", rows - ix.n_total, ix.d, seed))
    assert ix.n_total == rows


def _check_order(ix, tags, mask, qlo, qhi, ty, what, allow=None, sample=40):
    """The runs against numpy.searchsorted on the stably sorted masked column; the id set of every query against the rows
    numpy selects (ANDed with allow), then pads; a sample of the queries, ids and distance bytes, against exact_query."""
    rows, Qn, k = tags.shape[0], qlo.shape[0], 1024
    trip = _triple(mask, qlo, qhi)
    start, length = ix.tag_runs(trip)
    ws, wl = _runs_numpy(tags, mask, qlo, qhi)
    assert np.array_equal(_u32(start), ws) and np.array_equal(_u32(length), wl), what + ": runs"
    covered = np.zeros(rows, dtype=bool)
    for q in range(Qn):
        covered[ws[q]:ws[q] + wl[q]] = True
    assert covered.all() and wl.max() <= k  # the batch's runs cover every position of the order, and k holds a whole run
    order = np.argsort(tags & np.uint32(mask), kind="stable")
    got = _np(ix.query_sorted(ty, trip, k=k))
    for q in range(Qn):
        members = np.sort(order[ws[q]:ws[q] + wl[q]])
        if allow is not None:
            members = members[allow[members]]
        L = members.size
        assert np.array_equal(np.sort(got[0][q, :L]), members), (what, q)
        assert (got[0][q, L:] == rows).all() and np.isinf(got[1][q, L:]).all() and np.isfinite(got[1][q, :L]).all(), (what, q)
        assert (np.diff(got[1][q, :L]) >= 0).all(), (what, q)
    pick = np.sort(np.random.default_rng(rows).choice(Qn, min(sample, Qn), replace=False))
    sub = tuple(np.ascontiguousarray(w[pick]) for w in trip)
    want = _np(ix.exact_query(ty[torch.from_numpy(pick).cuda()].contiguous(), where=sub, k=k))
    assert _same_bits((got[0][pick], got[1][pick]), want), what + ": sample against exact_query"
    return got


B_ROWS = [8192, 8193, 20011, 1050001]


@pytest.mark.parametrize("rows", B_ROWS)
def test_tag_order_across_the_scan_chunk_and_the_grid_cap(rows):
    words = 256 * (-(-rows // SORT_ITEMS))  # tsort_scan_kernel's total
    if rows == B_ROWS[0]:
        assert words == SCAN_CHUNK  # the largest order whose scan is one chunk: the step lies between this case and the next
    else:
        assert words > SCAN_CHUNK   # a second chunk: carry += part[1023] decides where its digits go
    big = rows == B_ROWS[-1]
    assert not big or (rows > GRID_CAP and rows > PACK_ROWS)  # tsort_init_kernel's and filter_pack_kernel's second stride
    tp, ix = _small()
    _grow(ix, rows, 8200)
    tags, vals = _tag_column(rows, 8300 + rows % 97)
    nvals = vals.size
    assert rows == B_ROWS[0] or _digits_behind_the_first_chunk(tags, SUB)
    ix.set_tags(tags)
    ix.sort_tags(SUB)
    assert ix.tag_order == (SUB, rows)
    Qn = nvals  # one query per value
    assert not big or Qn > 4 * ORDER_TILE  # (this batch crosses the tiles of sorted_order_kernel as well)
    qv = vals[np.random.default_rng(8400).permutation(nvals)] << np.uint32(4)
    ty = _cuda(_rows("f32", Qn, ix.d, 8500))
    what = "rows=%d" % rows
    _check_order(ix, tags, SUB, qv, qv, ty, what)
    if rows == 8193:  # the full mask: four passes, every run an interval between two quantiles of the whole words
        assert _digits_behind_the_first_chunk(tags, FULL)
        ix.sort_tags()
        assert ix.tag_order == (FULL, rows)
        keys = np.sort(tags)
        cut = np.arange(0, rows, 1000)
        _check_order(ix, tags, FULL, keys[cut], keys[np.minimum(cut + 1000, rows) - 1], ty[:cut.size].contiguous(), what + " full mask")
    if big:  # an allow list packed on the device: share one half, other bits behind row 4096 x 4 x 64 than at the front
        allow = np.random.default_rng(8600).random(rows) < 0.5
        assert not np.array_equal(allow[PACK_ROWS:], allow[:rows - PACK_ROWS]) and allow[PACK_ROWS:].any() and not allow[PACK_ROWS:].all()
        ix.set_filter(_cuda(allow))
        assert ix.filter_count == int(allow.sum())
        assert ix.tag_order == (SUB, rows)
        got = _check_order(ix, tags, SUB, qv, qv, ty, what + " allow", allow=allow)
        real = got[0][got[0] < rows]
        assert allow[real].all() and (real >= PACK_ROWS).any()


# ------------------------------------------------------------------------------------------ C: more than 256 queries
def _shape_index(shape):
    if shape not in _built:
        prec, n, d, kg, T = shape
        tp = _cuda(_rows(prec, n, d, 8700 + d))
        A._lib.load(prec)
        torch.cuda.synchronize()
        O.srandom(8800 + d)
        ix = A.Index.precomp(tp, kg, T)
        ix.set_fixed(True)
        _built[shape] = (tp, ix)
    return _built[shape]


C_SHAPES = [SHAPES[0], SHAPES[5]]


@pytest.mark.parametrize("Qn", [257, 600])
@pytest.mark.parametrize("shape", C_SHAPES, ids=["f32-d64", "f64-d300"])
def test_sorted_scan_ranks_more_than_one_tile_of_queries(shape, Qn):
    assert Qn > ORDER_TILE  # a second LDS tile in every block's loop and a second block
    # the queries [a, b) ask for ONE run: they straddle the positions 255/256 (and 511/512), so the tie-break of equal
    # (start, end) across tiles, t0 + t < q, alone keeps their list slots apart
    a, b = (100, 257) if Qn == 257 else (200, 520)
    assert a < ORDER_TILE - 1 and b > ORDER_TILE and (Qn < 2 * ORDER_TILE or (b > 2 * ORDER_TILE and b - a >= 300))
    prec, n, d, kg, T = shape
    tp, ix = _shape_index(shape)
    tags, _ = _values(prec, n, d, 8900 + d)
    ix.set_tags(tags)
    ix.sort_tags()
    qlo, qhi = _intervals(Qn)
    qlo[a:b], qhi[a:b] = 5, 5
    y = _rows(prec, Qn, d, 9000 + d + Qn)
    y[a:b] = y[a + np.arange(b - a) % 3]  # three query vectors in turn: equal runs AND equal vectors must give equal rows
    ty = _cuda(y)
    for k in (None, 256):
        g = sorted_eq(ix, ty, FULL, qlo, qhi, "%s Q=%d k=%s" % (shape, Qn, k), k=k)
        groups = [np.arange(a + j, b, 3) for j in range(3)]
        assert any(grp[0] < ORDER_TILE <= grp[-1] for grp in groups)
        for j, grp in enumerate(groups):
            assert (g[0][grp] == g[0][grp[0]]).all() and (g[1][grp].view(np.uint8) == g[1][grp[0]].view(np.uint8)).all(), (k, j)


# ------------------------------------------------------------------------------------------ D: the hashed tail
D_SHAPE = ("f32", 20000, 32, 10, 10)  # d_short = 11: 2 049 counters per try


def _d_twins():
    if "twins" not in _built:
        _built["twins"] = _twins(*D_SHAPE, 9100)
    pts, tp, ix, twin = _built["twins"]
    ix.drop_tail()
    for i in (ix, twin):
        i.set_filter(None)
        i.set_probe(0)
    return pts, tp, ix, twin


def _d_crossed(ix):
    stride = (1 << ix.d_short) + 1  # the counters thash_scan_kernel scans per try
    assert ix.d_short >= 11 and stride > 2 * SCAN_CHUNK  # buckets 1 024 .. 2 047: a whole chunk behind the first carry


def _behind_the_first_chunk(exp, want, twin, ttail, n, mh):
    """Some expected hashed row hits ONLY in tries that file it in a bucket above 1 023."""
    ct = _codes_of(HipEngine(twin), ttail[:mh].contiguous(), twin.tries)
    for x, i in zip(*np.nonzero((want[0] >= n) & (want[0] < n + mh))):
        j = want[0][x, i] - n
        tries = exp.hit[x, j]
        if tries.any() and (ct[j][tries] >= SCAN_CHUNK).all():
            return
    raise AssertionError("no expected hashed row lies only in buckets behind the first scan chunk")


def _d_check(ix, twin, ttail, ty, n, mh, what):
    exp = Expect(twin, ttail, ty, mh)
    got, base = _np(ix.query(ty)), _np(twin.query(ty))
    k = got[0].shape[1]
    want = _want(exp, base, n, k, exp.knn(k))
    hash_eq(got, want, what)
    _nonvacuous(exp, want, n, base)
    _behind_the_first_chunk(exp, want, twin, ttail, n, mh)
    return got, exp


def test_hashed_tail_behind_the_first_scan_chunk():
    prec, n, d, kg, T = D_SHAPE
    pts, tp, ix, twin = _d_twins()
    _d_crossed(ix)
    mh, fresh, Qn = 3000, 23, 37
    tail = _rows(prec, mh + fresh, d, 9200)
    ty = _cuda(_rows(prec, Qn, d, 9201))
    ix.append(_cuda(tail[:mh]))
    ix.hash_tail()
    ix.append(_cuda(tail[mh:]))
    assert ix.tail_hashed == mh and ix.tail == mh + fresh
    for probe in (0, 2):
        ix.set_probe(probe), twin.set_probe(probe)
        _d_check(ix, twin, _cuda(tail), ty, n, mh, ("ds >= 11", probe))


def test_hashed_tail_counted_and_placed_in_two_grid_strides():
    prec, n, d, kg, T = D_SHAPE
    pts, tp, ix, twin = _d_twins()
    _d_crossed(ix)
    mh, fresh, Qn = 105000, 23, 8
    assert ix.tries == T and mh * T > GRID_CAP  # thash_count_kernel's and thash_place_kernel's second stride
    j0 = -(-GRID_CAP // T)  # the first tail row all of whose (row, try) items belong to the second stride
    assert j0 + 5 + Qn <= mh
    m = mh + fresh
    tail = _rows(prec, m, d, 9300)
    y = _rows(prec, Qn, d, 9301)
    tail[j0 + 5:j0 + 5 + Qn] = y  # a copy of every query among those rows: it hits in every try and is the nearest
    ty, ttail = _cuda(y), _cuda(tail)
    ix.append(_cuda(tail[:mh]))
    ix.hash_tail()
    ix.append(_cuda(tail[mh:]))
    assert ix.tail_hashed == mh and ix.tail == m
    allow = np.random.default_rng(9302).random(n + m) < 0.5
    allow[n + j0 + 5:n + j0 + 5 + Qn] = np.arange(Qn) % 2 == 0  # the copies of the even queries stay
    for probe in (0, 2):
        ix.set_probe(probe), twin.set_probe(probe)
        got, exp = _d_check(ix, twin, ttail, ty, n, mh, ("two strides", probe))
        assert np.array_equal(got[0][:, 0], n + j0 + 5 + np.arange(Qn)) and not got[1][:, 0].any()
        ix.set_filter(allow), twin.set_filter(allow[:n])
        got = _np(ix.query(ty))
        want = _want(exp, _np(twin.query(ty)), n, kg, exp.knn(kg, _valid(Qn, m, n, allow)))
        hash_eq(got, want, ("two strides, allow", probe))
        real = got[0][got[0] < n + m]
        assert allow[real].all() and ((real >= n) & (real < n + mh)).any()
        assert np.array_equal(got[0][::2, 0], n + j0 + 5 + np.arange(Qn)[::2]) and (got[0][1::2, 0] != n + j0 + 5 + np.arange(Qn)[1::2]).all()
        ix.set_filter(None), twin.set_filter(None)


# ------------------------------------------------------------------------------------------ F: the fresh rows' mask fill
def test_fresh_rows_behind_the_order_in_a_very_large_batch():
    """query_sorted with rows appended after the sort fills the batch's mask words with sorted_fill_kernel: Q above
    1024 x 256 takes its second grid stride.  k = 1, d = 16 and 2 008 rows: the batch is large, the work is not."""
    Qn, nf, nvals = FILL_CAP + 37, 8, 20
    assert Qn > FILL_CAP and Qn % 4
    tp, ix = _small()
    n = ix.n
    rng = np.random.default_rng(9400)
    junk = rng.integers(0, 1 << 32, size=n + nf, dtype=np.uint64).astype(np.uint32) & np.uint32(~SUB & FULL)
    qv = ((np.arange(Qn) % nvals).astype(np.uint32)) << np.uint32(4)
    tags = (rng.integers(0, nvals, size=n + nf).astype(np.uint32) << np.uint32(4)) | junk
    tags[n:] = qv[Qn - nf:] | junk[n:]  # the fresh rows: copies of the LAST queries, each under its query's value
    y = _rows("f32", Qn, ix.d, 9401)
    ix.set_tags(tags[:n])
    ix.sort_tags(SUB)
    ix.append(np.ascontiguousarray(y[Qn - nf:]), tags=tags[n:])
    assert ix.tag_order == (SUB, n) and ix.n_total == n + nf  # the rows are behind the order: the tail's scan, and its mask
    ty = _cuda(y)
    trip = _triple(SUB, qv, qv)
    got = _np(ix.query_sorted(ty, trip, k=1))
    want = _np(ix.exact_query(ty, where=trip, k=1))
    assert _same_bits(got, want)
    assert np.array_equal(got[0][Qn - nf:, 0], n + np.arange(nf)) and not got[1][Qn - nf:, 0].any()  # found behind the cap


def test_zz_close_the_shared_indexes():
    for v in _built.values():
        for ix in v[1:] if len(v) == 2 else v[2:]:
            ix.close()
    _built.clear()
