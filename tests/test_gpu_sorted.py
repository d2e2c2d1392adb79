"""GPU: the tag order and the exact scan of its runs (annhip_index_sort_tags, annhip_tag_runs, annhip_query_sorted and
Index.query_routed(scan_below=); include/ann_hip.h, ann_sorted_kernels.h).

The oracle is Index.exact_query(y, k=kq, where=(M, qlo, qhi)) with M[q] = the order's mask, and exact_query_radius: they
stream all n_total rows through exact_scan_kernel / tail_merge_kernel and never run the new kernels.  Every comparison is
on ids and distance bytes, with no tolerance.

The tag column gives the values 1..6 exact row counts around the scan's LDS tile, which _scan_tile computes from d and the
precision as the host does (exact_shape in ann_host.hip with sorted = true: no prefetch, 16 KB of rows, one row at least):
  value 1: 1 row, 2: tile - 1, 3: tile, 4: tile + 1, 5: 3 * tile + 5 (several tiles), 6: 3 rows (fewer than k: pads),
  7, 8, 9: nobody, 10..19: the other rows.
The batch of _intervals asks for identical runs (six queries on value 5), pairwise disjoint and touching runs (single
values; neighbouring values touch in the order), nested and overlapping windows, the whole index, a value nobody has and
qlo > qhi.  Shapes and helpers: tests/test_gpu_tail.py, tests/test_gpu_query_k.py."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests.test_gpu_query_k import _np, _same_bits, _tenants
from tests.test_gpu_tail import SHAPES, Q, _rows

pytestmark = pytest.mark.gpu

FULL = 0xFFFFFFFF
_built = {}


def _scan_tile(prec, d):
    """Rows of the sorted scan's LDS tile: exact_shape(..., sorted = true) restated -- it never prefetches."""
    return max(1, 16384 // (d * (4 if prec == "f32" else 8)))


def _index(shape):
    """One index per shape for the whole module (fixed mode on), handed out without tail, filter, tags or order."""
    if shape not in _built:
        prec, n, d, kg, T = shape
        tp = torch.from_numpy(_rows(prec, n, d, 7100 + d)).cuda()
        A._lib.load(prec)
        torch.cuda.synchronize()
        O.srandom(7200 + d)
        ix = A.Index.precomp(tp, kg, T)
        ix.set_fixed(True)
        _built[shape] = (tp, ix)
    tp, ix = _built[shape]
    ix.drop_tail()
    ix.set_rows("native")
    ix.set_filter(None)
    ix.set_tags(None)
    ix.profile(False)
    assert ix.tag_order is None
    return tp, ix


def _values(prec, n, d, seed, rows=None):
    """The value column described above -> uint32 [rows] (rows = n unless given), scattered over the row ids."""
    rows = n if rows is None else rows
    t = _scan_tile(prec, d)
    counts = {1: 1, 2: t - 1, 3: t, 4: t + 1, 5: 3 * t + 5, 6: 3}
    rng = np.random.default_rng(seed)
    v = rng.integers(10, 20, size=rows).astype(np.uint32)
    where = rng.permutation(rows)
    at = 0
    for val, c in counts.items():
        v[where[at:at + c]] = val
        at += c
    assert at < rows
    return v, counts


def _intervals(Qn):
    """(lo, hi) value intervals of a batch, cycled to Qn queries: see the module's docstring."""
    base = ([(5, 5)] * 6 + [(1, 1), (2, 2), (3, 3), (4, 4), (6, 6)] + [(2, 5), (3, 4), (4, 12), (10, 15), (12, 19)]
            + [(0, FULL), (7, 7), (9, 8), (11, 11), (13, 13), (19, 19), (6, 10)])
    iv = (base * (Qn // len(base) + 1))[:Qn]
    return np.array([a for a, _ in iv], dtype=np.uint32), np.array([b for _, b in iv], dtype=np.uint32)


def _queries(prec, Qn, d, seed):
    return torch.from_numpy(_rows(prec, Qn, d, seed)).cuda()


def _runs_numpy(tags, mask, qlo, qhi):
    keys = np.sort(tags & np.uint32(mask), kind="stable")
    start = np.searchsorted(keys, qlo, side="left")
    length = np.searchsorted(keys, qhi, side="right") - start
    empty = qlo > qhi
    return np.where(empty, 0, start).astype(np.int64), np.where(empty, 0, length).astype(np.int64)


def _u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _triple(mask, qlo, qhi):
    return (np.full(qlo.shape, mask, dtype=np.uint32), qlo, qhi)


def _eq(ix, y, mask, qlo, qhi, what, k=None, alias=False, **kw):
    got = ix.query_sorted(y, _triple(mask, qlo, qhi), k=k, alias=alias, **kw)
    want = ix.exact_query(y, alias=alias, where=_triple(mask, qlo, qhi), k=k)
    g, w = _np(got), _np(want)
    bad = np.nonzero((g[0] != w[0]).any(axis=1))[0]
    assert bad.size == 0, "%s: ids differ for queries %s, first: got %s want %s" % (what, bad[:8], g[0][bad[0]][:8], w[0][bad[0]][:8])
    assert _same_bits(g, w), "%s: distances not bit-identical" % what
    return g


# ------------------------------------------------------------------------------------------ 1: results and runs
@pytest.mark.parametrize("shape", SHAPES, ids=["%s-n%d-d%d-k%d-T%d" % s for s in SHAPES])
def test_sorted_scan_equals_the_exact_scan(shape):
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    tags, counts = _values(prec, n, d, 7300 + d)
    ix.set_tags(tags)
    ix.sort_tags()
    assert ix.tag_order == (FULL, n)
    qlo, qhi = _intervals(Q)
    y = _queries(prec, Q, d, 7400 + d)
    # the runs: numpy.searchsorted on the sorted masked column, and every length the module promises occurs
    start, length = ix.tag_runs(_triple(FULL, qlo, qhi))
    ws, wl = _runs_numpy(tags, FULL, qlo, qhi)
    assert np.array_equal(_u32(start), ws) and np.array_equal(_u32(length), wl)
    t = _scan_tile(prec, d)
    for L in (0, 1, t - 1, t, t + 1, 3 * t + 5, 3, n):
        assert (wl == L).any(), L
    assert (qlo > qhi).any() and 3 < kg
    assert (wl == 3 * t + 5).sum() > 4  # identical runs shared by more than the four queries of a wave
    pair = ix.tag_runs((np.full(Q, FULL, dtype=np.uint32), qlo))  # a pair is the interval [value, value]
    pw = _runs_numpy(tags, FULL, qlo, qlo)
    assert np.array_equal(_u32(pair[0]), pw[0]) and np.array_equal(_u32(pair[1]), pw[1])
    for k in (None, 1, 256, 1024):
        g = _eq(ix, y, FULL, qlo, qhi, "%s k=%s" % (shape, k), k=k)
        kk = g[0].shape[1]
        few = wl < kk
        assert few.any()
        for q in np.nonzero(few)[0]:  # pads (n_total, +inf) behind the rows the run has
            assert (g[0][q, wl[q]:] == n).all() and np.isinf(g[1][q, wl[q]:]).all() and (g[0][q, :wl[q]] < n).all()
    gp = ix.query_sorted(y, (np.full(Q, FULL, dtype=np.uint32), qlo))
    assert _same_bits(_np(gp), _np(ix.exact_query(y, where=(np.full(Q, FULL, dtype=np.uint32), qlo))))


@pytest.mark.parametrize("shape", SHAPES, ids=["%s-n%d-d%d-k%d-T%d" % s for s in SHAPES])
def test_sub_field_and_packed_masks(shape):
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    rng = np.random.default_rng(7500 + d)
    val, _ = _values(prec, n, d, 7300 + d)
    y = _queries(prec, Q, d, 7400 + d)
    qlo, qhi = _intervals(Q)
    qhi = np.minimum(qhi, 0xFF)
    # a sub-field: the value in bits 16-23, every other bit random
    tags = (val << np.uint32(16)) | rng.integers(0, 1 << 16, size=n).astype(np.uint32) | (rng.integers(0, 256, size=n).astype(np.uint32) << np.uint32(24))
    ix.set_tags(tags)
    ix.sort_tags(0x00FF0000)
    assert ix.tag_order == (0x00FF0000, n)
    lo, hi = qlo << np.uint32(16), qhi << np.uint32(16)
    start, length = ix.tag_runs(_triple(0x00FF0000, lo, hi))
    ws, wl = _runs_numpy(tags, 0x00FF0000, lo, hi)
    assert np.array_equal(_u32(start), ws) and np.array_equal(_u32(length), wl)
    _eq(ix, y, 0x00FF0000, lo, hi, "%s sub-field" % (shape,))
    # tenant in bits 16-27, day in bits 0-15, the top four bits random: "tenant t from day a to day b" is one interval
    tenant, _ = _tenants(n, Q, 7600 + d)
    day = rng.integers(0, 400, size=n).astype(np.uint32)
    tags = (rng.integers(0, 16, size=n).astype(np.uint32) << np.uint32(28)) | (tenant << np.uint32(16)) | day
    ix.set_tags(tags)
    assert ix.tag_order is None  # new tags drop the order
    ix.sort_tags(0x0FFFFFFF)
    qt = (np.arange(Q) % 4).astype(np.uint32)  # tenant 3 has no rows
    a = rng.integers(0, 380, size=Q).astype(np.uint32)
    b = a + rng.integers(0, 120, size=Q).astype(np.uint32)
    lo, hi = (qt << np.uint32(16)) | a, (qt << np.uint32(16)) | b
    lo[:6], hi[:6] = 1 << 16, (1 << 16) | 0xFFFF  # one tenant, all days, six times
    wl = _runs_numpy(tags, 0x0FFFFFFF, lo, hi)[1]
    assert (wl == 0).any() and (wl > _scan_tile(prec, d)).any()
    _eq(ix, y, 0x0FFFFFFF, lo, hi, "%s tenant/day" % (shape,))
    _eq(ix, y, 0x0FFFFFFF, lo, hi, "%s tenant/day k=1" % (shape,), k=1)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[5]], ids=["f32-d64", "f64-d300"])
def test_a_shared_run_straddles_workgroups(shape):
    """Q = 150: sixty queries on one run are more than one workgroup's share (48, or 16 in the any-d kernel) of the list."""
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    tags, _ = _values(prec, n, d, 7300 + d)
    ix.set_tags(tags)
    ix.sort_tags()
    Qn = 150
    qlo, qhi = _intervals(Qn)
    qlo[40:100], qhi[40:100] = 5, 5
    y = _queries(prec, Qn, d, 7700 + d)
    for k in (None, 256):
        _eq(ix, y, FULL, qlo, qhi, "%s Q=150 k=%s" % (shape, k), k=k)


# ------------------------------------------------------------------------------------------ 2: with the other features
@pytest.mark.parametrize("shape", SHAPES, ids=["%s-n%d-d%d-k%d-T%d" % s for s in SHAPES])
def test_sorted_scan_composes_with_the_other_features(shape):
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    rng = np.random.default_rng(7800 + d)
    m1, m2 = 41, 23  # rows appended before the sort and after it
    tags, _ = _values(prec, n, d, 7300 + d, rows=n + m1)
    qlo, qhi = _intervals(Q)
    y = _queries(prec, Q, d, 7400 + d)
    ya = tp[:Q].contiguous()
    what = "%s " % (shape,)
    ix.set_tags(tags[:n])
    ix.sort_tags()
    # alias, and narrow rows: the answer stays the native one
    _eq(ix, ya, FULL, qlo, qhi, what + "alias", alias=True)
    _eq(ix, ya, FULL, qlo, qhi, what + "alias k=1", alias=True, k=1)
    plain = _eq(ix, y, FULL, qlo, qhi, what + "plain")
    ix.set_rows("f16" if prec == "f32" else "f32")
    assert _same_bits(_np(ix.query_sorted(y, _triple(FULL, qlo, qhi))), plain), what + "narrow rows"
    ix.set_rows("native")
    # the allow list (share 0.4) is tested at scan time: the order stays
    allow = rng.random(n) < 0.4
    ix.set_filter(allow)
    assert ix.tag_order == (FULL, n)
    ga = _eq(ix, y, FULL, qlo, qhi, what + "allow")
    assert allow[ga[0][ga[0] < n]].all() and not _same_bits(ga, plain)
    _eq(ix, ya, FULL, qlo, qhi, what + "allow alias k=256", alias=True, k=256)
    ix.set_filter(None)
    # rows appended before the sort are inside the order ...
    tail1 = _rows(prec, m1, d, 7900 + d)
    ix.append(tail1, tags=tags[n:])
    assert ix.tag_order is not None  # append keeps the order: the rows are fresh
    _eq(ix, y, FULL, qlo, qhi, what + "fresh only")
    ix.hash_tail()  # a hashed tail changes nothing here
    ix.sort_tags()
    assert ix.tag_order == (FULL, n + m1)
    _eq(ix, y, FULL, qlo, qhi, what + "tail inside the order")
    g1 = _eq(ix, y, FULL, qlo, qhi, what + "tail inside the order k=64", k=64)
    assert (g1[0][g1[0] < n + m1] >= n).any()  # (41 of the rows are tail rows: some are among 37 x 64 neighbours)
    # ... rows appended after it are fresh: among them copies of queries, each its query's nearest
    tail2 = _rows(prec, m2, d, 8000 + d)
    hit = [q for q in range(Q) if qlo[q] <= qhi[q]][:5]
    ftags = rng.integers(10, 20, size=m2).astype(np.uint32)
    for j, q in enumerate(hit):
        tail2[j] = y[q].cpu().numpy()
        ftags[j] = qlo[q]
    ix.append(tail2, tags=ftags)
    assert ix.tag_order == (FULL, n + m1) and ix.n_total == n + m1 + m2
    g2 = _eq(ix, y, FULL, qlo, qhi, what + "fresh rows")
    for j, q in enumerate(hit):
        assert g2[0][q, 0] == n + m1 + j and g2[1][q, 0] == 0
    allow = rng.random(n + m1 + m2) < 0.4
    allow[n + m1:n + m1 + 2] = True
    ix.set_filter(allow)
    _eq(ix, y, FULL, qlo, qhi, what + "tail, fresh rows and allow list")
    _eq(ix, ya, FULL, qlo, qhi, what + "tail, fresh rows, allow list, alias, k=1024", alias=True, k=1024)
    # a workspace and a stream give the null stream's bits
    null = _np(ix.query_sorted(y, _triple(FULL, qlo, qhi), k=20))
    st, ws = torch.cuda.Stream(), ix.workspace()
    on = ix.query_sorted(y, _triple(FULL, qlo, qhi), k=20, ws=ws, stream=st)
    st.synchronize()
    assert _same_bits(_np(on), null), what + "stream"
    # radius: a finite one from the data, and +inf
    dist = null[1]
    fin = np.where(np.isfinite(dist), dist, 0)
    rad = np.ascontiguousarray(fin[:, : 20].max(axis=1) * 0.5).astype(dist.dtype)
    res = {}
    for r, tag in ((rad, "finite"), (float("inf"), "inf")):
        gi, gd, gc = ix.query_sorted(y, _triple(FULL, qlo, qhi), k=20, radius=r)
        wi, wd, wc = ix.exact_query_radius(y, r, 20, where=_triple(FULL, qlo, qhi))
        assert _same_bits(_np((gi, gd)), _np((wi, wd))), what + "radius " + tag
        assert np.array_equal(gc.cpu().numpy(), wc.cpu().numpy()), what + "radius counts " + tag
        res[tag] = (_np((gi, gd)), gc.cpu().numpy())
    assert _same_bits(res["inf"][0], null)
    assert (res["finite"][1] > 0).any() and (res["finite"][1] < res["inf"][1]).any()  # the finite radius cuts some rows
    on_r = ix.query_sorted(y, _triple(FULL, qlo, qhi), k=20, radius=rad, ws=ws, stream=st)
    st.synchronize()
    assert _same_bits(_np(on_r), res["finite"][0]) and np.array_equal(on_r[2].cpu().numpy(), res["finite"][1])


# ------------------------------------------------------------------------------------------ 3: the sharing
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[5]], ids=["f32-d64", "f64-d80", "f64-d300"])
def test_rows_fetched_show_the_sharing(shape):
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    tags, counts = _values(prec, n, d, 7300 + d)
    ix.set_tags(tags)
    ix.sort_tags()
    y = _queries(prec, Q, d, 7400 + d)
    ix.profile(True)

    def fetched(qlo, qhi, k=None):
        before = ix.stats()["other_rows"]
        ix.query_sorted(y, _triple(FULL, qlo, qhi), k=k)
        torch.cuda.synchronize()
        return int(ix.stats()["other_rows"] - before)

    # pairwise disjoint runs: every value at most once, whole values only
    vals = np.array(([1, 2, 3, 4, 5, 6, 7] + list(range(10, 20)) + [8, 9] * 10)[:Q], dtype=np.uint32)
    assert len(vals) == Q
    vals[19:] = 7  # nobody: empty runs
    wl = _runs_numpy(tags, FULL, vals, vals)[1]
    for k in (None, 1024):  # 1024: a few queries per workgroup, many workgroups
        got = fetched(vals, vals, k)
        print("disjoint runs k=%s: fetched %d rows, sum of the run lengths %d" % (k, got, wl.sum()))
        assert got == wl.sum()
    # one run of L rows asked by all 37 queries: once per workgroup, not once per query
    five = np.full(Q, 5, dtype=np.uint32)
    L = counts[5]
    got = fetched(five, five)
    print("one run of %d rows, %d queries: fetched %d rows" % (L, Q, got))
    assert L <= got <= L * ((Q + 3) // 4)
    ix.profile(False)


# ------------------------------------------------------------------------------------------ 4: the router
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[5]], ids=["f32-d64", "f32-d100", "f64-d300"])
def test_scan_below_routes_row_for_row(shape):
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    tags, counts = _values(prec, n, d, 7300 + d)
    ix.set_tags(tags)
    ix.sort_tags()
    qlo, qhi = _intervals(Q)
    y = _queries(prec, Q, d, 7400 + d)
    R = counts[4]
    wl = _runs_numpy(tags, FULL, qlo, qhi)[1]
    short = wl <= R
    assert short.any() and (~short).any()
    for k, where in ((None, _triple(FULL, qlo, qhi)), (7, _triple(FULL, qlo, qhi)), (7, (np.full(Q, FULL, dtype=np.uint32), qlo))):
        if len(where) == 2:
            short = _runs_numpy(tags, FULL, qlo, qlo)[1] <= R
            assert short.any() and (~short).any()
        got = _np(ix.query_routed(y, where, scan_below=R, k=k))
        exact = _np(ix.query_sorted(y, where, k=k))
        ann = _np(ix.query(y, where=where, k=k))
        for q in range(Q):
            src = exact if short[q] else ann
            assert np.array_equal(got[0][q], src[0][q]) and np.array_equal(got[1][q].view(np.uint8), src[1][q].view(np.uint8)), (k, q)
    everything = _np(ix.query_routed(y, _triple(FULL, qlo, qhi), scan_below=n))
    assert _same_bits(everything, _np(ix.query_sorted(y, _triple(FULL, qlo, qhi))))
    assert _same_bits(_np(ix.query_routed(y, _triple(FULL, qlo, qhi))), _np(ix.query(y, where=_triple(FULL, qlo, qhi))))  # None: today's call
    with pytest.raises(ValueError):
        ix.query_routed(tp[:Q].contiguous(), _triple(FULL, qlo, qhi), scan_below=R, alias=True)
    with pytest.raises(ValueError):
        ix.query_routed(y, _triple(0xFF, qlo, qhi), scan_below=R)
    ix.sort_tags(0)
    with pytest.raises(ValueError):
        ix.query_routed(y, _triple(FULL, qlo, qhi), scan_below=R)


# ------------------------------------------------------------------------------------------ 5: refusals and lifecycle
def _raw(ix, y, kq, qlo, qhi, ids, dists, alias=0):
    return ix.lib.annhip_query_sorted(ix.h, None, None, y.shape[0], y.data_ptr(), alias, kq, None,
                                      qlo.data_ptr() if qlo is not None else None, qhi.data_ptr(), ids.data_ptr(), dists.data_ptr(), None)


def test_refusals_and_lifecycle():
    shape = SHAPES[3]
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    tags, _ = _values(prec, n, d, 7300 + d)
    qlo, qhi = _intervals(Q)
    y = _queries(prec, Q, d, 7400 + d)
    dlo = torch.from_numpy(qlo.view(np.int32)).cuda()
    dhi = torch.from_numpy(qhi.view(np.int32)).cuda()
    ids = torch.full((Q, 1024), -7, dtype=torch.int64, device="cuda")
    dists = torch.full((Q, 1024), -3.0, dtype=y.dtype, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((ids == -7).all().item()) and bool((dists == -3.0).all().item())

    # no tags, no order
    with pytest.raises(ValueError):
        ix.sort_tags()
    assert ix.tag_order is None
    with pytest.raises(ValueError):
        ix.query_sorted(y, _triple(FULL, qlo, qhi))
    with pytest.raises(ValueError):
        ix.tag_runs(_triple(FULL, qlo, qhi))
    assert _raw(ix, y, kg, dlo, dhi, ids, dists) == -2 and untouched()
    start = torch.full((Q,), -5, dtype=torch.int32, device="cuda")
    assert ix.lib.annhip_tag_runs(ix.h, None, Q, dlo.data_ptr(), dhi.data_ptr(), start.data_ptr(), start.data_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((start == -5).all().item())
    ix.set_tags(tags)
    assert _raw(ix, y, kg, dlo, dhi, ids, dists) == -2 and untouched()  # tags, still no order
    for bad in (True, -1, 1 << 32, 1.5):
        with pytest.raises(ValueError):
            ix.sort_tags(bad)
    ix.sort_tags(0xFF)
    assert ix.tag_order == (0xFF, n)
    # a wrong mask: numpy and device input
    with pytest.raises(ValueError):
        ix.query_sorted(y, _triple(FULL, qlo, qhi))
    mixed = np.full(Q, 0xFF, dtype=np.uint32)
    mixed[-1] = 0xF
    with pytest.raises(ValueError):
        ix.query_sorted(y, (mixed, qlo, qhi))
    with pytest.raises(ValueError):
        ix.query_sorted(y, (torch.from_numpy(mixed.view(np.int32)).cuda(), dlo, dhi))
    dm = torch.full((Q,), 0xFF, dtype=torch.int32, device="cuda")
    assert _same_bits(_np(ix.query_sorted(y, (dm, dlo, dhi))), _np(ix.exact_query(y, where=(dm, dlo, dhi))))
    # kq of 0, 1025 and more than the rows on offer; a NULL array
    for kq in (0, 1025):
        assert _raw(ix, y, kq, dlo, dhi, ids, dists) == -2 and untouched(), kq
    assert _raw(ix, y, kg, None, dhi, ids, dists) == -2 and untouched()
    for k in (0, 1025, True, 2.0):
        with pytest.raises(ValueError):
            ix.query_sorted(y, _triple(0xFF, qlo, qhi), k=k)
    # what keeps the order and what drops it
    ix.set_filter(np.ones(n, dtype=bool))
    ix.set_probe(2), ix.set_rows("f16"), ix.set_rows("native"), ix.set_probe(0)
    ix.set_fixed(False), ix.set_fixed(True)
    assert ix.tag_order == (0xFF, n)
    ix.append(_rows(prec, 5, d, 1), tags=np.arange(5, dtype=np.uint32))
    ix.hash_tail()
    assert ix.tag_order == (0xFF, n)
    new = ix.compact(tries=T)
    try:
        assert new.tag_order == (0xFF, n + 5) and new.n == n + 5
        assert _same_bits(_np(new.query_sorted(y, _triple(0xFF, qlo, qhi))), _np(ix.query_sorted(y, _triple(0xFF, qlo, qhi))))
    finally:
        new.close()
    ix.drop_tail()
    assert ix.tag_order is None
    ix.sort_tags(0xFF)
    ix.set_tags(tags)
    assert ix.tag_order is None
    ix.sort_tags(0xFF)
    ix.sort_tags(None)
    assert ix.tag_order is None
    ix.sort_tags(0xFF)
    ix.set_tags(None)
    assert ix.tag_order is None
    # a resharded index: no tags, no order, and the call itself refuses
    ns = 600  # fewer rows than 1024: kq can exceed the rows on offer
    small = tp[:ns].contiguous()
    lone = A.Index.precomp(small, kg, T)
    try:
        lone.set_tags(tags[:ns])
        lone.sort_tags()
        for kq, alias in ((ns + 1, 0), (ns, 1)):
            assert _raw(lone, small[:Q].contiguous(), kq, dlo, dhi, ids, dists, alias) == -2 and untouched(), (kq, alias)
        whole = _triple(FULL, np.zeros(Q, dtype=np.uint32), np.full(Q, FULL, dtype=np.uint32))
        assert _same_bits(_np(lone.query_sorted(y, whole, k=ns)), _np(lone.exact_query(y, where=whole, k=ns)))  # fixed mode is off
        half = tp[: ns // 2].contiguous()
        lone.reshard(half, 0, ns // 2)
        assert lone.tag_order is None
        with pytest.raises(ValueError):
            lone.sort_tags()
        assert _raw(lone, y, kg, dlo, dhi, ids, dists) == -2 and untouched()
    finally:
        lone.close()


def test_zz_close_the_shared_indexes():
    for tp, ix in _built.values():
        ix.close()
    _built.clear()
