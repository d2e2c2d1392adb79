"""GPU: range predicates on the tag word (annhip_query_between, annhip_index_exact_query_between, annhip_exact_knn_between;
include/ann_hip.h).  Row i competes for query q iff qlo[q] <= (tags[i] & qmask[q]) <= qhi[q], unsigned.  The oracle is the
allow-list bitmap path, as in tests/test_gpu_tags.py: in fixed mode a query's answer depends on nothing but its own row,
codes and ranked bits, so for every predicate g of a batch the ranged batch's rows with predicate g must equal -- ids and
distance bytes, no tolerance -- the same rows of the whole batch queried under set_filter(allow_g), with
allow_g = lo_g <= (tags & mask_g) <= hi_g computed in numpy.

Radius calls: with radius +inf the row is, by the header's contract, query(k=, where=triple) followed by radius_trim, and
that is what is asserted.  With finite radii that equality is no part of the contract (stage 2 of a radius query follows
the graph edges of in-range stage-1 results only), so finite radii are held against the bitmap path's own query_radius,
group by group, like every other call shape here."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from tests.test_gpu_tags import SHAPES, _build, _np, _same_bits

pytestmark = pytest.mark.gpu

# (mask, lo, hi), dealt round-robin over the queries of every batch
PRED = [(0xFFFF, 100, 299),                         # day window
        (0xFFFFFF, 1 << 16 | 100, 1 << 16 | 299),   # tenant 1 and the window
        (0xFFFF, 7, 7),                             # degenerate interval
        (0, 0, 0),                                  # everything
        (0xFFFF, 0, 0xFFFF),                        # everything
        (0xFFFFFFFF, 0x80000000, 0xFFFFFFFF),       # exactly the bit-31 rows: a signed compare fails here
        (0xFFFF, 300, 100),                         # nobody
        (0xFFFF, 1, 0),                             # nobody: a wrapped span fails here
        (0xFFFF, 0x10000, 0x1FFFF),                 # nobody: lo above the mask
        (0xFFFF, 2000, 2001)]                       # fewer than k rows: pads
NOBODY, FEW = (6, 7, 8), 9


def _tags(n, k, seed):
    """day uniform 0..999 in bits 0-15, tenant uniform 0..3 in bits 16-23, bit 31 on a random half, then exactly
    max(1, k - 2) rows moved to the reserved days 2000-2001."""
    rng = np.random.default_rng(seed)
    tags = rng.integers(0, 1000, size=n).astype(np.uint32)
    tags |= rng.integers(0, 4, size=n).astype(np.uint32) << np.uint32(16)
    tags |= (rng.random(n) < 0.5).astype(np.uint32) << np.uint32(31)
    rows = rng.choice(n, size=max(1, k - 2), replace=False)
    tags[rows] = (tags[rows] & ~np.uint32(0xFFFF)) | (np.uint32(2000) + (rows & 1).astype(np.uint32))
    return tags


def _triple(Q, pred=PRED, shift=0):
    return tuple(np.array([pred[(q + shift) % len(pred)][j] for q in range(Q)], dtype=np.uint32) for j in range(3))


def _groups(Q, pred=PRED):
    return [np.arange(g, Q, len(pred)) for g in range(len(pred))]


def _allow(tags, p):
    t = tags & np.uint32(p[0])
    return (t >= np.uint32(p[1])) & (t <= np.uint32(p[2]))


def _oracle(ix, call, Q, tags, base=None, pred=PRED):
    """Rows of group g from the WHOLE batch under set_filter(allow_g [& base]); call() -> a tuple of arrays with Q rows.
    Leaves the filter at `base`."""
    out = None
    for g, rows in enumerate(_groups(Q, pred)):
        allow = _allow(tags, pred[g])
        ix.set_filter(allow if base is None else allow & base)
        r = call()
        if out is None:
            out = tuple(np.empty_like(a) for a in r)
        for o, a in zip(out, r):
            o[rows] = a[rows]
    ix.set_filter(base)
    return out


def _np3(t):
    return tuple(v.cpu().numpy() for v in t)


def _eq(got, want, what):
    assert _same_bits(got[:2], want[:2]), what
    for a, b in zip(got[2:], want[2:]):
        assert np.array_equal(a, b), what


def _check_pads(got, pad, Q, kq, few):
    gr = _groups(Q)
    for g in NOBODY:
        assert np.all(got[0][gr[g]] == pad) and np.all(np.isinf(got[1][gr[g]])), g
    if kq > few:
        assert np.all(got[0][gr[FEW]][:, -1] == pad) and np.all(np.isinf(got[1][gr[FEW]][:, -1]))


def _radii(dists, kq, dtype):
    """Finite radii from a [Q,kq] result: a distance out of the middle of each row (+inf where the row is short), every
    fifth query a negative radius, every seventh zero."""
    rad = dists[:, kq // 3].astype(dtype).copy()
    rad[::5] = -1.0
    rad[3::7] = 0.0
    return rad


def _all_shapes(ix, yy, alias, Q, tags, base, pad, k, what):
    """Every call shape of the approximate path on one batch against the bitmap oracle."""
    w = _triple(Q)
    few = max(1, k - 2)
    want = _oracle(ix, lambda: _np(ix.query(yy, alias=alias)), Q, tags, base)
    got = _np(ix.query(yy, alias=alias, where=w))
    _eq(got, want, (what, "query"))
    _check_pads(got, pad, Q, k, few)
    if alias:
        for x in range(Q):
            assert x not in got[0][x].tolist()
    for kq in (1, k, min(100, ix.max_query_k)):
        want = _oracle(ix, lambda: _np(ix.query(yy, alias=alias, k=kq)), Q, tags, base)
        r = ix.query(yy, alias=alias, k=kq, where=w)
        got = _np(r)
        _eq(got, want, (what, "query(k=%d)" % kq))
        _check_pads(got, pad, Q, kq, few)
        # radius +inf: the row of query(k=) followed by radius_trim
        inf = float("inf")
        ids, dd = r[0].clone(), r[1].clone()
        cnt = A.radius_trim(ids, dd, inf, pad)
        _eq(_np3(ix.query_radius(yy, inf, k=kq, alias=alias, where=w)), _np3((ids, dd, cnt)), (what, "radius inf k=%d" % kq))
        # finite radii: the bitmap path's own radius query, group by group
        rad = _radii(got[1], kq, got[1].dtype)
        want = _oracle(ix, lambda: _np3(ix.query_radius(yy, rad, k=kq, alias=alias)), Q, tags, base)
        got3 = _np3(ix.query_radius(yy, rad, k=kq, alias=alias, where=w))
        _eq(got3, want, (what, "radius k=%d" % kq))
        assert (got3[2] == 0).any() and (got3[2] > 0).any()


# ------------------------------------------------------------------------------------------ 1: mixed batch, group by group
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_mixed_batch_equals_the_bitmap_path_group_by_group(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 8100 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        tags = _tags(n, k, 81)
        ix.set_fixed(True)
        ix.set_tags(tags)
        for b in (0, 3, "all"):
            ix.set_probe(b)
            for yy, alias in ((ty, False), (ta, True)):
                _all_shapes(ix, yy, alias, yy.shape[0], tags, None, n, k, (b, alias))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 2: identities
PAIRS = [(0xFFFF, 7), (0xFF0000, 1 << 16), (0, 0), (0x80000000, 0x80000000), (0xFFFF, 0x10000), (0xFFFFFFFF, 2 << 16 | 500)]


@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_lo_equal_hi_gives_the_pair_form_bits(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 8200 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        ix.set_fixed(True)
        ix.set_tags(_tags(n, k, 82))
        for b in (0, 3):
            ix.set_probe(b)
            for yy, alias in ((ty, False), (ta, True)):
                Q = yy.shape[0]
                qm = np.array([PAIRS[q % len(PAIRS)][0] for q in range(Q)], dtype=np.uint32)
                qv = np.array([PAIRS[q % len(PAIRS)][1] for q in range(Q)], dtype=np.uint32)
                pair, tri = (qm, qv), (qm, qv, qv.copy())
                assert _same_bits(_np(ix.query(yy, alias=alias, where=tri)), _np(ix.query(yy, alias=alias, where=pair))), (b, alias)
                for kq in (1, k, 100):
                    want = _np(ix.query(yy, alias=alias, k=kq, where=pair))
                    assert _same_bits(_np(ix.query(yy, alias=alias, k=kq, where=tri)), want), (b, alias, kq)
                    rad = _radii(want[1], kq, want[1].dtype)
                    _eq(_np3(ix.query_radius(yy, rad, k=kq, alias=alias, where=tri)),
                        _np3(ix.query_radius(yy, rad, k=kq, alias=alias, where=pair)), (b, alias, kq, "radius"))
    finally:
        ix.close()


@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_everything_intervals_return_the_untagged_bits_and_row_count(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 8250 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        ix.set_fixed(True)
        ix.set_tags(_tags(n, k, 83))
        ix.profile(1)

        def rows_of(call):
            ix.stats(reset=True)
            r = _np(call())
            torch.cuda.synchronize()
            return r, ix.stats(reset=True)["s1_rows"]

        for b in (0, 3, "all"):
            ix.set_probe(b)
            for yy, alias in ((ty, False), (ta, True)):
                Q = yy.shape[0]
                z, f = np.zeros(Q, dtype=np.uint32), np.full(Q, 0xFFFFFFFF, dtype=np.uint32)
                for kw in ({}, {"k": 1}, {"k": 100}):
                    plain, rows_plain = rows_of(lambda: ix.query(yy, alias=alias, **kw))
                    for w in ((z, z, z), (f, z, f), (np.full(Q, 0xFFFF, dtype=np.uint32), z, f)):
                        got, rows_got = rows_of(lambda: ix.query(yy, alias=alias, where=w, **kw))
                        assert _same_bits(got, plain), (b, alias, kw)
                        assert rows_got == rows_plain, (b, alias, kw, rows_got, rows_plain)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 3: the test precedes the fetch
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_gathered_row_count_is_the_sum_over_the_groups(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 8300 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        tags = _tags(n, k, 84)
        ix.set_fixed(True)
        ix.set_tags(tags)
        ix.profile(1)
        for b in (0, 3):
            ix.set_probe(b)
            ix.stats(reset=True)
            ix.query(ty, where=_triple(80))
            torch.cuda.synchronize()
            rows_tag = ix.stats(reset=True)["s1_rows"]
            want = 0
            for g, rows in enumerate(_groups(80)):
                ix.set_filter(_allow(tags, PRED[g]))
                ix.stats(reset=True)
                ix.query(ty[torch.from_numpy(rows).cuda()].contiguous())
                torch.cuda.synchronize()
                want += ix.stats(reset=True)["s1_rows"]
            ix.set_filter(None)
            print("%s n %d d %d b %r: stage-1 rows ranged %d, bitmap path summed over the groups %d" % (prec, n, d, b, rows_tag, want))
            assert rows_tag == want, (b, rows_tag, want)
            for g in NOBODY:
                w = tuple(np.full(80, PRED[g][j], dtype=np.uint32) for j in range(3))
                for kw in ({}, {"k": 100}):
                    ix.stats(reset=True)
                    got = _np(ix.query(ty, where=w, **kw))
                    torch.cuda.synchronize()
                    assert ix.stats(reset=True)["s1_rows"] == 0, (b, PRED[g], kw)
                    assert np.all(got[0] == n) and np.all(np.isinf(got[1]))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 4: AND with the allow list
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_range_test_and_index_bitmap_both_apply(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 8400 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        tags = _tags(n, k, 85)
        m = np.random.default_rng(850).random(n) < 0.5
        ix.set_fixed(True)
        ix.set_tags(tags)
        for b in (0, 3):
            ix.set_probe(b)
            for yy, alias in ((ty, False), (ta, True)):
                ix.set_filter(m)
                _all_shapes(ix, yy, alias, yy.shape[0], tags, m, n, k, (b, alias))
                got = _np(ix.query(yy, alias=alias, where=_triple(yy.shape[0])))
                assert m[got[0][got[0] < n]].all()
            ix.set_filter(None)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 5: tail and hashed tail
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_range_predicates_over_the_tail_tiers(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 8500 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        tail = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(350 * d).reshape(350, d))).cuda()
        tags = np.concatenate([_tags(n, k, 86), _tags(350, k, 87)])
        ix.set_fixed(True)
        ix.set_tags(tags[:n])

        def check(m, what):
            nt = n + m
            assert ix.n_total == nt
            for b in (0, 3):
                ix.set_probe(b)
                for yy, alias in ((ty, False), (ta, True)):
                    Q = yy.shape[0]
                    w = _triple(Q)
                    for kw in ({}, {"k": 100}):
                        want = _oracle(ix, lambda: _np(ix.query(yy, alias=alias, **kw)), Q, tags[:nt])
                        got = _np(ix.query(yy, alias=alias, where=w, **kw))
                        _eq(got, want, (what, b, alias, kw))
                        _check_pads(got, nt, Q, kw.get("k", k), 2 * max(1, k - 2))
            return got

        ix.append(tail[:300].contiguous(), tags=tags[n:n + 300])
        got = check(300, "scanned tail")
        assert (got[0][got[0] < n + 300] >= n).any()  # tail rows are among the answers
        ix.hash_tail()
        check(300, "hashed tail")
        ix.append(tail[300:].contiguous(), tags=tags[n + 300:])
        check(350, "hashed tail + fresh rows")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 6: narrow rows
@pytest.mark.parametrize("prec,rows", [("f32", "f16"), ("f64", "f32")])
def test_range_predicates_compose_with_narrow_rows(prec, rows):
    n, d, k, T = 4000, 64, 7, 4
    orc, pts, tp, ix = _build(prec, n, d, k, T, 8600)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(60 * d).reshape(60, d))).cuda()
        tags = _tags(n, k, 88)
        ix.set_fixed(True)
        ix.set_tags(tags)
        for b in (0, 4):
            ix.set_probe(b)
            for setting in (rows, "native"):
                ix.set_rows(setting)
                res = {}
                for kw in ({}, {"k": 100}):
                    want = _oracle(ix, lambda: _np(ix.query(ty, **kw)), 60, tags)
                    got = _np(ix.query(ty, where=_triple(60), **kw))
                    _eq(got, want, (b, setting, kw))
                    res[len(kw)] = got
                if setting == "native":
                    native = res[0]
                else:
                    narrow = res[0]
            assert not np.array_equal(narrow[1].view(np.uint8), native[1].view(np.uint8))  # the narrow rows were read
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7: exact paths
def _exact_groups_equal(got, pts, y, k, tags, Q, self_exclude=False, base=None):
    for g, rows in enumerate(_groups(Q)):
        allow = _allow(tags, PRED[g]) if base is None else _allow(tags, PRED[g]) & base
        want = A.exact_knn(pts, y, k, self_exclude=self_exclude, allow=torch.from_numpy(allow).cuda())
        r = torch.from_numpy(rows).cuda()
        assert torch.equal(got[0][r], want[0][r]) and torch.equal(got[1][r].view(torch.uint8), want[1][r].view(torch.uint8)), (k, PRED[g])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("d", [128, 80, 100, 300])
def test_exact_knn_with_range_predicates(prec, d):
    n, Q = 3000, 70
    dt = torch.float32 if prec == "f32" else torch.float64
    gen = torch.Generator().manual_seed(870 + d)
    pts = torch.randn((n, d), generator=gen, dtype=torch.float64).to(dt).cuda()
    y = torch.randn((Q, d), generator=gen, dtype=torch.float64).to(dt).cuda()
    tags = _tags(n, 10, 89)  # 8 rows on the reserved days
    where = _triple(Q)
    gr = _groups(Q)
    for k in (1, 10, 100):
        got = A.exact_knn(pts, y, k, tags=tags, where=where)
        _exact_groups_equal(got, pts, y, k, tags, Q)
        for g in NOBODY:
            assert torch.all(got[0][gr[g]] == n) and torch.all(torch.isinf(got[1][gr[g]]))
        if k > 8:
            few = got[0][gr[FEW]]
            assert torch.all(few[:, 8:] == n) and torch.all(few[:, :8] < n) and torch.all(torch.isinf(got[1][gr[FEW]][:, 8:]))
    # the words as device tensors give the same bits
    dev = A.exact_knn(pts, y, 10, tags=torch.from_numpy(tags.view(np.int32)).cuda(),
                      where=tuple(torch.from_numpy(w.view(np.int32)).cuda() for w in where))
    ref = A.exact_knn(pts, y, 10, tags=tags, where=where)
    assert torch.equal(dev[0], ref[0]) and torch.equal(dev[1].view(torch.uint8), ref[1].view(torch.uint8))
    # lo == hi is the pair form
    pair = A.exact_knn(pts, y, 10, tags=tags, where=(where[0], where[1]))
    tri = A.exact_knn(pts, y, 10, tags=tags, where=(where[0], where[1], where[1]))
    assert torch.equal(pair[0], tri[0]) and torch.equal(pair[1].view(torch.uint8), tri[1].view(torch.uint8))
    # self_exclude with y = points
    yq = pts[:Q].contiguous()
    got = A.exact_knn(pts, yq, 10, self_exclude=True, tags=tags, where=where)
    _exact_groups_equal(got, pts, yq, 10, tags, Q, self_exclude=True)
    for q in range(Q):
        assert q not in got[0][q].tolist()
    # allow= given as well: ANDed with the range test
    m = np.random.default_rng(871).random(n) < 0.5
    got = A.exact_knn(pts, y, 10, tags=tags, where=where, allow=torch.from_numpy(m).cuda())
    _exact_groups_equal(got, pts, y, 10, tags, Q, base=m)


@pytest.mark.parametrize("prec,d", [("f32", 64), ("f64", 64), ("f32", 100), ("f64", 300)])
def test_index_exact_query_with_range_predicates(prec, d):
    n, m, k, Q = 2000, 300, 10, 90
    orc, pts, tp, ix = _build(prec, n, d, k, 3, 8750 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))).cuda()
        tail = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(m * d).reshape(m, d))).cuda()
        tags = np.concatenate([_tags(n, k, 90), _tags(m, k, 91)])
        base = np.random.default_rng(875).random(n + m) < 0.5
        ix.set_fixed(True)
        ix.set_tags(tags[:n])
        ix.append(tail, tags=tags[n:])
        allp = torch.cat([tp, tail]).contiguous()
        w = _triple(Q)
        for flt in (None, base):
            ix.set_filter(flt)
            for alias, yy in ((False, ty), (True, tp[:Q].contiguous())):
                for kq in (None, 1, 100):
                    got = ix.exact_query(yy, alias=alias, where=w, **({} if kq is None else {"k": kq}))
                    _exact_groups_equal(got, allp, yy, kq or k, tags, Q, self_exclude=alias, base=flt)
                # radius: exact_query(k=) under the predicate, trimmed
                kq = 100
                full = ix.exact_query(yy, alias=alias, where=w, k=kq)
                rad = _radii(full[1].cpu().numpy(), kq, full[1].cpu().numpy().dtype)
                ids, dd = full[0].clone(), full[1].clone()
                cnt = A.radius_trim(ids, dd, rad, n + m)
                _eq(_np3(ix.exact_query_radius(yy, rad, kq, alias=alias, where=w)), _np3((ids, dd, cnt)), (flt is None, alias))
        ix.set_filter(None)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 8: validation, streams
def test_refusals_leave_the_outputs_untouched():
    n, Q = 3000, 60
    orc, pts, tp, ix = _build("f32", n, 64, 10, 4, 8800)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * 64).reshape(Q, 64))).cuda()
        tags, w = _tags(n, 10, 92), _triple(Q)
        ids = torch.full((Q, 10), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((Q, 10), -7.0, dtype=torch.float32, device="cuda")

        def refused(**kw):
            for extra in ({}, {"k": 10}):
                with pytest.raises(ValueError):
                    ix.query(ty, out_ids=ids, out_dists=dd, **extra, **kw)
            torch.cuda.synchronize()
            assert torch.all(ids == -7) and torch.all(dd == -7.0)  # nothing was launched

        ix.set_tags(tags)
        refused(where=w)                 # fixed mode is off
        with pytest.raises(ValueError):
            ix.query_radius(ty, 1.0, where=w)
        ix.set_fixed(True)
        ix.set_tags(None)
        refused(where=w)                 # no tags
        for call in (lambda: ix.query_radius(ty, 1.0, where=w), lambda: ix.query_reranked(ty, where=w),
                     lambda: ix.exact_query(ty, where=w), lambda: ix.exact_query(ty, where=w, k=5),
                     lambda: ix.exact_query_radius(ty, 1.0, 10, where=w)):
            with pytest.raises(ValueError):
                call()
        ix.set_tags(tags)
        for bad in (w[0], (w[0],), w + (w[2],), (w[0], None, w[2]), (None, w[1], w[2]), (w[0], w[1], None),
                    (w[0][:-1], w[1], w[2]), (w[0], w[1], w[2][:-1]), (w[0], w[1].astype(np.int32), w[2]),
                    (w[0], w[1], w[2].astype(np.int64)),
                    tuple(torch.from_numpy(a.view(np.int32)) for a in w)):  # int32 tensors, but not on the device
            refused(where=bad)
            for call in (lambda: ix.query_radius(ty, 1.0, where=bad), lambda: ix.query_reranked(ty, where=bad),
                         lambda: ix.exact_query(ty, where=bad), lambda: ix.exact_query_radius(ty, 1.0, 10, where=bad),
                         lambda: A.exact_knn(tp, ty, 10, tags=tags, where=bad)):
                with pytest.raises(ValueError):
                    call()
        # the library's own refusal of a NULL array: -2, nothing launched
        dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in w]
        for hole in range(3):
            p = [t.data_ptr() for t in dev]
            p[hole] = None
            assert ix.lib.annhip_query_between(ix.h, None, None, Q, ty.data_ptr(), 0, 10, None, p[0], p[1], p[2],
                                               ids.data_ptr(), dd.data_ptr(), None) == -2
            assert ix.lib.annhip_index_exact_query_between(ix.h, Q, ty.data_ptr(), 0, 10, None, p[0], p[1], p[2],
                                                           ids.data_ptr(), dd.data_ptr(), None) != 0
            assert ix.lib.annhip_exact_knn_between(n, 64, 10, tp.data_ptr(), Q, ty.data_ptr(), 0, dev[0].data_ptr(), None,
                                                   p[0], p[1], p[2], ids.data_ptr(), dd.data_ptr()) != 0
        assert ix.lib.annhip_query_between(ix.h, None, None, Q, ty.data_ptr(), 0, 0, None, *[t.data_ptr() for t in dev],
                                           ids.data_ptr(), dd.data_ptr(), None) == -2  # kq == 0
        torch.cuda.synchronize()
        assert torch.all(ids == -7) and torch.all(dd == -7.0)
        # and the accepted call writes them; device tensors and numpy arrays give the same bits
        ix.query(ty, out_ids=ids, out_dists=dd, where=tuple(dev))
        assert _same_bits(_np((ids, dd)), _np(ix.query(ty, where=w)))
        assert not _same_bits(_np((ids, dd)), _np(ix.query(ty)))
    finally:
        ix.close()


def test_range_predicates_on_workspaces_and_streams():
    n = 5000
    orc, pts, tp, ix = _build("f32", n, 64, 10, 6, 8900)
    try:
        ta = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(500 * 64).reshape(500, 64))).cuda()
        tb = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(300 * 64).reshape(300, 64))).cuda()
        ix.set_fixed(True)
        ix.set_tags(_tags(n, 10, 93))
        wa, wb = _triple(500), _triple(300, shift=3)  # another dealing of the predicates
        for b in (0, 5):
            ix.set_probe(b)
            serial = [_np(ix.query(ta, where=wa)), _np(ix.query(tb, where=wb, k=40)), _np3(ix.query_radius(tb, 60.0, k=40, where=wb)),
                      _np(ix.query_reranked(ta, k=5, oversample=4, where=wa))]
            torch.cuda.synchronize()
            w1, w2, s1, s2 = ix.workspace(), ix.workspace(), torch.cuda.Stream(), torch.cuda.Stream()
            with torch.cuda.stream(s1):
                ga = ix.query(ta, ws=w1, stream=s1, where=wa)
                gd = ix.query_reranked(ta, k=5, oversample=4, where=wa, ws=w1, stream=s1)
            with torch.cuda.stream(s2):
                gb = ix.query(tb, ws=w2, stream=s2, where=wb, k=40)
                gc = ix.query_radius(tb, 60.0, k=40, where=wb, ws=w2, stream=s2)
            s1.synchronize(), s2.synchronize()
            assert _same_bits(_np(ga), serial[0]) and _same_bits(_np(gb), serial[1])
            _eq(_np3(gc), serial[2], b)
            assert _same_bits(_np(gd), serial[3])
    finally:
        ix.close()
