"""GPU: radius queries of fixed mode (annhip_query_radius, annhip_index_exact_query_radius, annhip_radius_trim;
include/ann_hip.h, ann_radius_kernels.h).

Every check is bit-exact on ids and distance bytes; no tolerance.  No expectation runs the new kernels: they come from
tests/test_gpu_query_k.py::Oracle (exported tables, the library's own codes and ranked bits, numpy validity and
A.exact_knn(points, y[x:x+1], kcap, allow=mask), which has the query path's arithmetic and order).  The expected radius row
of query x: Oracle._scan over the stage-1 candidates; keep id < n and distance <= r (S1); the mask of S1's ids plus their
valid graph neighbours; _scan again; keep <= r, pad (n, +inf), count.  With a tail, that row of the index BEFORE the append
is merged with the tail candidates by tests/test_gpu_tail_hash.py's Expect / _want and trimmed in numpy."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests.test_gpu_query_k import SHAPES, Oracle, _build, _dict, _np, _same_bits, _tenants
from tests.test_gpu_tail import _rows, _twins
from tests.test_gpu_tail_hash import Expect, _want

pytestmark = pytest.mark.gpu


def _np3(t):
    return tuple(v.cpu().numpy() for v in t)


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def trim_np(ids, dd, rad, pad):
    """The contract of annhip_radius_trim in numpy: an entry stays iff id != pad and distance <= radius."""
    ids, dd = ids.copy(), dd.copy()
    with np.errstate(invalid="ignore"):
        keep = (ids != pad) & (dd <= np.asarray(rad)[:, None])
    ids[~keep], dd[~keep] = pad, np.inf
    return ids, dd, keep.sum(axis=1).astype(np.int32)


def _eq3(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(_u8(got[1]), _u8(want[1])), (what, got[1], want[1])
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])


def radius_row(orac, x, kcap, r):
    """The expected radius row of query x (module docstring) -> ids [kcap], dists [kcap], count."""
    n = orac.n
    i1, d1 = orac._scan(x, kcap, orac.cand[x])
    with np.errstate(invalid="ignore"):
        real = i1[(i1 < n) & (d1 <= r)]  # S1
    s2 = np.zeros(n, dtype=bool)
    s2[real] = True
    nb = orac.graph[real].reshape(-1)
    nb = nb[nb < n]
    s2[nb[orac.valid[x, nb]]] = True
    i2, d2 = orac._scan(x, kcap, s2)
    wi, wd, wc = trim_np(i2[None, :], d2[None, :], np.array([r], dtype=d2.dtype), n)
    return wi[0], wd[0], int(wc[0])


def radius_rows(orac, kcap, rad, rows=None):
    Q = orac.ty.shape[0]
    out = [radius_row(orac, x, kcap, rad[x]) for x in (range(Q) if rows is None else rows)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32)


def stage1_dists(orac, upto):
    """Ascending distances of every query's `upto` nearest stage-1 candidates (+inf where fewer exist)."""
    return np.stack([orac._scan(x, upto, orac.cand[x])[1] for x in range(orac.ty.shape[0])])


def cycle_radii(s1d):
    """Per-query radii that cycle through: just below the nearest stage-1 candidate; the distance of stage-1 candidate j for
    j in {0, 2, 7, 40}; 1e30; +inf."""
    dt = s1d.dtype
    rad = np.empty(s1d.shape[0], dtype=dt)
    for x in range(s1d.shape[0]):
        c = x % 7
        if c == 0:
            rad[x] = np.nextafter(s1d[x, 0], dt.type(-np.inf))
        elif c <= 4:
            rad[x] = s1d[x, (0, 2, 7, 40)[c - 1]]
        else:
            rad[x] = dt.type(1e30) if c == 5 else dt.type(np.inf)
    return rad


def _queries(orc, tp, d, count=24):
    ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(count * d).reshape(count, d))).cuda()
    return ((ty, False), (tp[:count].contiguous(), True))


# ------------------------------------------------------------------------------------------ 1: the trim alone
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kcap", [1, 7, 64, 130])
def test_trim_alone_against_numpy(dt, kcap):
    Q, pad = 70, 5000
    rng = np.random.default_rng(7100 + kcap)
    dd = np.sort(rng.random((Q, kcap)).astype(dt) + dt(0.25), axis=1)
    ids = np.stack([rng.permutation(pad)[:kcap] for _ in range(Q)]).astype(np.int64)
    for q in range(Q):  # rows that already end in pads: 1..kcap of them in every third row
        if q % 3 == 1:
            m = kcap - 1 - (q % kcap)
            ids[q, m:], dd[q, m:] = pad, np.inf
    for q in range(Q):  # rows that start at distance +0, under the radii +0 and -0.0
        if q % 3 == 0 and q % 8 in (0, 1):
            dd[q, 0] = 0
    real_inf = [q for q in range(Q) if q % 3 == 2]  # a real id at distance +inf, the last real entry of its row
    for q in real_inf:
        dd[q, kcap - 1] = np.inf
    rad = np.empty(Q, dtype=dt)
    j = [min(q % 9, kcap - 1) for q in range(Q)]  # the entry whose distance the "exact" radii name
    for q in range(Q):
        c = q % 8
        ref = dd[q, j[q]] if np.isfinite(dd[q, j[q]]) else dt(0.5)
        rad[q] = (dt(0.0), dt(-0.0), dt(-1.5), dt(np.nan), dt(np.inf), ref, np.nextafter(ref, dt(-np.inf)), dt(2.0))[c]
    want = trim_np(ids, dd, rad, pad)
    # the cases are there: kept at exactly r, dropped just below; +0 / -0.0 keep a zero distance; the real +inf entry
    assert any(q % 8 == 5 and want[2][q] == j[q] + 1 for q in range(Q) if ids[q, j[q]] != pad and np.isfinite(dd[q, j[q]]))
    assert any(q % 8 == 6 and want[2][q] == j[q] for q in range(Q) if ids[q, j[q]] != pad and np.isfinite(dd[q, j[q]]))
    zero = [q for q in range(Q) if dd[q, 0] == 0 and ids[q, 0] != pad]
    assert {q % 8 for q in zero} >= {0, 1} and all(want[2][q] >= 1 for q in zero if q % 8 in (0, 1))
    assert all(want[2][q] == 0 for q in range(Q) if q % 8 in (2, 3))
    assert any(q % 8 == 4 and want[0][q, kcap - 1] != pad for q in real_inf)
    assert all(want[0][q, kcap - 1] == pad for q in real_inf if q % 8 != 4)

    ti, td, tr = torch.from_numpy(ids).cuda(), torch.from_numpy(dd).cuda(), torch.from_numpy(rad).cuda()
    counts = A.radius_trim(ti, td, tr, pad)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (Q,)
    _eq3(_np3((ti, td, counts)), want, "device radius")
    ti, td = torch.from_numpy(ids).cuda(), torch.from_numpy(dd).cuda()
    _eq3(_np3((ti, td, A.radius_trim(ti, td, rad, pad))), want, "numpy radius")
    ti, td = torch.from_numpy(ids).cuda(), torch.from_numpy(dd).cuda()
    _eq3(_np3((ti, td, A.radius_trim(ti, td, 0.5, pad))), trim_np(ids, dd, np.full(Q, 0.5, dtype=dt), pad), "float radius")
    # counts_dev == NULL
    lib = A._lib.load("f32" if dt == np.float32 else "f64")
    ti, td = torch.from_numpy(ids).cuda(), torch.from_numpy(dd).cuda()
    torch.cuda.synchronize()
    assert lib.annhip_radius_trim(Q, kcap, pad, tr.data_ptr(), ti.data_ptr(), td.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ti.cpu().numpy(), want[0]) and np.array_equal(_u8(td.cpu().numpy()), _u8(want[1]))
    # the NULL-pointer refusal: -1, outputs untouched
    ti, td = torch.from_numpy(ids).cuda(), torch.from_numpy(dd).cuda()
    cc = torch.full((Q,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.annhip_radius_trim(Q, kcap, pad, None, ti.data_ptr(), td.data_ptr(), cc.data_ptr(), None) == -1
    assert lib.annhip_radius_trim(Q, kcap, pad, tr.data_ptr(), None, td.data_ptr(), cc.data_ptr(), None) == -1
    assert lib.annhip_radius_trim(Q, kcap, pad, tr.data_ptr(), ti.data_ptr(), None, cc.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(ti.cpu().numpy(), ids) and np.array_equal(_u8(td.cpu().numpy()), _u8(dd)) and bool((cc == -7).all())
    with pytest.raises(ValueError):
        A.radius_trim(ti, td, rad[:-1], pad)
    with pytest.raises(ValueError):
        A.radius_trim(ti, td, rad.astype(np.float64 if dt == np.float32 else np.float32), pad)


# ------------------------------------------------------------------------------------------ 2: matches the oracle
@pytest.mark.parametrize("prec,n,d,kg,T", SHAPES)
def test_query_radius_matches_the_oracle(prec, n, d, kg, T):
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 7200 + d)
    try:
        sd = _dict(ix)
        ix.set_fixed(True)
        seen = dict(empty=0, partial=0, full_more=0)
        differ = rows = 0
        for yy, alias in _queries(orc, tp, d):
            orac = Oracle(ix, sd, tp, yy, alias)
            s1d = stage1_dists(orac, 41)
            rad = cycle_radii(s1d)
            trad = torch.from_numpy(rad).cuda()
            with np.errstate(invalid="ignore"):
                inrange1 = np.array([int((orac._scan(x, 128, orac.cand[x])[1] <= rad[x]).sum()) for x in range(24)])
            for kcap in (1, 3, kg, kg + 7, 100):
                want = radius_rows(orac, kcap, rad)
                seen["empty"] += int((want[2] == 0).sum())
                seen["partial"] += int(((want[2] > 0) & (want[2] < kcap)).sum())
                seen["full_more"] += int(((want[2] == kcap) & (inrange1 > kcap)).sum())
                got = ix.query_radius(yy, trad, k=kcap, alias=alias)
                assert tuple(got[0].shape) == (24, kcap) and got[0].dtype == torch.int64 and got[1].dtype == yy.dtype
                assert tuple(got[2].shape) == (24,) and got[2].dtype == torch.int32
                _eq3(_np3(got), want, (prec, d, alias, kcap))
                _eq3(_np3(ix.query_radius(yy, rad, k=kcap, alias=alias)), want, (prec, d, alias, kcap, "numpy radius"))
                if alias:
                    for x in range(24):
                        assert x not in want[0][x].tolist()
                plain = _np(ix.query(yy, alias=alias, k=kcap))
                trimmed = trim_np(plain[0], plain[1], rad, n)
                differ += int((trimmed[0] != want[0]).any(axis=1).sum())
                rows += 24
        print("%s d=%d: %d of %d expected radius rows differ from the trimmed query(k=kcap) row" % (prec, d, differ, rows))
        assert seen["empty"] > 0 and seen["partial"] > 0 and seen["full_more"] > 0, seen
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 3: the +inf equality
def _inf_equal(ix, yy, alias, kg, kcaps, what, pad, **kw):
    for kcap in kcaps:
        base = _np(ix.query(yy, alias=alias, k=kcap, **kw))
        got = _np3(ix.query_radius(yy, float("inf"), k=kcap, alias=alias, **kw))
        assert _same_bits(got[:2], base), (what, kcap)
        assert np.array_equal(got[2], (base[0] != pad).sum(axis=1)), (what, kcap)
        if kcap == kg:
            assert _same_bits(got[:2], _np(ix.query(yy, alias=alias, **kw))), (what, "plain call")
            assert _same_bits(_np3(ix.query_radius(yy, float("inf"), alias=alias, **kw))[:2], base), (what, "k=None")


@pytest.mark.parametrize("prec,n,d,kg,T,rows", [("f32", 5000, 64, 10, 6, "f16"), ("f64", 2500, 80, 8, 3, "f32")])
def test_an_infinite_radius_returns_the_bits_of_query_k(prec, n, d, kg, T, rows):
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 7300 + d)
    try:
        ix.set_fixed(True)
        kcaps = (kg, 1, 37)
        allow = np.random.default_rng(73).random(n) < 0.5
        tags, where = _tenants(n, 24, 74)
        for yy, alias in _queries(orc, tp, d):
            _inf_equal(ix, yy, alias, kg, kcaps, "plain", n)
            ix.set_probe(3)
            _inf_equal(ix, yy, alias, kg, kcaps, "probe 3", n)
            ix.set_probe(0)
            ix.set_filter(allow)
            _inf_equal(ix, yy, alias, kg, kcaps, "allow", n)
            ix.set_tags(tags)
            _inf_equal(ix, yy, alias, kg, kcaps, "allow+where", n, where=where)
            ix.set_filter(None)
            _inf_equal(ix, yy, alias, kg, kcaps, "where", n, where=where)
            ix.set_tags(None)
            ix.set_rows(rows)
            _inf_equal(ix, yy, alias, kg, kcaps, "narrow rows", n)
            ix.set_rows("native")
        # two workspaces on two streams with different kcap
        ta = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(300 * d).reshape(300, d))).cuda()
        tb = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(200 * d).reshape(200, d))).cuda()
        sa, sb = _np(ix.query(ta, k=21)), _np(ix.query(tb, k=2))
        torch.cuda.synchronize()
        w1, w2, s1, s2 = ix.workspace(), ix.workspace(), torch.cuda.Stream(), torch.cuda.Stream()
        ga = ix.query_radius(ta, float("inf"), k=21, ws=w1, stream=s1)
        gb = ix.query_radius(tb, float("inf"), k=2, ws=w2, stream=s2)
        s1.synchronize(), s2.synchronize()
        assert _same_bits(_np3(ga)[:2], sa) and _same_bits(_np3(gb)[:2], sb)
        assert np.array_equal(_np3(ga)[2], (sa[0] != n).sum(axis=1)) and np.array_equal(_np3(gb)[2], (sb[0] != n).sum(axis=1))
        # an exact tail of 50 rows, then 700 appended rows of which 500 are hashed
        yy, alias = _queries(orc, tp, d)[0]
        tail = _rows(prec, 700, d, 75)
        ix.append(torch.from_numpy(tail[:50]).cuda())
        _inf_equal(ix, yy, alias, kg, kcaps, "exact tail", n + 50)
        ix.append(torch.from_numpy(tail[50:500]).cuda())
        ix.hash_tail()
        ix.append(torch.from_numpy(tail[500:]).cuda())
        assert ix.tail == 700 and ix.tail_hashed == 500
        for probe in (0, 3):
            ix.set_probe(probe)
            _inf_equal(ix, yy, alias, kg, kcaps, "hashed tail", n + 700)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 4: finite radii, everything on
def test_finite_radii_with_probe_allow_list_and_tags():
    prec, n, d, kg, T = "f32", 5000, 64, 10, 6
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 7400)
    try:
        sd = _dict(ix)
        ix.set_fixed(True)
        allow = np.random.default_rng(76).random(n) < 0.3
        tags, where = _tenants(n, 24, 77)
        ix.set_probe(3), ix.set_filter(allow), ix.set_tags(tags)
        for yy, alias in _queries(orc, tp, d):
            orac = Oracle(ix, sd, tp, yy, alias, allow=allow, tags=tags, where=where)
            rad = cycle_radii(stage1_dists(orac, 41))
            for kcap in (2 * kg + 1, 2):
                want = radius_rows(orac, kcap, rad)
                _eq3(_np3(ix.query_radius(yy, rad, k=kcap, alias=alias, where=where)), want, (alias, kcap))
                for x in range(24):
                    live = want[0][x][:want[2][x]]
                    assert np.all((tags[live] & where[0][x]) == where[1][x]) and allow[live].all()
            assert (want[2] > 0).any()
    finally:
        ix.close()


@pytest.mark.parametrize("prec,rows,narrow", [("f32", "f16", np.float16), ("f64", "f32", np.float32)])
def test_finite_radii_on_narrow_rows(prec, rows, narrow):
    n, d, kg, T = 4000, 64, 7, 4
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 7500)
    try:
        yy, alias = _queries(orc, tp, d)[0]
        sd = _dict(ix)
        ix.set_fixed(True)
        ix.set_rows(rows)
        rounded = torch.from_numpy(pts.astype(narrow).astype(pts.dtype)).cuda()  # the oracle scans the rounded-and-widened rows
        orac = Oracle(ix, sd, rounded, yy, False)
        rad = cycle_radii(stage1_dists(orac, 41))
        for kcap in (2 * kg + 1, 2):
            _eq3(_np3(ix.query_radius(yy, rad, k=kcap)), radius_rows(orac, kcap, rad), (rows, kcap))
        ix.set_rows("native")
        orac = Oracle(ix, sd, tp, yy, False)
        for kcap in (2 * kg + 1, 2):
            _eq3(_np3(ix.query_radius(yy, rad, k=kcap)), radius_rows(orac, kcap, rad), ("native", kcap))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 5: the tail with finite radii
def _tail_want(orac, exp, n, kcap, rad):
    base = radius_rows(orac, kcap, rad)  # R(q): the radius row of the index before the append
    merged = _want(exp, base[:2], n, kcap, exp.knn(kcap))
    return trim_np(merged[0], merged[1], rad, n + exp.m)


def test_the_tail_with_finite_radii():
    prec, n, d, kg, T = "f32", 5000, 64, 10, 6
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 7600)
    try:
        Qn = 24
        y = _rows(prec, Qn, d, 78)
        ty = torch.from_numpy(y).cuda()
        sd = _dict(twin)
        orac = Oracle(twin, sd, tp, ty, False)
        s1d = stage1_dists(orac, 41)
        rad = cycle_radii(s1d)
        tail = _rows(prec, 50 + 400 + 300, d, 79)
        tail[0] = y[2] + np.float32(1e-3)  # inside r = candidate 2's distance and nearer than every built result
        rad[2] = s1d[2, 2]
        tail[1] = y[9] + np.float32(0.05)  # at distance exactly r (kept): r is that distance, from the query path's arithmetic
        at_r = A.exact_knn(torch.from_numpy(tail[1:2]).cuda(), ty[9:10].contiguous(), 1)[1][0, 0].item()
        rad[9] = np.float32(at_r)
        tail[2] = y[16] + np.float32(0.05)  # and a row just outside of query 16's radius
        out_r = A.exact_knn(torch.from_numpy(tail[2:3]).cuda(), ty[16:17].contiguous(), 1)[1][0, 0].item()
        rad[16] = np.nextafter(np.float32(out_r), np.float32(-np.inf))
        tail[460] = y[5] + np.float32(0.02)  # a fresh row behind the hashed ones, the nearest of query 5 (radius 1e30)
        for m, mh in ((1, 0), (50, 0), (450, 450), (750, 450)):
            if mh and not ix.tail_hashed:
                ix.append(torch.from_numpy(tail[ix.tail:mh]).cuda())
                ix.hash_tail()
            if ix.tail < m:
                ix.append(torch.from_numpy(tail[ix.tail:m]).cuda())
            assert ix.tail == m and ix.tail_hashed == mh
            ttail = torch.from_numpy(tail[:m]).cuda()
            exp = Expect(twin, ttail, ty, mh)
            for kcap in (kg, 37):
                want = _tail_want(orac, exp, n, kcap, rad)
                _eq3(_np3(ix.query_radius(ty, rad, k=kcap)), want, (m, mh, kcap))
                assert want[0][2, 0] == n and want[2][2] >= 1
                if m >= 50 and not mh:
                    assert (n + 1) in want[0][9].tolist()  # kept at exactly r (the fresh tier scans every row)
                    assert (n + 2) not in want[0][16].tolist()
            assert ((want[0] >= n) & (want[0] < n + m)).any()
        assert rad[5] == np.float32(1e30) and want[0][5, 0] == n + 460  # a fresh row behind the hashed ones
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 6: ground truth
@pytest.mark.parametrize("prec,n,d,kg,T", [("f32", 5000, 64, 10, 6), ("f64", 2500, 80, 8, 3)])
def test_exact_query_radius_is_exact_query_trimmed(prec, n, d, kg, T):
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 7700 + d)
    try:
        ix.set_fixed(True)
        allow = np.random.default_rng(80).random(n) < 0.4
        tags, where = _tenants(n, 24, 81)
        subset = 0

        def radii(yy, alias):
            ex = _np(ix.exact_query(yy, alias=alias, k=50))
            rad = np.ascontiguousarray(ex[1][np.arange(24), np.arange(24) % 50])  # the distance of exact neighbour q % 50
            rad[5], rad[6], rad[7] = np.inf, -1.0, np.nextafter(ex[1][7, 0], rad.dtype.type(-np.inf))
            return rad

        def check(yy, alias, rad, pad, what, **kw):
            nonlocal subset
            for kcap in (1, kg, 64):
                full = _np(ix.exact_query(yy, alias=alias, k=kcap, **kw))
                want = trim_np(full[0], full[1], rad, pad)
                truth = _np3(ix.exact_query_radius(yy, rad, kcap, alias=alias, **kw))
                _eq3(truth, want, (what, alias, kcap))
                got = _np3(ix.query_radius(yy, rad, k=kcap, alias=alias, **kw))
                for x in np.nonzero(want[2] < kcap)[0]:  # the truth is complete: every id returned is in its row
                    for t in range(got[2][x]):
                        at = np.nonzero(want[0][x] == got[0][x, t])[0]
                        assert len(at) == 1, (what, alias, kcap, x, got[0][x], want[0][x])
                        assert _u8(got[1][x, t:t + 1]).tobytes() == _u8(want[1][x, at[0]:at[0] + 1]).tobytes()
                        subset += 1
            assert (want[2] == 0).any() and ((want[2] > 0) & (want[2] < 64)).any(), what

        for yy, alias in _queries(orc, tp, d):
            rad = radii(yy, alias)
            check(yy, alias, rad, n, "plain")
            ix.set_filter(allow)
            check(yy, alias, rad, n, "allow")
            ix.set_filter(None)
            ix.set_tags(tags)
            check(yy, alias, rad, n, "where", where=where)
            ix.set_tags(None)
        assert subset > 0
        yy, alias = _queries(orc, tp, d)[0]
        ix.append(torch.from_numpy(_rows(prec, 60, d, 82)).cuda())
        rad = radii(yy, alias)
        check(yy, alias, rad, n + 60, "tail")
        with pytest.raises(ValueError):
            ix.exact_query_radius(yy, rad, 0)
        with pytest.raises(ValueError):
            ix.exact_query_radius(yy, rad, 1025)
        with pytest.raises(ValueError):
            ix.exact_query_radius(yy, rad[:-1], 3)
        with pytest.raises(ValueError):
            ix.exact_query_radius(yy, rad, 3, where=where)  # no tags
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_and_lifecycle():
    """Every refusal raises ValueError (the library returns -2), launches nothing -- pre-filled outputs stay as they are --
    and leaves the index as it was: the plain ix.query(y) that follows returns its old bits.  The resharded index comes
    last and is followed by no plain fixed-mode query (that path ends the process on such an index by design)."""
    n, d, kg, T, Q = 5000, 64, 10, 6, 120
    orc, pts, tp, ix = _build("f32", n, d, kg, T, 7800)
    try:
        y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
        ty = torch.from_numpy(y).cuda()
        sd = _dict(ix)
        want = orc.query(sd, pts, y)
        lib = ix.lib
        ids = torch.full((Q, 4), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((Q, 4), -7.0, dtype=torch.float32, device="cuda")
        cc = torch.full((Q,), -7, dtype=torch.int32, device="cuda")
        rad = torch.full((Q,), 50.0, dtype=torch.float32, device="cuda")
        tags, where = _tenants(n, Q, 83)
        qm = torch.from_numpy(where[0].view(np.int32)).cuda()
        qv = torch.from_numpy(where[1].view(np.int32)).cuda()
        torch.cuda.synchronize()

        def raw(kcap=4, radius=rad, m=None, v=None, out=ids):
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            return lib.annhip_query_radius(ix.h, None, None, Q, ty.data_ptr(), 0, kcap, p(radius), p(m), p(v), p(out),
                                           dd.data_ptr(), cc.data_ptr())

        def untouched(what):
            torch.cuda.synchronize()
            assert bool((ids == -7).all()) and bool((dd == -7.0).all()) and bool((cc == -7).all()), what

        def refused(**kw):
            with pytest.raises(ValueError):
                ix.query_radius(ty, kw.pop("radius", rad), **kw)

        parity = _np(ix.query(ty))
        assert raw() == -2  # fixed mode is off
        untouched("fixed mode off")
        refused(k=4)
        assert _same_bits(_np(ix.query(ty)), parity)
        ix.set_fixed(True)
        plain = _np(ix.query(ty))
        kmax = ix.max_query_k
        for kw in (dict(k=0), dict(k=True), dict(k=2.5), dict(k=kmax + 1), dict(k=4, where=where),  # ..., where= without tags
                   dict(k=4, radius=rad.double()), dict(k=4, radius=rad[:-1]), dict(k=4, radius=None),
                   dict(k=4, radius=np.full(Q, 50.0)), dict(k=4, radius=np.full(Q + 1, 50.0, dtype=np.float32))):
            refused(**kw)
            assert _same_bits(_np(ix.query(ty)), plain), kw
        assert raw(kcap=0) == -2 and raw(kcap=kmax + 1) == -2 and raw(radius=None) == -2 and raw(out=None) == -2
        assert raw(m=qm, v=qv) == -2  # a tagged call on an index without tags
        untouched("k, NULL arrays, no tags")
        ix.set_tags(tags)
        assert raw(m=qm) == -2 and raw(v=qv) == -2  # exactly one of the two predicate arrays
        untouched("one predicate array")
        assert lib.annhip_query_radius(ix.h, None, None, 0, ty.data_ptr(), 0, 4, rad.data_ptr(), None, None, ids.data_ptr(),
                                       dd.data_ptr(), cc.data_ptr()) == 0  # ycnt == 0
        untouched("ycnt == 0")
        assert raw(m=qm, v=qv) == 0  # and an accepted call writes all three
        torch.cuda.synchronize()
        assert bool((ids >= 0).all()) and bool((cc >= 0).all()) and bool((dd >= 0).all())
        ix.set_tags(None)
        assert _same_bits(_np(ix.query(ty)), plain)
        # the switch goes back: parity mode again, bit for bit the reference's answer
        ix.set_fixed(False)
        ids0, dd0, _ = ix.query(ty)
        assert np.array_equal(ids0.cpu().numpy().astype(np.uint64), want[0])
        assert np.array_equal(dd0.cpu().numpy().view(np.uint8), want[1].view(np.uint8))
        # a resharded index is refused, not aborted on
        ix.set_fixed(True)
        ids.fill_(-7), dd.fill_(-7.0), cc.fill_(-7)
        ix.reshard(tp[: n // 2].contiguous(), 0, n // 2)
        assert raw() == -2
        untouched("resharded")
        refused(k=4)
        with pytest.raises(ValueError):
            ix.exact_query_radius(ty, rad, 4)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 8, 9: the largest kcap; Q = 0
def test_the_largest_kcap_and_an_empty_batch():
    prec, n, d, kg, T = "f32", 2000, 32, 10, 2
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 7900)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(4 * d).reshape(4, d))).cuda()
        ix.set_fixed(True)
        kmax = ix.max_query_k
        base = _np(ix.query(ty, k=kmax))
        got = _np3(ix.query_radius(ty, float("inf"), k=kmax))
        assert _same_bits(got[:2], base) and np.array_equal(got[2], (base[0] != n).sum(axis=1))
        rad = np.ascontiguousarray(base[1][:, 5])
        _eq3(_np3(ix.query_radius(ty, rad, k=kmax)), radius_rows(Oracle(ix, _dict(ix), tp, ty, False), kmax, rad), "kmax, finite")
        empty = ix.query_radius(ty[:0].contiguous(), 1.0, k=3)
        assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0, 3) and tuple(empty[2].shape) == (0,)
        e2 = ix.exact_query_radius(ty[:0].contiguous(), 1.0, 3)
        assert tuple(e2[0].shape) == (0, 3) and tuple(e2[2].shape) == (0,)
    finally:
        ix.close()
