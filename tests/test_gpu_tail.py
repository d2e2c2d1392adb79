"""GPU: rows appended to a built index -- the tail that every fixed-mode query scans exactly (annhip_index_append and its
companions; include/ann_hip.h, ann_tail_kernels.h).

Every check is bit-exact on ids and distance bytes; no tolerance.  The references never run the new kernel:
  - queries: a TWIN index built from the same rows and the same random() seed (hence the same tables and graph) gives R(q);
    the expected row is the CPU lexsort merge, by (distance bits, id), of R(q) without its pads and
    A.exact_knn(tail, y, min(k, m), allow=..., tags=..., where=...) with ids shifted by n, padded with (n_total, +inf).
    A.exact_knn has the query path's distance arithmetic bit for bit (tests/test_gpu_exact_knn.py).
  - exact_query: A.exact_knn over torch.cat([points, tail]).
Tail lengths sit around the LDS tile of the scan, which _tile_rows computes from d, the precision and k by the host's
formula (exact_shape in ann_host.hip): 192 rows at d = 32 f32 with 12 waves.  Helpers and shapes: tests/test_gpu_query_k.py."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd import _lib
from tests.test_gpu_query_k import _np, _same_bits, _tenants

pytestmark = pytest.mark.gpu

# power of two, static lane groups, folded, any-d, kg >= 32 (one shape per kernel family); then a generic layout
# (tail_merge_generic_kernel) and one with 8 chunks per lane (8 waves, no prefetch: the ex_fill_tile branch of the tile loop)
SHAPES = [("f32", 5000, 64, 10, 6), ("f64", 2500, 80, 8, 3), ("f32", 3000, 100, 10, 3), ("f32", 2000, 33, 6, 2),
          ("f64", 2000, 16, 33, 2), ("f64", 1500, 300, 5, 2), ("f32", 2000, 384, 6, 2)]
Q = 37  # the last query group of a wave (4 queries) and of a workgroup is ragged


def _tile_rows(prec, d, k, filtered=0):
    """Rows of the scan's LDS tile: exact_shape (ann_host.hip) restated.  filtered: 0 none, 1 allow list, 2 tags."""
    fb, key = (4, 8) if prec == "f32" else (8, 16)
    vec, row = 16 // fb, d * fb
    code = _lib.load(prec).annhip_layout_code(d)
    generic = code in (0, -246, -247)
    if generic:
        max_w, pf = 4, False
    elif code > 0:
        max_w, pf = 12, True  # RowLay: at most 4 chunks per lane
    else:
        ua = code in (-241, -243, -244, -245)
        c = 1 if ua else (-code) % 16
        max_w, pf = (12 if c <= 4 else 8), (not ua and c <= 4)
    cap = k + 64
    npairs = min(max(1024 // d, 1), 64)
    wave = key * (4 * cap + k) + ((((1 + npairs) * row + 15) & ~15) if generic else 0)

    def tile(w, p):
        return max(1, (2 * 64 * w * 16 if p else 16384) // row)

    def smem(w, p):
        t = tile(w, p)
        return ((t * row + 15) & ~15) + w * wave + (4 * t if filtered == 2 else 0) + (4 * (t // 32 + 2) if filtered else 0)

    w = max_w
    while w > 1 and smem(w, pf) > 150 * 1024:
        w -= 1
    if pf and row > 2 * 64 * w * 16:
        pf = False
    if pf and filtered == 2 and tile(w, True) > 64 * w:
        pf = False
    return tile(w, pf)


def _rows(prec, count, d, seed):
    dt = np.float32 if prec == "f32" else np.float64
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((count, d)).astype(dt))


def _twins(prec, n, d, k, T, seed):
    """Two indexes with the same rows, tables and graph, both in fixed mode.  Nothing may draw from libc random() between
    the seed and the build's own draws (loading a library, the first copy to the device and the runtime's initialisation
    all may), so the rows are on the device and the library is loaded before the seed is set."""
    from oracle import oracle_py as O
    pts = _rows(prec, n, d, seed)
    tp = torch.from_numpy(pts).cuda()
    _lib.load(prec)
    torch.cuda.synchronize()
    built = []
    for _ in range(2):
        O.srandom(seed + 1)
        built.append(A.Index.precomp(tp, k, T))
    ix, twin = built
    assert ix.checksum() == twin.checksum()  # the same tables and graph
    ix.set_fixed(True), twin.set_fixed(True)
    return pts, tp, ix, twin


def _bits(d):
    return d.view(np.uint32 if d.dtype == np.float32 else np.uint64)


def _merge(base, tail_knn, n, m, k):
    """The contract: the k smallest (distance bits, id) of base (pads dropped) and the tail's exact neighbours (ids + n)."""
    Qn = base[0].shape[0]
    ids = np.full((Qn, k), n + m, dtype=np.int64)
    dd = np.full((Qn, k), np.inf, dtype=base[1].dtype)
    for q in range(Qn):
        kb, kt = base[0][q] < n, tail_knn[0][q] < m
        i = np.concatenate([base[0][q][kb], tail_knn[0][q][kt] + n])
        d = np.concatenate([base[1][q][kb], tail_knn[1][q][kt]])
        o = np.lexsort((i, _bits(d)))[:k]
        ids[q, :len(o)], dd[q, :len(o)] = i[o], d[o]
    return ids, dd


def _tail_knn(ttail, ty, k, allow=None, tags=None, where=None):
    m = ttail.shape[0]
    return _np(A.exact_knn(ttail, ty, min(k, m), allow=None if allow is None else torch.from_numpy(allow).cuda(),
                           tags=tags, where=where))


def _check(ix, twin, ttail, ty, n, alias=False, k=None, allow=None, tags=None, where=None, what=None):
    """ix (with the tail) against the merge of twin's row and the tail's exact neighbours.  allow / tags: [n_total]."""
    m = ttail.shape[0]
    kw = dict(alias=alias)
    if k is not None:
        kw["k"] = k
    if where is not None:
        kw["where"] = where
    got = _np(ix.query(ty, **kw))
    base = _np(twin.query(ty, **kw))
    kk = got[0].shape[1]
    want = _merge(base, _tail_knn(ttail, ty, kk, None if allow is None else allow[n:], None if tags is None else tags[n:],
                                  where if tags is not None else None), n, m, kk)
    assert np.array_equal(got[0], want[0]), (what, k, alias)
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, k, alias)
    return got


# ------------------------------------------------------------------------------------------ 1: query results
@pytest.mark.parametrize("prec,n,d,kg,T", SHAPES)
def test_queries_merge_the_tail(prec, n, d, kg, T):
    m = 700
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9100 + d)
    try:
        tail = _rows(prec, m, d, 91)
        tail[5] = pts[7]  # a duplicate of a built row
        ttail = torch.from_numpy(tail).cuda()
        ty = torch.from_numpy(_rows(prec, Q, d, 92)).cuda()
        ta = tp[:Q].contiguous()
        assert ix.append(ttail) == n and ix.tail == m and ix.n_total == n + m and ix.n == n
        allow = np.random.default_rng(93).random(n + m) < 0.4
        tags, where = _tenants(n + m, Q, 94)
        for probe in (0, 3):
            ix.set_probe(probe), twin.set_probe(probe)
            for yy, alias in ((ty, False), (ta, True)):
                for k in (None, 1, kg, 256):
                    _check(ix, twin, ttail, yy, n, alias, k, what="plain")
                ix.set_filter(allow), twin.set_filter(allow[:n])
                assert ix.filter_count == int(allow.sum())
                for k in (None, 1, 256):
                    got = _check(ix, twin, ttail, yy, n, alias, k, allow=allow, what="allow")
                    assert allow[got[0][got[0] < n + m]].all()
                ix.set_tags(tags), twin.set_tags(tags[:n])
                for k in (None, 256):
                    _check(ix, twin, ttail, yy, n, alias, k, allow=allow, tags=tags, where=where, what="allow+where")
                ix.set_filter(None), twin.set_filter(None)
                for k in (None, 1, kg, 256):
                    _check(ix, twin, ttail, yy, n, alias, k, tags=tags, where=where, what="where")
                ix.set_tags(None), twin.set_tags(None)
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 2: exact results
@pytest.mark.parametrize("prec,n,d,kg,T", SHAPES)
def test_exact_query_covers_the_tail(prec, n, d, kg, T):
    m = 700
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9200 + d)
    try:
        ttail = torch.from_numpy(_rows(prec, m, d, 95)).cuda()
        ty = torch.from_numpy(_rows(prec, Q, d, 96)).cuda()
        ta = tp[:Q].contiguous()
        ix.append(ttail)
        both = torch.cat([tp, ttail]).contiguous()
        allow = np.random.default_rng(97).random(n + m) < 0.4
        tallow = torch.from_numpy(allow).cuda()
        tags, where = _tenants(n + m, Q, 98)
        for yy, alias in ((ty, False), (ta, True)):
            for k in (None, 1, kg, 256):
                kk = kg if k is None else k
                assert _same_bits(_np(ix.exact_query(yy, alias=alias, k=k)), _np(A.exact_knn(both, yy, kk, self_exclude=alias)))
            ix.set_filter(allow)
            for k in (None, 256):
                kk = kg if k is None else k
                assert _same_bits(_np(ix.exact_query(yy, alias=alias, k=k)),
                                  _np(A.exact_knn(both, yy, kk, self_exclude=alias, allow=tallow)))
            ix.set_tags(tags)
            for k in (None, 256):
                kk = kg if k is None else k
                assert _same_bits(_np(ix.exact_query(yy, alias=alias, where=where, k=k)),
                                  _np(A.exact_knn(both, yy, kk, self_exclude=alias, allow=tallow, tags=tags, where=where)))
            ix.set_filter(None)
            assert _same_bits(_np(ix.exact_query(yy, alias=alias, where=where)),
                              _np(A.exact_knn(both, yy, kg, self_exclude=alias, tags=tags, where=where)))
            ix.set_tags(None)
        with pytest.raises(ValueError):
            ix.exact_query(ty, k=1025)
    finally:
        ix.close(), twin.close()


@pytest.mark.parametrize("prec,d", [("f32", 32), ("f64", 300)])  # 300: the generic kernel's seeding with fewer than k rows
def test_exact_query_k_beyond_the_built_rows(prec, d):
    """k > n - alias was refused; with a tail the limit is n_total - alias, and the built rows fill only part of a row."""
    n, m = 40, 30
    pts, tp, ix, twin = _twins(prec, n, d, 5, 1, 9250)
    try:
        ttail = torch.from_numpy(_rows(prec, m, d, 99)).cuda()
        ix.append(ttail)
        both = torch.cat([tp, ttail]).contiguous()
        ta = both[:16].contiguous()
        assert _same_bits(_np(ix.exact_query(ta, k=n + m)), _np(A.exact_knn(both, ta, n + m)))
        assert _same_bits(_np(ix.exact_query(ta, alias=True, k=n + m - 1)), _np(A.exact_knn(both, ta, n + m - 1, self_exclude=True)))
        assert _same_bits(_np(ix.exact_query(ta, alias=True, k=n)), _np(A.exact_knn(both, ta, n, self_exclude=True)))
        with pytest.raises(ValueError):
            ix.exact_query(ta, alias=True, k=n + m)
        with pytest.raises(ValueError):
            ix.exact_query(ta, k=n + m + 1)
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 3: tail lengths
@pytest.mark.parametrize("prec,n,d,kg,T", SHAPES)
def test_tail_lengths_around_the_tile(prec, n, d, kg, T):
    assert _tile_rows("f32", 32, 10) == 192  # the documented case of the formula
    tile = _tile_rows(prec, d, kg)
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9300 + d)
    try:
        full = _rows(prec, max(1500, tile + 1), d, 100)
        ty = torch.from_numpy(_rows(prec, Q, d, 101)).cuda()
        print("%s d %d k %d: tile %d rows" % (prec, d, kg, tile))
        for m in (1, tile - 1, tile, tile + 1, 1500):
            ttail = torch.from_numpy(full[:m]).cuda()
            ix.drop_tail()
            ix.append(ttail)
            assert ix.tail == m
            _check(ix, twin, ttail, ty, n, what=m)
            both = torch.cat([tp, ttail]).contiguous()
            assert _same_bits(_np(ix.exact_query(ty)), _np(A.exact_knn(both, ty, kg))), m
        allow = np.random.default_rng(102).random(n + 1500) < 0.5  # the filtered and tagged forms across several tiles
        tags, where = _tenants(n + 1500, Q, 103)
        ix.set_filter(allow), twin.set_filter(allow[:n])
        _check(ix, twin, ttail, ty, n, allow=allow, what="allow")
        ix.set_tags(tags), twin.set_tags(tags[:n])
        _check(ix, twin, ttail, ty, n, allow=allow, tags=tags, where=where, what="allow+where")
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 4: appending in pieces
def test_appending_in_pieces_equals_one_append():
    prec, n, d, kg, T = "f32", 5000, 64, 10, 6
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9400)
    try:
        tail = _rows(prec, 1500, d, 104)
        ttail = torch.from_numpy(tail).cuda()
        ty = torch.from_numpy(_rows(prec, Q, d, 105)).cuda()
        tags, where = _tenants(n + 1500, Q, 106)
        ix.set_tags(tags[:n]), twin.set_tags(tags[:n])
        allow = np.random.default_rng(107).random(n) < 0.5
        ix.set_filter(allow), twin.set_filter(allow)
        # three calls, each beyond twice the capacity before it: two reallocations after the first allocation
        assert ix.append(tail[:10], tags=tags[n:n + 10]) == n                      # numpy rows, numpy tags
        assert ix.append(ttail[10:510], tags=tags[n + 10:n + 510]) == n + 10       # device rows
        assert ix.append(tail[510:], tags=torch.from_numpy(tags[n + 510:].view(np.int32)).cuda()) == n + 510
        assert ix.tail == 1500 and ix.filter_count == int(allow.sum()) + 1500
        twin.reserve_tail(1500)
        twin.append(ttail, tags=tags[n:])
        for kw in (dict(), dict(k=64), dict(where=where), dict(alias=True)):
            assert _same_bits(_np(ix.query(ty, **kw)), _np(twin.query(ty, **kw))), kw
        assert torch.equal(ix.rows_tensor(0, n + 1500), torch.cat([tp, ttail]))
        assert torch.equal(ix.rows_tensor(n - 3, n + 7), torch.cat([tp[n - 3:], ttail[:7]]))
        with pytest.raises(ValueError):
            ix.rows_tensor(0, n + 1501)
        twin.drop_tail()  # and the one-append twin is itself right
        full_allow = np.concatenate([allow, np.ones(1500, dtype=bool)])
        _check(ix, twin, ttail, ty, n, allow=full_allow, what="pieces")
        _check(ix, twin, ttail, ty, n, allow=full_allow, tags=tags, where=where, what="pieces where")
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 5: edge cases
def test_edge_cases():
    prec, n, d, kg, T = "f32", 3000, 64, 10, 4
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9500)
    try:
        m = 300
        tail = _rows(prec, m, d, 108)
        y = _rows(prec, Q, d, 109)
        tail[17] = y[3]      # a tail row equal to a query
        tail[40] = pts[11]   # a tail row that duplicates a built row ...
        y[5] = pts[11]       # ... which a query sits on
        ttail, ty = torch.from_numpy(tail).cuda(), torch.from_numpy(y).cuda()
        ix.append(ttail)
        got = _check(ix, twin, ttail, ty, n, what="edge")
        assert got[0][3, 0] == n + 17 and got[1][3, 0] == 0
        assert got[0][5, 0] == 11 and got[0][5, 1] == n + 40 and got[1][5, 0] == 0 and got[1][5, 1] == 0
        # an allow list that leaves fewer than k rows in total: pads carry n_total
        allow = np.zeros(n + m, dtype=bool)
        allow[[11, 12, n + 17, n + 40]] = True
        ix.set_filter(allow), twin.set_filter(allow[:n])
        got = _check(ix, twin, ttail, ty, n, allow=allow, what="few")
        assert np.all(got[0][:, 4:] == n + m) and np.all(np.isinf(got[1][:, 4:]))
        for x in range(Q):  # the tail is scanned exactly: both allowed tail rows are in every row; built rows 11 and 12
            real = got[0][x][got[0][x] < n + m].tolist()  # only where the index's buckets offer them to the query
            assert set(real) <= {11, 12, n + 17, n + 40} and {n + 17, n + 40} <= set(real), (x, real)
        assert got[0][5, 0] == 11 and got[0][5, 1] == n + 40  # the query that sits on row 11 finds it, then its copy
        ix.set_filter(None), twin.set_filter(None)
        # an aliased batch of all n_total rows: query n + j leaves out tail row j (and query q < n built row q)
        allrows = ix.rows_tensor(0, n + m)
        gi, gd = _np(ix.query(allrows, alias=True))
        assert not np.any(gi == np.arange(n + m)[:, None])
        ei, ed = _np(ix.exact_query(allrows, alias=True))
        both = torch.cat([tp, ttail]).contiguous()
        assert _same_bits((ei, ed), _np(A.exact_knn(both, both, kg, self_exclude=True)))
        # query n + 40 is a copy of built row 11: it finds row 11 at distance 0, never itself
        assert gi[n + 40, 0] == 11 and gd[n + 40, 0] == 0
        base = _np(twin.query(allrows, alias=True))  # the twin excludes q < n only; the tail part of the reference excludes j
        tk = _np(A.exact_knn(ttail, allrows[n:], kg, self_exclude=True))
        want_tail_q = _merge((base[0][n:], base[1][n:]), tk, n, m, kg)
        assert np.array_equal(gi[n:], want_tail_q[0]) and np.array_equal(_bits(gd[n:]), _bits(want_tail_q[1]))
        want_built_q = _merge((base[0][:n], base[1][:n]), _tail_knn(ttail, allrows[:n], kg), n, m, kg)
        assert np.array_equal(gi[:n], want_built_q[0]) and np.array_equal(_bits(gd[:n]), _bits(want_built_q[1]))
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 6: tail-empty paths
def test_tail_empty_paths_and_filter_lengths():
    prec, n, d, kg, T = "f32", 5000, 64, 10, 6
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9600)
    try:
        m = 200
        ttail = torch.from_numpy(_rows(prec, m, d, 110)).cuda()
        ty = torch.from_numpy(_rows(prec, Q, d, 111)).cuda()
        tags, where = _tenants(n + m, Q, 112)
        allow = np.random.default_rng(113).random(n + m) < 0.5

        def same_as_twin():
            a, b = ix, twin
            for kw in (dict(), dict(k=3), dict(k=64), dict(alias=True)):
                assert _same_bits(_np(a.query(ty, **kw)), _np(b.query(ty, **kw))), kw
            assert _same_bits(_np(a.exact_query(ty)), _np(b.exact_query(ty)))
            a.set_filter(allow[:n]), b.set_filter(allow[:n])
            a.set_tags(tags[:n]), b.set_tags(tags[:n])
            assert a.filter_count == b.filter_count == int(allow[:n].sum())
            assert _same_bits(_np(a.query(ty, where=where)), _np(b.query(ty, where=where)))
            assert _same_bits(_np(a.exact_query(ty, where=where, k=20)), _np(b.exact_query(ty, where=where, k=20)))
            a.set_filter(None), b.set_filter(None), a.set_tags(None), b.set_tags(None)

        assert ix.tail == 0 and ix.n_total == n
        same_as_twin()                      # m = 0
        ix.append(ttail[:0])                # count == 0 does nothing
        assert ix.tail == 0
        ix.reserve_tail(m)
        same_as_twin()                      # a reserved but empty tail
        # rows appended after set_filter are allowed and found; clearing their bits removes them
        ix.set_filter(allow[:n]), twin.set_filter(allow[:n])
        ix.append(ttail)
        assert ix.filter_count == int(allow[:n].sum()) + m
        ones = np.concatenate([allow[:n], np.ones(m, dtype=bool)])
        got = _check(ix, twin, ttail, ty, n, allow=ones, what="appended after set_filter")
        with pytest.raises(ValueError):     # the lengths follow n_total
            ix.set_filter(allow[:n])
        with pytest.raises(ValueError):
            ix.set_tags(tags[:n])
        cleared = ones.copy()
        cleared[n:] = False
        ix.set_filter(cleared)
        assert ix.filter_count == int(allow[:n].sum())
        gi, gd = _np(ix.query(ty))
        bi, bd = _np(twin.query(ty))
        assert not np.any((gi >= n) & (gi < n + m))
        assert np.array_equal(np.where(gi >= n, n, gi), bi) and np.array_equal(_bits(gd), _bits(bd))  # only the pad id differs
        ix.set_filter(allow), ix.set_tags(tags)
        assert ix.filter_count == int(allow.sum())
        ix.set_filter(None), twin.set_filter(None), ix.set_tags(None)
        ix.drop_tail()
        assert ix.tail == 0 and ix.n_total == n
        same_as_twin()                      # after drop_tail
        # set_fixed(False) keeps the tail stored; parity-mode queries never see it
        ix.append(ttail)
        ix.set_fixed(False), twin.set_fixed(False)
        assert ix.tail == m
        assert _same_bits(_np(ix.query(ty)), _np(twin.query(ty)))
        ix.set_fixed(True), twin.set_fixed(True)
        _check(ix, twin, ttail, ty, n, what="fixed again")
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_leave_everything_as_it_was():
    prec, n, d, kg, T = "f32", 3000, 64, 10, 4
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9700)
    try:
        m = 100
        tail = _rows(prec, m, d, 114)
        ttail = torch.from_numpy(tail).cuda()
        ty = torch.from_numpy(_rows(prec, Q, d, 115)).cuda()
        tags, _ = _tenants(n + 2 * m, Q, 116)
        ix.append(ttail)
        before = _np(ix.query(ty))

        def refused(rows, tags=None, call=None):
            with pytest.raises(ValueError):
                (call or ix.append)(rows, **({} if tags is None else dict(tags=tags)))
            assert ix.tail == m and _same_bits(_np(ix.query(ty)), before)

        refused(tail[:, :d - 1])                                 # wrong shape
        refused(tail.astype(np.float64))                         # wrong dtype
        refused(tail, tags=tags[:m])                             # tags given, the index has none
        ix.set_tags(tags[:n + m])
        refused(tail)                                            # the index has tags, none given
        refused(tail, tags=tags[:m - 1])                         # wrong tag length
        ix.set_tags(None)
        ix.set_fixed(False)                                      # fixed mode off
        with pytest.raises(ValueError):
            ix.append(tail)
        with pytest.raises(ValueError):
            ix.reserve_tail(10 * m)
        ix.set_fixed(True)
        assert ix.tail == m and _same_bits(_np(ix.query(ty)), before)
        with pytest.raises(ValueError):                          # ids must fit 32 bits
            ix.reserve_tail(0xFFFFFFF0)
        assert ix.tail == m and _same_bits(_np(ix.query(ty)), before)
        # narrow rows and a tail do not compose, in either order
        with pytest.raises(ValueError):
            ix.set_rows("f16")
        assert ix.rows == "native" and _same_bits(_np(ix.query(ty)), before)
        ix.drop_tail()
        ix.set_rows("f16")
        assert ix.rows == "f16"
        with pytest.raises(ValueError):
            ix.append(tail)
        assert ix.tail == 0
        ix.set_rows("native")
        ix.append(ttail)
        assert _same_bits(_np(ix.query(ty)), before)
        # a resharded index: reshard drops the tail, and appends are refused
        ix.reshard(tp[: n // 2].contiguous(), 0, n // 2)
        assert ix.tail == 0
        with pytest.raises(ValueError):
            ix.append(tail)
        with pytest.raises(ValueError):
            ix.rows_tensor(0, 10)
        assert ix.tail == 0
    finally:
        ix.close(), twin.close()


def test_f64_index_refuses_its_narrow_rows_while_a_tail_exists():
    prec, n, d, kg, T = "f64", 2000, 16, 33, 2
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9750)
    try:
        ix.append(_rows(prec, 50, d, 117))
        with pytest.raises(ValueError):
            ix.set_rows("f32")
        ix.drop_tail()
        ix.set_rows("f32")
        assert ix.rows == "f32"
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 8: workspaces and streams
def test_workspaces_streams_and_the_host_stream():
    prec, n, d, kg, T = "f32", 5000, 64, 10, 6
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9800)
    try:
        ttail = torch.from_numpy(_rows(prec, 700, d, 118)).cuda()
        ya, yb = _rows(prec, 300, d, 119), _rows(prec, 150, d, 120)
        ta, tb = torch.from_numpy(ya).cuda(), torch.from_numpy(yb).cuda()
        ix.append(ttail)
        serial_a, serial_b = _np(ix.query(ta)), _np(ix.query(tb, k=21))
        assert np.any(serial_a[0] >= n)
        torch.cuda.synchronize()
        w1, w2, s1, s2 = ix.workspace(), ix.workspace(), torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            ga = ix.query(ta, ws=w1, stream=s1)
        with torch.cuda.stream(s2):
            gb = ix.query(tb, ws=w2, stream=s2, k=21)
        s1.synchronize(), s2.synchronize()
        assert _same_bits(_np(ga), serial_a) and _same_bits(_np(gb), serial_b)
        hs = ix.host_stream(300, lanes=2)
        try:
            out = list(hs.map([ya, yb]))
        finally:
            hs.close()
        assert np.array_equal(np.asarray(out[0][0]).astype(np.int64), serial_a[0])
        assert np.array_equal(_bits(np.asarray(out[0][1])), _bits(serial_a[1]))
        assert np.array_equal(np.asarray(out[1][0]).astype(np.int64), _np(ix.query(tb))[0])
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 9: compaction
def test_compact_carries_rows_settings_and_ids_over():
    prec, n, d, kg, T = "f32", 3000, 64, 10, 4
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9900)
    new = None
    try:
        m = 400
        ttail = torch.from_numpy(_rows(prec, m, d, 121)).cuda()
        ty = torch.from_numpy(_rows(prec, Q, d, 122)).cuda()
        tags, where = _tenants(n + m, Q, 123)
        allow = np.random.default_rng(124).random(n + m) < 0.5
        ix.append(ttail)
        ix.set_probe(3), ix.set_filter(allow), ix.set_tags(tags)
        from oracle import oracle_py as O
        O.srandom(77)
        new = ix.compact(tries=T)
        assert new.n == n + m and new.tail == 0 and new.n_total == n + m and new.k == kg and ix.tail == m
        assert new.probe == 3 and new.filter_count == int(allow.sum()) and new.has_tags
        assert torch.equal(new.rows_tensor(0, n + m), torch.cat([tp, ttail]))
        for kw in (dict(), dict(where=where), dict(where=where, k=40), dict(alias=True)):
            assert _same_bits(_np(new.exact_query(ty, **kw)), _np(ix.exact_query(ty, **kw))), kw
        got = _np(new.query(ty, where=where))  # fixed mode came along: a tagged query is accepted
        live = got[0] < n + m
        assert allow[got[0][live]].all()
    finally:
        ix.close(), twin.close()
        if new is not None:
            new.close()


# ------------------------------------------------------------------------------------------ 10: recall
def test_appended_rows_are_found():
    """300 queries = appended rows plus 1 % noise: the exact scan of the tail must return the source row first.  A condition
    that follows from the exact scan, not a measurement.  The twin without the tail cannot return those ids at all."""
    prec, n, d, kg, T = "f32", 20000, 32, 10, 10
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9950)
    try:
        m, nq = 2000, 300
        tail = _rows(prec, m, d, 125)
        src = np.random.default_rng(126).choice(m, size=nq, replace=False)
        y = (tail[src] + 0.01 * _rows(prec, nq, d, 127)).astype(np.float32)
        ttail, ty = torch.from_numpy(tail).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda()
        ix.append(ttail)
        gi, _, _ = ix.query(ty)
        ei, _ = ix.exact_query(ty)
        assert np.array_equal(ei[:, 0].cpu().numpy(), n + src)
        assert A.recall_at_k(gi[:, :1], ei[:, :1]) == 1.0
        ix.stats(reset=True)
        ix.profile(True)
        ix.query(ty)
        assert ix.stats()["other_rows"] >= nq * m  # the (query, tail row) pairs are counted while profiling
        ix.profile(False)
        ti, _, _ = twin.query(ty)
        assert not bool((ti >= n).logical_and(ti < n + m).any()) and A.recall_at_k(ti[:, :1], ei[:, :1]) == 0.0
    finally:
        ix.close(), twin.close()
