"""GPU: appended rows looked up by hash code (annhip_index_hash_tail; include/ann_hip.h, ann_tail_hash_kernels.h).

Every check is bit-exact on ids and distance bytes; no tolerance.  No expectation runs the new kernel:
  - a TWIN index built from the same rows and seed (tests/test_gpu_tail.py::_twins) gives R(q);
  - the library's hash kernels give the codes of the queries and of the tail rows (HipEngine.sh_codes on each), and
    Index.probe_bits the ranked bits;
  - numpy evaluates the contract's hit test, ORs in the fresh rows [mh, m) and ANDs the validity rules;
  - A.exact_knn(tail, y[x:x+1], k, allow=mask) -- the query path's distance bits (tests/test_gpu_exact_knn.py) -- with
    ids + n, lexsort-merged with R(q) without its pads, is the expected row.
Preconditions on the expectation (_nonvacuous) keep a case from passing vacuously.  Shapes: tests/test_gpu_tail.py."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd.sharded import HipEngine
from tests.test_gpu_query_k import _codes_of, _np, _ranked, _same_bits, _tenants
from tests.test_gpu_tail import SHAPES, Q, _bits, _merge, _rows, _twins

pytestmark = pytest.mark.gpu

M = 1500
RPW = 8  # rows per wave pass at d = 64 f32 (RowLay: 16 chunks, 8 lanes per row)


def _popcount(x):
    c = np.zeros(x.shape, dtype=np.int64)
    for i in range(32):
        c += (x >> i) & 1
    return c


def hit_matrix(cq, ct, ranked, ds):
    """The contract's hit test: [Q, m, T] bool from the queries' codes [Q, T], the tail rows' [m, T] and the ranked bits."""
    pm = np.zeros(cq.shape, dtype=np.int64)
    for u in range(ranked.shape[2]):
        pm |= np.int64(1) << (ds - 1 - ranked[:, :, u].astype(np.int64))
    x = cq[:, None, :] ^ ct[None, :, :]
    pc = _popcount(x)
    return (pc <= 1) | ((pc == 2) & ((x & ~pm[:, None, :]) == 0))


class Expect:
    """The tail side of the contract for one batch and one probe setting.  ref: an index with the same tables and the same
    probe setting as the one under test (the twin, or the index itself: only its hash kernels run)."""

    def __init__(self, ref, ttail, ty, mh):
        T, m = ref.tries, ttail.shape[0]
        eng = HipEngine(ref)
        self.ttail, self.ty, self.m, self.mh = ttail, ty, m, mh
        self.hit = hit_matrix(_codes_of(eng, ty, T), _codes_of(eng, ttail, T), _ranked(ref, ty), ref.d_short)
        self.cand = self.hit.any(axis=2)
        self.cand[:, mh:] = True  # the fresh rows are scanned exactly

    def knn(self, kmax, valid=None):
        """Per query the kmax nearest tail candidates (ids < m, pads (m, +inf)) -- slice [:, :k] for a smaller k."""
        mask = self.cand if valid is None else self.cand & valid
        kk = min(kmax, self.m)
        tm = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
        out = [_np(A.exact_knn(self.ttail, self.ty[x:x + 1], kk, allow=tm[x].contiguous())) for x in range(self.ty.shape[0])]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _valid(Qn, m, n, allow=None, tags=None, where=None):
    v = np.ones((Qn, m), dtype=bool)
    if allow is not None:
        v &= allow[None, n:]
    if tags is not None:
        v &= (tags[None, n:] & where[0][:, None]) == where[1][:, None]
    return v


def _want(exp, base, n, k, knn):
    return _merge(base, (knn[0][:, :k], knn[1][:, :k]), n, exp.m, k)


def _nonvacuous(exp, want, n, base):
    """Some hashed rows hit and some do not for most queries; a nearer tail row is not a candidate somewhere; a hashed id is
    expected somewhere; a tail row hits in two tries."""
    Qn, mh = exp.cand.shape[0], exp.mh
    c = exp.hit.any(axis=2)[:, :mh]
    mixed = int((c.any(axis=1) & (~c).any(axis=1)).sum())
    assert 2 * mixed > Qn, ("too few queries with hits and misses", mixed)
    k = want[0].shape[1]
    full = _np(A.exact_knn(exp.ttail, exp.ty, min(k, exp.m)))
    exact_row = _merge(base, full, n, exp.m, k)
    assert (exact_row[0] != want[0]).any(), "no expected row differs from the exact-tail row"
    assert ((want[0] >= n) & (want[0] < n + mh)).any(), "no hashed tail id in any expected row"
    assert (exp.hit[:, :mh].sum(axis=2) >= 2).any(), "no tail row hits in two tries"


def _eq(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what


# ------------------------------------------------------------------------------------------ 1: every kernel family
@pytest.mark.parametrize("prec,n,d,kg,T", SHAPES)
def test_queries_find_the_hashed_tail(prec, n, d, kg, T):
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9100 + d)
    try:
        ttail = torch.from_numpy(_rows(prec, M, d, 191)).cuda()
        ty = torch.from_numpy(_rows(prec, Q, d, 192)).cuda()
        ta = tp[:Q].contiguous()
        ix.append(ttail)
        before = _np(ix.exact_query(ty))
        assert ix.tail_hashed == 0
        ix.hash_tail()
        assert ix.tail_hashed == M and ix.tail == M
        assert _same_bits(_np(ix.exact_query(ty)), before)  # the exact entries do not change
        allow = np.random.default_rng(193).random(n + M) < 0.4
        tags, where = _tenants(n + M, Q, 194)
        plain0 = {}
        for probe in (0, 1, 3, "all"):
            ix.set_probe(probe), twin.set_probe(probe)
            for yy, alias in ((ty, False), (ta, True)):
                if probe == 1:  # no pair exists: bit for bit what probe 0 returns
                    assert _same_bits(_np(ix.query(yy, alias=alias)), plain0[alias])
                    continue
                exp = Expect(twin, ttail, yy, M)
                what = (prec, d, probe, alias)
                knn = exp.knn(256)
                for k in (None, 1, kg, 256):
                    kw = dict(alias=alias, **({} if k is None else dict(k=k)))
                    base = _np(twin.query(yy, **kw))
                    got = _np(ix.query(yy, **kw))
                    want = _want(exp, base, n, got[0].shape[1], knn)
                    _eq(got, want, what + ("plain", k))
                    if k is None:
                        _nonvacuous(exp, want, n, base)
                        if probe == 0:
                            plain0[alias] = got
                ix.set_filter(allow), twin.set_filter(allow[:n])
                knn = exp.knn(256, _valid(Q, M, n, allow))
                for k in (None, 256):
                    kw = dict(alias=alias, **({} if k is None else dict(k=k)))
                    got = _np(ix.query(yy, **kw))
                    _eq(got, _want(exp, _np(twin.query(yy, **kw)), n, got[0].shape[1], knn), what + ("allow", k))
                    assert allow[got[0][got[0] < n + M]].all()
                ix.set_tags(tags), twin.set_tags(tags[:n])
                knn = exp.knn(256, _valid(Q, M, n, allow, tags, where))
                for k in (None, 256):
                    kw = dict(alias=alias, where=where, **({} if k is None else dict(k=k)))
                    got = _np(ix.query(yy, **kw))
                    _eq(got, _want(exp, _np(twin.query(yy, **kw)), n, got[0].shape[1], knn), what + ("allow+where", k))
                ix.set_filter(None), twin.set_filter(None)
                knn = exp.knn(256, _valid(Q, M, n, None, tags, where))
                for k in (None, 1, 256):
                    kw = dict(alias=alias, where=where, **({} if k is None else dict(k=k)))
                    got = _np(ix.query(yy, **kw))
                    _eq(got, _want(exp, _np(twin.query(yy, **kw)), n, got[0].shape[1], knn), what + ("where", k))
                ix.set_tags(None), twin.set_tags(None)
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 2: lengths and tiers
def _fixture(seed, prec="f32", n=5000, d=64, kg=10, T=6):
    return (prec, n, d, kg, T) + _twins(prec, n, d, kg, T, seed)


def _check(ix, twin, ttail, ty, n, mh, what, nonvacuous=False, **kw):
    exp = Expect(twin, ttail, ty, mh)
    got = _np(ix.query(ty, **kw))
    base = _np(twin.query(ty, **kw))
    k = got[0].shape[1]
    want = _want(exp, base, n, k, exp.knn(k))
    _eq(got, want, what)
    if nonvacuous:
        _nonvacuous(exp, want, n, base)
    return got, want, exp


def test_tail_lengths_around_a_wave_pass():
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9300)
    try:
        ty = torch.from_numpy(_rows(prec, Q, d, 195)).cuda()
        src = _rows(prec, 64, d, 196)
        src[0] = ty[3].cpu().numpy()  # the only row of the shortest tail is found by a query
        for m in (1, 2, RPW - 1, RPW, RPW + 1):
            ttail = torch.from_numpy(src[:m].copy()).cuda()
            ix.drop_tail()
            ix.append(ttail)
            ix.hash_tail()
            assert ix.tail_hashed == m
            for probe in (0, 3):
                ix.set_probe(probe), twin.set_probe(probe)
                got, _, _ = _check(ix, twin, ttail, ty, n, m, ("m", m, probe))
                assert got[0][3, 0] == n and got[1][3, 0] == 0
    finally:
        ix.close(), twin.close()


def test_fresh_rows_behind_the_hashed_ones_and_rehash():
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9310)
    try:
        y = _rows(prec, Q, d, 197)
        ty = torch.from_numpy(y).cuda()
        tail = _rows(prec, M + 1 + 700 + 300, d, 198)
        tail[10] = y[4]           # a hashed row nearer than every fresh row of query 4 ...
        tail[M] = y[5]            # ... and the first fresh row nearer than every hashed row of query 5
        tail[M + 1] = y[4] + 1.0  # (a far fresh row of query 4)
        ix.append(torch.from_numpy(tail[:M]).cuda())
        ix.hash_tail()
        for upto in (M + 1, M + 1 + 700):
            ix.append(torch.from_numpy(tail[ix.tail:upto]).cuda())
            assert ix.tail == upto and ix.tail_hashed == M
            ttail = torch.from_numpy(tail[:upto]).cuda()
            for probe in (0, 3):
                ix.set_probe(probe), twin.set_probe(probe)
                got, want, exp = _check(ix, twin, ttail, ty, n, M, ("fresh", upto, probe), nonvacuous=True)
                assert got[0][4, 0] == n + 10 and got[0][5, 0] == n + M
                _check(ix, twin, ttail, ty, n, M, ("fresh k", upto, probe), k=256)
        # re-hash after further appends: all rows are hashed again, over the whole tail
        ix.append(torch.from_numpy(tail[ix.tail:]).cuda())
        ix.hash_tail()
        assert ix.tail_hashed == ix.tail == tail.shape[0]
        _check(ix, twin, torch.from_numpy(tail).cuda(), ty, n, tail.shape[0], "rehash", nonvacuous=True)
    finally:
        ix.close(), twin.close()


@pytest.mark.parametrize("prec,n,d,kg,T", [SHAPES[0], SHAPES[4], SHAPES[5]])  # 8-byte keys; 16-byte keys; the generic form
def test_the_largest_k_of_a_call(prec, n, d, kg, T):
    """k = max_query_k: the selection buffers fill the LDS and the host takes the waves of a workgroup down."""
    pts, tp, ix, twin = _twins(prec, n, d, kg, T, 9380 + d)
    try:
        ty = torch.from_numpy(_rows(prec, Q, d, 213)).cuda()
        ttail = torch.from_numpy(_rows(prec, M, d, 214)).cuda()
        ix.append(ttail[:1200].contiguous())
        ix.hash_tail()
        ix.append(ttail[1200:].contiguous())
        k = ix.max_query_k
        assert k >= 256 and k == twin.max_query_k
        for probe in (0, 3):
            ix.set_probe(probe), twin.set_probe(probe)
            _check(ix, twin, ttail, ty, n, 1200, ("k max", prec, d, probe), k=k)
    finally:
        ix.close(), twin.close()


def test_a_bucket_longer_than_a_chunk_of_equal_rows():
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9320)
    try:
        y = _rows(prec, Q, d, 199)
        tail = _rows(prec, 500, d, 200)
        tail[100:400] = y[6]  # 300 exact copies: one bucket per try, longer than a candidate chunk of 256
        ty, ttail = torch.from_numpy(y).cuda(), torch.from_numpy(tail).cuda()
        ix.append(ttail)
        ix.hash_tail()
        for probe in (0, "all"):
            ix.set_probe(probe), twin.set_probe(probe)
            for k in (None, 256):
                got, want, exp = _check(ix, twin, ttail, ty, n, 500, ("copies", probe, k), **({} if k is None else dict(k=k)))
                assert exp.hit[6, 100:400].all()  # the query equal to the row hits it in every try
                kk = got[0].shape[1]
                assert np.array_equal(got[0][6], n + 100 + np.arange(kk)) and not got[1][6].any()
                for x in range(Q):
                    real = got[0][x][got[0][x] < n + 500]
                    assert np.unique(real).size == real.size
    finally:
        ix.close(), twin.close()


def test_extreme_codes_empty_buckets_and_allow_lists():
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9330)
    try:
        ds = ix.d_short
        eng = HipEngine(twin)
        # rows whose code is 0 / 2^ds - 1 in some try: searched among random rows with the library's codes
        pool = _rows(prec, 40000, d, 201)
        pc = _codes_of(eng, torch.from_numpy(pool).cuda(), T)
        lo, hi = np.flatnonzero((pc == 0).any(axis=1)), np.flatnonzero((pc == (1 << ds) - 1).any(axis=1))
        assert lo.size and hi.size, (ds, lo.size, hi.size)
        y = _rows(prec, Q, d, 202)
        y[0], y[1] = pool[lo[0]], pool[hi[0]]
        tail = np.concatenate([pool[lo[:20]], pool[hi[:20]], _rows(prec, 300, d, 203)])
        m = tail.shape[0]
        ty, ttail = torch.from_numpy(y).cuda(), torch.from_numpy(tail).cuda()
        ix.append(ttail)
        ix.hash_tail()
        for probe in (0, 3, "all"):
            ix.set_probe(probe), twin.set_probe(probe)
            got, want, exp = _check(ix, twin, ttail, ty, n, m, ("extreme", probe), k=64)
            assert got[0][0, 0] == n and got[0][1, 0] == n + lo[:20].size
        # a query whose probed buckets are all empty returns R(q) unchanged: keep only the rows no query 2 bucket holds
        ix.set_probe(0), twin.set_probe(0)
        exp = Expect(twin, ttail, ty, m)
        keep = np.flatnonzero(~exp.cand[2])
        assert keep.size > 50
        ix.drop_tail()
        tkeep = torch.from_numpy(tail[keep].copy()).cuda()
        ix.append(tkeep)
        ix.hash_tail()
        got, want, exp = _check(ix, twin, tkeep, ty, n, keep.size, "empty buckets")
        base = _np(twin.query(ty))
        assert not exp.cand[2].any() and np.array_equal(got[0][2], base[0][2]) and np.array_equal(_bits(got[1][2]), _bits(base[1][2]))
        # an allow list that removes every hashed candidate of every query: R(q) under the list, nothing else
        mk = keep.size
        allow = np.ones(n + mk, dtype=bool)
        allow[n:] = ~exp.cand.any(axis=0)
        assert allow[n:].any() and not allow[n:].all()
        ix.set_filter(allow), twin.set_filter(allow[:n])
        got = _np(ix.query(ty))
        _eq(got, _want(exp, _np(twin.query(ty)), n, kg, exp.knn(kg, _valid(Q, mk, n, allow))), "no candidate allowed")
        assert ((got[0] < n) | (got[0] == n + mk)).all()
        # an allow list leaving fewer than k rows: pads (n_total, +inf)
        allow = np.zeros(n + mk, dtype=bool)
        allow[[3, 17, n + 1]] = True
        allow[n:] |= exp.cand[7] & (np.arange(mk) < 40)
        ix.set_filter(allow), twin.set_filter(allow[:n])
        got = _np(ix.query(ty))
        _eq(got, _want(exp, _np(twin.query(ty)), n, kg, exp.knn(kg, _valid(Q, mk, n, allow))), "few allowed")
        assert (got[0] == n + mk).any() and np.isinf(got[1][got[0] == n + mk]).all()
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 3: lifecycle
def test_empty_paths_refusals_and_lifecycle():
    from tests.test_gpu_tail import _check as exact_tail_check
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9340)
    try:
        ty = torch.from_numpy(_rows(prec, Q, d, 204)).cuda()
        tail = _rows(prec, 900, d, 205)
        ttail = torch.from_numpy(tail).cuda()
        ix.hash_tail()  # m = 0: accepted, nothing to do
        assert ix.tail_hashed == 0 and _same_bits(_np(ix.query(ty)), _np(twin.query(ty)))
        ix.append(ttail[:600].contiguous())
        exact_tail_check(ix, twin, ttail[:600].contiguous(), ty, n, what="mh = 0")  # today's result: twin plus exact tail
        ix.hash_tail()
        _check(ix, twin, ttail[:600].contiguous(), ty, n, 600, "hashed", nonvacuous=True)
        # set_fixed(False) keeps the structure; parity-mode queries never see the tail; hashing is refused meanwhile
        ix.set_fixed(False), twin.set_fixed(False)
        assert ix.tail_hashed == 600 and _same_bits(_np(ix.query(ty)), _np(twin.query(ty)))
        with pytest.raises(ValueError):
            ix.hash_tail()
        assert ix.tail_hashed == 600
        ix.set_fixed(True), twin.set_fixed(True)
        _check(ix, twin, ttail[:600].contiguous(), ty, n, 600, "fixed again")
        # a change of the probe setting needs no rebuild
        ix.set_probe(3), twin.set_probe(3)
        _check(ix, twin, ttail[:600].contiguous(), ty, n, 600, "probe changed", nonvacuous=True)
        ix.set_probe(0), twin.set_probe(0)
        # drop_tail: mh = 0; new appends without re-hashing are scanned exactly
        ix.drop_tail()
        assert ix.tail_hashed == 0 and ix.tail == 0 and _same_bits(_np(ix.query(ty)), _np(twin.query(ty)))
        ix.append(ttail[600:].contiguous())
        assert ix.tail_hashed == 0
        exact_tail_check(ix, twin, ttail[600:].contiguous(), ty, n, what="after drop_tail")
        # compact() from a hashed tail equals compact() from the same unhashed tail; the new index has mh = 0
        from oracle import oracle_py as O
        O.srandom(77)
        c0 = ix.compact(tries=2)
        ix.hash_tail()
        O.srandom(77)
        c1 = ix.compact(tries=2)
        try:
            assert c0.checksum() == c1.checksum() and c1.tail_hashed == 0 and c1.tail == 0 and c1.n == n + 300
            assert _same_bits(_np(c0.query(ty)), _np(c1.query(ty)))
        finally:
            c0.close(), c1.close()
        # a resharded index: reshard drops the structure, hashing is refused
        ix.reshard(tp[: n // 2].contiguous(), 0, n // 2)
        assert ix.tail_hashed == 0 and ix.tail == 0
        with pytest.raises(ValueError):
            ix.hash_tail()
    finally:
        ix.close(), twin.close()


def test_reallocating_appends_keep_the_structure():
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9350)
    try:
        ty = torch.from_numpy(_rows(prec, Q, d, 206)).cuda()
        tail = _rows(prec, 5800, d, 207)
        results = []
        cuts = [400, 1300, 2800, 5800]  # every append goes beyond twice the capacity the one before left
        for reserve in (False, True):
            ix.drop_tail()
            ix.append(torch.from_numpy(tail[:400]).cuda())
            ix.hash_tail()
            if reserve:  # one append into reserved room
                ix.reserve_tail(tail.shape[0])
                assert ix.tail_hashed == 400
                ix.append(torch.from_numpy(tail[400:]).cuda())
            else:        # three reallocating appends
                for a, b in zip(cuts[:-1], cuts[1:]):
                    ix.append(torch.from_numpy(tail[a:b]).cuda())
            assert ix.tail_hashed == 400 and ix.tail == tail.shape[0]
            results.append(_check(ix, twin, torch.from_numpy(tail).cuda(), ty, n, 400, ("realloc", reserve), nonvacuous=True)[0])
        assert _same_bits(results[0], results[1])
    finally:
        ix.close(), twin.close()


def test_workspaces_streams_and_the_host_stream():
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9360)
    try:
        ttail = torch.from_numpy(_rows(prec, M, d, 208)).cuda()
        ya, yb = _rows(prec, 300, d, 209), _rows(prec, 150, d, 210)
        ta, tb = torch.from_numpy(ya).cuda(), torch.from_numpy(yb).cuda()
        ix.append(ttail)
        ix.hash_tail()
        ix.set_probe(3), twin.set_probe(3)
        serial_a = _check(ix, twin, ttail, ta, n, M, "serial a", nonvacuous=True)[0]
        serial_b = _check(ix, twin, ttail, tb, n, M, "serial b", k=21)[0]
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
    finally:
        ix.close(), twin.close()


# ------------------------------------------------------------------------------------------ 4: recall without a threshold
def test_copies_of_hashed_rows_are_found_first():
    prec, n, d, kg, T, pts, tp, ix, twin = _fixture(9370)
    try:
        tail = _rows(prec, M, d, 211)
        tail[700] = tail[20]  # a duplicate: its query may return the lower id
        ttail = torch.from_numpy(tail).cuda()
        src = np.random.default_rng(212).choice(M, 300, replace=False)
        src[0] = 700
        ty = torch.from_numpy(tail[src].copy()).cuda()
        ix.append(ttail)
        ix.hash_tail()
        ids, dd = _np(ix.query(ty))
        first = ids[:, 0] - n
        assert not dd[:, 0].any()
        assert ((first == src) | ((first >= 0) & (first < src) & (tail[np.clip(first, 0, M - 1)] == tail[src]).all(axis=1))).all()
        assert first[0] == 20
        assert (_np(twin.query(ty))[0] < n).all()  # the twin cannot return these rows at all
    finally:
        ix.close(), twin.close()
