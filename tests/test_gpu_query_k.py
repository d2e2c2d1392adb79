"""GPU: fixed-mode queries and the exact scan with a k chosen per call (annhip_query_k, annhip_index_max_query_k,
annhip_index_exact_query_k; include/ann_hip.h).  kg = the index's k (the graph width), kq = the k of the call.

The oracle is bit-exact and needs no tolerance.  For one query x the stage-1 candidate set is computed on the CPU from the
exported tables, the library's own hash codes and (with pair bits) its ranked bits, ANDed with the validity rules of the
call (not x itself when aliased, the allow list, the query's tag test), and handed as a bool mask to
A.exact_knn(points, y[x:x+1], kq, allow=mask): that scan has the query path's distance arithmetic bit for bit, the same
(distance, id) order and the same (n, +inf) pad.  Its real ids plus their valid graph neighbours graph[id][0..kg) are the
stage-2 set; a second exact_knn over that set must equal the library's row, ids and distance bytes.  Helpers follow
tests/test_gpu_filter.py."""
import itertools

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd.sharded import HipEngine
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

# power of two, power of two, static lane groups, folded, kg >= 32
SHAPES = [("f64", 3000, 32, 5, 4), ("f32", 5000, 64, 10, 6), ("f64", 2500, 80, 8, 3), ("f32", 3000, 100, 10, 3),
          ("f64", 2000, 16, 33, 2)]


def _build(prec, n, d, k, T, seed):
    orc = O.CpuBackend(prec, "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    O.srandom(seed + 1)
    tp = torch.from_numpy(pts).cuda()
    ix = A.Index.precomp(tp, k, T)
    return orc, pts, tp, ix


def _codes_of(eng, ty, T):
    codes = torch.empty((ty.shape[0], T), dtype=torch.int32, device="cuda")
    with eng.use(None):
        eng.sh_codes(ty, 0, ty.shape[0], codes)
    torch.cuda.synchronize()
    return codes.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _masks(ds, ranked):
    """The contract's mask set: 0, every single bit, and the pairs among bit(o[0..b)); bit(s) = 1 << (ds-1-s)."""
    bits = [1 << (ds - 1 - int(s)) for s in ranked]
    return [0] + [1 << z for z in range(ds)] + [p | q for p, q in itertools.combinations(bits, 2)]


def _ranked(ix, ty):
    if ix.probe:
        return ix.probe_bits(ty)[1].cpu().numpy()
    return np.zeros((ty.shape[0], ix.tries, 0), dtype=np.uint8)


def _np(t):
    return tuple(v.cpu().numpy() for v in t[:2])


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def _dict(ix):
    save = ix.export()
    sd = save.to_dict()
    save.free()
    return sd


class Oracle:
    """The contract of annhip_query_k for one batch: valid[x] (bool [n]) and the stage-1 candidate set cand[x] (bool [n]) do
    not depend on kq and are computed once; row(x, kq) is the expected output row."""

    def __init__(self, ix, sd, tp, ty, alias, allow=None, tags=None, where=None):
        n, T, ds = ix.n, sd["tries"], sd["d_short"]
        Q = ty.shape[0]
        self.n, self.tp, self.ty = n, tp, ty
        self.graph = np.asarray(sd["graph"]).reshape(n, ix.k).astype(np.int64)
        tabs = [np.asarray(sd["which_par"][t]).reshape(1 << ds, -1) for t in range(T)]
        codes, ranked = _codes_of(HipEngine(ix), ty, T), _ranked(ix, ty)
        self.valid = np.ones((Q, n), dtype=bool)
        if allow is not None:
            self.valid &= allow[None, :]
        if tags is not None:
            self.valid &= (tags[None, :] & where[0][:, None]) == where[1][:, None]
        self.cand = np.zeros((Q, n), dtype=bool)
        for x in range(Q):
            if alias:
                self.valid[x, x] = False
            for t in range(T):
                for m in _masks(ds, ranked[x][t]):
                    row = tabs[t][int(codes[x, t]) ^ m]
                    self.cand[x, row[row < n].astype(np.int64)] = True
        self.cand &= self.valid

    def _scan(self, x, kq, mask):
        i, d = A.exact_knn(self.tp, self.ty[x:x + 1], kq, allow=torch.from_numpy(mask).cuda())
        return i[0].cpu().numpy(), d[0].cpu().numpy()

    def row(self, x, kq):
        i1, _ = self._scan(x, kq, self.cand[x])
        real = i1[i1 < self.n]  # a pad contributes nothing
        s2 = np.zeros(self.n, dtype=bool)
        s2[real] = True
        nb = self.graph[real].reshape(-1)
        nb = nb[nb < self.n]
        s2[nb[self.valid[x, nb]]] = True
        return self._scan(x, kq, s2)

    def check(self, got, kq, rows=None, what=None):
        for x in (range(self.ty.shape[0]) if rows is None else rows):
            wi, wd = self.row(x, kq)
            assert np.array_equal(got[0][x], wi), (what, kq, x, got[0][x], wi)
            assert np.array_equal(got[1][x].view(np.uint8), wd.view(np.uint8)), (what, kq, x, got[1][x], wd)


# ------------------------------------------------------------------------------------------ 1: matches the oracle
@pytest.mark.parametrize("prec,n,d,kg,T", SHAPES)
def test_query_k_matches_the_oracle(prec, n, d, kg, T):
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 8100 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(24 * d).reshape(24, d))).cuda()
        ta = tp[:24].contiguous()
        sd = _dict(ix)
        ix.set_fixed(True)
        for yy, alias in ((ty, False), (ta, True)):
            orac = Oracle(ix, sd, tp, yy, alias)
            for kq in (1, 3, kg, kg + 7, 100):
                got = ix.query(yy, alias=alias, k=kq)
                assert tuple(got[0].shape) == (24, kq) and tuple(got[1].shape) == (24, kq) and got[2] == 0
                got = _np(got)
                orac.check(got, kq, what=alias)
                if alias:
                    for x in range(24):
                        assert x not in got[0][x].tolist()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 2: pads
def test_rows_end_in_pads_where_fewer_than_kq_candidates_exist():
    n, d, kg, T, kq = 300, 32, 5, 1, 200
    orc, pts, tp, ix = _build("f32", n, d, kg, T, 8200)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(24 * d).reshape(24, d))).cuda()
        sd = _dict(ix)
        ix.set_fixed(True)
        got = _np(ix.query(ty, k=kq))
        Oracle(ix, sd, tp, ty, False).check(got, kq)
        for x in range(24):
            m = int((got[0][x] < n).sum())
            assert 0 < m < kq, (x, m)
            assert np.all(got[0][x, m:] == n) and np.all(np.isinf(got[1][x, m:]))
            assert np.all(got[0][x, :m] < n) and np.all(np.isfinite(got[1][x, :m]))
            assert len(set(got[0][x, :m].tolist())) == m
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 3: kq == kg is today's call
@pytest.mark.parametrize("prec,n,d,kg,T", [("f32", 5000, 64, 10, 6), ("f64", 2000, 16, 33, 2), ("f32", 3000, 100, 10, 3)])
def test_kq_equal_kg_returns_the_bits_of_todays_call(prec, n, d, kg, T):
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 8300 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(60 * d).reshape(60, d))).cuda()
        ta = tp[:40].contiguous()
        ix.set_fixed(True)
        for yy, alias in ((ty, False), (ta, True)):
            assert _same_bits(_np(ix.query(yy, alias=alias, k=kg)), _np(ix.query(yy, alias=alias)))
            ix.set_probe(3)
            assert _same_bits(_np(ix.query(yy, alias=alias, k=kg)), _np(ix.query(yy, alias=alias)))
            ix.set_probe(0)
            ix.set_filter(np.random.default_rng(83).random(n) < 0.5)
            assert _same_bits(_np(ix.query(yy, alias=alias, k=kg)), _np(ix.query(yy, alias=alias)))
            ix.set_filter(None)
            Q = yy.shape[0]
            tags, where = _tenants(n, Q, 84)  # a mixed-tenant batch
            ix.set_tags(tags)
            assert _same_bits(_np(ix.query(yy, alias=alias, where=where, k=kg)), _np(ix.query(yy, alias=alias, where=where)))
            ix.set_tags(None)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 4: composition
def _tenants(n, Q, seed):
    """Rows of three tenants; the queries ask for tenant 0, 1, 2 and for everything, in turn."""
    tags = np.random.default_rng(seed).integers(0, 3, size=n).astype(np.uint32)
    qm = np.array([0xFF, 0xFF, 0xFF, 0] * Q, dtype=np.uint32)[:Q]
    qv = np.array([0, 1, 2, 0] * Q, dtype=np.uint32)[:Q]
    return tags, (qm, qv)


def test_query_k_composes_with_probe_filter_and_tags():
    prec, n, d, kg, T = "f32", 5000, 64, 10, 6
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 8400)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(24 * d).reshape(24, d))).cuda()
        ta = tp[:24].contiguous()
        sd = _dict(ix)
        ix.set_fixed(True)
        allow = np.random.default_rng(85).random(n) < 0.3
        tags, where = _tenants(n, 24, 86)
        for yy, alias in ((ty, False), (ta, True)):
            ix.set_probe(3)
            orac = Oracle(ix, sd, tp, yy, alias)
            for kq in (2 * kg + 1, 2):
                orac.check(_np(ix.query(yy, alias=alias, k=kq)), kq, what="probe")
            ix.set_probe(0)
            ix.set_filter(allow)
            orac = Oracle(ix, sd, tp, yy, alias, allow=allow)
            for kq in (2 * kg + 1, 2):
                got = _np(ix.query(yy, alias=alias, k=kq))
                orac.check(got, kq, what="filter")
                assert allow[got[0][got[0] < n]].all()
            ix.set_tags(tags)
            orac = Oracle(ix, sd, tp, yy, alias, allow=allow, tags=tags, where=where)
            for kq in (2 * kg + 1, 2):
                got = _np(ix.query(yy, alias=alias, where=where, k=kq))
                orac.check(got, kq, what="tags and filter")
                for x in range(24):
                    live = got[0][x][got[0][x] < n]
                    assert np.all((tags[live] & where[0][x]) == where[1][x]) and allow[live].all()
            ix.set_tags(None)
            ix.set_filter(None)
    finally:
        ix.close()


@pytest.mark.parametrize("prec,rows,narrow", [("f32", "f16", np.float16), ("f64", "f32", np.float32)])
def test_query_k_composes_with_narrow_rows(prec, rows, narrow):
    n, d, kg, T = 4000, 64, 7, 4
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 8500)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(24 * d).reshape(24, d))).cuda()
        sd = _dict(ix)
        ix.set_fixed(True)
        ix.set_rows(rows)
        rounded = torch.from_numpy(pts.astype(narrow).astype(pts.dtype)).cuda()  # the oracle scans the rounded-and-widened rows
        orac = Oracle(ix, sd, rounded, ty, False)
        for kq in (2 * kg + 1, 2):
            orac.check(_np(ix.query(ty, k=kq)), kq, what=rows)
        ix.set_rows("native")
        orac = Oracle(ix, sd, tp, ty, False)
        for kq in (2 * kg + 1, 2):
            orac.check(_np(ix.query(ty, k=kq)), kq, what="native")
    finally:
        ix.close()


def test_two_workspaces_on_two_streams_with_different_kq():
    n = 6000
    orc, pts, tp, ix = _build("f32", n, 64, 10, 6, 8600)
    try:
        ta = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(700 * 64).reshape(700, 64))).cuda()
        tb = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(300 * 64).reshape(300, 64))).cuda()
        ix.set_fixed(True)
        tags, _ = _tenants(n, 1, 87)
        ix.set_tags(tags)
        wb = (np.full(300, 0xFF, dtype=np.uint32), (np.arange(300) % 3).astype(np.uint32))
        serial_a, serial_b = _np(ix.query(ta, k=21)), _np(ix.query(tb, k=2, where=wb))
        torch.cuda.synchronize()
        w1, w2, s1, s2 = ix.workspace(), ix.workspace(), torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            ga = ix.query(ta, ws=w1, stream=s1, k=21)
        with torch.cuda.stream(s2):
            gb = ix.query(tb, ws=w2, stream=s2, k=2, where=wb)
        s1.synchronize(), s2.synchronize()
        assert _same_bits(_np(ga), serial_a) and _same_bits(_np(gb), serial_b)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 5: the largest kq
@pytest.mark.parametrize("prec,n,d,kg,T", [("f64", 2000, 16, 33, 2), ("f32", 2000, 32, 10, 2)])
def test_the_largest_kq(prec, n, d, kg, T):
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 8700 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(4 * d).reshape(4, d))).cuda()
        sd = _dict(ix)
        ix.set_fixed(True)
        kmax = ix.max_query_k
        print("%s d %d kg %d: max_query_k %d" % (prec, d, kg, kmax))
        assert 256 <= kmax <= 1024
        Oracle(ix, sd, tp, ty, False).check(_np(ix.query(ty, k=kmax)), kmax)
        ids = torch.full((4, kmax + 1), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((4, kmax + 1), -7.0, dtype=ty.dtype, device="cuda")
        with pytest.raises(ValueError):
            ix.query(ty, k=kmax + 1, out_ids=ids, out_dists=dd)
        torch.cuda.synchronize()
        assert bool((ids == -7).all()) and bool((dd == -7.0).all())
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 6: exact_query(k=)
@pytest.mark.parametrize("prec,n,d,kg,T", [("f32", 5000, 64, 10, 6), ("f64", 2500, 80, 8, 3)])
def test_exact_query_with_k(prec, n, d, kg, T):
    orc, pts, tp, ix = _build(prec, n, d, kg, T, 8800 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(40 * d).reshape(40, d))).cuda()
        ta = tp[:40].contiguous()
        for kq in (1, kg, 64):
            assert _same_bits(_np(ix.exact_query(ty, k=kq)), _np(A.exact_knn(tp, ty, kq)))
            assert _same_bits(_np(ix.exact_query(ta, alias=True, k=kq)), _np(A.exact_knn(tp, ta, kq, self_exclude=True)))
        ix.set_fixed(True)
        allow = np.random.default_rng(88).random(n) < 0.3
        ta_allow = torch.from_numpy(allow).cuda()
        ix.set_filter(allow)
        assert _same_bits(_np(ix.exact_query(ty, k=64)), _np(A.exact_knn(tp, ty, 64, allow=ta_allow)))
        ix.set_filter(None)
        tags, where = _tenants(n, 40, 89)
        with pytest.raises(ValueError):  # where= without tags
            ix.exact_query(ty, where=where, k=3)
        ix.set_tags(tags)
        assert _same_bits(_np(ix.exact_query(ty, where=where, k=64)), _np(A.exact_knn(tp, ty, 64, tags=tags, where=where)))
        with pytest.raises(ValueError):
            ix.exact_query(ty, k=n + 1)
        with pytest.raises(ValueError):
            ix.exact_query(ty, k=1025)
        for bad in (0, True, 2.5):
            with pytest.raises(ValueError):
                ix.exact_query(ty, k=bad)
    finally:
        ix.close()


def test_exact_query_refuses_k_beyond_the_rows_on_offer():
    n, d = 40, 32
    orc, pts, tp, ix = _build("f32", n, d, 5, 1, 8900)
    try:
        ta = tp[:8].contiguous()
        assert _same_bits(_np(ix.exact_query(ta, k=n)), _np(A.exact_knn(tp, ta, n)))
        assert _same_bits(_np(ix.exact_query(ta, alias=True, k=n - 1)), _np(A.exact_knn(tp, ta, n - 1, self_exclude=True)))
        with pytest.raises(ValueError):  # k > n - alias
            ix.exact_query(ta, alias=True, k=n)
        with pytest.raises(ValueError):
            ix.exact_query(ta, k=n + 1)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7: refusals and lifecycle
def test_refusals_and_lifecycle():
    """Every refusal raises ValueError, launches nothing (pre-filled outputs stay as they are) and leaves the index as it
    was: the plain ix.query(y) that follows returns its old bits.  The resharded index comes last and is followed by no
    plain fixed-mode query: that path ends the process on such an index by design (annhip_query, fixed mode)."""
    n, d, kg, T = 5000, 64, 10, 6
    orc, pts, tp, ix = _build("f32", n, d, kg, T, 9000)
    try:
        y = np.ascontiguousarray(orc.gen_rand(120 * d).reshape(120, d))
        ty = torch.from_numpy(y).cuda()
        sd = _dict(ix)
        want = orc.query(sd, pts, y)
        ids = torch.full((120, 4), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((120, 4), -7.0, dtype=torch.float32, device="cuda")

        def refused(**kw):
            with pytest.raises(ValueError):
                ix.query(ty, out_ids=ids, out_dists=dd, **kw)
            torch.cuda.synchronize()
            assert bool((ids == -7).all()) and bool((dd == -7.0).all()), kw

        parity = _np(ix.query(ty))
        refused(k=4)                      # fixed mode is off
        assert _same_bits(_np(ix.query(ty)), parity)
        ix.set_fixed(True)
        plain = _np(ix.query(ty))
        tags, where = _tenants(n, 120, 90)
        for kw in (dict(k=0), dict(k=True), dict(k=2.5), dict(k=4, where=where)):  # ..., where= without tags
            refused(**kw)
            assert _same_bits(_np(ix.query(ty)), plain), kw
        lib = ix.lib  # exactly one of the two predicate arrays
        ix.set_tags(tags)
        qm = torch.from_numpy(where[0].view(np.int32)).cuda()
        assert lib.annhip_query_k(ix.h, None, None, 120, ty.data_ptr(), 0, 4, qm.data_ptr(), None, ids.data_ptr(), dd.data_ptr()) == -2
        assert lib.annhip_query_k(ix.h, None, None, 120, ty.data_ptr(), 0, 4, None, qm.data_ptr(), ids.data_ptr(), dd.data_ptr()) == -2
        assert lib.annhip_query_k(ix.h, None, None, 0, ty.data_ptr(), 0, 4, None, None, ids.data_ptr(), dd.data_ptr()) == 0  # ycnt == 0
        torch.cuda.synchronize()
        assert bool((ids == -7).all()) and bool((dd == -7.0).all())
        ix.set_tags(None)
        assert _same_bits(_np(ix.query(ty)), plain)
        got = ix.query(ty, k=4, out_ids=ids, out_dists=dd)  # and an accepted call writes them
        assert got[0] is ids and bool((ids >= 0).all())
        # the switch goes back: parity mode again, bit for bit the reference's answer
        ix.set_fixed(False)
        ids0, dd0, _ = ix.query(ty)
        assert np.array_equal(ids0.cpu().numpy().astype(np.uint64), want[0])
        assert np.array_equal(dd0.cpu().numpy().view(np.uint8), want[1].view(np.uint8))
        # a resharded index is refused, not aborted on
        ix.set_fixed(True)
        ids.fill_(-7), dd.fill_(-7.0)
        ix.reshard(tp[: n // 2].contiguous(), 0, n // 2)
        refused(k=4)
        with pytest.raises(ValueError):
            ix.exact_query(ty, k=4)
    finally:
        ix.close()
