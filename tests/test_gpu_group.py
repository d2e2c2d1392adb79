"""GPU: grouped queries by collapse (annhip_collapse, annhip_query_grouped, annhip_index_exact_query_grouped;
include/ann_hip.h, ann_group_kernels.h).

Every check is bit-exact on ids, distance bytes, counts and short; no tolerance.  The expectation of every grouped call is
tests/group_model.py::collapse_model -- a loop per row written from the contract -- applied to the row that the existing
call it ends (query(k=K'), exact_query(k=K'), A.exact_knn) returns for the same arguments.

One small clustered index per precision serves sections 2 to 7: n = 3000, d = 32, 4 tries, k = 10; the 8 rows of group
id // 8 lie near each other, as the chunks of one document do, so that a list of neighbours holds several rows of a group.
The tag word is (group << 8) | tenant with tenant = group % 8: a tenant predicate leaves whole groups, 376 rows at most."""
import itertools

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests.group_model import collapse_model

pytestmark = pytest.mark.gpu

GMASK = 0xFFFFFF00
N, D, KG, TRIES, Q = 3000, 32, 10, 4, 24
COMBOS = list(itertools.product((10, 40, 256), (1, 10), (1, 3)))  # K', k, per_group


def _dt(prec):
    return np.float32 if prec == "f32" else np.float64


def _npall(t):
    return tuple(v.cpu().numpy() for v in t)


def _eq4(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint8), np.ascontiguousarray(want[1]).view(np.uint8)), (what, got[1], want[1])
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])
    assert got[3].dtype == np.bool_ and np.array_equal(got[3], want[3]), (what, got[3], want[3])


def _clustered(rng, n, d, dt, per=8):
    centres = rng.standard_normal(((n + per - 1) // per, d))
    return np.ascontiguousarray((np.repeat(centres, per, axis=0)[:n] + 0.35 * rng.standard_normal((n, d))).astype(dt))


def _tags(n, first=0):
    grp = (np.arange(first, first + n) // 8).astype(np.uint32)
    return (grp << np.uint32(8)) | (grp % np.uint32(8))


def _make(prec, n, d, seed):
    rng = np.random.default_rng(seed)
    pts = _clustered(rng, n, d, _dt(prec))
    tp = torch.from_numpy(pts).cuda()
    O.srandom(seed)
    ix = A.Index.precomp(tp, KG, TRIES)
    ix.set_fixed(True)
    tags = _tags(n)
    ix.set_tags(tags)
    # queries near rows of 24 different groups, and the first 24 rows themselves for the aliased calls
    pick = rng.permutation(n // 8)[:Q] * 8 + 3
    y = np.ascontiguousarray((pts[pick] + 0.2 * rng.standard_normal((Q, d))).astype(_dt(prec)))
    return {"prec": prec, "n": n, "d": d, "pts": pts, "tp": tp, "ix": ix, "tags": tags, "ty": torch.from_numpy(y).cuda(),
            "ta": tp[:Q].contiguous(), "pick": pick}


@pytest.fixture(scope="module", params=["f32", "f64"])
def world(request):
    w = _make(request.param, N, D, 9300 + (request.param == "f64"))
    yield w
    w["ix"].close()


def _where_pair(w):
    """every query asks for the tenant of the group it lies in: at most 376 valid rows, the query's neighbours among them"""
    return (np.full(Q, 0xFF, dtype=np.uint32), (w["pick"] // 8 % 8).astype(np.uint32))


def _where_range(w):
    """two tenants, the query's own among them"""
    t = (w["pick"] // 8 % 8).astype(np.uint32)
    lo = (t - (t > 0)).astype(np.uint32)
    return (np.full(Q, 0xFF, dtype=np.uint32), lo, (lo + 1).astype(np.uint32))


def _check_against_query(ix, yy, tags, what, where=None, alias=False, combos=COMBOS, **kw):
    """query_grouped(candidates=K') == collapse_model(query(k=K', where=...)) for every (K', k, per_group) -> the number of
    rows in which the collapse dropped an entry and of short rows (so that a caller can tell the case was exercised)"""
    nt = ix.n_total
    dropped = shorts = 0
    for kc, k, g in combos:
        li, ld, _ = ix.query(yy, alias=alias, where=where, k=kc, **kw)
        torch.cuda.synchronize()
        li, ld = li.cpu().numpy(), ld.cpu().numpy()
        want = collapse_model(li, ld, tags, GMASK, k, g, nt, nt)
        got = ix.query_grouped(yy, GMASK, k=k, per_group=g, candidates=kc, where=where, alias=alias, **kw)
        torch.cuda.synchronize()
        assert got[0].dtype == torch.int64 and got[2].dtype == torch.int32 and got[3].dtype == torch.bool
        assert tuple(got[0].shape) == (yy.shape[0], k) and tuple(got[1].shape) == (yy.shape[0], k)
        _eq4(_npall(got), want, (what, kc, k, g))
        dropped += int((want[0] != li[:, :k]).any(axis=1).sum())
        shorts += int(want[3].sum())
    return dropped, shorts


# ------------------------------------------------------------------------------------------ 1: the collapse alone
def _lists(rng, L, rows, groups, dt):
    """[37][L] lists in ascending distance with, over the rows: pads at the end, a pad in the middle, ids >= rows (rows + 9,
    2^32 + 5, -1), a repeated id, a NaN and a +inf distance.  tags: `groups` values in the group field, noise below it."""
    Qc = 37
    tags = (rng.integers(0, groups, size=rows).astype(np.uint32) << np.uint32(8)) | rng.integers(0, 256, size=rows).astype(np.uint32)
    ids = np.stack([rng.permutation(rows)[:L] for _ in range(Qc)]).astype(np.int64)
    dd = np.sort(rng.random((Qc, L)).astype(dt) + dt(0.25), axis=1)
    odd = np.array([rows, rows + 9, 2 ** 32 + 5, -1], dtype=np.int64)
    for q in range(Qc):
        c = q % 6
        if c == 1:  # pads at the end: 1..L of them
            m = L - 1 - (q % L)
            ids[q, m:], dd[q, m:] = rows, np.inf
        elif c == 2:  # a pad of some kind in the middle (at the start where L == 1)
            ids[q, L // 2] = odd[q % 4]
        elif c == 3 and L > 1:  # a repeated id
            ids[q, L - 1] = ids[q, L // 3]
        elif c == 4:  # NaN and +inf are ordinary values
            dd[q, L // 2] = np.nan
            dd[q, L - 1] = np.inf
        elif c == 5:  # several odd entries
            ids[q, ::5] = odd[(np.arange(len(ids[q, ::5])) + q) % 4]
    return ids, dd, tags


def _cases():
    seen, out = set(), []
    cross = itertools.product((1, 63, 64, 65, 200, 1024), (1, 10, 0), (1, 2, 5, 0), (1, 3, 0))  # 0: L
    for i, (L, k, g, groups) in enumerate(cross):
        case = (L, min(k, L) if k else L, g if g else L, groups if groups else max(L, 2))
        if i % 7 in (0, 2) and case not in seen:
            seen.add(case)
            out.append(("f64" if len(out) % 2 else "f32",) + case)
    return out


CASES = _cases()


def test_the_thinned_cross_product_keeps_every_value():
    assert 50 <= len(CASES) <= 70
    for col, vals in ((1, {1, 63, 64, 65, 200, 1024}), (3, {1, 2, 5})):
        assert {c[col] for c in CASES} >= vals
    for L in (63, 64, 65, 200, 1024):  # at every L above 1: k in {1, 10, L}, per_group = L, 1, 3 and about L groups
        here = [c for c in CASES if c[1] == L]
        assert {c[2] for c in here} == {1, 10, L} and L in {c[3] for c in here} and {c[4] for c in here} == {1, 3, L}, L
    assert {c[0] for c in CASES if c[1] == 1024} == {"f32", "f64"}
    assert any(c[2] == c[1] == 1024 for c in CASES) and any(c[3] == 1024 for c in CASES)


@pytest.mark.parametrize("prec,L,k,g,groups", CASES)
def test_collapse_matches_the_model(prec, L, k, g, groups):
    rows = 5000
    rng = np.random.default_rng(9000 + 7 * L + 3 * k + g + groups)
    ids, dd, tags = _lists(rng, L, rows, groups, _dt(prec))
    want = collapse_model(ids, dd, tags, GMASK, k, g, rows, rows)
    ti, td = torch.from_numpy(ids).cuda(), torch.from_numpy(dd).cuda()
    got = A.collapse(ti, td, tags, GMASK, k, per_group=g)
    torch.cuda.synchronize()
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.bool and tuple(got[0].shape) == (37, k)
    _eq4(_npall(got), want, "fresh outputs")
    assert np.array_equal(ti.cpu().numpy(), ids) and np.array_equal(td.cpu().numpy().view(np.uint8), dd.view(np.uint8))
    # tags on the device, rows below len(tags) and a pad id of the caller's own
    tt = torch.from_numpy(tags.view(np.int32)).cuda()
    got = A.collapse(ti, td, tt, GMASK, k, per_group=g, rows=rows - 100, pad_id=77777)
    torch.cuda.synchronize()
    _eq4(_npall(got), collapse_model(ids, dd, tags, GMASK, k, g, rows - 100, 77777), "rows and pad_id")
    if k == L:  # in place: the library call with its outputs on its inputs
        cc = torch.full((37,), -7, dtype=torch.int32, device="cuda")
        ss = torch.full((37,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert A._lib.load(prec).annhip_collapse(37, L, k, g, GMASK, tt.data_ptr(), rows, rows, ti.data_ptr(), td.data_ptr(),
                                                 ti.data_ptr(), td.data_ptr(), cc.data_ptr(), ss.data_ptr(), None) == 0
        torch.cuda.synchronize()
        _eq4(_npall((ti, td, cc, ss.bool())), want, "in place")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_collapse_without_counts_or_short_and_on_a_stream(prec):
    rows, L, k, g = 900, 130, 20, 2
    rng = np.random.default_rng(9050)
    ids, dd, tags = _lists(rng, L, rows, 40, _dt(prec))
    want = collapse_model(ids, dd, tags, GMASK, k, g, rows, rows)
    lib = A._lib.load(prec)
    ti, td = torch.from_numpy(ids).cuda(), torch.from_numpy(dd).cuda()
    tt = torch.from_numpy(tags.view(np.int32)).cuda()
    for with_counts, with_short in ((False, False), (True, False), (False, True)):
        oi = torch.full((37, k), -7, dtype=torch.int64, device="cuda")
        od = torch.full((37, k), -7.0, dtype=td.dtype, device="cuda")
        cc = torch.full((37,), -7, dtype=torch.int32, device="cuda")
        ss = torch.full((37,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.annhip_collapse(37, L, k, g, GMASK, tt.data_ptr(), rows, rows, ti.data_ptr(), td.data_ptr(), oi.data_ptr(),
                                   od.data_ptr(), cc.data_ptr() if with_counts else None,
                                   ss.data_ptr() if with_short else None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(oi.cpu().numpy(), want[0])
        assert np.array_equal(od.cpu().numpy().view(np.uint8), want[1].view(np.uint8))
        assert np.array_equal(cc.cpu().numpy(), want[2] if with_counts else np.full(37, -7, dtype=np.int32))
        assert np.array_equal(ss.cpu().numpy(), want[3].astype(np.uint8) if with_short else np.full(37, 9, dtype=np.uint8))
    st = torch.cuda.Stream()
    got = A.collapse(ti, td, tt, GMASK, k, per_group=g, stream=st)
    torch.cuda.synchronize()
    _eq4(_npall(got), want, "stream")


# ------------------------------------------------------------------------------------------ 2: identity
def test_distinct_keys_give_the_row_of_query_k(world):
    ix, ty = world["ix"], world["ty"]
    ix.set_tags(np.arange(N, dtype=np.uint32))
    try:
        for kc, k in ((10, 10), (40, 10), (40, 1), (256, 10), (256, 256)):
            li, ld, _ = ix.query(ty, k=kc)
            got = ix.query_grouped(ty, 0xFFFFFFFF, k=k, per_group=1, candidates=kc)
            torch.cuda.synchronize()
            li, ld = li.cpu().numpy(), ld.cpu().numpy()
            gi, gd, gc, gs = _npall(got)
            assert np.array_equal(gi, li[:, :k]) and np.array_equal(gd.view(np.uint8), np.ascontiguousarray(ld[:, :k]).view(np.uint8))
            real = (li < N).sum(axis=1)
            assert np.array_equal(gc, np.minimum(real, k).astype(np.int32))
            assert not gs.any()  # a full list of distinct keys holds k of them
    finally:
        ix.set_tags(world["tags"])


# ------------------------------------------------------------------------------------------ 3: composition
def _v_plain(w):
    return _check_against_query(w["ix"], w["ty"], w["tags"], "plain")


def _v_pair(w):
    return _check_against_query(w["ix"], w["ty"], w["tags"], "pair", where=_where_pair(w))


def _v_range(w):
    return _check_against_query(w["ix"], w["ty"], w["tags"], "range", where=_where_range(w))


def _v_allow(w):
    ix = w["ix"]
    ix.set_filter(np.random.default_rng(93).random(N) < 0.6)
    try:
        return _check_against_query(ix, w["ty"], w["tags"], "allow list")
    finally:
        ix.set_filter(None)


def _v_probe(w):
    ix = w["ix"]
    ix.set_probe(2)
    try:
        return _check_against_query(ix, w["ty"], w["tags"], "probe")
    finally:
        ix.set_probe(0)


def _v_narrow(w):
    ix = w["ix"]
    ix.set_rows("f16" if w["prec"] == "f32" else "f32")
    try:
        return _check_against_query(ix, w["ty"], w["tags"], "narrow rows")
    finally:
        ix.set_rows("native")


def _v_alias(w):
    return _check_against_query(w["ix"], w["ta"], w["tags"], "alias", alias=True)


def _v_ws_stream(w):
    ix = w["ix"]
    return _check_against_query(ix, w["ty"], w["tags"], "workspace and stream", ws=ix.workspace(), stream=torch.cuda.Stream())


def _with_tail(w, hashed):
    """70 tagged rows near the queries, in groups that built rows belong to as well"""
    ix, rng = w["ix"], np.random.default_rng(94)
    y = w["ty"].cpu().numpy()
    rows = np.ascontiguousarray((y[np.arange(70) % Q] + 0.15 * rng.standard_normal((70, D))).astype(y.dtype))
    ttags = w["tags"][w["pick"][np.arange(70) % Q]]  # the groups the queries lie in
    ix.append(rows, tags=ttags)
    try:
        if hashed:
            ix.hash_tail()
        assert ix.n_total == N + 70 and ix.tail_hashed == (70 if hashed else 0)
        tags = np.concatenate([w["tags"], ttags])
        res = _check_against_query(ix, w["ty"], tags, "tail, hashed = %r" % hashed)
        got = ix.query_grouped(w["ty"], GMASK, k=10, candidates=40)[0]
        assert bool((got >= N).logical_and(got < N + 70).any()), "no tail row in any result"
        return res
    finally:
        ix.drop_tail()


def _v_tail(w):
    return _with_tail(w, False)


def _v_tail_hashed(w):
    return _with_tail(w, True)


VARIANTS = {"plain": _v_plain, "pair": _v_pair, "range": _v_range, "allow": _v_allow, "probe": _v_probe, "narrow": _v_narrow,
            "alias": _v_alias, "ws_stream": _v_ws_stream, "tail": _v_tail, "tail_hashed": _v_tail_hashed}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_query_grouped_is_the_collapse_of_query_k(world, variant):
    dropped, shorts = VARIANTS[variant](world)
    assert dropped > 0, "no row in which the collapse dropped anything: the case checks nothing"
    if variant == "plain":
        assert shorts > 0  # K' = 10 of one or two groups, k = 10


@pytest.mark.parametrize("prec,d", [("f64", 80), ("f32", 100)])
def test_query_grouped_through_the_other_row_layouts(prec, d):
    w = _make(prec, 2000, d, 9400 + d)
    try:
        dropped, _ = _check_against_query(w["ix"], w["ty"], w["tags"], d, combos=[(40, 10, 1), (256, 10, 3), (10, 1, 1)])
        assert dropped > 0
    finally:
        w["ix"].close()


# ------------------------------------------------------------------------------------------ 4: ground truth
def test_exact_query_grouped_is_the_collapse_of_exact_query(world):
    ix, ty, tags = world["ix"], world["ty"], world["tags"]
    for where in (None, _where_pair(world), _where_range(world)):
        for kc, k, g in ((10, 10, 1), (40, 10, 1), (256, 10, 3), (600, 10, 2), (40, 1, 1)):
            li, ld = ix.exact_query(ty, where=where, k=kc)
            want = collapse_model(li.cpu().numpy(), ld.cpu().numpy(), tags, GMASK, k, g, N, N)
            got = ix.exact_query_grouped(ty, GMASK, k=k, per_group=g, candidates=kc, where=where)
            _eq4(_npall(got), want, ("exact", where is not None, kc, k, g))
    ga = ix.exact_query_grouped(world["ta"], GMASK, k=10, candidates=40, alias=True)
    li, ld = ix.exact_query(world["ta"], alias=True, k=40)
    _eq4(_npall(ga), collapse_model(li.cpu().numpy(), ld.cpu().numpy(), tags, GMASK, 10, 1, N, N), "exact alias")


def test_exact_query_grouped_is_complete_where_not_short(world):
    """A tenant predicate leaves at most 376 valid rows; with K' = 600 every list ends in pads, short is all zero, and the result is
    the collapse of ALL valid rows in (distance, id) order: A.exact_knn over the row tensor under the same predicate."""
    ix, ty, tags = world["ix"], world["ty"], world["tags"]
    tp = ix.rows_tensor(0, ix.n_total)
    where = _where_pair(world)
    assert max(int(((tags & 0xFF) == t).sum()) for t in range(8)) <= 500
    ai, ad = A.exact_knn(tp, ty, 500, tags=tags, where=where)
    ai, ad = ai.cpu().numpy(), ad.cpu().numpy()
    assert all(sorted(ai[q][ai[q] < N].tolist()) == np.nonzero((tags & 0xFF) == where[1][q])[0].tolist() for q in range(Q))
    for k, g in ((10, 1), (10, 3), (64, 1), (1, 1)):
        got = _npall(ix.exact_query_grouped(ty, GMASK, k=k, per_group=g, candidates=600, where=where))
        assert not got[3].any()
        want = collapse_model(ai, ad, tags, GMASK, k, g, N, N)
        assert not want[3].any()
        _eq4(got, want, ("complete", k, g))
    # the approximate call scored against it: recall runs and is a share
    gi = ix.query_grouped(ty, GMASK, k=10, candidates=40, where=where)[0]
    ti = ix.exact_query_grouped(ty, GMASK, k=10, candidates=600, where=where)[0]
    torch.cuda.synchronize()
    rec = A.recall_at_k(gi, ti)
    print("group-recall@10 of query_grouped(candidates=40) under a tenant predicate: %.4f" % rec)
    assert 0.0 <= rec <= 1.0


# ------------------------------------------------------------------------------------------ 5: short
def test_short_tells_a_full_list_with_too_few_groups(world):
    ix, ty = world["ix"], world["ty"]
    # all rows but 5 in one group; tenant 1 = the 32 rows around the first four queries: the 5 rows of groups of their own
    # and 27 of the big group
    near = np.concatenate([world["pick"][q] // 8 * 8 + np.arange(8) for q in range(4)])
    t2 = np.full(N, 7 << 8, dtype=np.uint32)
    t2[near[:5]] = (100 + np.arange(5, dtype=np.uint32)) << np.uint32(8)
    t2[near] |= 1
    ix.set_tags(t2)
    try:
        li = ix.query(ty, k=40)[0].cpu().numpy()
        gi, gd, gc, gs = _npall(ix.query_grouped(ty, GMASK, k=10, per_group=1, candidates=40))
        full = (li < N).all(axis=1)
        assert full.any()
        assert np.all(gc[full] < 10) and np.all(gs[full]) and not gs[~full].any()
        _eq4((gi, gd, gc, gs), collapse_model(li, ix.query(ty, k=40)[1].cpu().numpy(), t2, GMASK, 10, 1, N, N), "one big group")
        # fewer valid rows than K': the list ends in pads, nothing more can be found
        where = (np.full(Q, 0xFF, dtype=np.uint32), np.ones(Q, dtype=np.uint32))
        wi = ix.query(ty, k=40, where=where)[0].cpu().numpy()
        assert np.all((wi < N).sum(axis=1) <= 32) and np.all(np.isin(wi[wi < N], near)) and (wi[:4] < N).any()
        _, _, wc, ws = _npall(ix.query_grouped(ty, GMASK, k=10, per_group=1, candidates=40, where=where))
        assert not ws.any()
        distinct = [len({int(t2[i]) & GMASK for i in row[row < N]}) for row in wi]
        assert np.array_equal(wc, np.array(distinct, dtype=np.int32)) and 1 < max(distinct) <= 6
    finally:
        ix.set_tags(world["tags"])


# ------------------------------------------------------------------------------------------ 6: refusals
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_collapse_refusals(prec):
    lib = A._lib.load(prec)
    Qc, L, k, rows = 5, 8, 4, 100
    ft = torch.float32 if prec == "f32" else torch.float64
    ti = torch.arange(Qc * L, dtype=torch.int64, device="cuda").reshape(Qc, L).contiguous()
    td = torch.rand((Qc, L), dtype=ft, device="cuda")
    tt = torch.arange(rows, dtype=torch.int32, device="cuda")
    oi = torch.full((Qc, k), -7, dtype=torch.int64, device="cuda")
    od = torch.full((Qc, k), -7.0, dtype=ft, device="cuda")
    cc = torch.full((Qc,), -7, dtype=torch.int32, device="cuda")
    ss = torch.full((Qc,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def raw(ycnt=Qc, L=L, k=k, g=1, gmask=0xFF, tags=tt.data_ptr(), rows=rows, i=ti.data_ptr(), d=td.data_ptr(), o=oi.data_ptr(),
            e=od.data_ptr()):
        return lib.annhip_collapse(ycnt, L, k, g, gmask, tags, rows, rows, i, d, o, e, cc.data_ptr(), ss.data_ptr(), None)

    for what, kw in (("L == 0", dict(L=0, k=0)), ("L > 1024", dict(L=1025)), ("k == 0", dict(k=0)), ("k > L", dict(k=L + 1)),
                     ("per_group == 0", dict(g=0)), ("gmask == 0", dict(gmask=0)), ("tags NULL", dict(tags=None)),
                     ("ids_in NULL", dict(i=None)), ("dists_in NULL", dict(d=None)), ("ids_out NULL", dict(o=None)),
                     ("dists_out NULL", dict(e=None)), ("rows beyond 32 bits", dict(rows=0xFFFFFFF0))):
        assert raw(**kw) == -1, what
    assert raw(ycnt=0) == 0
    torch.cuda.synchronize()
    assert bool((oi == -7).all()) and bool((od == -7.0).all()) and bool((cc == -7).all()) and bool((ss == 9).all())
    assert raw() == 0  # and an accepted call writes all four
    torch.cuda.synchronize()
    assert bool((oi >= 0).all()) and bool((od >= 0).all()) and bool((cc == k).all()) and bool((ss == 0).all())
    for bad in (dict(k=True), dict(k=2.0), dict(per_group=0), dict(per_group=True), dict(group=0), dict(group=1 << 32),
                dict(group=1.0), dict(k=L + 1), dict(rows=rows + 1), dict(rows=True)):
        kw = dict(group=0xFF, k=k)
        kw.update(bad)
        with pytest.raises(ValueError):
            A.collapse(ti, td, tt, **kw)
    with pytest.raises(ValueError):
        A.collapse(ti.int(), td, tt, 0xFF, k)
    with pytest.raises(ValueError):
        A.collapse(ti, td[:, :4], tt, 0xFF, k)


def test_grouped_refusals(capfd):
    """Every refusal returns -2 (non-zero from the exact call), launches nothing -- pre-filled outputs stay as they are --
    and raises ValueError in Python.  The resharded index comes last."""
    w = _make("f32", 1500, 32, 9500)
    ix, ty, n = w["ix"], w["ty"], w["n"]
    try:
        lib = ix.lib
        kmax = ix.max_query_k
        ids = torch.full((Q, 4), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((Q, 4), -7.0, dtype=torch.float32, device="cuda")
        cc = torch.full((Q,), -7, dtype=torch.int32, device="cuda")
        ss = torch.full((Q,), 9, dtype=torch.uint8, device="cuda")
        qm, ql, qh = (torch.from_numpy(a.view(np.int32)).cuda() for a in _where_range(w))
        torch.cuda.synchronize()

        def fixed(ycnt=Q, lst=16, k=4, g=1, gmask=GMASK, m=None, lo=None, hi=None, i=ids.data_ptr()):
            return lib.annhip_query_grouped(ix.h, None, None, ycnt, ty.data_ptr(), 0, lst, k, g, gmask, m, lo, hi, i, dd.data_ptr(),
                                            cc.data_ptr(), ss.data_ptr())

        def exact(ycnt=Q, lst=16, k=4, g=1, gmask=GMASK, m=None, lo=None, hi=None, i=ids.data_ptr(), d=dd.data_ptr()):
            return lib.annhip_index_exact_query_grouped(ix.h, ycnt, ty.data_ptr(), 0, lst, k, g, gmask, m, lo, hi, i, d, cc.data_ptr(),
                                                        ss.data_ptr())

        def untouched(what):
            torch.cuda.synchronize()
            assert bool((ids == -7).all()) and bool((dd == -7.0).all()) and bool((cc == -7).all()) and bool((ss == 9).all()), what

        shared = (("gmask == 0", dict(gmask=0)), ("per_group == 0", dict(g=0)), ("k == 0", dict(k=0)), ("k > list", dict(lst=3)),
                  ("list == 0", dict(lst=0, k=0)), ("qmask only", dict(m=qm.data_ptr())),
                  ("qlo and qhi only", dict(lo=ql.data_ptr(), hi=qh.data_ptr())),
                  ("qmask and qlo only", dict(m=qm.data_ptr(), lo=ql.data_ptr())), ("ids NULL", dict(i=None)))
        capfd.readouterr()
        assert fixed(gmask=0) == -2
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and err.startswith("annhip_query_grouped: ")
        for what, kw in shared + (("list > max_query_k", dict(lst=kmax + 1)),):
            assert fixed(**kw) == -2, what
            untouched(what)
        for what, kw in shared + (("list > 1024", dict(lst=1025)), ("dists NULL", dict(d=None))):
            assert exact(**kw) != 0, what
            untouched(what)
        assert fixed(ycnt=0) == 0 and exact(ycnt=0) == 0
        untouched("ycnt == 0")
        # Python: ValueError before or from the library
        for bad in (dict(k=True), dict(k=1.5), dict(k=0), dict(per_group=0), dict(per_group=False), dict(group=0), dict(group=2 ** 32),
                    dict(group=3.0), dict(candidates=3, k=4), dict(candidates=True), dict(candidates=4.0), dict(oversample=0),
                    dict(oversample=True), dict(where=(qm,))):
            kw = dict(group=GMASK, k=4)
            kw.update(bad)
            with pytest.raises(ValueError):
                ix.query_grouped(ty, **kw)
            with pytest.raises(ValueError):
                ix.exact_query_grouped(ty, **kw)
        with pytest.raises(ValueError):
            ix.query_grouped(ty, GMASK, k=4, candidates=kmax + 1)
        with pytest.raises(ValueError):
            ix.exact_query_grouped(ty, GMASK, k=4, candidates=1025)
        # an accepted call writes all four, and the defaults hold: k = the index's, candidates = 4 k
        assert fixed(m=qm.data_ptr(), lo=ql.data_ptr(), hi=qh.data_ptr()) == 0
        torch.cuda.synchronize()
        assert bool((ids >= 0).all()) and bool((dd >= 0).all()) and bool((cc >= 0).all()) and bool((ss <= 1).all())
        got = _npall(ix.query_grouped(ty, GMASK))
        li, ld, _ = ix.query(ty, k=4 * KG)
        _eq4(got, collapse_model(li.cpu().numpy(), ld.cpu().numpy(), w["tags"], GMASK, KG, 1, n, n), "defaults")
        e0 = ix.exact_query_grouped(ty[:0], GMASK)
        assert tuple(e0[0].shape) == (0, KG) and tuple(ix.query_grouped(ty[:0], GMASK)[0].shape) == (0, KG)
        # no tags
        ids.fill_(-7), dd.fill_(-7.0), cc.fill_(-7), ss.fill_(9)
        ix.set_tags(None)
        assert fixed() == -2 and exact() != 0
        untouched("no tags")
        with pytest.raises(ValueError):
            ix.query_grouped(ty, GMASK, k=4)
        with pytest.raises(ValueError):
            ix.exact_query_grouped(ty, GMASK, k=4)
        ix.set_tags(w["tags"])
        # fixed mode off: the query refuses; the exact call does not need it
        ix.set_fixed(False)
        assert fixed() == -2
        untouched("fixed mode off")
        with pytest.raises(ValueError):
            ix.query_grouped(ty, GMASK, k=4)
        assert exact() == 0
        ix.set_fixed(True)
        # a resharded index is refused, not aborted on
        ids.fill_(-7), dd.fill_(-7.0), cc.fill_(-7), ss.fill_(9)
        ix.reshard(w["tp"][: n // 2].contiguous(), 0, n // 2)
        assert fixed() == -2 and exact() != 0
        untouched("resharded")
        with pytest.raises(ValueError):
            ix.query_grouped(ty, GMASK, k=4)
        with pytest.raises(ValueError):
            ix.exact_query_grouped(ty, GMASK, k=4)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7: no change elsewhere
def test_the_other_calls_return_their_old_bits_after_a_grouped_call(world):
    ix, ty = world["ix"], world["ty"]
    ws, st = ix.workspace(), torch.cuda.Stream()

    def run(call, **kw):  # (a call on a stream of its own returns before its results are there)
        out = call(ty, **kw)
        torch.cuda.synchronize()
        return _npall(v for v in out if isinstance(v, torch.Tensor))

    for kw in ({}, {"ws": ws, "stream": st}):
        before_k = run(ix.query, k=40, **kw)[:2]
        before = run(ix.query, **kw)[:2]
        g1 = run(ix.query_grouped, group=GMASK, k=10, candidates=256, **kw)
        after_k = run(ix.query, k=40, **kw)[:2]
        after = run(ix.query, **kw)[:2]
        # the grouped call's list lives in buffers of its own: a plain call in between does not disturb the next grouped one
        g2 = run(ix.query_grouped, group=GMASK, k=10, candidates=256, **kw)
        for a, b in ((before_k, after_k), (before, after)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))
        _eq4(g2, g1, "grouped again")
    # without a dists array the distances go to the workspace and the ids are the same
    ids = torch.full((Q, 10), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert ix.lib.annhip_query_grouped(ix.h, None, None, Q, ty.data_ptr(), 0, 256, 10, 1, GMASK, None, None, None, ids.data_ptr(),
                                       None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), g1[0])
