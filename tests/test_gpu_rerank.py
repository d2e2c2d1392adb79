"""GPU: rerank -- the exact top-k of caller-supplied candidates on native rows (annhip_rerank, annhip_index_rerank;
include/ann_hip.h, ann_rerank_kernels.h).

Every check is bit-exact on ids and distance bytes; no tolerance.  The expectation never runs the new kernel.  It is numpy,
per query: drop the ids >= rows (compared as unsigned 64-bit values), np.unique, distances by np_dists
(tests/test_gpu_exact_knn.py: the reference's halving tree, pinned to the oracle there) on the native rows,
np.lexsort((id, distance bits)), the first k, padded with (rows, +inf).  Shapes: the seven kernel families of
tests/test_gpu_tail.py at n = 1500, Q = 37."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd import _lib
from oracle import oracle_py as O
from tests.test_gpu_exact_knn import lattice, np_dists
from tests.test_gpu_query_k import _np, _same_bits, _tenants
from tests.test_gpu_tail import SHAPES, Q, _bits, _rows

pytestmark = pytest.mark.gpu

N = 1500
FAMILIES = [(prec, d, kg, T) for prec, _, d, kg, T in SHAPES]
IDS = ["%s-d%d" % (p, d) for p, d, _, _ in FAMILIES]
CS = (1, 63, 64, 65, 257, 1024)


def expect(dist, cand, k, rows):
    """dist [Q, rows] (np_dists), cand int64 [Q, C] -> the contract's (ids int64 [Q, k], dists [Q, k])"""
    Qn = cand.shape[0]
    ids = np.full((Qn, k), rows, dtype=np.int64)
    dd = np.full((Qn, k), np.inf, dtype=dist.dtype)
    for q in range(Qn):
        c = cand[q].view(np.uint64)
        u = np.unique(c[c < np.uint64(rows)]).astype(np.int64)
        dq = dist[q][u]
        o = np.lexsort((u, _bits(dq)))[:k]
        ids[q, :len(o)], dd[q, :len(o)] = u[o], dq[o]
    return ids, dd


def same(got, want, what):
    gi, gd = (got[0].cpu().numpy(), got[1].cpu().numpy()) if torch.is_tensor(got[0]) else got
    bad = np.nonzero((gi != want[0]).any(axis=1))[0]
    assert bad.size == 0, "%s: ids differ for %d queries, first %d: got %s want %s" % (
        what, bad.size, bad[0], gi[bad[0]][:12], want[0][bad[0]][:12])
    assert gd.dtype == want[1].dtype and np.array_equal(_bits(gd), _bits(want[1])), "%s: distances not bit-identical" % what


def salted(rng, Qn, C, rows):
    """Lists drawn with replacement from [0, rows), a tenth of the entries replaced by rows (the pad), -1 and 2^32 + 5; then
    the special queries: 0 all pads, 1 one id C times, 2 a duplicate inside its first 64-entry block, 3 a duplicate more
    than 256 positions apart (C > 300), 4 three distinct valid ids and pads."""
    cand = rng.integers(0, rows, size=(Qn, C)).astype(np.int64)
    salt = np.array([rows, -1, 2 ** 32 + 5], dtype=np.int64)
    hit = rng.random((Qn, C)) < 0.1
    cand[hit] = salt[rng.integers(0, 3, size=int(hit.sum()))]
    cand[0] = rows
    cand[1] = 5
    if C >= 2:
        cand[2, 0] = 11
        cand[2, 1] = 11
    if C > 300:
        cand[3, 5] = 12
        cand[3, 300] = 12
    cand[4] = rows
    cand[4, :3] = [7, 3, 7] if C >= 3 else 7
    return np.ascontiguousarray(cand)


def _valid(row, rows):
    c = row.view(np.uint64)
    return c[c < np.uint64(rows)].astype(np.int64)


def _dup_within(row, rows, lo, hi):
    """a valid id occurs twice at positions inside [lo, hi)"""
    v = _valid(row[lo:hi], rows)
    return len(np.unique(v)) < len(v)


def _dup_far(row, rows, gap):
    c = row.view(np.uint64)
    pos = {}
    for i, x in enumerate(c.tolist()):
        if x < rows:
            if x in pos and i - pos[x] > gap:
                return True
            pos.setdefault(x, i)
    return False


# ------------------------------------------------------------------------------------------ 1: against numpy
@pytest.mark.parametrize("prec,d,kg,T", FAMILIES, ids=IDS)
def test_against_numpy(prec, d, kg, T):
    pts, y = _rows(prec, N, d, 7300 + d), _rows(prec, Q, d, 7301 + d)
    tp, ty = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda()
    dist = np_dists(pts, y)
    rng = np.random.default_rng(7302 + d)
    seen = dict(near=False, far=False, short=False, pads=False, copies=False, big=False)
    for C in CS:
        cand = salted(rng, Q, C, N)
        tc = torch.from_numpy(cand).cuda()
        seen["near"] |= any(_dup_within(cand[q], N, 0, 64) for q in range(Q))
        seen["far"] |= any(_dup_far(cand[q], N, 256) for q in range(Q))
        seen["pads"] |= bool((cand[0] == N).all())
        seen["copies"] |= C == 1024 and bool((cand[1] == 5).all())
        seen["big"] |= bool((cand == 2 ** 32 + 5).any()) and bool((cand == -1).any())
        for k in sorted({1, 10, C, 1024}):
            seen["short"] |= any(len(np.unique(_valid(cand[q], N))) < k for q in range(Q))
            want = expect(dist, cand, k, N)
            assert (want[0][0] == N).all() and np.isinf(want[1][0]).all()  # the list of pads gives a row of pads
            assert want[0][1].tolist() == [5] + [N] * (k - 1)
            got = A.rerank(tp, ty, tc, k)
            assert got[0].dtype == torch.int64 and tuple(got[0].shape) == (Q, k) and got[1].dtype == ty.dtype
            same(got, want, "%s d=%d C=%d k=%d" % (prec, d, C, k))
    assert all(seen.values()), seen


# ------------------------------------------------------------------------------------------ 2: identity with the query path
def _index(prec, d, kg, T, seed, n=N, rows=None):
    pts = _rows(prec, n, d, seed) if rows is None else rows
    tp = torch.from_numpy(pts).cuda()
    _lib.load(prec)
    torch.cuda.synchronize()
    O.srandom(seed + 1)
    ix = A.Index.precomp(tp, kg, T)
    ix.set_fixed(True)
    return pts, tp, ix


@pytest.mark.parametrize("prec,d,kg,T", FAMILIES, ids=IDS)
def test_rerank_of_a_query_row_is_that_row(prec, d, kg, T):
    pts, tp, ix = _index(prec, d, kg, T, 7400 + d)
    try:
        ix.set_probe(3)
        ty = torch.from_numpy(_rows(prec, Q, d, 7402 + d)).cuda()
        ta = tp[:Q].contiguous()

        def identity(what):
            lists = []
            for kq in (1, kg, 100):
                for yy, alias in ((ty, False), (ta, True)):
                    ids, dd, _ = ix.query(yy, alias=alias, k=kq)
                    got = ix.rerank(yy, ids, kq)
                    assert _same_bits(_np(got), _np((ids, dd))), (what, kq, alias)
                    lists.append(ids.cpu().numpy())
            return lists

        identity("built rows")
        tail = _rows(prec, 700, d, 7403 + d)
        ix.append(tail[:400])
        ix.hash_tail()
        ix.append(tail[400:])
        assert ix.tail == 700 and ix.tail_hashed == 400 and ix.n_total == N + 700
        lists = identity("with a tail")
        big = lists[-2]  # kq = 100, not aliased
        assert (big < N).any() and ((big >= N) & (big < N + 400)).any() and ((big >= N + 400) & (big < N + 700)).any()
        # and the index call against numpy over the built rows and the tail, duplicates and pads included
        rows = N + 700
        allp = np.concatenate([pts, tail])
        assert np.array_equal(ix.rows_tensor(0, rows).cpu().numpy().view(np.uint8), allp.view(np.uint8))
        y = ty.cpu().numpy()
        dist = np_dists(allp, y)
        cand = salted(np.random.default_rng(7404 + d), Q, 257, rows)
        assert (cand == rows).any() and ((cand >= N) & (cand < rows)).any()
        for k in (10, 257):
            same(ix.rerank(ty, torch.from_numpy(cand).cuda(), k), expect(dist, cand, k, rows), "index call k=%d" % k)
        assert ix.rerank(ty, torch.from_numpy(cand).cuda())[0].shape[1] == kg  # k=None: the index's k
        ix.set_fixed(False)  # rerank does not need fixed mode
        assert ix.n_total == rows
        same(ix.rerank(ty, torch.from_numpy(cand[:, :64].copy()).cuda(), 10), expect(dist, cand[:, :64], 10, rows), "fixed mode off")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 3: all rows
@pytest.mark.parametrize("prec,d,kg,T", FAMILIES, ids=IDS)
def test_all_rows_is_exact_knn(prec, d, kg, T):
    n = 700
    pts, y = _rows(prec, n, d, 7500 + d), _rows(prec, Q, d, 7501 + d)
    tp, ty = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda()
    rng = np.random.default_rng(7502 + d)
    cand = np.stack([rng.permutation(n) for _ in range(Q)]).astype(np.int64)
    for k in (1, 10, 700):
        want = A.exact_knn(tp, ty, k)
        got = A.rerank(tp, ty, torch.from_numpy(cand).cuda(), k)
        assert _same_bits(_np(got), _np(want)), k


# ------------------------------------------------------------------------------------------ 4: narrow rows
@pytest.mark.parametrize("prec,narrow", [("f32", "f16"), ("f64", "f32")])
def test_narrow_candidates_are_rescored_on_the_native_rows(prec, narrow):
    n, d, k, T, Qn = 3000, 128, 10, 5, 100
    pts = np.ascontiguousarray((1000.0 + 1e-3 * _rows("f64", n, d, 7600)).astype(pts_dtype(prec)))
    y = np.ascontiguousarray((1000.0 + 1e-3 * _rows("f64", Qn, d, 7601)).astype(pts_dtype(prec)))
    _, tp, ix = _index(prec, d, k, T, 7602, rows=pts)
    try:
        ty = torch.from_numpy(y).cuda()
        nat = ix.query(ty, k=k)[0].cpu().numpy()
        ix.set_rows(narrow)
        nar_ids, nar_d, _ = ix.query(ty, k=k)
        differ = (nar_ids.cpu().numpy() != nat).any(axis=1)
        assert differ.any(), "the narrow rows answer as the native rows: the data does not do what it is here for"
        dist = np_dists(pts, y)
        got = ix.rerank(ty, nar_ids, k)
        same(got, expect(dist, nar_ids.cpu().numpy(), k, n), "narrow candidates")
        assert not np.array_equal(_bits(got[1].cpu().numpy()), _bits(nar_d.cpu().numpy()))  # native distances, not narrow ones
        wide = ix.query(ty, k=3 * k)[0]
        want = ix.rerank(ty, wide, k)
        same(want, expect(dist, wide.cpu().numpy(), k, n), "oversampled candidates")
        assert _same_bits(_np(ix.query_reranked(ty, k, oversample=3)), _np(want))
        assert _same_bits(_np(ix.query_reranked(ty, oversample=3)), _np(want))  # k=None: the index's k
        assert _same_bits(_np(ix.query_reranked(ty, k, oversample=1)), _np(got))
        assert ix.rows == narrow
    finally:
        ix.close()


def pts_dtype(prec):
    return np.float32 if prec == "f32" else np.float64


# ------------------------------------------------------------------------------------------ 5: ties and infinity
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ties_on_the_integer_lattice(prec):
    n, d = 1500, 32
    pts, y = lattice(prec, n, d, Q, 7700)
    pts[900] = pts[5]
    pts[1499] = pts[5]
    y[0] = pts[5]
    dist = np_dists(pts, y)
    rng = np.random.default_rng(7701)
    cand = rng.integers(0, n, size=(Q, 600)).astype(np.int64)
    cand[0, :3] = [1499, 5, 900]
    want = expect(dist, cand, 10, n)
    tied = sum(len(set(row.tolist())) < 10 for row in want[1])
    assert tied >= Q - 5, tied  # nearly every row has equal distances: a wrong tie order cannot pass
    assert want[0][0][:3].tolist() == [5, 900, 1499]
    tp, ty, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(cand).cuda()
    same(A.rerank(tp, ty, tc, 10), want, "lattice")
    for k in (1, 2):  # a tie exactly at rank k
        same(A.rerank(tp, ty, tc, k), expect(dist, cand, k, n), "lattice k=%d" % k)


def test_overflow_to_inf_sorts_last_by_id_and_before_the_pads():
    n, d = 500, 32
    pts, y = _rows("f32", n, d, 7710), _rows("f32", 6, d, 7711)
    far = [3, 17, 200, 499]
    pts[far] = np.float32(3e19)
    pts[far, ::2] = np.float32(-3e19)
    dist = np_dists(pts, y)
    cand = np.stack([np.random.default_rng(7712 + q).permutation(n)[:60] for q in range(6)]).astype(np.int64)
    cand[:, 10:14] = [499, 200, 17, 3]
    cand[:, 20:30] = n  # pads: fewer than 64 distinct valid ids
    want = expect(dist, cand, 64, n)
    nv = [len(np.unique(_valid(cand[q], n))) for q in range(6)]
    for q in range(6):
        assert want[0][q][nv[q] - 4:nv[q]].tolist() == far and np.isinf(want[1][q][nv[q] - 4:]).all()
        assert (want[0][q][nv[q]:] == n).all() and nv[q] < 64
    same(A.rerank(torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(cand).cuda(), 64), want, "inf")


# ------------------------------------------------------------------------------------------ 6: no validity rules
def test_forbidden_and_untagged_candidates_are_scored():
    prec, d, kg, T = "f32", 64, 10, 6
    pts, tp, ix = _index(prec, d, kg, T, 7800)
    try:
        allow = np.arange(N) % 2 == 0
        ix.set_filter(allow)
        tags, where = _tenants(N, Q, 7801)
        ix.set_tags(tags)
        ta = tp[:Q].contiguous()  # aliased queries: the query itself is a candidate too
        ids, _, _ = ix.query(ta, alias=True, k=20, where=where)
        got_ids = ids.cpu().numpy()
        assert ((got_ids % 2 == 0) | (got_ids >= N)).all() and not (got_ids == np.arange(Q)[:, None]).any()
        forbidden = np.stack([np.random.default_rng(7802 + q).permutation(N // 2)[:50] * 2 + 1 for q in range(Q)]).astype(np.int64)
        forbidden[:, 0] = np.arange(Q)  # the query's own row
        forbidden[:, 1] = 1  # an odd row for everyone, whatever its tenant
        assert not allow[forbidden[:, 1:]].any()
        dist = np_dists(pts, pts[:Q])
        want = expect(dist, forbidden, 40, N)
        assert (want[0] < N).all() and (want[0][:, 0] == np.arange(Q)).all()
        same(ix.rerank(ta, torch.from_numpy(forbidden).cuda(), 40), want, "forbidden ids")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7: in place and streams
@pytest.mark.parametrize("prec,d,kg,T", [FAMILIES[0], FAMILIES[5]], ids=[IDS[0], IDS[5]])
def test_in_place_streams_and_batch_sizes(prec, d, kg, T):
    pts, tp, ix = _index(prec, d, kg, T, 7900 + d)
    try:
        ty = torch.from_numpy(_rows(prec, Q, d, 7901)).cuda()
        rng = np.random.default_rng(7902)
        for C in (kg, 100):
            cand = salted(rng, Q, C, N)
            out_of_place = _np(ix.rerank(ty, torch.from_numpy(cand).cuda(), C))
            tc = torch.from_numpy(cand).cuda()
            ids, dd = ix.rerank(ty, tc, C, out_ids=tc)
            assert ids is tc and _same_bits(_np((ids, dd)), out_of_place)
            tc = torch.from_numpy(cand).cuda()
            ids, dd = A.rerank(tp, ty, tc, C, out_ids=tc)
            assert ids is tc and _same_bits(_np((ids, dd)), out_of_place)
        # two streams, their own outputs
        cands = [torch.from_numpy(salted(rng, Q, 257, N)).cuda() for _ in range(2)]
        null = [_np(ix.rerank(ty, c, 33)) for c in cands]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(2)]
        outs = [ix.rerank(ty, c, 33, stream=s) for c, s in zip(cands, streams)]
        for s in streams:
            s.synchronize()
        for o, w in zip(outs, null):
            assert _same_bits(_np(o), w)
        with torch.cuda.stream(streams[0]):  # the stand-alone call runs on the current stream
            o = A.rerank(tp, ty, cands[0], 33)
        streams[0].synchronize()
        assert _same_bits(_np(o), null[0])
        # Q = 0 and Q = 1
        e = ix.rerank(ty[:0], cands[0][:0], 5)
        assert tuple(e[0].shape) == (0, 5) and tuple(e[1].shape) == (0, 5) and e[0].dtype == torch.int64
        e = A.rerank(tp, ty[:0], cands[0][:0], 5)
        assert tuple(e[0].shape) == (0, 5) and tuple(e[1].shape) == (0, 5)
        one = ix.rerank(ty[:1].contiguous(), cands[0][:1].contiguous(), 33)
        assert _same_bits(_np(one), (null[0][0][:1], null[0][1][:1]))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_leave_the_outputs_untouched():
    prec, d, kg, T = "f32", 64, 10, 6
    pts, tp, ix = _index(prec, d, kg, T, 8000)
    try:
        ty = torch.from_numpy(_rows(prec, 4, d, 8001)).cuda()

        def refused(call, k, C, cand=None):
            ids = torch.full((4, k), -7, dtype=torch.int64, device="cuda")
            dd = torch.full((4, k), -7.0, dtype=torch.float32, device="cuda")
            tc = torch.zeros((4, C), dtype=torch.int64, device="cuda") if cand is None else cand
            with pytest.raises(ValueError):
                call(tc, k, ids, dd)
            torch.cuda.synchronize()
            assert (ids == -7).all() and (dd == -7.0).all()

        index_call = lambda tc, k, ids, dd: ix.rerank(ty, tc, k, out_ids=ids, out_dists=dd)  # noqa: E731
        plain_call = lambda tc, k, ids, dd: A.rerank(tp, ty, tc, k, out_ids=ids, out_dists=dd)  # noqa: E731
        for call in (index_call, plain_call):
            refused(call, 0, 8)
            refused(call, 1025, 8)
            refused(call, 5, 0)
            refused(call, 5, 1025)
            refused(call, 5, 8, cand=torch.zeros((4, 8), dtype=torch.float32, device="cuda"))
            refused(call, 5, 8, cand=torch.zeros((4, 8), dtype=torch.int32, device="cuda"))
            refused(call, 5, 8, cand=torch.zeros((4, 16), dtype=torch.int64, device="cuda")[:, ::2])  # not contiguous
            refused(call, 5, 8, cand=torch.zeros((3, 8), dtype=torch.int64, device="cuda"))  # not one row per query
            refused(call, 5, 8, cand=torch.zeros((4, 8), dtype=torch.int64))  # not on the device
        for bad in (True, 2.0, "5"):
            with pytest.raises(ValueError):
                ix.rerank(ty, torch.zeros((4, 8), dtype=torch.int64, device="cuda"), bad)
        # the library itself: -1, nothing launched
        lib = _lib.load(prec)
        ids = torch.full((4, 5), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((4, 5), -7.0, dtype=torch.float32, device="cuda")
        tc = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
        args = (ty.data_ptr(), 8, tc.data_ptr())
        assert lib.annhip_rerank(N, 0, tp.data_ptr(), 4, *args, 5, ids.data_ptr(), dd.data_ptr(), None) == -1  # d == 0
        assert lib.annhip_rerank(0xFFFFFFF0, d, tp.data_ptr(), 4, *args, 5, ids.data_ptr(), dd.data_ptr(), None) == -1
        assert lib.annhip_rerank(N, d, tp.data_ptr(), 0, *args, 5, ids.data_ptr(), dd.data_ptr(), None) == 0  # ycnt == 0
        assert lib.annhip_index_rerank(ix.h, None, 4, *args, 1025, ids.data_ptr(), dd.data_ptr()) == -1
        torch.cuda.synchronize()
        assert (ids == -7).all() and (dd == -7.0).all()
        # mixed and unsupported dtypes of the stand-alone call
        with pytest.raises(ValueError):
            A.rerank(tp, ty.double(), tc, 5)
        with pytest.raises(ValueError):
            A.rerank(tp.half(), ty.half(), tc, 5)
        # a row that no carve-up of one CU's LDS holds (any-d kernel: query + tree scratch = 2 rows of 240 000 bytes)
        long_p = torch.zeros((3, 30000), dtype=torch.float64, device="cuda")
        out_i = torch.full((4, 2), -7, dtype=torch.int64, device="cuda")
        out_d = torch.full((4, 2), -7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            A.rerank(long_p, torch.zeros((4, 30000), dtype=torch.float64, device="cuda"), tc, 2, out_ids=out_i, out_dists=out_d)
        torch.cuda.synchronize()
        assert (out_i == -7).all() and (out_d == -7.0).all()
        # oversample
        for bad in (0, -1, 1.5, "2", True):
            with pytest.raises(ValueError):
                ix.query_reranked(ty, 5, oversample=bad)
        ix.query_reranked(ty, 5, oversample=1)
        ix.set_fixed(False)  # query_reranked needs fixed mode, as query(k=) does
        with pytest.raises(ValueError):
            ix.query_reranked(ty, 5)
        ix.set_fixed(True)
        # a resharded index
        shard = tp[500:1000].contiguous()
        ix.reshard(shard, 500, 1000)
        refused(index_call, 5, 8)
    finally:
        ix.close()
