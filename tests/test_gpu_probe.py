"""GPU: query-directed multi-probe, the recall knob of fixed mode (annhip_index_set_probe; include/ann_hip.h).  Like fixed
mode itself it has no counterpart in the reference, so it is checked against what it promises: the ranking against
float64 projections, the results against a brute force (numpy, float64) over exactly the buckets the contract lists, the
whole Hamming-2 ball without any ranking, and recall against the exact neighbours.  Helpers follow
tests/test_gpu_fixed_mode.py."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd.sharded import HipEngine
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


def _build(prec, n, d, k, T, seed):
    orc = O.CpuBackend(prec, "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    O.srandom(seed + 1)
    tp = torch.from_numpy(pts).cuda()
    ix = A.Index.precomp(tp, k, T)
    return orc, pts, tp, ix


def pts_bytes(prec):
    return 4 if prec == "f32" else 8


def _build_host(prec, n, d, k, T, seed):
    """_build with the tables and the graph from the oracle's precomp on the host (the device's are bit-identical to them):
    for rows of more than 4096 bytes, which the device precomp's hashing kernel has no room for."""
    orc = O.CpuBackend(prec, "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    tp = torch.from_numpy(pts).cuda()
    O.srandom(seed + 1)
    ix = A.Index.from_save(A.Save.from_dict(prec, orc.precomp(pts, k, T)[2]), tp)
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


def _brute(save, pts, y, codes, k, ranked, alias_ids=None):
    """k smallest distinct (distance, id) among the candidates of fixed mode with pair bits, both stages; float64.
    ranked[x][t] = the projection indices whose pairs are flipped (the library's own bits, or range(ds) for the ball)."""
    n, T, ds = len(pts), save["tries"], save["d_short"]
    graph = np.asarray(save["graph"]).reshape(n, k)
    tabs = [np.asarray(save["which_par"][t]).reshape(1 << ds, -1) for t in range(T)]
    p64 = pts.astype(np.float64)
    out_i, out_d = [], []
    for x in range(len(y)):
        cand = []
        for t in range(T):
            c = int(codes[x, t])
            for m in _masks(ds, ranked[x][t]):
                row = tabs[t][c ^ m]
                cand.append(row[row < n])
        cand = np.unique(np.concatenate(cand)).astype(np.int64)
        if alias_ids is not None:
            cand = cand[cand != alias_ids[x]]

        def best(ids):
            dd = ((p64[ids] - y[x].astype(np.float64)) ** 2).sum(1)
            o = np.lexsort((ids, dd))[:k]
            return ids[o], dd[o]
        top, _ = best(cand)
        c2 = np.unique(np.concatenate([top, graph[top].reshape(-1)])).astype(np.int64)
        c2 = c2[c2 < n]
        if alias_ids is not None:
            c2 = c2[c2 != alias_ids[x]]
        i2, d2 = best(c2)
        out_i.append(i2), out_d.append(d2)
    return out_i, out_d


def _check_topk(ids, dd, want_i, want_d, pts, y, n, tol):
    """The assertions of test_fixed_mode_is_the_exact_top_k_of_its_candidate_sets."""
    for x in range(len(y)):
        m = len(want_i[x])
        assert np.allclose(dd[x, :m], want_d[x], rtol=tol, atol=0), (x, dd[x], want_d[x])
        assert np.all(np.isinf(dd[x, m:])) and np.all(ids[x, m:] == n)
        same = ids[x, :m] == want_i[x]
        if not same.all():   # a different id only where two candidates are (nearly) equally far
            bad = np.flatnonzero(~same)
            gd = ((pts[ids[x, bad]].astype(np.float64) - y[x]) ** 2).sum(1)
            assert np.allclose(gd, want_d[x][bad], rtol=tol * 10, atol=0)
        assert len(set(ids[x, :m].tolist())) == m


def _np(t):
    return tuple(v.cpu().numpy() for v in t[:2])


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_zero_pair_bits_is_todays_fixed_mode(prec):
    orc, pts, tp, ix = _build(prec, 4000, 64, 8, 5, 5100)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(300 * 64).reshape(300, 64))).cuda()
        ix.set_fixed(True)
        assert ix.probe == 0
        fresh = _np(ix.query(ty))
        fresh_a = _np(ix.query(tp[:200].contiguous(), alias=True))
        ix.set_probe(3)
        ix.set_probe(0)
        assert ix.probe == 0
        assert _same_bits(_np(ix.query(ty)), fresh) and _same_bits(_np(ix.query(tp[:200].contiguous(), alias=True)), fresh_a)
        codes = torch.empty((300, ix.tries), dtype=torch.int32, device="cuda")
        bits = torch.empty((300, ix.tries, 1), dtype=torch.uint8, device="cuda")
        assert ix.lib.annhip_probe_bits(ix.h, None, 300, ty.data_ptr(), codes.data_ptr(), bits.data_ptr()) == -1
        with pytest.raises(ValueError):
            ix.probe_bits(ty)
    finally:
        ix.close()


# 100: a folded layout; 300: the any-d hash kernel.  MORE: with the five above, a row length for every layout code of the
# precision (tests/test_layout_table.py checks that none is missing); these run 64 queries, the first five 200.
RANKING_D = [32, 80, 33, 100, 300]
RANKING_MORE = {"f32": [16, 64, 128, 256, 512, 1024, 96, 160, 192, 320, 384, 24, 48, 28, 280, 112, 224, 50, 150, 260, 2084, 40],
                "f64": [16, 64, 128, 256, 512, 40, 48, 96, 160, 192, 12, 24, 20, 14, 28, 56, 112, 36, 150, 2084]}
RANKING_CASES = [(p, d) for d in RANKING_D for p in ("f32", "f64")] + [(p, d) for p in ("f32", "f64") for d in RANKING_MORE[p]]


@pytest.mark.parametrize("prec,d", RANKING_CASES, ids=["%d-%s" % (d, p) for p, d in RANKING_CASES])
def test_ranking_is_the_smallest_projection_magnitudes(prec, d):
    """codes = the hash kernels' codes; bits = the b smallest |projection|, ascending, against float64 projections: two
    magnitudes may swap (or swap across the b-th place) only when they differ by less than the rounding bound of a
    length-d dot product, d * eps * |y - means| * |base| -- an absolute bound (the smallest magnitudes are ~1e-5 of the terms)."""
    T, Q = 4, 200 if d in RANKING_D else 64
    orc, pts, tp, ix = (_build_host if d * pts_bytes(prec) > 4096 else _build)(prec, 3000, d, 5, T, 5200 + d)
    try:
        y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
        ty = torch.from_numpy(y).cuda()
        save = ix.export()
        sd = save.to_dict()
        ds = int(sd["d_short"])
        eng = HipEngine(ix)
        ix.set_fixed(True)
        want_codes = _codes_of(eng, ty, T)
        cen = y.astype(np.float64) - np.asarray(sd["row_means"]).astype(np.float64)
        bases = np.asarray(sd["bases"]).reshape(T, ds, d).astype(np.float64)
        proj = np.einsum("qd,tsd->qts", cen, bases)
        mag = np.abs(proj)
        eps = np.finfo(np.float32 if prec == "f32" else np.float64).eps
        bound = d * eps * np.linalg.norm(cen, axis=1)[:, None, None] * np.linalg.norm(bases, axis=2)[None, :, :]  # [Q,T,ds]
        # the float64 projections are the hash's: their signs are the code bits (a sign may differ inside the bound only)
        code_bit = (want_codes[:, :, None] >> (ds - 1 - np.arange(ds))) & 1
        off = code_bit != np.signbit(proj)
        assert np.all(mag[off] < bound[off]) and off.sum() <= 2, off.sum()
        for b in (1, 4, ds):
            ix.set_probe(b)
            codes, bits = ix.probe_bits(ty)
            assert np.array_equal(codes.cpu().numpy(), want_codes)
            bits = bits.cpu().numpy()
            assert bits.shape == (Q, T, b) and bits.dtype == np.uint8
            relaxed = 0
            for q in range(Q):
                for t in range(T):
                    l = bits[q, t].astype(np.int64)
                    assert l.max() < ds and len(set(l.tolist())) == b, (q, t, l)
                    m, bd = mag[q, t], bound[q, t]
                    for u in range(b - 1):  # ascending
                        if m[l[u]] > m[l[u + 1]]:
                            assert m[l[u]] - m[l[u + 1]] < max(bd[l[u]], bd[l[u + 1]]), (q, t, u, l, m)
                            relaxed += 1
                    rest = np.setdiff1d(np.arange(ds), l)
                    for s in rest:          # nothing left out is smaller than anything listed
                        for v in l:
                            if m[s] < m[v]:
                                assert m[v] - m[s] < max(bd[s], bd[v]), (q, t, s, v, m)
                                relaxed += 1
            print("prec %s d %d b %d: %d of %d (query, try) lists needed the rounding relaxation" % (prec, d, b, relaxed, Q * T))
            assert relaxed <= Q * T // 20  # the relaxation is for a handful of near-ties, not a way to pass
        save.free()
    finally:
        ix.close()


SHAPES = [("f64", 3000, 32, 5, 4), ("f32", 5000, 64, 10, 6), ("f64", 2500, 80, 8, 3), ("f64", 2000, 16, 33, 2),
          ("f32", 2500, 33, 6, 3), ("f32", 2000, 100, 6, 3), ("f64", 1500, 300, 5, 2)]  # + unaligned, folded, any-d hash


@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_probe_is_the_exact_top_k_of_its_candidate_sets(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 4100 + d)
    try:
        y = np.ascontiguousarray(orc.gen_rand(60 * d).reshape(60, d))
        ty, ta = torch.from_numpy(y).cuda(), tp[:50].contiguous()
        save = ix.export()
        sd = save.to_dict()
        ds = int(sd["d_short"])
        eng = HipEngine(ix)
        ix.set_fixed(True)
        codes, codes_a = _codes_of(eng, ty, T), _codes_of(eng, ta, T)
        plain, plain_a = _np(ix.query(ty)), _np(ix.query(ta, alias=True))
        tol = 1e-9 if prec == "f64" else 2e-5
        for b in (1, 3, ds):
            ix.set_probe(b)
            assert ix.probe == b
            got_codes, bits = ix.probe_bits(ty)
            assert np.array_equal(got_codes.cpu().numpy(), codes)
            got, got_a = _np(ix.query(ty)), _np(ix.query(ta, alias=True))
            if b == 1:  # no pair to flip: the new kernels on today's candidate sets
                assert _same_bits(got, plain) and _same_bits(got_a, plain_a)
            wi, wd = _brute(sd, pts, y, codes, k, bits.cpu().numpy())
            _check_topk(got[0], got[1], wi, wd, pts, y, n, tol)
            _, bits_a = ix.probe_bits(ta)
            wi, wd = _brute(sd, pts, pts[:50], codes_a, k, bits_a.cpu().numpy(), alias_ids=np.arange(50))
            _check_topk(got_a[0], got_a[1], wi, wd, pts, pts[:50], n, tol)
            for x in range(50):
                assert x not in got_a[0][x].tolist()
        save.free()
    finally:
        ix.close()


@pytest.mark.parametrize("prec,n,d,k,T", [SHAPES[1], SHAPES[2], SHAPES[4]])
def test_the_whole_ball_needs_no_ranking(prec, n, d, k, T):
    """b = "all": every pair of bits is flipped, so the candidate sets follow from the codes alone."""
    orc, pts, tp, ix = _build(prec, n, d, k, T, 4300 + d)
    try:
        y = np.ascontiguousarray(orc.gen_rand(60 * d).reshape(60, d))
        ty = torch.from_numpy(y).cuda()
        save = ix.export()
        sd = save.to_dict()
        ds = int(sd["d_short"])
        eng = HipEngine(ix)
        ix.set_fixed(True)
        codes = _codes_of(eng, ty, T)
        ix.set_probe("all")
        assert ix.probe == ds
        got = _np(ix.query(ty))
        wi, wd = _brute(sd, pts, y, codes, k, [[range(ds)] * T] * 60)
        _check_topk(got[0], got[1], wi, wd, pts, y, n, 1e-9 if prec == "f64" else 2e-5)
        save.free()
    finally:
        ix.close()


def test_recall_moves_the_way_the_model_says():
    """The issue's recipe (n = 20000, d = 32, k = 10, T = 10, 300 queries; the CPU model gives 0.6930 / 0.8550 / 0.9697 for
    b = 0 / 5 / all).  (i) each recall equals the float64 model's on the library's own bits -- at most 2 of the 3 000
    returned neighbours may differ (a cap for an f32 near-tie at the k-th place, not a measurement); (ii) strictly
    increasing in b."""
    n, d, k, T, Q = 20000, 32, 10, 10, 300
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(777)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
    O.srandom(778)
    tp, ty = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda()
    ix = A.Index.precomp(tp, k, T)
    try:
        save = ix.export()
        sd = save.to_dict()
        ds = int(sd["d_short"])
        truth, _ = ix.exact_query(ty)
        eng = HipEngine(ix)
        ix.set_fixed(True)
        codes = _codes_of(eng, ty, T)
        recalls = []
        for b in (0, 5, "all"):
            ix.set_probe(b)
            ids = ix.query(ty)[0].cpu()
            if ix.probe:
                ranked = ix.probe_bits(ty)[1].cpu().numpy()
            else:
                ranked = np.zeros((Q, T, 0), dtype=np.uint8)
            wi, _ = _brute(sd, pts, y, codes, k, ranked)
            model = torch.from_numpy(np.stack(wi))
            differ = sum(len(set(ids[x].tolist()) ^ set(wi[x].tolist())) // 2 for x in range(Q))
            r_lib, r_model = A.recall_at_k(ids.cpu(), truth.cpu()), A.recall_at_k(model, truth.cpu())
            print("pair bits %r: recall@10 library %.4f, float64 model on the library's bits %.4f, neighbours that differ %d"
                  % (b, r_lib, r_model, differ))
            assert differ <= 2 and abs(r_lib - r_model) <= 2.0 / (Q * k) + 1e-12, (b, r_lib, r_model, differ)
            recalls.append(r_lib)
        assert recalls[0] < recalls[1] < recalls[2], recalls
        save.free()
    finally:
        ix.close()


def test_probe_is_ignored_while_fixed_mode_is_off():
    orc, pts, tp, ix = _build("f32", 5000, 64, 10, 6, 5300)
    try:
        y = np.ascontiguousarray(orc.gen_rand(120 * 64).reshape(120, 64))
        save = ix.export()
        sd = save.to_dict()
        want = orc.query(sd, pts, y)
        ix.set_probe(4)
        ids0, dd0, _ = ix.query(torch.from_numpy(y).cuda())
        assert np.array_equal(ids0.cpu().numpy().astype(np.uint64), want[0])
        assert np.array_equal(dd0.cpu().numpy().view(np.uint8), want[1].view(np.uint8))
        ix.set_fixed(True)   # and after a round trip through fixed mode
        ix.query(torch.from_numpy(y).cuda())
        ix.set_fixed(False)
        ids0, dd0, _ = ix.query(torch.from_numpy(y).cuda())
        assert np.array_equal(ids0.cpu().numpy().astype(np.uint64), want[0])
        assert np.array_equal(dd0.cpu().numpy().view(np.uint8), want[1].view(np.uint8))
        save.free()
    finally:
        ix.close()


@pytest.mark.parametrize("prec,rows,narrow", [("f32", "f16", np.float16), ("f64", "f32", np.float32)])
def test_probe_composes_with_narrow_rows(prec, rows, narrow):
    n, d, k, T = 4000, 64, 7, 4
    orc, pts, tp, ix = _build(prec, n, d, k, T, 5400)
    try:
        y = np.ascontiguousarray(orc.gen_rand(60 * d).reshape(60, d))
        ty = torch.from_numpy(y).cuda()
        save = ix.export()
        sd = save.to_dict()
        eng = HipEngine(ix)
        ix.set_fixed(True)
        codes = _codes_of(eng, ty, T)
        ix.set_probe(4)
        ix.set_rows(rows)
        got = _np(ix.query(ty))
        rounded = pts.astype(narrow).astype(pts.dtype)
        wi, wd = _brute(sd, rounded, y, codes, k, ix.probe_bits(ty)[1].cpu().numpy())
        _check_topk(got[0], got[1], wi, wd, rounded, y, n, 1e-9 if prec == "f64" else 2e-5)
        ix.set_rows("native")
        wi, wd = _brute(sd, pts, y, codes, k, ix.probe_bits(ty)[1].cpu().numpy())
        got = _np(ix.query(ty))
        _check_topk(got[0], got[1], wi, wd, pts, y, n, 1e-9 if prec == "f64" else 2e-5)
        save.free()
    finally:
        ix.close()


def test_probe_on_workspaces_streams_and_host_streams():
    orc, pts, tp, ix = _build("f32", 6000, 64, 10, 6, 5500)
    try:
        ya = np.ascontiguousarray(orc.gen_rand(700 * 64).reshape(700, 64))
        yb = np.ascontiguousarray(orc.gen_rand(300 * 64).reshape(300, 64))
        ta, tb = torch.from_numpy(ya).cuda(), torch.from_numpy(yb).cuda()
        ix.set_fixed(True)
        ix.set_probe(5)
        serial_a, serial_b = _np(ix.query(ta)), _np(ix.query(tb))
        torch.cuda.synchronize()
        w1, w2, s1, s2 = ix.workspace(), ix.workspace(), torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            ga = ix.query(ta, ws=w1, stream=s1)
        with torch.cuda.stream(s2):
            gb = ix.query(tb, ws=w2, stream=s2)
        s1.synchronize(), s2.synchronize()
        assert _same_bits(_np(ga), serial_a) and _same_bits(_np(gb), serial_b)
        hs = ix.host_stream(max_ycnt=700, lanes=2)
        parts = list(hs.map([ya, yb, ya]))
        hs.close()
        for got, want in zip(parts, (serial_a, serial_b, serial_a)):
            assert np.array_equal(got[0].astype(np.int64), want[0]) and np.array_equal(got[1].view(np.uint8), want[1].view(np.uint8))
    finally:
        ix.close()


def test_refused_settings_leave_the_value_unchanged():
    orc, pts, tp, ix = _build("f64", 2000, 32, 5, 3, 5600)
    try:
        ds = ix.d_short
        ix.set_probe(2)
        for bad in (ds + 1, -2, 1000, "some", 2.0, True):
            with pytest.raises(ValueError):
                ix.set_probe(bad)
            assert ix.probe == 2
        ix.set_probe(ds)
        assert ix.probe == ds
        ix.set_probe(-1)
        assert ix.probe == ds
        ix.set_probe(0)
        assert ix.probe == 0
        assert ix.lib.annhip_index_set_probe(ix.h, C.c_int(ds + 1)) == -1 and ix.probe == 0
    finally:
        ix.close()


@pytest.mark.parametrize("prec,d", [("f32", 64), ("f64", 32), ("f32", 80)])
def test_other_kernel_forms_give_the_same_bits_and_results(prec, d, monkeypatch):
    """The lanes-per-row hash kernel where the lane-per-query one is the default (ANN_HIP_CODES_LPQ=0), a table scanned
    without segment words (ANN_HIP_SLOT_SCAN, read when the index is made) and other wave counts per query
    (ANN_HIP_S1_WAVES): same codes, same ranked bits, same results, bit for bit."""
    n, k, T = 4000, 9, 5

    def run():
        orc, pts, tp, ix = _build(prec, n, d, k, T, 5700 + d)
        try:
            ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(150 * d).reshape(150, d))).cuda()
            ix.set_fixed(True)
            ix.set_probe(4)
            codes, bits = ix.probe_bits(ty)
            return (codes.cpu().numpy(), bits.cpu().numpy(), _np(ix.query(ty)), _np(ix.query(tp[:100].contiguous(), alias=True)))
        finally:
            ix.close()
    want = run()
    for env in ({"ANN_HIP_CODES_LPQ": "0"}, {"ANN_HIP_SLOT_SCAN": "1"}, {"ANN_HIP_S1_WAVES": "1"}, {"ANN_HIP_S1_WAVES": "3"}):
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        A._lib.reload_env()
        try:
            got = run()
        finally:
            for kk in env:
                monkeypatch.delenv(kk)
            A._lib.reload_env()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), env
        assert _same_bits(got[2], want[2]) and _same_bits(got[3], want[3]), env


@pytest.mark.parametrize("prec,d", [("f32", 64), ("f64", 16), ("f32", 256), ("f32", 80), ("f64", 33)])
def test_zero_projections_rank_first_in_index_order(prec, d):
    """A query equal to the column means projects to +-0 everywhere: magnitude 0, so the ranking is 0, 1, 2 ... by the
    tie rule (s ascending), whatever the signs of the zeros."""
    ft = np.float32 if prec == "f32" else np.float64
    n, k, T = 4096, 5, 4
    rng = np.random.default_rng(d)
    pts = rng.integers(-3, 4, size=(n, d)).astype(ft)
    pts[:, ::5] = 0
    means = (pts.astype(np.float64).sum(axis=0) / n).astype(ft)  # exact: small integers, n a power of two
    y = pts[rng.integers(0, n, size=100)].copy()
    y[:40] = means
    O.srandom(5)
    ix = A.Index.precomp(torch.from_numpy(np.ascontiguousarray(pts)).cuda(), k, T)
    try:
        ix.set_fixed(True)
        ix.set_probe("all")
        _, bits = ix.probe_bits(torch.from_numpy(np.ascontiguousarray(y)).cuda())
        bits = bits.cpu().numpy()
        assert np.array_equal(bits[:40], np.broadcast_to(np.arange(ix.d_short, dtype=np.uint8), (40, T, ix.d_short)))
        assert all(sorted(bits[q, t].tolist()) == list(range(ix.d_short)) for q in range(100) for t in range(T))
    finally:
        ix.close()
