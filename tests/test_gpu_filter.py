"""GPU: the allow-list row filter of fixed mode and of the exact scan (annhip_index_set_filter, annhip_exact_knn_filtered;
include/ann_hip.h).  A filter narrows what fixed mode calls a valid id, so it is checked against that sentence: an
all-ones filter changes nothing, a filtered query equals an unfiltered query of an index whose tables and graph had the
disallowed ids taken out, both equal a float64 brute force over the contract's candidate sets restricted to the mask, and
the gathered-row counter shows that the test happens before a row is fetched.  Helpers follow tests/test_gpu_probe.py."""
import itertools

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd.sharded import HipEngine
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

SHAPES = [("f64", 3000, 32, 5, 4), ("f32", 5000, 64, 10, 6), ("f64", 2500, 80, 8, 3), ("f64", 2000, 16, 33, 2),
          ("f32", 2500, 33, 6, 3), ("f32", 2000, 100, 6, 3), ("f64", 1500, 300, 5, 2)]  # + unaligned, folded, any-d hash


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


def _brute(save, pts, y, codes, k, ranked, allow, alias_ids=None):
    """k smallest distinct (distance, id) among the ALLOWED candidates of fixed mode with pair bits, both stages; float64.
    Also the number of allowed valid ids over the probed buckets (repeats across tries counted, self included)."""
    n, T, ds = len(pts), save["tries"], save["d_short"]
    graph = np.asarray(save["graph"]).reshape(n, k)
    tabs = [np.asarray(save["which_par"][t]).reshape(1 << ds, -1) for t in range(T)]
    p64 = pts.astype(np.float64)
    out_i, out_d, handed = [], [], 0
    for x in range(len(y)):
        cand = []
        for t in range(T):
            c = int(codes[x, t])
            for m in _masks(ds, ranked[x][t]):
                row = tabs[t][c ^ m]
                row = row[row < n].astype(np.int64)
                row = row[allow[row]]
                handed += len(row)
                cand.append(row)
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
        c2 = c2[allow[c2]]
        if alias_ids is not None:
            c2 = c2[c2 != alias_ids[x]]
        i2, d2 = best(c2)
        out_i.append(i2), out_d.append(d2)
    return out_i, out_d, handed


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


def _allow_masks(n, k, seed):
    """Random masks with allowed share 0.5 and 0.05 from a fixed seed, and one that leaves fewer than k rows allowed."""
    rng = np.random.default_rng(seed)
    few = np.zeros(n, dtype=bool)
    few[rng.choice(n, size=max(1, k - 2), replace=False)] = True
    return [("0.5", rng.random(n) < 0.5), ("0.05", rng.random(n) < 0.05), ("few", few)]


def _ranked(ix, ty):
    if ix.probe:
        return ix.probe_bits(ty)[1].cpu().numpy()
    return np.zeros((ty.shape[0], ix.tries, 0), dtype=np.uint8)


# ------------------------------------------------------------------------------------------ 1: all-ones is a no-op
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_all_ones_filter_returns_the_unfiltered_bits(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 6100 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        ix.set_fixed(True)
        ix.profile(1)
        for b in (0, 3, "all"):
            ix.set_probe(b)
            ix.set_filter(None)
            assert ix.filter_count is None
            ix.stats(reset=True)
            plain = _np(ix.query(ty))
            torch.cuda.synchronize()
            rows_plain = ix.stats(reset=True)["s1_rows"]
            plain_a = _np(ix.query(ta, alias=True))
            ix.set_filter(np.ones(n, dtype=bool))
            assert ix.filter_count == n
            ix.stats(reset=True)
            got = _np(ix.query(ty))
            torch.cuda.synchronize()
            rows_ones = ix.stats(reset=True)["s1_rows"]
            assert _same_bits(got, plain), b
            assert _same_bits(_np(ix.query(ta, alias=True)), plain_a), b
            assert rows_ones == rows_plain, (b, rows_ones, rows_plain)  # every valid id is handed to the gather, as before
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 2: an edited index
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_filtered_query_equals_a_query_of_the_index_without_the_disallowed_ids(prec, n, d, k, T):
    """Every disallowed id in the bucket tables and in the graph replaced by the sentinel n gives the same candidate sets
    without a filter: ids and distance bytes must be equal."""
    orc, pts, tp, ix = _build(prec, n, d, k, T, 6200 + d)
    ix2 = None
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        save = ix.export()
        sd = save.to_dict()
        save.free()
        ix.set_fixed(True)
        for name, allow in _allow_masks(n, k, 62):
            ed = dict(sd)
            lut = np.where(allow, np.arange(n, dtype=np.uint64), np.uint64(n))
            lut = np.concatenate([lut, np.full(1, n, dtype=np.uint64)])
            ed["which_par"] = [lut[np.minimum(np.asarray(w), n).astype(np.int64)] for w in sd["which_par"]]
            ed["graph"] = lut[np.minimum(np.asarray(sd["graph"]), n).astype(np.int64)]
            save2 = A.Save.from_dict(prec, ed)
            ix2 = A.Index.from_save(save2, tp)
            ix2.set_fixed(True)
            ix.set_filter(allow)
            for b in (0, 3, "all"):
                ix.set_probe(b), ix2.set_probe(b)
                got, want = _np(ix.query(ty)), _np(ix2.query(ty))
                assert _same_bits(got, want), (name, b)
                if name == "few":  # fewer than k candidates: both pad with (n, +inf), in the f64 library too
                    assert np.all(want[0][:, -1] == n) and np.all(np.isinf(want[1][:, -1])), (name, b)
                got, want_a = _np(ix.query(ta, alias=True)), _np(ix2.query(ta, alias=True))
                assert _same_bits(got, want_a), (name, b, "alias")
                # the edited tables have no sorted-prefix layout: a filter on THEM runs the slot-scan form of the filtered
                # stage 1.  The same mask, and all-ones, remove nothing more.
                for again in (allow, np.ones(n, dtype=bool)):
                    ix2.set_filter(again)
                    assert _same_bits(_np(ix2.query(ty)), want), (name, b, "slot scan")
                    assert _same_bits(_np(ix2.query(ta, alias=True)), want_a), (name, b, "slot scan, alias")
                ix2.set_filter(None)
            ix2.close()
            ix2 = None
    finally:
        if ix2 is not None:
            ix2.close()
        ix.close()


@pytest.mark.parametrize("prec,d", [("f32", 64), ("f64", 32), ("f32", 80)])
def test_other_kernel_forms_give_the_same_filtered_results(prec, d, monkeypatch):
    """A table scanned without segment words (ANN_HIP_SLOT_SCAN, read when the index is made) and other wave counts per
    query (ANN_HIP_S1_WAVES): the filtered results and the gathered-row counter are the same, bit for bit."""
    n, k, T = 4000, 9, 5
    allow = np.random.default_rng(66).random(n) < 0.5

    def run():
        orc, pts, tp, ix = _build(prec, n, d, k, T, 6600 + d)
        try:
            ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(150 * d).reshape(150, d))).cuda()
            ix.set_fixed(True)
            ix.set_filter(allow)
            ix.profile(1)
            out = []
            for b in (0, 4):
                ix.set_probe(b)
                ix.stats(reset=True)
                out.append(_np(ix.query(ty)))
                out.append(_np(ix.query(tp[:100].contiguous(), alias=True)))
                torch.cuda.synchronize()
                out.append(ix.stats(reset=True)["s1_rows"])
            return out
        finally:
            ix.close()
    want = run()
    for env in ({"ANN_HIP_SLOT_SCAN": "1"}, {"ANN_HIP_S1_WAVES": "1"}, {"ANN_HIP_S1_WAVES": "3"}):
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        A._lib.reload_env()
        try:
            got = run()
        finally:
            for kk in env:
                monkeypatch.delenv(kk)
            A._lib.reload_env()
        for g, w in zip(got, want):
            assert (g == w) if not isinstance(w, tuple) else _same_bits(g, w), env


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_unfiltered_fixed_mode_pads_with_n_and_inf_where_fewer_than_k_candidates_exist(prec):
    """No filter anywhere: an index whose tables and graph hold k - 2 ids only.  Fixed mode promises (n, +inf) in the
    tail.  The f64 library used to return (4294967295, NaN) there: its largest key, key_max(), carried a 64-bit id half
    that did not survive the 32-bit lane exchange of wave_min_key(), so wave_select_smallest() never saw "nothing left"."""
    n, d, k, T = 2000, 32, 8, 3
    orc, pts, tp, ix = _build(prec, n, d, k, T, 6650)
    ix2 = None
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        save = ix.export()
        sd = save.to_dict()
        save.free()
        keep = np.zeros(n, dtype=bool)
        keep[np.random.default_rng(6650).choice(n, size=k - 2, replace=False)] = True
        lut = np.concatenate([np.where(keep, np.arange(n, dtype=np.uint64), np.uint64(n)), np.full(1, n, dtype=np.uint64)])
        ed = dict(sd)
        ed["which_par"] = [lut[np.minimum(np.asarray(w), n).astype(np.int64)] for w in sd["which_par"]]
        ed["graph"] = lut[np.minimum(np.asarray(sd["graph"]), n).astype(np.int64)]
        ix2 = A.Index.from_save(A.Save.from_dict(prec, ed), tp)
        ix2.set_fixed(True)
        for b in (0, 3, "all"):
            ix2.set_probe(b)
            for yy, alias in ((ty, False), (tp[:60].contiguous(), True)):
                ids, dd = _np(ix2.query(yy, alias=alias))
                assert not np.isnan(dd).any(), (b, alias)
                assert np.all(ids <= n) and keep[ids[ids < n]].all(), (b, alias)
                pad = ids == n
                assert pad[:, -2:].all() and np.all(np.isinf(dd[pad])) and np.all(np.isfinite(dd[~pad])), (b, alias)
                assert np.all(pad[:, :-1] <= pad[:, 1:]), (b, alias)  # the padding is a tail
    finally:
        if ix2 is not None:
            ix2.close()
        ix.close()


# ------------------------------------------------------------------------------------------ 3 + 4: brute force, counter
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_filtered_query_is_the_exact_top_k_of_the_allowed_candidates(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 6300 + d)
    try:
        y = np.ascontiguousarray(orc.gen_rand(50 * d).reshape(50, d))
        ty, ta = torch.from_numpy(y).cuda(), tp[:40].contiguous()
        save = ix.export()
        sd = save.to_dict()
        save.free()
        eng = HipEngine(ix)
        ix.set_fixed(True)
        ix.profile(1)
        codes, codes_a = _codes_of(eng, ty, T), _codes_of(eng, ta, T)
        tol = 1e-9 if prec == "f64" else 2e-5
        for name, allow in _allow_masks(n, k, 63):
            ix.set_filter(allow)
            assert ix.filter_count == int(allow.sum())
            for b in (0, 3, "all"):
                ix.set_probe(b)
                ix.stats(reset=True)
                got = _np(ix.query(ty))
                torch.cuda.synchronize()
                rows = ix.stats(reset=True)["s1_rows"]
                wi, wd, handed = _brute(sd, pts, y, codes, k, _ranked(ix, ty), allow)
                print("%s share %s b %r: stage-1 rows %d, brute-force count of allowed valid ids %d" % (prec, name, b, rows, handed))
                _check_topk(got[0], got[1], wi, wd, pts, y, n, tol)
                assert rows == handed, (name, b, rows, handed)  # 4: the filter acts before the gather (exact, an integer)
                assert allow[got[0][got[0] < n]].all()
                if name == "few":
                    assert np.all(got[0][:, -1] == n) and np.all(np.isinf(got[1][:, -1]))
                ix.stats(reset=True)
                got_a = _np(ix.query(ta, alias=True))
                torch.cuda.synchronize()
                rows_a = ix.stats(reset=True)["s1_rows"]
                wi, wd, handed_a = _brute(sd, pts, pts[:40], codes_a, k, _ranked(ix, ta), allow, alias_ids=np.arange(40))
                _check_topk(got_a[0], got_a[1], wi, wd, pts, pts[:40], n, tol)
                assert rows_a == handed_a, (name, b, rows_a, handed_a)  # (the query itself is counted when it is allowed)
                assert allow[got_a[0][got_a[0] < n]].all()
                for x in range(40):
                    assert x not in got_a[0][x].tolist()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 5: exact k-NN
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("d", [128, 80, 100, 300])
def test_exact_knn_over_the_allowed_rows(prec, d, monkeypatch):
    n, Q = 3000, 70
    dt = torch.float32 if prec == "f32" else torch.float64
    g = torch.Generator().manual_seed(640 + d)
    pts = torch.randn((n, d), generator=g, dtype=torch.float64).to(dt).cuda()
    y = torch.randn((Q, d), generator=g, dtype=torch.float64).to(dt).cuda()
    rng = np.random.default_rng(64)
    for share in (0.5, 0.05):
        m = torch.from_numpy(rng.random(n) < share).cuda()
        back = torch.nonzero(m).reshape(-1)
        sub = pts[m].contiguous()
        for k in (1, 10, 100):
            want_i, want_d = A.exact_knn(sub, y, k)
            got_i, got_d = A.exact_knn(pts, y, k, allow=m)
            assert torch.equal(got_i, back[want_i]) and torch.equal(got_d.view(torch.uint8), want_d.view(torch.uint8)), (share, k)
            monkeypatch.setenv("ANN_HIP_EXACT_RANGES", "3")  # another split of the rows changes nothing
            A._lib.reload_env()
            try:
                r_i, r_d = A.exact_knn(pts, y, k, allow=m)
            finally:
                monkeypatch.delenv("ANN_HIP_EXACT_RANGES")
                A._lib.reload_env()
            assert torch.equal(r_i, got_i) and torch.equal(r_d.view(torch.uint8), got_d.view(torch.uint8)), (share, k)
        # self_exclude with y = points: the query's own row is left out, allowed or not
        yq = pts[:Q].contiguous()
        got_i, got_d = A.exact_knn(pts, yq, 10, self_exclude=True, allow=m)
        full_i, full_d = A.exact_knn(pts, yq, 11, allow=m)
        for q in range(Q):
            keep = full_i[q] != q
            assert torch.equal(got_i[q], full_i[q][keep][:10]) and torch.equal(got_d[q], full_d[q][keep][:10])
            assert q not in got_i[q].tolist()
    # fewer than k allowed rows: the (n, +inf) tail
    few = torch.zeros(n, dtype=torch.bool)
    few[torch.from_numpy(rng.choice(n, size=7, replace=False))] = True
    few = few.cuda()
    got_i, got_d = A.exact_knn(pts, y, 10, allow=few)
    want_i, want_d = A.exact_knn(pts[few].contiguous(), y, 7)
    assert torch.equal(got_i[:, :7], torch.nonzero(few).reshape(-1)[want_i]) and torch.equal(got_d[:, :7], want_d)
    assert torch.all(got_i[:, 7:] == n) and torch.all(torch.isinf(got_d[:, 7:]))
    # allow=None is today's call; an all-ones mask gives its bits too
    a, b = A.exact_knn(pts, y, 10), A.exact_knn(pts, y, 10, allow=None)
    c = A.exact_knn(pts, y, 10, allow=torch.ones(n, dtype=torch.bool, device="cuda"))
    for o in (b, c):
        assert torch.equal(a[0], o[0]) and torch.equal(a[1].view(torch.uint8), o[1].view(torch.uint8))
    with pytest.raises(ValueError):
        A.exact_knn(pts, y, 10, allow=torch.ones(n - 1, dtype=torch.bool, device="cuda"))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_index_exact_query_honours_the_filter(prec):
    orc, pts, tp, ix = _build(prec, 4000, 64, 10, 4, 6500)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(90 * 64).reshape(90, 64))).cuda()
        plain = ix.exact_query(ty)
        allow = np.random.default_rng(65).random(4000) < 0.5
        ix.set_fixed(True)
        ix.set_filter(allow)
        m = torch.from_numpy(allow).cuda()
        for alias, yy in ((False, ty), (True, tp[:90].contiguous())):
            got = ix.exact_query(yy, alias=alias)
            want = A.exact_knn(tp, yy, 10, self_exclude=alias, allow=m)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.uint8), want[1].view(torch.uint8))
        ix.set_filter(None)
        again = ix.exact_query(ty)
        assert torch.equal(again[0], plain[0]) and torch.equal(again[1].view(torch.uint8), plain[1].view(torch.uint8))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 6: recall
def test_recall_is_stated_against_the_filtered_truth():
    """The probe test's recipe (n = 20000, d = 32, k = 10, T = 10, 300 queries, seeds 777 / 778) with half the rows allowed:
    recall_at_k(filtered query, filtered exact_query) equals the float64 model's recall on the library's own bits -- at most
    2 of the 3 000 neighbours may differ (the probe test's allowance for an f32 near-tie at the k-th place: a condition, not
    a measurement) -- and rises strictly with b."""
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
        save.free()
        allow = np.random.default_rng(777).random(n) < 0.5
        eng = HipEngine(ix)
        ix.set_fixed(True)
        ix.set_filter(allow)
        truth, _ = ix.exact_query(ty)
        assert allow[truth.cpu().numpy()].all()
        codes = _codes_of(eng, ty, T)
        recalls = []
        for b in (0, 5, "all"):
            ix.set_probe(b)
            ids = ix.query(ty)[0].cpu()
            wi, _, _ = _brute(sd, pts, y, codes, k, _ranked(ix, ty), allow)
            model = torch.from_numpy(np.stack(wi))
            differ = sum(len(set(ids[x].tolist()) ^ set(wi[x].tolist())) // 2 for x in range(Q))
            r_lib, r_model = A.recall_at_k(ids, truth.cpu()), A.recall_at_k(model, truth.cpu())
            print("share 0.5, pair bits %r: recall@10 library %.4f, float64 model on the library's bits %.4f, neighbours that "
                  "differ %d" % (b, r_lib, r_model, differ))
            assert differ <= 2 and abs(r_lib - r_model) <= 2.0 / (Q * k) + 1e-12, (b, r_lib, r_model, differ)
            recalls.append(r_lib)
        assert recalls[0] < recalls[1] < recalls[2], recalls
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7: refusals and lifecycle
def test_refusals_and_lifecycle():
    n = 5000
    orc, pts, tp, ix = _build("f32", n, 64, 10, 6, 6700)
    try:
        y = np.ascontiguousarray(orc.gen_rand(120 * 64).reshape(120, 64))
        ty = torch.from_numpy(y).cuda()
        save = ix.export()
        sd = save.to_dict()
        save.free()
        want = orc.query(sd, pts, y)
        allow = np.random.default_rng(67).random(n) < 0.5
        with pytest.raises(ValueError):  # fixed mode is off
            ix.set_filter(allow)
        assert ix.filter_count is None
        ix.set_filter(None)              # clearing is always accepted
        ix.set_fixed(True)
        plain = _np(ix.query(ty))
        for bad in (allow[:-1], np.ones(n + 1, dtype=bool), torch.ones(n - 1, dtype=torch.bool, device="cuda"),
                    allow.tolist(), torch.from_numpy(allow)):  # neither an ndarray nor a device tensor
            with pytest.raises(ValueError):
                ix.set_filter(bad)
            assert ix.filter_count is None
        ix.set_filter(allow)
        assert ix.filter_count == int(allow.sum())
        from_numpy = _np(ix.query(ty))
        assert not _same_bits(from_numpy, plain)
        ix.set_filter(torch.from_numpy(allow).cuda())   # a device bool tensor and a numpy array give the same results
        assert ix.filter_count == int(allow.sum())
        assert _same_bits(_np(ix.query(ty)), from_numpy)
        ix.set_filter(torch.from_numpy(allow.astype(np.uint8)).cuda())
        assert _same_bits(_np(ix.query(ty)), from_numpy)
        with pytest.raises(ValueError):  # a refused call leaves the setting as it was
            ix.set_filter(allow[:-1])
        assert ix.filter_count == int(allow.sum()) and _same_bits(_np(ix.query(ty)), from_numpy)
        ix.set_filter(None)
        assert ix.filter_count is None and _same_bits(_np(ix.query(ty)), plain)
        ix.set_filter(allow)
        ix.set_fixed(False)              # leaving fixed mode drops the filter: parity mode returns the reference's bytes
        assert ix.filter_count is None
        ids0, dd0, _ = ix.query(ty)
        assert np.array_equal(ids0.cpu().numpy().astype(np.uint64), want[0])
        assert np.array_equal(dd0.cpu().numpy().view(np.uint8), want[1].view(np.uint8))
        ix.set_fixed(True)
        assert ix.filter_count is None and _same_bits(_np(ix.query(ty)), plain)
        ix.set_filter(allow)             # a resharded index drops the filter and refuses a new one
        half = tp[: n // 2].contiguous()
        ix.reshard(half, 0, n // 2)
        assert ix.filter_count is None
        with pytest.raises(ValueError):
            ix.set_filter(allow)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 8: composition
@pytest.mark.parametrize("prec,rows,narrow", [("f32", "f16", np.float16), ("f64", "f32", np.float32)])
def test_filter_composes_with_narrow_rows(prec, rows, narrow):
    n, d, k, T = 4000, 64, 7, 4
    orc, pts, tp, ix = _build(prec, n, d, k, T, 6800)
    try:
        y = np.ascontiguousarray(orc.gen_rand(60 * d).reshape(60, d))
        ty = torch.from_numpy(y).cuda()
        save = ix.export()
        sd = save.to_dict()
        save.free()
        eng = HipEngine(ix)
        ix.set_fixed(True)
        codes = _codes_of(eng, ty, T)
        allow = np.random.default_rng(68).random(n) < 0.5
        ix.set_filter(allow)
        tol = 1e-9 if prec == "f64" else 2e-5
        for b in (0, 4):
            ix.set_probe(b)
            ix.set_rows(rows)
            got = _np(ix.query(ty))
            rounded = pts.astype(narrow).astype(pts.dtype)
            wi, wd, _ = _brute(sd, rounded, y, codes, k, _ranked(ix, ty), allow)
            _check_topk(got[0], got[1], wi, wd, rounded, y, n, tol)
            assert allow[got[0][got[0] < n]].all()
            ix.set_rows("native")
            got = _np(ix.query(ty))
            wi, wd, _ = _brute(sd, pts, y, codes, k, _ranked(ix, ty), allow)
            _check_topk(got[0], got[1], wi, wd, pts, y, n, tol)
    finally:
        ix.close()


def test_filter_on_workspaces_streams_and_host_streams():
    n = 6000
    orc, pts, tp, ix = _build("f32", n, 64, 10, 6, 6900)
    try:
        ya = np.ascontiguousarray(orc.gen_rand(700 * 64).reshape(700, 64))
        yb = np.ascontiguousarray(orc.gen_rand(300 * 64).reshape(300, 64))
        ta, tb = torch.from_numpy(ya).cuda(), torch.from_numpy(yb).cuda()
        ix.set_fixed(True)
        ix.set_filter(np.random.default_rng(69).random(n) < 0.5)
        for b in (0, 5):
            ix.set_probe(b)
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
