"""GPU: opt-in binary32 point rows of the f64 library (annhip_index_set_rows with ANNHIP_ROWS_F32, include/ann_hip.h).
The contract: every single-device query entry point returns exactly what the reference returns for query(save, f(P), y),
f(P) = the double rows rounded to binary32 and widened back (numpy: P.astype(np.float32).astype(np.float64)); save is
built from the double rows and the queries stay double.  So the oracle checks it unchanged, run on f(P).  Bit-exact ids
and distance bits everywhere."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd.sharded import HipEngine
from oracle import oracle_py as O
from tests.test_layout_table import F64
from tests.util import bits_equal

pytestmark = pytest.mark.gpu


def _f(p):
    with np.errstate(over="ignore", under="ignore"):  # overflow to +-inf and binary32 subnormals are part of the rounding
        return np.ascontiguousarray(np.asarray(p, dtype=np.float64).astype(np.float32).astype(np.float64))


def _data(n, d, Q, seed):
    orc = O.CpuBackend("f64", "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
    assert pts.dtype == np.float64
    return orc, pts, y


def _index(pts, k, T, seed):
    """precomp on the device from the DOUBLE rows; returns (index, torch rows, save dict for the oracle)."""
    tp = torch.from_numpy(pts).cuda()
    O.srandom(seed)
    ix = A.Index.precomp(tp, k, T)
    assert ix.prec == "f64"
    save = ix.export()
    sd = save.to_dict()
    save.free()
    return ix, tp, sd


def _index_cpu(orc, pts, k, T, seed):
    """The same from the oracle's precomp (host): for rows longer than the device precomp's hashing takes (8-byte
    elements: d > 512)."""
    tp = torch.from_numpy(pts).cuda()
    O.srandom(seed)
    _, _, sd = orc.precomp(pts, k, T)
    save = A.Save.from_dict("f64", sd)
    ix = A.Index.from_save(save, tp)
    return ix, tp, sd


def _np(got):
    ids, dd = got
    ids = ids.cpu().numpy().astype(np.uint64) if torch.is_tensor(ids) else np.asarray(ids).astype(np.uint64)
    dd = dd.cpu().numpy() if torch.is_tensor(dd) else np.asarray(dd)
    return ids, dd


def _same(got, want, what):
    ids, dd = _np(got)
    assert dd.dtype == np.float64
    assert np.array_equal(ids, want[0]), "%s: ids differ in %d places" % (what, int(np.sum(ids != want[0])))
    assert bits_equal(dd, want[1]), "%s: distances not bit-identical" % what


# d -> layout code of the f64 library: one row length for every code its query layout table returns
# (tests/test_layout_table.py::F64)
LAYOUTS = sorted(F64.items())


@pytest.mark.parametrize("d,code", LAYOUTS, ids=[str(d) for d, _ in LAYOUTS])
def test_f32_rows_match_the_oracle_on_rounded_rows(d, code):
    assert A._lib.load("f64").annhip_layout_code(d) == code
    n, k, T, Q = (2000, 5, 3, 64) if d > 1000 else (3000, 10, 5, 300)
    orc, pts, y = _data(n, d, Q, 6300 + d)
    ix, tp, sd = _index_cpu(orc, pts, k, T, 17) if d > 512 else _index(pts, k, T, 17)
    try:
        fp = _f(pts)
        want = orc.query(sd, fp, y)
        ty = torch.from_numpy(y).cuda()
        ix.set_rows("f32")
        assert ix.rows == "f32"
        for mode in (0, 1):  # selection path with exact fallback / exact path for every query
            _same(ix.query(ty, mode=mode)[:2], want, "d=%d (code %d) mode %d" % (d, code, mode))
        qa = 100
        want_a = orc.query(sd, fp, qa, alias=True)  # alias: query x excludes point x; the oracle's form needs y = f(P)
        tf = torch.from_numpy(fp[:qa].copy()).cuda()
        for mode in (0, 1):
            _same(ix.query(tf, alias=True, mode=mode)[:2], want_a, "d=%d alias mode %d" % (d, mode))
    finally:
        ix.close()


@pytest.mark.parametrize("d,k,Q,alias", [(128, 33, 200, False), (40, 33, 150, True), (128, 10, 2500, False),
                                         (48, 10, 2300, True), (100, 10, 2100, False), (64, 10, 40, False),
                                         (64, 10, 40, True), (256, 33, 2200, False)])
def test_f32_rows_stage2_forms_and_batch_sizes(d, k, Q, alias):
    """k = 33: stage-2 rows longer than the fused kernel's LDS row (stage2_select_kernel); Q > 2048: stage 1 and the
    fused stage-2 kernel as separate launches; small Q: stage 2 in the tail of the stage-1 workgroup.  Aliased
    (y = the first Q rows of f(P), query x excludes point x) and not."""
    orc, pts, y = _data(4000, d, Q, 7300 + d + k)
    ix, tp, sd = _index(pts, k, 6, 23)
    try:
        fp = _f(pts)
        if alias:
            want = orc.query(sd, fp, Q, alias=True)
            ty = torch.from_numpy(fp[:Q].copy()).cuda()
        else:
            want = orc.query(sd, fp, y)
            ty = torch.from_numpy(y).cuda()
        ix.set_rows("f32")
        for mode in (0, 1):
            _same(ix.query(ty, alias=alias, mode=mode)[:2], want, "d=%d k=%d Q=%d mode %d" % (d, k, Q, mode))
    finally:
        ix.close()


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_f32_rows_ties_take_the_exact_and_tie_paths(fuse, monkeypatch):
    """Small-integer rows are exact in binary32 and give exact distance ties (2 % of the rows also exist twice): the
    results equal the oracle, and the statistics show flagged queries and tie-path answers on binary32 rows."""
    monkeypatch.setenv("ANN_HIP_FUSE", fuse)
    A._lib.reload_env()
    n, d, k, T, Q = 6000, 32, 10, 6, 600
    rng = np.random.default_rng(31)
    pts = rng.integers(-30, 31, size=(n, d)).astype(np.float64)
    src = rng.choice(n, size=n // 50, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(n), src), size=src.size, replace=False)
    pts[dst] = pts[src]
    y = rng.integers(-30, 31, size=(Q, d)).astype(np.float64)
    y[:100] = pts[src[:100]] + rng.integers(-1, 2, size=(100, d)).astype(np.float64)
    pts, y = np.ascontiguousarray(pts), np.ascontiguousarray(y)
    assert np.array_equal(_f(pts), pts)
    orc = O.CpuBackend("f64", "oracle")
    ix, tp, sd = _index(pts, k, T, 41)
    try:
        ix.set_rows("f32")
        ix.stats(reset=True)
        _same(ix.query(torch.from_numpy(y).cuda())[:2], orc.query(sd, pts, y), "integer rows")
        _same(ix.query(tp[:500].contiguous(), alias=True)[:2], orc.query(sd, pts, 500, alias=True), "integer rows, alias")
        torch.cuda.synchronize()
        st = ix.stats()
        assert st["exact_queries"] > 0 and st["tie_queries"] > 0, st
    finally:
        ix.close()
        monkeypatch.delenv("ANN_HIP_FUSE")
        A._lib.reload_env()


def test_f32_rows_where_rounding_moves_neighbours():
    """Rows with a large common offset, P = 1000 + 1e-3 N(0,1), queries likewise: rounding to binary32 (spacing 6.1e-5
    at 1000) moves neighbours, so the answers on f(P) differ from those on P in ids, not only in low distance bits
    (oracle, n=4000 d=128 k=10 T=6 Q=300: 29 % of the ids).  An implementation that rounds the wrong way or keeps
    reading the native rows fails on ids."""
    n, d, k, T, Q = 4000, 128, 10, 6, 300
    orc, pts, y = _data(n, d, Q, 7700)
    pts = np.ascontiguousarray(1000.0 + 1e-3 * pts)
    y = np.ascontiguousarray(1000.0 + 1e-3 * y)
    ix, tp, sd = _index(pts, k, T, 29)
    try:
        want_n, want_f = orc.query(sd, pts, y), orc.query(sd, _f(pts), y)
        share = float(np.mean(want_n[0] != want_f[0]))
        print("oracle: share of result ids that differ between query(P) and query(f(P)): %.4f" % share)
        assert share > 0.05, share  # the data does what it is here for
        ty = torch.from_numpy(y).cuda()
        nat = _np(ix.query(ty)[:2])
        _same(nat, want_n, "native rows")
        ix.set_rows("f32")
        for mode in (0, 1):
            got = _np(ix.query(ty, mode=mode)[:2])
            _same(got, want_f, "offset rows mode %d" % mode)
            assert not np.array_equal(got[0], nat[0]), "binary32 rows answered as native rows"
            assert float(np.mean(got[0] != nat[0])) > 0.05
    finally:
        ix.close()


def _edge_scale(rng, rows, d):
    """A scale per element, about 10^U(-50, 45): a row exponent U(-48, 43) plus an element exponent U(-2, 2).  The row
    part keeps a row's elements within a few decades of each other, so that rows near 1e-42 have distances BUILT from
    binary32 subnormals (under one exponent per element alone the largest element of a row would swamp them)."""
    return 10.0 ** (rng.uniform(-48, 43, size=(rows, 1)) + rng.uniform(-2, 2, size=(rows, d)))


@pytest.mark.parametrize("d", [128, 40, 33])
def test_f32_rows_conversion_edges(d):
    """Elements across the binary32 range and beyond: some become binary32 subnormals, some flush to +-0, some overflow
    to +-inf.  Results equal the oracle on numpy's astype(np.float32) rows.  That this pins the rounding of subnormals is
    checked on the oracle first: its answers contain finite distances to rows with subnormal elements, and they change
    when those elements are flushed to zero or truncated instead of rounded to nearest."""
    n, k, T, Q = 3000, 10, 5, 300
    orc, pts, y = _data(n, d, Q, 8300 + d)
    rng = np.random.default_rng(d)
    pts = np.ascontiguousarray(pts * _edge_scale(rng, n, d))
    y = np.ascontiguousarray(y * _edge_scale(rng, Q, d))
    fp = _f(pts)
    a = np.abs(fp)
    tiny = float(np.finfo(np.float32).tiny)
    sub = (a > 0) & (a < tiny)
    assert np.isinf(a).any() and sub.any() and ((a == 0) & (pts != 0)).any() and ((a >= 1) & np.isfinite(a)).any()
    ix, tp, sd = _index(pts, k, T, 5)
    try:
        want = orc.query(sd, fp, y)
        # the precondition: finite answers that rest on subnormal elements, and that move under a wrong conversion
        hit = want[0] < n
        rows_hit = want[0][hit].astype(np.int64)
        assert (np.isfinite(want[1][hit]) & sub[rows_hit].any(axis=1)).any()
        flushed = np.where(sub, 0.0, fp)
        assert not bits_equal(orc.query(sd, flushed, y)[1], want[1]), "flushing subnormals would go unnoticed"
        with np.errstate(over="ignore", under="ignore"):
            f32 = pts.astype(np.float32)
            over = np.abs(f32.astype(np.float64)) > np.abs(pts)  # rounded away from zero: step back = truncation
            trunc = np.where(over, np.nextafter(f32, np.float32(0)), f32).astype(np.float64)
        assert not bits_equal(orc.query(sd, np.ascontiguousarray(trunc), y)[1], want[1])
        ix.set_rows("f32")
        ty = torch.from_numpy(y).cuda()
        for mode in (0, 1):
            _same(ix.query(ty, mode=mode)[:2], want, "edges d=%d mode %d" % (d, mode))
        assert ix.lib.annhip_index_rows(ix.h) == 2
    finally:
        ix.close()


def test_f32_rows_toggle_back_is_bit_identical():
    orc, pts, y = _data(4000, 128, 400, 9100)
    ix, tp, sd = _index(pts, 10, 6, 3)
    try:
        ty = torch.from_numpy(y).cuda()
        want, want_f = orc.query(sd, pts, y), orc.query(sd, _f(pts), y)
        first = _np(ix.query(ty)[:2])
        _same(first, want, "native")
        ix.set_rows("f32")
        _same(ix.query(ty)[:2], want_f, "f32")
        ix.set_rows("native")
        assert ix.rows == "native"
        last = _np(ix.query(ty)[:2])
        _same(last, want, "native again")
        assert np.array_equal(first[0], last[0]) and bits_equal(first[1], last[1])
        # the second enable does not reconvert: the copy is the one made by the first (the native rows have changed since)
        tp.mul_(2.0)
        torch.cuda.synchronize()
        ix.set_rows("f32")
        _same(ix.query(ty)[:2], want_f, "f32 again, from the kept copy")
    finally:
        ix.close()


@pytest.mark.parametrize("d", [128, 40])
def test_f32_rows_other_entry_points(d):
    """annhip_query_on (own workspace and stream), annhip_stream_* (HostStream) and annhip_query_slice over two slices
    (the replica sequence of sharded.py: annhip_sh_codes, then one codes array for the whole batch)."""
    n, k, T, Q = 4000, 10, 6, 500
    orc, pts, y = _data(n, d, Q, 9300 + d)
    ix, tp, sd = _index(pts, k, T, 9)
    try:
        ix.set_rows("f32")
        fp = _f(pts)
        want = orc.query(sd, fp, y)
        ty = torch.from_numpy(y).cuda()
        ws, st = ix.workspace(), torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = ix.query(ty, ws=ws, stream=st)
        st.synchronize()
        _same(got[:2], want, "query_on")
        hs = ix.host_stream(max_ycnt=Q, lanes=2)  # a batch is answered as a whole (Q2): one oracle call per batch
        parts = list(hs.map([y, y[:200], y]))
        hs.close()
        for got, w in zip(parts, (want, orc.query(sd, fp, y[:200]), want)):
            _same(got, w, "HostStream")
        eng = HipEngine(ix)
        codes = torch.empty((Q * T,), dtype=torch.int32, device="cuda")
        with eng.use(None):
            eng.sh_codes(ty, 0, Q, codes)
        ids = torch.empty((Q, k), dtype=torch.int64, device="cuda")
        dd = torch.empty((Q, k), dtype=torch.float64, device="cuda")
        h = 230
        for q_lo, nq in ((0, h), (h, Q - h)):
            ix.lib.annhip_query_slice(ix.h, None, None, Q, q_lo, nq, ty[q_lo:].data_ptr(), codes.data_ptr(), 0,
                                      ids[q_lo:].data_ptr(), dd[q_lo:].data_ptr())
        torch.cuda.synchronize()
        _same((ids, dd), want, "query_slice")
    finally:
        ix.close()


def _codes_of(eng, ty, T):
    codes = torch.empty((ty.shape[0], T), dtype=torch.int32, device="cuda")
    with eng.use(None):
        eng.sh_codes(ty, 0, ty.shape[0], codes)
    torch.cuda.synchronize()
    return codes.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _brute(save, pts, y, codes, k):
    """k smallest distinct (distance, id) among the candidates of the fixed mode, both stages; float64 arithmetic
    (as in tests/test_gpu_fixed_mode.py)."""
    n, T, ds = len(pts), save["tries"], save["d_short"]
    graph = np.asarray(save["graph"]).reshape(n, k)
    out_i, out_d = [], []
    for x in range(len(y)):
        cand = []
        for t in range(T):
            tab = np.asarray(save["which_par"][t]).reshape(1 << ds, -1)
            c = int(codes[x, t])
            for yy in range(ds + 1):
                row = tab[c ^ ((1 << (yy - 1)) if yy else 0)]
                cand.append(row[row < n])
        cand = np.unique(np.concatenate(cand)).astype(np.int64)

        def best(ids):
            dd = ((pts[ids] - y[x]) ** 2).sum(1)
            o = np.lexsort((ids, dd))[:k]
            return ids[o], dd[o]
        top, _ = best(cand)
        c2 = np.unique(np.concatenate([top, graph[top].reshape(-1)])).astype(np.int64)
        c2 = c2[c2 < n]
        i2, d2 = best(c2)
        out_i.append(i2), out_d.append(d2)
    return out_i, out_d


def test_f32_rows_with_fixed_mode():
    """set_fixed + binary32 rows: the exact top-k of the candidate sets, on f(P).  The rows carry a common offset so that
    the top-k on f(P) is not the top-k on P.  Tolerance: both sides sum d = 64 non-negative float64 terms, each term
    within 3 roundings of exact, in different orders: relative error below (d + 3) * 2^-53 = 7.4e-15 each; 1e-12 (the
    bound tests/test_gpu_fixed_mode.py uses for f64 is 1e-9) leaves two decades of margin and is seven decades below the
    effect of the rounding to binary32 on this data."""
    n, d, k, T = 5000, 64, 10, 6
    orc, pts, y = _data(n, d, 60, 9500)
    pts = np.ascontiguousarray(1000.0 + 1e-3 * pts)
    y = np.ascontiguousarray(1000.0 + 1e-3 * y)
    ix, tp, sd = _index(pts, k, T, 13)
    try:
        fp = _f(pts)
        ty = torch.from_numpy(y).cuda()
        eng = HipEngine(ix)
        ix.set_fixed(True)
        ix.set_rows("f32")
        codes = _codes_of(eng, ty, T)
        ids, dd, _ = ix.query(ty)
        ids, dd = ids.cpu().numpy(), dd.cpu().numpy()
        want_i, want_d = _brute(sd, fp, y, codes, k)
        nat_i, _ = _brute(sd, pts, y, codes, k)
        assert any(not np.array_equal(a, b) for a, b in zip(want_i, nat_i))  # f(P) matters here
        tol = 1e-12
        for x in range(60):
            m = len(want_i[x])
            assert np.allclose(dd[x, :m], want_d[x], rtol=tol, atol=0), (x, dd[x], want_d[x])
            assert np.all(np.isinf(dd[x, m:])) and np.all(ids[x, m:] == n)
            same = ids[x, :m] == want_i[x]
            if not same.all():  # a different id only where two candidates are (nearly) equally far
                bad = np.flatnonzero(~same)
                gd = ((fp[ids[x, bad]] - y[x]) ** 2).sum(1)
                assert np.allclose(gd, want_d[x][bad], rtol=tol * 10, atol=0)
            assert len(set(ids[x, :m].tolist())) == m
    finally:
        ix.close()


def test_f32_rows_drop_in_switch():
    """ANN_HIP_ROWS=f32 + annhip_reload_env(): query() (query_gpu, resident index) answers as the oracle on f(P); unset +
    reload: on P again; and once more each way (the copy is kept)."""
    orc, pts, y = _data(4000, 40, 300, 9700)
    pts = np.ascontiguousarray(1000.0 + 1e-3 * pts)
    y = np.ascontiguousarray(1000.0 + 1e-3 * y)
    O.srandom(19)
    _, _, save = A.precomp(pts, 10, 6)
    old = os.environ.pop("ANN_HIP_ROWS", None)
    try:
        sd = save.to_dict()
        want_n, want_f = orc.query(sd, pts, y), orc.query(sd, _f(pts), y)
        assert not np.array_equal(want_n[0], want_f[0])
        A._lib.reload_env()
        _same(A.query(save, pts, y), want_n, "ANN_HIP_ROWS unset (first)")
        for _ in range(2):
            os.environ["ANN_HIP_ROWS"] = "f32"
            A._lib.reload_env()
            _same(A.query(save, pts, y), want_f, "ANN_HIP_ROWS=f32")
            del os.environ["ANN_HIP_ROWS"]
            A._lib.reload_env()
            _same(A.query(save, pts, y), want_n, "ANN_HIP_ROWS unset")
        os.environ["ANN_HIP_ROWS"] = "f32"
        A._lib.reload_env()
        _same(A.query(save, pts, y), want_f, "ANN_HIP_ROWS=f32")
        os.environ["ANN_HIP_ROWS"] = "f16"  # not this library's narrow type: a warning, native rows (also right after f32)
        A._lib.reload_env()
        _same(A.query(save, pts, y), want_n, "ANN_HIP_ROWS=f16 in the f64 library")
    finally:
        if old is None:
            os.environ.pop("ANN_HIP_ROWS", None)
        else:
            os.environ["ANN_HIP_ROWS"] = old
        A._lib.reload_env()
        A._lib.load("f64").annhip_cache_clear()
        save.free()


def test_f32_rows_refusals():
    """f32 index with "f32" or code 2, f64 index with "f16" or code 1, a resharded f64 index, unknown values: refused,
    the setting and the results unchanged.  reshard of an index with binary32 rows returns it to native rows."""
    o32 = O.CpuBackend("f32", "oracle")
    O.srandom(77)
    o32.rand_norm_reset()
    n, d, k, T = 3000, 32, 10, 4
    p32 = np.ascontiguousarray(o32.gen_rand(n * d).reshape(n, d))
    y32 = torch.from_numpy(np.ascontiguousarray(o32.gen_rand(200 * d).reshape(200, d))).cuda()
    t32 = torch.from_numpy(p32).cuda()
    O.srandom(3)
    ix32 = A.Index.precomp(t32, k, T)
    try:
        assert ix32.prec == "f32"
        before = _np(ix32.query(y32)[:2])
        for bad in ("f32", 2):
            with pytest.raises(ValueError):
                ix32.set_rows(bad)
            assert ix32.rows == "native"
        assert ix32.lib.annhip_index_set_rows(ix32.h, C.c_int(2)) == -1
        assert ix32.lib.annhip_index_rows(ix32.h) == 0
        ix32.set_rows("native")  # always accepted
        after = _np(ix32.query(y32)[:2])
        assert np.array_equal(before[0], after[0]) and bits_equal(before[1], after[1])
        ix32.set_rows("f16")  # refusing the other library's type leaves its own in place
        with pytest.raises(ValueError):
            ix32.set_rows("f32")
        assert ix32.rows == "f16"
    finally:
        ix32.close()

    orc, pts, y = _data(n, d, 200, 9900)
    pts = np.ascontiguousarray(1000.0 + 1e-3 * pts)
    y = np.ascontiguousarray(1000.0 + 1e-3 * y)
    ix, tp, sd = _index(pts, k, T, 7)
    try:
        ty = torch.from_numpy(y).cuda()
        want_n, want_f = orc.query(sd, pts, y), orc.query(sd, _f(pts), y)
        assert not np.array_equal(want_n[0], want_f[0])
        for bad in ("f16", 1, 7, -1, "bf16", None):  # refused while native
            with pytest.raises(ValueError):
                ix.set_rows(bad)
            assert ix.rows == "native"
        assert ix.lib.annhip_index_set_rows(ix.h, C.c_int(1)) == -1
        _same(ix.query(ty)[:2], want_n, "native after refusals")
        ix.set_rows("f32")
        for bad in ("f16", 1, 7, "bf16"):  # refused while binary32
            with pytest.raises(ValueError):
                ix.set_rows(bad)
            assert ix.rows == "f32"
        assert ix.lib.annhip_index_set_rows(ix.h, C.c_int(7)) == -1
        assert ix.lib.annhip_index_rows(ix.h) == 2
        _same(ix.query(ty)[:2], want_f, "f32 after refusals")
        # point-sharded: rows [lo, hi) only -> native rows, and binary32 refused
        lo, hi = 1000, 2000
        shard = tp[lo:hi].contiguous()
        ix.reshard(shard, lo, hi)
        assert ix.rows == "native"
        for bad in ("f32", 2):
            with pytest.raises(ValueError):
                ix.set_rows(bad)
            assert ix.rows == "native"
        ix.set_rows("native")
    finally:
        ix.close()
