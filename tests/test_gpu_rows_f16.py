"""GPU: opt-in binary16 point rows (annhip_index_set_rows, include/ann_hip.h).  The contract: with ANNHIP_ROWS_F16 every
single-device query entry point returns exactly what the reference returns for query(save, h(P), y), h(P) = the rows
rounded to binary16 and widened back (numpy: P.astype(np.float16).astype(np.float32)); save is built from the float rows.
So the oracle checks it unchanged, run on h(P).  Bit-exact ids and distance bits everywhere."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd.sharded import HipEngine
from oracle import oracle_py as O
from tests.util import bits_equal

pytestmark = pytest.mark.gpu


def _h(p):
    with np.errstate(over="ignore"):  # overflow to +-inf is part of the rounding
        return np.ascontiguousarray(np.asarray(p, dtype=np.float32).astype(np.float16).astype(np.float32))


def _data(n, d, Q, seed):
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
    return orc, pts, y


def _index(pts, k, T, seed):
    """precomp on the device from the FLOAT rows; returns (index, torch rows, save dict for the oracle)."""
    tp = torch.from_numpy(pts).cuda()
    O.srandom(seed)
    ix = A.Index.precomp(tp, k, T)
    save = ix.export()
    sd = save.to_dict()
    save.free()
    return ix, tp, sd


def _index_cpu(orc, pts, k, T, seed):
    """The same from the oracle's precomp (host): for rows longer than the device precomp's hashing takes (d > 1024)."""
    tp = torch.from_numpy(pts).cuda()
    O.srandom(seed)
    _, _, sd = orc.precomp(pts, k, T)
    save = A.Save.from_dict("f32", sd)
    ix = A.Index.from_save(save, tp)
    return ix, tp, sd


def _same(got, want, what):
    ids, dd = got
    ids = ids.cpu().numpy().astype(np.uint64) if torch.is_tensor(ids) else np.asarray(ids).astype(np.uint64)
    dd = dd.cpu().numpy() if torch.is_tensor(dd) else np.asarray(dd)
    assert np.array_equal(ids, want[0]), "%s: ids differ in %d places" % (what, int(np.sum(ids != want[0])))
    assert bits_equal(dd, want[1]), "%s: distances not bit-identical" % what


# d -> the layout code layout_code() picks in the f32 library (approximatenn_amd/csrc/ann_host.hip; pinned by
# tests/test_layout_table.py)
LAYOUTS = [
    (128, "128: power of two"),
    (80, "-84: static 5 lanes x 4 chunks"),
    (96, "-100: static 6 lanes x 4 chunks"),
    (160, "-164: static 10 lanes x 4 chunks"),
    (192, "-104: static 6 lanes x 8 chunks"),
    (320, "-168: static 10 lanes x 8 chunks"),
    (384, "-200: static 12 lanes x 8 chunks"),
    (24, "-50: static 3 lanes x 2 chunks"),
    (48, "-52: static 3 lanes x 4 chunks"),
    (28, "-1: run-time oc = 7 lanes, 1 chunk"),
    (280, "-2: run-time oc = 35 lanes, 2 chunks"),
    (112, "-4: run-time oc = 7 lanes, 4 chunks"),
    (224, "-8: run-time oc = 7 lanes, 8 chunks"),
    (100, "ANN_D_FOLD3, aligned rows"),
    (70, "ANN_D_FOLD3, d % 4 != 0 (element-wise loads)"),
    (50, "ANN_D_FOLD2, d % 4 != 0"),
    (36, "ANN_D_FOLD2, aligned rows"),
    (150, "ANN_D_FOLD4 (d % 4 != 0)"),
    (30, "ANN_D_UNALIGNED"),
    (260, "ANN_D_FOLD4G: no lanes-per-row layout"),
    (300, "ANN_D_FOLD5G: no lanes-per-row layout"),
    (2084, "0: generic, literal tree through LDS"),
]


@pytest.mark.parametrize("d,what", LAYOUTS, ids=[str(d) for d, _ in LAYOUTS])
def test_f16_rows_match_the_oracle_on_rounded_rows(d, what):
    n, k, T, Q = (2000, 5, 3, 64) if d > 1000 else (3000, 10, 5, 300)
    orc, pts, y = _data(n, d, Q, 6100 + d)
    ix, tp, sd = _index_cpu(orc, pts, k, T, 17) if d > 1024 else _index(pts, k, T, 17)
    try:
        hp = _h(pts)
        want = orc.query(sd, hp, y)
        ty = torch.from_numpy(y).cuda()
        ix.set_rows("f16")
        assert ix.rows == "f16"
        for mode in (0, 1):  # selection path with exact fallback / exact path for every query
            _same(ix.query(ty, mode=mode)[:2], want, "d=%d (%s) mode %d" % (d, what, mode))
        qa = 100
        want_a = orc.query(sd, hp, qa, alias=True)  # alias: query x excludes point x; the oracle's form needs y = h(P)
        th = torch.from_numpy(hp[:qa].copy()).cuda()
        for mode in (0, 1):
            _same(ix.query(th, alias=True, mode=mode)[:2], want_a, "d=%d alias mode %d" % (d, mode))
    finally:
        ix.close()


@pytest.mark.parametrize("d,k,Q", [(128, 33, 200), (80, 33, 150), (128, 10, 2500), (96, 10, 2300), (100, 10, 2100),
                                   (64, 10, 40)])
def test_f16_rows_stage2_select_and_batch_sizes(d, k, Q):
    """k = 33: stage-2 rows longer than the fused kernel's LDS row (stage2_select_kernel); Q > 2048: stage 1 and the
    fused stage-2 kernel as separate launches; small Q: stage 2 in the tail of the stage-1 workgroup."""
    orc, pts, y = _data(4000, d, Q, 7100 + d + k)
    ix, tp, sd = _index(pts, k, 6, 23)
    try:
        want = orc.query(sd, _h(pts), y)
        ix.set_rows("f16")
        ty = torch.from_numpy(y).cuda()
        for mode in (0, 1):
            _same(ix.query(ty, mode=mode)[:2], want, "d=%d k=%d Q=%d mode %d" % (d, k, Q, mode))
    finally:
        ix.close()


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_f16_rows_ties_take_the_exact_and_tie_paths(fuse, monkeypatch):
    """Small-integer rows are exact in binary16 and give exact distance ties (2 % of the rows also exist twice): the
    results equal the oracle, and the statistics show flagged queries and tie-path answers on binary16 rows."""
    monkeypatch.setenv("ANN_HIP_FUSE", fuse)
    A._lib.reload_env()
    n, d, k, T, Q = 6000, 32, 10, 6, 600
    rng = np.random.default_rng(31)
    pts = rng.integers(-30, 31, size=(n, d)).astype(np.float32)
    src = rng.choice(n, size=n // 50, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(n), src), size=src.size, replace=False)
    pts[dst] = pts[src]
    y = rng.integers(-30, 31, size=(Q, d)).astype(np.float32)
    y[:100] = pts[src[:100]] + rng.integers(-1, 2, size=(100, d)).astype(np.float32)
    pts, y = np.ascontiguousarray(pts), np.ascontiguousarray(y)
    assert np.array_equal(_h(pts), pts)
    orc = O.CpuBackend("f32", "oracle")
    ix, tp, sd = _index(pts, k, T, 41)
    try:
        ix.set_rows("f16")
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


@pytest.mark.parametrize("d", [128, 80, 70])
def test_f16_rows_conversion_edges(d):
    """Rows scaled by 10^U(-9, 6): binary16 subnormals, normals and overflow to +-inf all occur; results equal the
    oracle on the np.float16-rounded rows."""
    n, k, T, Q = 3000, 10, 5, 300
    orc, pts, y = _data(n, d, Q, 8100 + d)
    rng = np.random.default_rng(d)
    pts = np.ascontiguousarray(pts * (10.0 ** rng.uniform(-9, 6, size=(n, 1))).astype(np.float32))
    y = np.ascontiguousarray(y * (10.0 ** rng.uniform(-9, 6, size=(Q, 1))).astype(np.float32))
    hp = _h(pts)
    a = np.abs(_h(pts))
    assert np.isinf(a).any() and ((a > 0) & (a < np.float16(6.104e-05))).any() and ((a >= 1) & np.isfinite(a)).any()
    ix, tp, sd = _index(pts, k, T, 5)
    try:
        ix.set_rows("f16")
        ty = torch.from_numpy(y).cuda()
        want = orc.query(sd, hp, y)
        for mode in (0, 1):
            _same(ix.query(ty, mode=mode)[:2], want, "edges d=%d mode %d" % (d, mode))
        assert ix.lib.annhip_index_rows(ix.h) == 1
    finally:
        ix.close()


def test_f16_rows_toggle_back_is_bit_identical():
    orc, pts, y = _data(4000, 128, 400, 9100)
    ix, tp, sd = _index(pts, 10, 6, 3)
    try:
        ty = torch.from_numpy(y).cuda()
        want = orc.query(sd, pts, y)
        first = [t.cpu().numpy() for t in ix.query(ty)[:2]]
        _same(first, want, "native")
        ix.set_rows("f16")
        _same(ix.query(ty)[:2], orc.query(sd, _h(pts), y), "f16")
        ix.set_rows("native")
        assert ix.rows == "native"
        last = [t.cpu().numpy() for t in ix.query(ty)[:2]]
        _same(last, want, "native again")
        assert np.array_equal(first[0], last[0]) and bits_equal(first[1], last[1])
    finally:
        ix.close()


@pytest.mark.parametrize("d", [128, 80])
def test_f16_rows_other_entry_points(d):
    """annhip_query_on (own workspace and stream), annhip_stream_* (HostStream) and annhip_query_slice over two slices
    (the replica sequence of sharded.py: annhip_sh_codes, then one codes array for the whole batch)."""
    n, k, T, Q = 4000, 10, 6, 500
    orc, pts, y = _data(n, d, Q, 9300 + d)
    ix, tp, sd = _index(pts, k, T, 9)
    try:
        ix.set_rows("f16")
        want = orc.query(sd, _h(pts), y)
        ty = torch.from_numpy(y).cuda()
        ws, st = ix.workspace(), torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = ix.query(ty, ws=ws, stream=st)
        st.synchronize()
        _same(got[:2], want, "query_on")
        hs = ix.host_stream(max_ycnt=Q, lanes=2)  # a batch is answered as a whole (Q2): one oracle call per batch
        parts = list(hs.map([y, y[:200], y]))
        hs.close()
        for got, w in zip(parts, (want, orc.query(sd, _h(pts), y[:200]), want)):
            _same(got, w, "HostStream")
        eng = HipEngine(ix)
        codes = torch.empty((Q * T,), dtype=torch.int32, device="cuda")
        with eng.use(None):
            eng.sh_codes(ty, 0, Q, codes)
        ids = torch.empty((Q, k), dtype=torch.int64, device="cuda")
        dd = torch.empty((Q, k), dtype=torch.float32, device="cuda")
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
            dd = ((pts[ids].astype(np.float64) - y[x].astype(np.float64)) ** 2).sum(1)
            o = np.lexsort((ids, dd))[:k]
            return ids[o], dd[o]
        top, _ = best(cand)
        c2 = np.unique(np.concatenate([top, graph[top].reshape(-1)])).astype(np.int64)
        c2 = c2[c2 < n]
        i2, d2 = best(c2)
        out_i.append(i2), out_d.append(d2)
    return out_i, out_d


def test_f16_rows_with_fixed_mode():
    """set_fixed + binary16 rows: the exact top-k of the candidate sets, on h(P)."""
    n, d, k, T = 5000, 64, 10, 6
    orc, pts, y = _data(n, d, 60, 9500)
    ix, tp, sd = _index(pts, k, T, 13)
    try:
        hp = _h(pts)
        ty = torch.from_numpy(y).cuda()
        eng = HipEngine(ix)
        ix.set_fixed(True)
        ix.set_rows("f16")
        codes = _codes_of(eng, ty, T)
        ids, dd, _ = ix.query(ty)
        ids, dd = ids.cpu().numpy(), dd.cpu().numpy()
        want_i, want_d = _brute(sd, hp, y, codes, k)
        for x in range(60):
            m = len(want_i[x])
            assert np.allclose(dd[x, :m], want_d[x], rtol=2e-5, atol=0), (x, dd[x], want_d[x])
            assert np.all(np.isinf(dd[x, m:])) and np.all(ids[x, m:] == n)
            same = ids[x, :m] == want_i[x]
            if not same.all():  # a different id only where two candidates are (nearly) equally far
                bad = np.flatnonzero(~same)
                gd = ((hp[ids[x, bad]].astype(np.float64) - y[x]) ** 2).sum(1)
                assert np.allclose(gd, want_d[x][bad], rtol=2e-4, atol=0)
            assert len(set(ids[x, :m].tolist())) == m
    finally:
        ix.close()


def test_f16_rows_drop_in_switch():
    """ANN_HIP_ROWS=f16 + annhip_reload_env(): query() (query_gpu, resident index) answers as the oracle on h(P); unset +
    reload: on P again."""
    orc, pts, y = _data(4000, 80, 300, 9700)
    O.srandom(19)
    _, _, save = A.precomp(pts, 10, 6)
    old = os.environ.pop("ANN_HIP_ROWS", None)
    try:
        sd = save.to_dict()
        want_n, want_h = orc.query(sd, pts, y), orc.query(sd, _h(pts), y)
        os.environ["ANN_HIP_ROWS"] = "f16"
        A._lib.reload_env()
        _same(A.query(save, pts, y), want_h, "ANN_HIP_ROWS=f16")
        del os.environ["ANN_HIP_ROWS"]
        A._lib.reload_env()
        _same(A.query(save, pts, y), want_n, "ANN_HIP_ROWS unset")
    finally:
        if old is None:
            os.environ.pop("ANN_HIP_ROWS", None)
        else:
            os.environ["ANN_HIP_ROWS"] = old
        A._lib.reload_env()
        A._lib.load("f32").annhip_cache_clear()
        save.free()


def test_f16_rows_refusals():
    """f64 index, resharded index, unknown value: ValueError, the setting and the results unchanged.  reshard of an
    index with binary16 rows returns it to native rows."""
    orc = O.CpuBackend("f64", "oracle")
    O.srandom(77)
    orc.rand_norm_reset()
    n, d, k, T = 3000, 32, 10, 4
    p64 = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y64 = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(200 * d).reshape(200, d))).cuda()
    t64 = torch.from_numpy(p64).cuda()
    O.srandom(3)
    ix64 = A.Index.precomp(t64, k, T)
    try:
        before = [t.cpu().numpy() for t in ix64.query(y64)[:2]]
        with pytest.raises(ValueError):
            ix64.set_rows("f16")
        assert ix64.rows == "native"
        ix64.set_rows("native")  # always accepted
        after = [t.cpu().numpy() for t in ix64.query(y64)[:2]]
        assert np.array_equal(before[0], after[0]) and bits_equal(before[1], after[1])
    finally:
        ix64.close()

    _, pts, y = _data(n, d, 200, 9900)
    ix, tp, sd = _index(pts, k, T, 7)
    try:
        ty = torch.from_numpy(y).cuda()
        ix.set_rows("f16")
        before = [t.cpu().numpy() for t in ix.query(ty)[:2]]
        for bad in (7, "bf16"):
            with pytest.raises(ValueError):
                ix.set_rows(bad)
            assert ix.rows == "f16"
        after = [t.cpu().numpy() for t in ix.query(ty)[:2]]
        assert np.array_equal(before[0], after[0]) and bits_equal(before[1], after[1])
        assert ix.lib.annhip_index_set_rows(ix.h, C.c_int(7)) == -1
        # point-sharded: rows [lo, hi) only -> native rows, and binary16 refused
        lo, hi = 1000, 2000
        shard = tp[lo:hi].contiguous()
        ix.reshard(shard, lo, hi)
        assert ix.rows == "native"
        with pytest.raises(ValueError):
            ix.set_rows("f16")
        assert ix.rows == "native"
    finally:
        ix.close()
