"""GPU: the pruned stage 1 of the parity path (annhip_index_set_prune, include/ann_hip.h).  The contract: nothing about
the results changes -- ids and distance bits equal the native path's and the oracle's -- whether a query is certified,
flagged by finalize1's test, or not certified and answered by the exact path.  Pruning is forced on at small shapes (the
auto rule keeps indexes of this size on the native path, which is tested too)."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests import prune_model as M
from tests.util import bits_equal, load_golden

pytestmark = pytest.mark.gpu


def _data(n, d, Q, seed):
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
    return orc, pts, y


def _index(pts, k, T, seed):
    tp = torch.from_numpy(pts).cuda()
    O.srandom(seed)
    ix = A.Index.precomp(tp, k, T)
    save = ix.export()
    sd = save.to_dict()
    save.free()
    return ix, tp, sd


def _np(got):
    ids, dd = got[0], got[1]
    torch.cuda.synchronize()
    return ids.cpu().numpy().astype(np.uint64), dd.cpu().numpy()


def _same(got, want, what):
    ids, dd = got
    assert np.array_equal(ids, np.asarray(want[0]).astype(np.uint64)), \
        "%s: ids differ in %d places" % (what, int(np.sum(ids != np.asarray(want[0]).astype(np.uint64))))
    assert bits_equal(dd, want[1]), "%s: distances not bit-identical" % what


def _both(ix, ty, alias=False):
    """The batch through the pruned and through the native stage 1, with each run's statistics."""
    ix.set_prune("on")
    assert ix.prune
    ix.stats(reset=True)
    pruned = _np(ix.query(ty, alias=alias))
    st_p = ix.stats(reset=True)
    ix.set_prune("off")
    assert not ix.prune
    native = _np(ix.query(ty, alias=alias))
    st_n = ix.stats(reset=True)
    # a certified query is flagged exactly when the native path flags it; an uncertified one always
    assert st_p["uncertified_queries"] <= st_p["exact_queries"] <= st_n["exact_queries"] + st_p["uncertified_queries"]
    assert st_n["uncertified_queries"] == 0
    return pruned, native, st_p, st_n


@pytest.mark.parametrize("k", [3, 10, 20])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_pruned_equals_native_and_oracle(d, k):
    n, Q, T = 20000, 500, 10
    orc, pts, y = _data(n, d, Q, 9000 + d + k)
    ix, tp, sd = _index(pts, k, T, 29)
    try:
        assert not ix.prune, "auto mode keeps an index of this size on the native path"
        want = orc.query(sd, pts, y)
        pruned, native, st_p, _ = _both(ix, torch.from_numpy(y).cuda())
        _same(native, want, "native d=%d k=%d" % (d, k))
        _same(pruned, want, "pruned d=%d k=%d" % (d, k))
        assert st_p["uncertified_queries"] < Q / 2, "iid rows: the certificate should hold for most queries"
    finally:
        ix.close()


def test_golden_pow2_d128():
    g = load_golden("pow2_d128_f32")
    save = A.Save.from_dict("f32", g["save"])
    pts = torch.from_numpy(np.ascontiguousarray(g["points"])).cuda()
    ix = A.Index.from_save(save, pts)
    try:
        assert not ix.prune
        pruned, native, _, _ = _both(ix, torch.from_numpy(g["y"]).cuda())
        _same(native, (g["query_ids"], g["query_dists"]), "golden native")
        _same(pruned, (g["query_ids"], g["query_dists"]), "golden pruned")
        qa = len(g["alias_ids"])
        pruned, native, _, _ = _both(ix, pts[:qa], alias=True)
        _same(native, (g["alias_ids"], g["alias_dists"]), "golden alias native")
        _same(pruned, (g["alias_ids"], g["alias_dists"]), "golden alias pruned")
    finally:
        ix.close()


def test_aliased_batch():
    n, d, k, T = 20000, 64, 10, 10
    orc, pts, _ = _data(n, d, 2, 9300)
    ix, tp, sd = _index(pts, k, T, 31)
    try:
        qa = 500
        want = orc.query(sd, pts, qa, alias=True)
        pruned, native, _, _ = _both(ix, tp[:qa], alias=True)
        _same(native, want, "alias native")
        _same(pruned, want, "alias pruned")
    finally:
        ix.close()


def test_duplicated_points_are_flagged_and_answered():
    """2 % of the rows exist twice: equal distances among the k+1 smallest keys, finalize1's test rejects those queries
    on the rescored keys exactly as on the native ones."""
    n, d, k, T, Q = 20000, 32, 10, 10, 500
    orc, pts, y = _data(n, d, Q, 9400)
    rng = np.random.default_rng(3)
    src = rng.choice(n, size=n // 50, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(n), src), size=src.size, replace=False)
    pts[dst] = pts[src]
    y[:200] = pts[src[:200]] + (rng.standard_normal((200, d)) * 0.05).astype(np.float32)  # queries next to a twin pair
    pts, y = np.ascontiguousarray(pts), np.ascontiguousarray(y)
    ix, tp, sd = _index(pts, k, T, 37)
    try:
        want = orc.query(sd, pts, y)
        pruned, native, st_p, st_n = _both(ix, torch.from_numpy(y).cuda())
        _same(native, want, "duplicates native")
        _same(pruned, want, "duplicates pruned")
        assert st_n["exact_queries"] > 0 and st_p["exact_queries"] > 0, "twin rows must send queries to the exact path"
        assert st_p["exact_queries"] >= st_n["exact_queries"] - st_p["uncertified_queries"]
    finally:
        ix.close()


def test_scaled_rows_certified_and_not():
    """A few rows scaled by 60 raise E to ~0.12: the numpy model (tests/prune_model.py) certifies some queries of such
    a set and refuses others at every candidate count between 200 and 3000; both must occur on the device, and every
    answer stays the native one."""
    n, d, k, T, Q = 20000, 64, 10, 10, 500
    orc, pts, y = _data(n, d, Q, 9500)
    pts[::4000] *= 60.0
    pts = np.ascontiguousarray(pts)
    E = M.row_error(pts)
    assert 0.08 < E < 0.16
    rng = np.random.default_rng(8)
    hp = M.h(pts)
    for count in (200, 3000):  # the model, on the CPU: both outcomes at either end of the candidate counts
        certs = []
        for yy in y[:60]:
            ids = np.sort(rng.choice(n, size=count, replace=False)).astype(np.uint32)
            certs.append(M.prune_query(yy, pts[ids], hp[ids], ids, k, M.default_keys(k), E)[0])
        assert 0 < sum(certs) < len(certs), "model at %d candidates: %d of %d certified" % (count, sum(certs), len(certs))
    ix, tp, sd = _index(pts, k, T, 41)
    try:
        want = orc.query(sd, pts, y)
        pruned, native, st_p, _ = _both(ix, torch.from_numpy(y).cuda())
        _same(native, want, "scaled native")
        _same(pruned, want, "scaled pruned")
        uncert = st_p["uncertified_queries"]
        assert uncert > 0, "no query failed the certificate"
        assert Q - uncert > 0, "no query was certified"
    finally:
        ix.close()


def test_overflowing_row_is_refused():
    """A row of 1e6 becomes +inf in binary16: there is no error bound, mode 1 is refused, auto stays off.  (Such a row
    drags the row means along and the whole set lands in one bucket: the set is small so that the oracle stays quick.)"""
    n, d, k, T, Q = 1500, 32, 10, 3, 64
    orc, pts, y = _data(n, d, Q, 9600)
    pts[1234] = 1e6
    pts = np.ascontiguousarray(pts)
    ix, tp, sd = _index(pts, k, T, 43)
    try:
        want = orc.query(sd, pts, y)
        assert not ix.prune
        with pytest.raises(ValueError):
            ix.set_prune("on")
        assert not ix.prune
        ix.set_prune("auto")
        assert not ix.prune
        _same(_np(ix.query(torch.from_numpy(y).cuda())), want, "overflowing row")
    finally:
        ix.close()


def test_tiny_index_every_preselection_is_complete():
    """So few candidates per query that the preselection holds them all (m < K'): certified without the bound."""
    n, d, k, T, Q = 64, 32, 24, 1, 100  # one try of 60 slots: P1 = 32 < K' = 37, and k + 1 = 25 keys still fit a query
    orc, pts, y = _data(n, d, Q, 9700)
    O.srandom(47)
    _, _, sd = orc.precomp(pts, k, T)
    ix = A.Index.from_save(A.Save.from_dict("f32", sd), torch.from_numpy(pts).cuda())
    try:
        assert k <= ix.P1 < M.default_keys(k), "the whole candidate row is shorter than the preselection"
        want = orc.query(sd, pts, y)
        pruned, native, st_p, _ = _both(ix, torch.from_numpy(y).cuda())
        _same(native, want, "tiny native")
        _same(pruned, want, "tiny pruned")
        assert st_p["uncertified_queries"] == 0
    finally:
        ix.close()


def test_modes_and_what_wins():
    n, d, k, T, Q = 5000, 64, 10, 6, 300
    orc, pts, y = _data(n, d, Q, 9800)
    ix, tp, sd = _index(pts, k, T, 53)
    try:
        ty = torch.from_numpy(y).cuda()
        want = orc.query(sd, pts, y)
        ix.set_prune("auto")
        assert not ix.prune, "auto: off at this size"
        ix.set_prune("on")
        assert ix.prune
        ix.profile(True)
        ix.stats(reset=True)
        _same(_np(ix.query(ty)), want, "pruned, profiled")
        st = ix.stats(reset=True)
        ix.profile(False)
        assert st["s1_launches"] == 1 and st["s1_ms"] > 0, "preselection and rescoring are one stage-1 launch"
        ix.set_prune("off")
        ix.profile(True)
        _same(_np(ix.query(ty)), want, "native, profiled")
        st_n = ix.stats(reset=True)
        ix.profile(False)
        assert 0 < st["s1_rows"] < 0.75 * st_n["s1_rows"], "native-row equivalents: about half the native rows"
        ix.set_prune("on")
        ix.set_rows("f16")             # an explicit narrow-row setting wins and keeps its meaning
        assert not ix.prune and ix.rows == "f16"
        _same(_np(ix.query(ty)), orc.query(sd, M.h(pts), y), "f16 rows with prune on")
        ix.set_rows("native")
        assert ix.prune
        ix.set_fixed(True)             # fixed mode is not pruned
        assert not ix.prune
        ix.set_fixed(False)
        assert ix.prune
        _same(_np(ix.query(ty, mode=1)), want, "mode 1 takes the exact path")
        with pytest.raises(ValueError):
            ix.set_prune(7)
    finally:
        ix.close()


def test_f64_library_refuses():
    orc = O.CpuBackend("f64", "oracle")
    O.srandom(9900)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(2000 * 32).reshape(2000, 32))
    O.srandom(59)
    ix = A.Index.precomp(torch.from_numpy(pts).cuda(), 5, 3)
    try:
        with pytest.raises(ValueError):
            ix.set_prune("on")
        ix.set_prune("auto")
        ix.set_prune("off")
        assert not ix.prune
    finally:
        ix.close()
