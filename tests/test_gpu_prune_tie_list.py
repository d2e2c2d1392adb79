"""GPU: the pruned stage 1 hands the exact step the candidate lists of its flagged queries (PruneArgs::tie_d / tie_i,
ann_prune_kernels.h).  A query that is certified but fails finalize1's test gets the k+1 smallest rescored keys: the
list native stage 1 would have written, so the tie path (ann_tie.h) starts from it instead of deriving it from the
whole row.  A query the certificate refuses gets an empty list and the row derives its own, as before.  Nothing about
the results may change: ids and distance bits equal the native path's and the oracle's, and the tie path takes the
same rows."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests import prune_model as M
from tests.util import bits_equal

pytestmark = pytest.mark.gpu


def _np(got):
    torch.cuda.synchronize()
    return got[0].cpu().numpy().astype(np.uint64), got[1].cpu().numpy()


def _same(got, want, what):
    ids, dd = got
    wi = np.asarray(want[0]).astype(np.uint64)
    assert np.array_equal(ids, wi), "%s: ids differ in %d places" % (what, int(np.sum(ids != wi)))
    assert bits_equal(dd, np.asarray(want[1])), "%s: distances not bit-identical" % what


def _both(ix, ty):
    """The batch through the pruned and through the native stage 1, with each run's statistics."""
    ix.set_prune("on")
    assert ix.prune
    ix.stats(reset=True)
    pruned = _np(ix.query(ty))
    st_p = ix.stats(reset=True)
    ix.set_prune("off")
    assert not ix.prune
    native = _np(ix.query(ty))
    st_n = ix.stats(reset=True)
    return pruned, native, st_p, st_n


def _twins(pts, y, rng, nq, lo=0):
    """2 % of the rows from `lo` on exist twice; the first nq queries sit next to a twin pair."""
    n, d = pts.shape
    src = rng.choice(np.arange(lo, n), size=n // 50, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(lo, n), src), size=src.size, replace=False)
    pts[dst] = pts[src]
    y[:nq] = pts[src[:nq]] + (rng.standard_normal((nq, d)) * 0.05).astype(np.float32)


def test_duplicated_rows_the_tie_path_takes_the_same_rows():
    n, d, k, T, Q = 20000, 32, 10, 10, 500
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(9410)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
    _twins(pts, y, np.random.default_rng(5), 200)
    pts, y = np.ascontiguousarray(pts), np.ascontiguousarray(y)
    tp = torch.from_numpy(pts).cuda()
    O.srandom(39)
    ix = A.Index.precomp(tp, k, T)
    try:
        save = ix.export()
        sd = save.to_dict()
        save.free()
        want = orc.query(sd, pts, y)
        pruned, native, st_p, st_n = _both(ix, torch.from_numpy(y).cuda())
        print("pruned %r\nnative %r" % (st_p, st_n))
        _same(native, want, "duplicates native")
        _same(pruned, want, "duplicates pruned")
        unc = st_p["uncertified_queries"]
        assert st_n["exact_queries"] > 0 and st_n["tie_queries"] > 0, "twin rows must reach the tie path"
        assert st_p["exact_queries"] == st_n["exact_queries"] + unc
        assert abs(st_p["tie_queries"] - st_n["tie_queries"]) <= unc, "the certified flagged rows must take the tie path as natively"
    finally:
        ix.close()


_MIXED = {}


def _mixed_case():
    """Trap clusters (the certificate refuses some of their queries) in the first rows, twin rows behind them, and the
    model's word on every query: certified or not, and whether its k+1 smallest exact keys hold a tie."""
    if _MIXED:
        return _MIXED["c"]
    from types import SimpleNamespace
    n, d, k, T, Q = 3000, 128, 10, 3, 192
    pts, y, nq = M.trap_points(n, d, Q, M.MAIN_SEED[d])
    pts, y = pts.copy(), y.copy()
    rng = np.random.default_rng(6)
    ytw = np.empty((40, d), dtype=np.float32)
    _twins(pts, ytw, rng, 40, lo=1200)  # the clusters are rows [0, 1200)
    y[nq:nq + 40] = ytw                 # behind the clustered queries; the rest stay iid
    pts, y = np.ascontiguousarray(pts), np.ascontiguousarray(y)
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(1007)
    _, _, sd = orc.precomp(pts, k, T)
    model = M.DeviceModel(sd, pts)
    cands = model.gather(y)
    dec = model.decide(cands, M.default_keys(k), M.row_error(pts))
    tied = []
    for ids, dh, dx in cands:
        o = M.keys_sorted(dx, ids)[:k + 1]
        b = dx[o].view(np.uint32)
        tied.append(bool(np.any(b[1:] == b[:-1])))
    c = SimpleNamespace(pts=pts, y=y, sd=sd, k=k, Q=Q, dec=dec, tied=np.array(tied), want=orc.query(sd, pts, y))
    _MIXED["c"] = c
    return c


@pytest.mark.parametrize("tie", ["1", "0"])
def test_mixed_batch(monkeypatch, tie):
    """One batch with certified-and-tied, uncertified and clean queries; with ANN_HIP_TIE=0 the lists are ignored and the
    literal network answers every flagged row."""
    c = _mixed_case()
    cert, tied = c.dec.certified, c.tied
    kinds = (int(np.sum(cert & tied)), int(np.sum(~cert)), int(np.sum(cert & ~tied)))
    print("certified and tied %d, uncertified %d, clean %d; %r" % (kinds + (c.dec,)))
    assert min(kinds) >= 1, "the batch must hold every kind of query: %s" % (kinds,)
    assert c.dec.wrong == 0 and float(c.dec.margin.min()) >= 2.0 ** -30
    if tie == "0":
        monkeypatch.setenv("ANN_HIP_TIE", "0")
        A._lib.reload_env()
    ix = A.Index.from_save(A.Save.from_dict("f32", c.sd), torch.from_numpy(c.pts).cuda())
    try:
        pruned, native, st_p, st_n = _both(ix, torch.from_numpy(c.y).cuda())
        print("pruned %r\nnative %r" % (st_p, st_n))
        _same(native, c.want, "mixed native")
        _same(pruned, c.want, "mixed pruned")
        assert st_p["uncertified_queries"] == c.dec.uncertified
        assert st_p["exact_queries"] >= kinds[0] + kinds[1]
        if tie == "0":
            assert st_p["tie_queries"] == 0 and st_n["tie_queries"] == 0
        else:
            assert st_n["tie_queries"] > 0
            assert abs(st_p["tie_queries"] - st_n["tie_queries"]) <= st_p["uncertified_queries"]
    finally:
        ix.close()
        if tie == "0":
            monkeypatch.delenv("ANN_HIP_TIE")
            A._lib.reload_env()
