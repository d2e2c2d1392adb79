"""GPU: stage 1 with its running selection in registers (stage1_select_kernel<..., REGS>), through Index.query against
the oracle, bit for bit.  The list holds K1 = k + 1 keys on the native path and K' (ANN_HIP_PRUNE_K) on the pruned one:
one register per lane up to 64 keys, two up to 128, the LDS buffer beyond.  The shapes sit on those edges, on the wave
counts the merge sees, and on what the selection must get right besides: duplicates across waves, ties (the flagged
path), fewer candidates than keys (the pads) and the self-exclusion of an aliased batch."""
import functools

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests.util import bits_equal

pytestmark = pytest.mark.gpu

N, Q, T = 20000, 500, 10


@functools.lru_cache(maxsize=None)
def _data(prec, n, d, q, seed, twins=False):
    orc = O.CpuBackend(prec, "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y = np.ascontiguousarray(orc.gen_rand(q * d).reshape(q, d))
    if twins:  # every row exists twice
        pts[n // 2:] = pts[:n // 2]
    pts.setflags(write=False)
    y.setflags(write=False)
    return orc, pts, y


def _index(pts, k, tries, seed):
    tp = torch.from_numpy(np.array(pts)).cuda()
    O.srandom(seed)
    ix = A.Index.precomp(tp, k, tries)
    save = ix.export()
    sd = save.to_dict()
    save.free()
    return ix, tp, sd


def _np(got):
    torch.cuda.synchronize()
    return got[0].cpu().numpy().astype(np.uint64), got[1].cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[0], np.asarray(want[0]).astype(np.uint64)), \
        "%s: ids differ in %d places" % (what, int(np.sum(got[0] != np.asarray(want[0]).astype(np.uint64))))
    assert bits_equal(got[1], want[1]), "%s: distances not bit-identical" % what


def _with_env(monkeypatch, env, f):
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    A._lib.reload_env()
    try:
        return f()
    finally:
        for kk in env:
            monkeypatch.delenv(kk)
        A._lib.reload_env()


# K1 = k + 1 = 2 | 64, 65: the last list of one register and the first of two | 128: the last of two | 129: the first that
# falls back to the LDS buffer (the parity path admits any k up to its sorted prefix P1; beyond that the exact path answers)
@pytest.mark.parametrize("d,k", [(32, 1), (32, 63), (32, 64), (32, 127), (32, 128), (128, 1), (128, 63), (128, 64)])
def test_native_list_sizes(d, k):
    orc, pts, y = _data("f32", N, d, Q, 7000 + d)
    ix, tp, sd = _index(pts, k, T, 61)
    try:
        assert k <= ix.P1, "stage 1 must run for this k"
        _same(_np(ix.query(torch.from_numpy(np.array(y)).cuda())), orc.query(sd, pts, y), "native d=%d k=%d" % (d, k))
    finally:
        ix.close()


@pytest.mark.parametrize("d", [32, 128])
def test_pruned_list_sizes(d, monkeypatch):
    k = 10
    orc, pts, y = _data("f32", N, d, Q, 7000 + d)
    ix, tp, sd = _index(pts, k, T, 67)
    try:
        want = orc.query(sd, pts, y)
        ty = torch.from_numpy(np.array(y)).cuda()
        for kp in (k + 1, 16, 33, 64):
            # K' is fixed when pruning is switched on (prune_setup), not by the query: the variable is set around both
            ix.set_prune("off")
            _with_env(monkeypatch, {"ANN_HIP_PRUNE_K": str(kp)}, lambda: ix.set_prune("on"))
            assert ix.prune
            assert ix.prune_bound[1] == kp
            ix.stats(reset=True)
            got = _with_env(monkeypatch, {"ANN_HIP_PRUNE_K": str(kp)}, lambda: _np(ix.query(ty)))
            _same(got, want, "pruned d=%d K'=%d" % (d, kp))
            unc = ix.stats(reset=True)["uncertified_queries"]
            if kp > k + 1:
                assert unc < Q / 2, "iid rows: the certificate should hold for most queries"
            else:
                # K' = k + 1 (which never ran while the variable was set around the query only): tau is the largest
                # exact distance of the same k + 1 rows whose largest narrow distance is B, and the row x that has B
                # has sqrt(exact) >= sqrt(B) - ||x - h(x)|| >= sqrt(B) - E, while LB > tau needs sqrt(tau) below
                # sqrt(B (1 - 2^-16)) - E: a full preselection of k + 1 keys is never certified, whatever the rows
                assert unc == Q, "K' = k + 1: the certificate cannot hold (%d of %d refused)" % (unc, Q)
    finally:
        ix.close()


def test_wave_counts(monkeypatch):
    d, k = 128, 10
    orc, pts, y = _data("f32", N, d, Q, 7000 + d)
    ix, tp, sd = _index(pts, k, T, 67)
    try:
        want = orc.query(sd, pts, y)
        ty = torch.from_numpy(np.array(y)).cuda()
        for waves in ("1", "2", "4"):
            for mode in ("off", "on"):
                ix.set_prune(mode)
                got = _with_env(monkeypatch, {"ANN_HIP_S1_WAVES": waves}, lambda: _np(ix.query(ty)))
                _same(got, want, "waves=%s prune=%s" % (waves, mode))
    finally:
        ix.close()


def test_every_row_twice_takes_the_flagged_path():
    d, k = 32, 10
    orc, pts, y = _data("f32", N, d, Q, 7100, True)
    ix, tp, sd = _index(pts, k, T, 71)
    try:
        want = orc.query(sd, pts, y)
        ty = torch.from_numpy(np.array(y)).cuda()
        for mode in ("off", "on"):
            ix.set_prune(mode)
            ix.stats(reset=True)
            _same(_np(ix.query(ty)), want, "twins prune=%s" % mode)
            assert ix.stats(reset=True)["exact_queries"] > 0, "tied distances must send queries to the exact path"
    finally:
        ix.close()


def test_fewer_candidates_than_keys():
    n, d, k, q = 40, 32, 10, 100
    orc, pts, y = _data("f32", n, d, q, 7200)
    O.srandom(73)
    _, _, sd = orc.precomp(pts, k, 1)
    ix = A.Index.from_save(A.Save.from_dict("f32", sd), torch.from_numpy(np.array(pts)).cuda())
    try:
        want = orc.query(sd, pts, y)
        ty = torch.from_numpy(np.array(y)).cuda()
        for mode in ("off", "on"):
            ix.set_prune(mode)
            _same(_np(ix.query(ty)), want, "n=40 prune=%s" % mode)
    finally:
        ix.close()


def test_aliased_batch():
    d, k = 128, 10
    orc, pts, _ = _data("f32", N, d, Q, 7000 + d)
    ix, tp, sd = _index(pts, k, T, 79)
    try:
        want = orc.query(sd, pts, Q, alias=True)
        for mode in ("off", "on"):
            ix.set_prune(mode)
            _same(_np(ix.query(tp[:Q], alias=True)), want, "alias prune=%s" % mode)
    finally:
        ix.close()


@pytest.mark.parametrize("k", [10, 64])
def test_f64_library(k):
    d = 32
    orc, pts, y = _data("f64", N, d, Q, 7300)
    ix, tp, sd = _index(pts, k, T, 83)
    try:
        _same(_np(ix.query(torch.from_numpy(np.array(y)).cuda())), orc.query(sd, pts, y), "f64 k=%d" % k)
    finally:
        ix.close()
