"""GPU: the certificate of the pruned stage 1 (annhip_index_set_prune, ann_prune_kernels.h) where it has to refuse.

On benign rows the binary16 preselection already holds the true k+1 smallest keys, so a certificate that always said
yes would return the right bits.  The data here (tests/prune_model.py::trap_case) has clusters tighter than binary16
resolves: the narrow rows of a cluster tie, ties go to the lowest ids, and for some queries the rescored preselection is
NOT the answer -- only a refusal keeps the result right.  The exact numpy model (DeviceModel: candidates from the
oracle's hash codes, the query path's distance bits on the rows and on h(rows), the order (distance bits, id), the
certificate with the device's own E and K') says for every query whether the device certifies it, and the device's
uncertified_queries is compared with that count, batch by batch and query by query.  Every answer, pruned and native,
is compared on ids and distance bits with the oracle's."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests import prune_model as M
from tests.util import bits_equal

pytestmark = pytest.mark.gpu


def _index(c):
    tp = torch.from_numpy(np.array(c.pts)).cuda()
    return A.Index.from_save(A.Save.from_dict("f32", c.sd), tp), tp


def _np(got):
    torch.cuda.synchronize()
    return got[0].cpu().numpy().astype(np.uint64), got[1].cpu().numpy()


def _same(got, want, what):
    ids, dd = got
    wi = np.asarray(want[0]).astype(np.uint64)
    assert np.array_equal(ids, wi), "%s: ids differ in %d places" % (what, int(np.sum(ids != wi)))
    assert bits_equal(dd, np.asarray(want[1])), "%s: distances not bit-identical" % what


def _run(ix, ty, alias=False):
    """One batch with the statistics reset: (ids, distances), the queries the certificate refused."""
    ix.stats(reset=True)
    got = _np(ix.query(ty, alias=alias))
    return got, int(ix.stats(reset=True)["uncertified_queries"])


def _prune_on(ix, kp_want, pts):
    """Pruning on; the device's (E, K'), with E checked against the double-precision numpy maximum."""
    ix.set_prune("on")
    assert ix.prune
    E, kp = ix.prune_bound
    assert kp == kp_want
    E_true = M.row_error_true(pts)
    assert E_true <= E <= E_true * (1 + 2.0 ** -19), "E = %r, the rows' %r" % (E, E_true)
    return E, kp


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


def _alone(c, upto):
    """The model's candidates for each of the first `upto` queries asked as a batch of one (a query alone reads its hash
    codes at other places than inside a batch, so its candidate row is another one), with the oracle's answers."""
    cands, want = [], []
    for x in range(upto):
        cands += c.model.gather(c.y[x:x + 1])
        want.append(c.orc.query(c.sd, c.pts, c.y[x:x + 1]))
    return cands, want


@pytest.mark.parametrize("d", [64, 128])
def test_decision_per_query(d):
    """The whole batch's count, then every clustered query alone: refused exactly when the model refuses it (which
    includes every trap query; check() has made sure the model refuses those).  The model's certified counts at E, E / 2
    and 2 E are three different numbers on these data, so a bound off by a factor of two shows in the first count."""
    k = 10
    c, dec_np = M.trap_case(3000, d, k, 3, 192, seed=M.MAIN_SEED[d], three_counts=True)
    kp = M.default_keys(k)
    alone_cands, alone_want = _alone(c, c.nq)
    c.model.decide(alone_cands, kp, c.E).check("d=%d, the clustered queries alone" % d)
    print("d=%d batch: %r" % (d, dec_np))
    ix, tp = _index(c)
    try:
        ty = torch.from_numpy(np.array(c.y)).cuda()
        assert not ix.prune and ix.prune_bound is None, "auto keeps an index of this size native, without a bound"
        _same(_np(ix.query(ty)), c.want, "native d=%d" % d)
        E, kp = _prune_on(ix, kp, c.pts)
        dec = c.model.decide(c.cands, kp, E)
        dec.check("d=%d at the device's E" % d)
        got, unc = _run(ix, ty)
        print("d=%d device: uncertified %d, model %d" % (d, unc, dec.uncertified))
        _same(got, c.want, "pruned d=%d" % d)
        assert unc == dec.uncertified, "the device refused %d queries, the model %d" % (unc, dec.uncertified)
        alone = c.model.decide(alone_cands, kp, E)
        alone.check("d=%d alone at the device's E" % d)
        print("d=%d alone: %r" % (d, alone))
        bad = []
        for x in range(c.nq):
            got, unc = _run(ix, ty[x:x + 1])
            _same(got, alone_want[x], "pruned d=%d, query %d alone" % (d, x))
            if unc != int(not alone.certified[x]):
                bad.append((x, unc, bool(alone.trap[x]), float(alone.margin[x])))
        assert not bad, "(query, device's refusals, trap, margin) where device and model decide differently: %s" % bad[:10]
    finally:
        ix.close()


def test_aliased_trap():
    """The queries are the first rows themselves, which cover every cluster: self is excluded and the narrow rows of the
    query's cluster tie massively.  Only a prefix of the rows can be an aliased batch, so the per-query comparison of the
    test above is made on prefixes of several lengths here (each prefix reads its hash codes at its own places)."""
    d, k, Q = 128, 10, 192
    c, dec_np = M.trap_case(3000, d, k, 3, Q, alias=True)
    kp = M.default_keys(k)
    prefixes = {m: (c.model.gather(c.pts[:m], alias=True), c.orc.query(c.sd, c.pts, m, alias=True)) for m in (1, 2, 13, 50, 101)}
    ix, tp = _index(c)
    try:
        _same(_np(ix.query(tp[:Q], alias=True)), c.want, "aliased native")
        E, kp = _prune_on(ix, kp, c.pts)
        dec = c.model.decide(c.cands, kp, E)
        dec.check("aliased at the device's E")
        got, unc = _run(ix, tp[:Q], alias=True)
        print("aliased: %r; device uncertified %d" % (dec, unc))
        _same(got, c.want, "aliased pruned")
        assert unc == dec.uncertified
        for m, (cands, want) in prefixes.items():
            dm = c.model.decide(cands, kp, E)
            assert dm.wrong == 0 and float(dm.margin.min()) >= 2.0 ** -30
            got, unc = _run(ix, tp[:m], alias=True)
            _same(got, want, "aliased pruned, first %d rows" % m)
            assert unc == dm.uncertified, "first %d rows: device %d, model %d (%r)" % (m, unc, dm.uncertified, dm)
    finally:
        ix.close()


@pytest.mark.parametrize("d", [24, 80, 100, 128, 1024])
def test_row_error_bound(d):
    """prune_rowerr_kernel and the host's rounding of E against numpy in double: E_true <= E <= E_true (1 + 2^-19) (the
    host multiplies by 1 + 2^-20, the double sums differ by about d 2^-53).  One row scaled by 30 holds the maximum; it
    sits first, last and in the middle of n = 1501 rows (not a multiple of the 4 rows a workgroup's waves take)."""
    n, k, T, Q = 1501, 3, 1, 5
    rng = np.random.default_rng(400 + d)
    base = rng.standard_normal((n, d)).astype(np.float32)
    y = np.ascontiguousarray(rng.standard_normal((Q, d)).astype(np.float32))
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(401)
    _, _, sd = orc.precomp(base, k, T)
    plain = M.row_error_true(base)
    for row in (0, n - 1, n // 2):
        pts = base.copy()
        pts[row] *= 30.0
        pts = np.ascontiguousarray(pts)
        E_true = M.row_error_true(pts)
        assert E_true > 5 * plain, "the scaled row must hold the maximum by far"
        want = orc.query(sd, pts, y)
        ix = A.Index.from_save(A.Save.from_dict("f32", sd), torch.from_numpy(pts).cuda())
        try:
            ix.set_prune("on")
            E, kp = ix.prune_bound
            print("d=%d row=%d: E_dev / E_true - 1 = %.3g" % (d, row, E / E_true - 1))
            assert E_true <= E <= E_true * (1 + 2.0 ** -19), "d=%d, row %d scaled: E = %r, numpy %r" % (d, row, E, E_true)
            assert kp == 16
            _same(_np(ix.query(torch.from_numpy(y).cuda())), want, "d=%d, row %d scaled" % (d, row))
            ix.set_prune("off")
            assert ix.prune_bound is None
        finally:
            ix.close()


def test_keys_are_fixed_when_pruning_is_switched_on(monkeypatch):
    """ANN_HIP_PRUNE_K is read by set_prune, clamped to k + 1 ... 64; the count of refusals is the model's at that K'."""
    d, k = 128, 10
    c, _ = M.trap_case(3000, d, k, 3, 192, seed=M.MAIN_SEED[d], three_counts=True)
    ix, tp = _index(c)
    try:
        ty = torch.from_numpy(np.array(c.y)).cuda()
        seen = set()
        for asked, kp in ((k + 1, 11), (16, 16), (33, 33), (64, 64), (200, 64), (5, 11)):
            assert M.clamp_keys(k, asked) == kp
            ix.set_prune("off")
            _with_env(monkeypatch, {"ANN_HIP_PRUNE_K": str(asked)}, lambda: ix.set_prune("on"))
            E, got_kp = ix.prune_bound
            assert got_kp == kp, "ANN_HIP_PRUNE_K=%d: K' = %d" % (asked, got_kp)
            dec = c.model.decide(c.cands, kp, E)
            assert dec.wrong == 0 and float(dec.margin.min()) >= 2.0 ** -30, "K'=%d: %r" % (kp, dec)
            got, unc = _run(ix, ty)
            print("K'=%d: %r; device uncertified %d" % (kp, dec, unc))
            _same(got, c.want, "pruned K'=%d" % kp)
            assert unc == dec.uncertified, "K'=%d: device %d, model %d" % (kp, unc, dec.uncertified)
            seen.add(dec.uncertified)
        assert len(seen) >= 3, "the list sizes must tell in the count: %s" % sorted(seen)
    finally:
        ix.close()


def test_batches_that_do_not_fill_a_workgroup():
    """Q = 1, 2, 3, 5, 7: the last workgroup of prune_rescore_kernel has waves without a query.  The query path reads
    the hash codes of a batch at places that depend on the batch's size (the oracle's "read layout != write layout"), so
    the first m queries asked as a batch have other candidate rows, and other answers, than rows [0, m) of the full
    batch's answer: the expectation is the oracle's and the model's for that batch of m."""
    d, k = 128, 10
    c, _ = M.trap_case(3000, d, k, 3, 192, seed=M.MAIN_SEED[d], three_counts=True)
    subs = {m: (c.model.gather(c.y[:m]), c.orc.query(c.sd, c.pts, c.y[:m])) for m in (1, 2, 3, 5, 7)}
    ix, tp = _index(c)
    try:
        E, kp = _prune_on(ix, M.default_keys(k), c.pts)
        ty = torch.from_numpy(np.array(c.y)).cuda()
        total = 0
        for m, (cands, want) in subs.items():
            dm = c.model.decide(cands, kp, E)
            assert dm.wrong == 0 and float(dm.margin.min()) >= 2.0 ** -30
            got, unc = _run(ix, ty[:m])
            _same(got, want, "pruned, the first %d queries" % m)
            assert unc == dm.uncertified, "first %d queries: device %d, model %d" % (m, unc, dm.uncertified)
            total += dm.uncertified
            ix.set_prune("off")
            _same(_np(ix.query(ty[:m])), want, "native, the first %d queries" % m)
            ix.set_prune("on")
        assert total > 0, "some of these queries must be refused"
    finally:
        ix.close()


@pytest.mark.parametrize("k,kp,ladder", [(1, 16, False), (31, 48, True)])
def test_smallest_and_largest_k(k, kp, ladder):
    """k + 1 = 2 and the documented limit k + 1 = 32 (K' = 48).  Two keys are hard to lose among sixteen: k = 1 has its
    traps where every cluster is tighter than binary16 resolves (one spread), k = 31 on the ladder of spreads."""
    d = 128
    c, dec_np = M.trap_case(3000, d, k, 3, 192, ladder=ladder)
    ix, tp = _index(c)
    try:
        ty = torch.from_numpy(np.array(c.y)).cuda()
        _same(_np(ix.query(ty)), c.want, "native k=%d" % k)
        E, kp = _prune_on(ix, kp, c.pts)
        dec = c.model.decide(c.cands, kp, E)
        dec.check("k=%d at the device's E" % k)
        got, unc = _run(ix, ty)
        print("k=%d: %r; device uncertified %d" % (k, dec, unc))
        _same(got, c.want, "pruned k=%d" % k)
        assert unc == dec.uncertified, "k=%d: device %d, model %d" % (k, unc, dec.uncertified)
    finally:
        ix.close()


def test_k_32_is_refused():
    n, d, k, T, Q = 1500, 128, 32, 3, 37
    rng = np.random.default_rng(32)
    pts = np.ascontiguousarray(rng.standard_normal((n, d)).astype(np.float32))
    y = np.ascontiguousarray(rng.standard_normal((Q, d)).astype(np.float32))
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(33)
    _, _, sd = orc.precomp(pts, k, T)
    want = orc.query(sd, pts, y)
    ix = A.Index.from_save(A.Save.from_dict("f32", sd), torch.from_numpy(pts).cuda())
    try:
        with pytest.raises(ValueError):
            ix.set_prune("on")
        assert not ix.prune and ix.prune_bound is None
        ix.set_prune("auto")
        assert not ix.prune and ix.prune_bound is None
        got, unc = _run(ix, torch.from_numpy(y).cuda())
        _same(got, want, "k=32")
        assert unc == 0
    finally:
        ix.close()
