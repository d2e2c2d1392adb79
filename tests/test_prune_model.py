"""CPU: the certificate of the pruned stage 1 (annhip_index_set_prune), restated in numpy on float32 data.  Whenever it
certifies a query, the true k+1 smallest keys over ALL candidates lie inside the preselection made on the binary16 rows,
so rescoring the preselection gives exactly them.  It must never certify wrongly; it may refuse as often as it likes,
but the tests also pin that it is not vacuous (iid rows certify) and that it does refuse where it has to (scaled rows).
The last tests run the exact model of the device's decision on the trap data of the GPU tests (tests/prune_model.py)."""
import numpy as np
import pytest

from tests import prune_model as M


def _run(pts, ys, k, kp, cand_count, seed, E=None):
    """Every query against a random candidate subset of cand_count rows; returns (certified, wrong, inside)."""
    rng = np.random.default_rng(seed)
    hp = M.h(pts)
    E = M.row_error(pts) if E is None else E
    certified = wrong = 0
    for y in ys:
        ids = np.sort(rng.choice(pts.shape[0], size=min(cand_count, pts.shape[0]), replace=False)).astype(np.uint32)
        cert, rescored, truth = M.prune_query(y, pts[ids], hp[ids], ids, k, kp, E)
        same = np.array_equal(rescored[1], truth[1]) and np.array_equal(rescored[0].view(np.uint32), truth[0].view(np.uint32))
        certified += cert
        wrong += cert and not same
    return certified, wrong


@pytest.mark.parametrize("d,k", [(32, 3), (64, 10), (128, 10), (128, 20)])
def test_iid_rows_certify_and_never_wrongly(d, k):
    rng = np.random.default_rng(100 + d + k)
    pts = rng.standard_normal((4000, d)).astype(np.float32)
    ys = rng.standard_normal((150, d)).astype(np.float32)
    for kp in sorted({k + 1, 16, M.default_keys(k), 64} - set(range(k + 1))):
        certified, wrong = _run(pts, ys, k, kp, 1400, 7)
        assert wrong == 0, "K'=%d: %d queries certified with a wrong answer" % (kp, wrong)
        if kp >= M.default_keys(k):
            assert certified >= 0.9 * len(ys), "K'=%d certified only %d of %d iid queries" % (kp, certified, len(ys))


def test_clustered_rows_with_near_equal_distances():
    """Tight clusters: many candidates at almost the same distance from a query, closer together than binary16 resolves.
    The certificate has to refuse most of these; what it certifies must still be right."""
    rng = np.random.default_rng(5)
    d, k = 64, 10
    centres = rng.standard_normal((40, d)).astype(np.float32) * 4
    pts = (centres[rng.integers(0, 40, size=4000)] + rng.standard_normal((4000, d)).astype(np.float32) * 1e-3).astype(np.float32)
    ys = (centres[rng.integers(0, 40, size=150)] + rng.standard_normal((150, d)).astype(np.float32) * 1e-3).astype(np.float32)
    for kp in (16, 24, 64):
        certified, wrong = _run(pts, ys, k, kp, 1400, 11)
        assert wrong == 0
    # exact duplicates and exact ties
    pts[1000:1100] = pts[:100]
    certified, wrong = _run(pts, ys, k, 24, 4000, 12)
    assert wrong == 0


def test_scaled_rows_make_it_refuse_but_never_lie():
    rng = np.random.default_rng(9)
    d, k = 64, 10
    pts = rng.standard_normal((4000, d)).astype(np.float32)
    ys = rng.standard_normal((150, d)).astype(np.float32)
    base, _ = _run(pts, ys, k, 24, 1400, 3)
    pts[::500] *= 3000.0    # binary16's spacing at 3000 is 2: E grows to several units
    assert M.row_error(pts) > 1.0
    certified, wrong = _run(pts, ys, k, 24, 1400, 3)
    assert wrong == 0
    assert certified < base, "a larger E has to cost certificates (%d vs %d)" % (certified, base)


def test_too_few_candidates_is_certified_and_odd_values_fail_safe():
    rng = np.random.default_rng(2)
    pts = rng.standard_normal((500, 32)).astype(np.float32)
    ys = rng.standard_normal((20, 32)).astype(np.float32)
    certified, wrong = _run(pts, ys, 3, 24, 15, 1)   # 15 candidates < K': nothing is left out
    assert certified == len(ys) and wrong == 0
    E = 0.01
    assert not M.certify(np.float32("nan"), 1.0, E) and not M.certify(4.0, np.float32("nan"), E)
    assert not M.certify(np.float32("inf"), np.float32("inf"), E)
    assert not M.certify(4.0, 1.0, np.inf) and not M.certify(4.0, 1.0, np.nan)
    assert not M.certify(1e-40, 0.0, 0.0)            # B below 2^-100
    assert not M.certify(1e-4, 0.0, 0.02)            # the root does not clear E
    assert M.certify(4.0, 1.0, E)
    with np.errstate(over="ignore"):
        big = np.full((4, 8), 1e6, dtype=np.float32)
    assert M.row_error(big) == np.inf                # overflows binary16: no bound, never eligible


@pytest.mark.parametrize("d", [64, 80])
def test_exact_model_on_trap_data(d):
    """The exact model (DeviceModel: the device's candidates, distance bits and order) on the trap data the GPU tests
    use.  trap_case asserts the conditions on the inputs: at least 3 queries whose rescored preselection is not the
    truth, none of them certified, both outcomes, no decision within 2^-30 of flipping, and three different certified
    counts at E, E / 2 and 2 E.  With E = 0 the same model certifies wrong answers: these inputs tell a broken bound
    from a sound one, which iid rows never do."""
    k = 10
    c, dec = M.trap_case(3000, d, k, 3, 192, seed=M.MAIN_SEED[d], three_counts=True)
    kp = M.default_keys(k)
    broken = c.model.decide(c.cands, kp, 0.0)
    assert broken.wrong >= 1, "E = 0 must certify a wrong answer on these data (%r)" % broken
    assert np.array_equal(broken.trap, dec.trap), "what the preselection holds does not depend on E"
    counts = [int(c.model.decide(c.cands, kp, e).certified.sum()) for e in (0.0, c.E / 2, c.E, 2 * c.E, 1e3)]
    assert counts == sorted(counts, reverse=True) and counts[-1] < counts[0], "a larger E certifies no more: %s" % counts
    # the sizes of the list: at K' = k + 1 the certificate can hold only where B > tau by the margin, and more keys can
    # only shrink the set of traps
    traps = [int(c.model.decide(c.cands, q, c.E).trap.sum()) for q in (k + 1, 16, 33, 64)]
    assert traps == sorted(traps, reverse=True) and traps[0] > traps[-1], traps
    for q in (k + 1, 16, 33, 64):
        assert c.model.decide(c.cands, q, c.E).wrong == 0
    # K' = k + 1: the row that has B is among the k + 1 rescored rows, and its exact distance alone keeps tau above LB
    assert not c.model.decide(c.cands, k + 1, c.E).certified.any()


def test_exact_model_is_the_stage1_of_the_cpu_engine():
    """The model's truth -- the k+1 smallest keys over the distinct valid candidates, on the numpy tree -- against
    CpuShardEngine.stage1_local, which computes every distance through the oracle's own tree: same ids, same bits."""
    import torch
    c, _ = M.trap_case(3000, 64, 10, 3, 192, seed=M.MAIN_SEED[64], three_counts=True)
    m, K1, qs = c.model, c.k + 1, 12
    y = np.array(c.y[:qs])
    codes = torch.from_numpy(m.eng.orc.query_codes(m.eng.hs, y).astype(np.uint32).view(np.int32).copy())
    cd, ci, _ = m.eng.stage1_local(torch.from_numpy(y), False, codes)
    for x, (ids, dh, dx) in enumerate(m.gather(y)):
        o = M.keys_sorted(dx, ids)[:K1]
        assert np.array_equal(ids[o], ci.numpy().view(np.uint32)[x])
        assert np.array_equal(dx[o].view(np.uint32), cd.numpy().view(np.uint32)[x])


def test_keys_clamp():
    assert [M.clamp_keys(10, a) for a in (0, 11, 16, 33, 64, 200, 5)] == [16, 11, 16, 33, 64, 64, 11]
    assert M.clamp_keys(31, 0) == 48 and M.clamp_keys(1, 0) == 16
