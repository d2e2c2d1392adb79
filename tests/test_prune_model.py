"""CPU: the certificate of the pruned stage 1 (annhip_index_set_prune), restated in numpy on float32 data.  Whenever it
certifies a query, the true k+1 smallest keys over ALL candidates lie inside the preselection made on the binary16 rows,
so rescoring the preselection gives exactly them.  It must never certify wrongly; it may refuse as often as it likes,
but the tests also pin that it is not vacuous (iid rows certify) and that it does refuse where it has to (scaled rows)."""
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
