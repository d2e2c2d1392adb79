"""GPU: annhip_query_sorted_set at a row length of every layout code (tests/test_gpu_exact_knn.py::SWEEP), as
tests/test_gpu_sorted_layouts.py sweeps annhip_query_sorted: the set form of the scan (sorted_scan_kernel<D, V, true> and
sorted_scan_generic_kernel<true>) is instantiated once per code and validity form.

Per row length one small index (n = 700, kg = 6, T = 2) with 60 appended rows of which the last 20 come after sort_tags,
and one batch of 37 queries with sets of 0 to 7 intervals, unsplit and cut every 64 rows, with and without an allow list,
aliased and not, at k = kg and 100.  The ground truth is tests/test_gpu_sorted_set.py::_truth (exact_query per interval
rank, merged on the CPU).  Bit-exact on ids and distance bytes."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from tests.test_gpu_exact_knn import SWEEP_CASES
from tests.test_gpu_probe import _build_host, pts_bytes
from tests.test_gpu_query_k import _build
from tests.test_gpu_sorted import FULL, _scan_tile
from tests.test_gpu_sorted_set import _check, _sets, _set_runs_numpy, _truth

pytestmark = pytest.mark.gpu

N, KG, T, Q, M1, M2 = 700, 6, 2, 37, 40, 20


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_the_set_scan_at_every_layout(prec, d):
    orc, pts, tp, ix = (_build_host if d * pts_bytes(prec) > 4096 else _build)(prec, N, d, KG, T, 9700 + d)
    try:
        rng = np.random.default_rng(9800 + d)
        ix.set_fixed(True)  # (append needs it)
        y = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))).cuda()
        ya = tp[:Q].contiguous()
        rows = N + M1 + M2
        t = min(_scan_tile(prec, d), 100)  # (the value column's counts must fit n)
        tags = rng.integers(10, 20, size=rows).astype(np.uint32)
        where_rows = rng.permutation(N + M1)
        at = 0
        for val, c in ((1, 1), (2, max(t - 1, 1)), (3, t), (4, t + 1), (5, 3 * t + 5), (6, 3)):
            tags[where_rows[at:at + c]] = val
            at += c
        tail = np.ascontiguousarray(rng.standard_normal((M1 + M2, d)).astype(pts.dtype))
        ix.set_tags(tags[:N])
        ix.append(tail[:M1], tags=tags[N:N + M1])
        ix.sort_tags()
        ix.append(tail[M1:], tags=tags[N + M1:])
        assert ix.tag_order == (FULL, N + M1) and ix.n_total == rows
        where = A.where_in(FULL, _sets(Q))
        wl = _set_runs_numpy(tags[:N + M1], where)[1]
        assert (wl == 0).any() and (wl == N + M1).any() and ((wl > 64) & (wl < N + M1)).any()
        allow = rng.random(rows) < 0.4
        for form in ("plain", "allow"):
            ix.set_filter(allow if form == "allow" else None)
            for yy, alias in ((y, False), (ya, True)):
                for k in (None, 100):
                    what = "%s d=%d %s alias=%d k=%s" % (prec, d, form, alias, k)
                    want = _truth(ix, yy, where, k=k, alias=alias)
                    _check(ix, yy, where, what, want=want, k=k, alias=alias)
                    _, entries = _check(ix, yy, where, what + " split", want=want, k=k, alias=alias, split=64)
                    assert entries == A.set_pieces(*_set_runs_numpy(tags[:N + M1], where), 64)[0].size
    finally:
        ix.close()
