"""GPU: the sorted scan at a row length of every layout code (tests/test_gpu_exact_knn.py::SWEEP; tests/test_layout_table.py
proves the list complete), as tests/test_gpu_tail_hash_layouts.py sweeps the hashed tail.  sorted_scan_kernel is
instantiated once per code and validity form -- its own lane map, chunk count, wave count and LDS carve-up -- and the
generic form serves the codes without a register layout.

Per row length one small index (n = 700, kg = 6, T = 2) with 60 appended rows of which the last 20 come after sort_tags,
and one batch of 37 queries with identical, disjoint and ragged (nested, overlapping, empty) runs, with and without an
allow list, aliased and not, at k = kg, 1 and 100.  The oracle is Index.exact_query(where=(M, qlo, qhi)), as in
tests/test_gpu_sorted.py.  Rows longer than 4096 bytes take their tables from the oracle's host precomp.  Bit-exact on ids
and distance bytes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_exact_knn import SWEEP_CASES
from tests.test_gpu_probe import _build_host, pts_bytes
from tests.test_gpu_query_k import _build
from tests.test_gpu_sorted import FULL, _eq, _intervals, _runs_numpy, _scan_tile

pytestmark = pytest.mark.gpu

N, KG, T, Q, M1, M2 = 700, 6, 2, 37, 40, 20
KS = (None, 1, 100)


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_the_sorted_scan_at_every_layout(prec, d):
    orc, pts, tp, ix = (_build_host if d * pts_bytes(prec) > 4096 else _build)(prec, N, d, KG, T, 9700 + d)
    try:
        rng = np.random.default_rng(9800 + d)
        ix.set_fixed(True)  # (append needs it)
        y = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))).cuda()
        ya = tp[:Q].contiguous()
        rows = N + M1 + M2
        t = min(_scan_tile(prec, d), 100)  # (the value column's counts must fit n)
        tags = rng.integers(10, 20, size=rows).astype(np.uint32)
        where = rng.permutation(N + M1)
        at = 0
        for val, c in ((1, 1), (2, max(t - 1, 1)), (3, t), (4, t + 1), (5, 3 * t + 5), (6, 3)):
            tags[where[at:at + c]] = val
            at += c
        tail = np.ascontiguousarray(rng.standard_normal((M1 + M2, d)).astype(pts.dtype))
        ix.set_tags(tags[:N])
        ix.append(tail[:M1], tags=tags[N:N + M1])
        ix.sort_tags()
        ix.append(tail[M1:], tags=tags[N + M1:])
        assert ix.tag_order == (FULL, N + M1) and ix.n_total == rows
        qlo, qhi = _intervals(Q)
        wl = _runs_numpy(tags, FULL, qlo, qhi)[1]
        assert (wl == 0).any() and (wl == rows).any() and (wl == 3).any() and ((wl > 3) & (wl < rows)).sum() > 10
        allow = rng.random(rows) < 0.4
        for form in ("plain", "allow"):
            ix.set_filter(allow if form == "allow" else None)
            for yy, alias in ((y, False), (ya, True)):
                for k in KS:
                    _eq(ix, yy, FULL, qlo, qhi, "%s d=%d %s alias=%d k=%s" % (prec, d, form, alias, k), k=k, alias=alias)
    finally:
        ix.close()
