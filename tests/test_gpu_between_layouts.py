"""GPU: the range predicate at a row length of every layout code (tests/test_gpu_exact_knn.py::SWEEP; tests/
test_layout_table.py proves the list complete), as tests/test_gpu_radius_layouts.py sweeps the radius family.  The tag
kernels of stage 1 and stage 2, the k-per-call stage 2, the exact scan's EX_TAGS form and the tail merge are instantiated
once per code -- each with its own lane map, chunk count and LDS carve-up -- and all of them evaluate the interval.

Per row length one index (n = 1500, kg = 6, T = 2), 24 free and 24 aliased queries, the first four predicates of
tests/test_gpu_between.py dealt over the batch; query(where=triple), query(k=100, where=triple) and exact_query(where=triple)
against the bitmap path group by group, without and with a 40-row tail, at probe 0 and 3.  Rows longer than 4096 bytes take
their tables from the oracle's host precomp (tests/test_gpu_probe.py::_build_host).  Bit-exact on ids and distance bytes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_between import PRED, _eq, _np, _oracle, _tags, _triple
from tests.test_gpu_exact_knn import SWEEP_CASES
from tests.test_gpu_probe import _build_host, pts_bytes
from tests.test_gpu_query_k import _build

pytestmark = pytest.mark.gpu

N, KG, T, Q, M = 1500, 6, 2, 24, 40
FOUR = PRED[:4]


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_the_range_predicate_at_every_layout(prec, d):
    orc, pts, tp, ix = (_build_host if d * pts_bytes(prec) > 4096 else _build)(prec, N, d, KG, T, 9900 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))).cuda()
        ta = tp[:Q].contiguous()
        tail = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(M * d).reshape(M, d))).cuda()
        tags = np.concatenate([_tags(N, KG, 9950 + d), _tags(M, KG, 9960 + d)])
        w = _triple(Q, FOUR)
        ix.set_fixed(True)
        ix.set_tags(tags[:N])
        for m in (0, M):
            if m:
                ix.append(tail, tags=tags[N:])
            tg = tags[:N + m]
            for probe in (0, 3):
                ix.set_probe(probe)
                for yy, alias in ((ty, False), (ta, True)):
                    what = "%s d=%d tail=%d probe=%d alias=%d" % (prec, d, m, probe, alias)
                    for kw in ({}, {"k": 100}):
                        want = _oracle(ix, lambda: _np(ix.query(yy, alias=alias, **kw)), Q, tg, pred=FOUR)
                        _eq(_np(ix.query(yy, alias=alias, where=w, **kw)), want, (what, kw))
                    if probe == 0:  # the exact scan does not read the probe setting
                        want = _oracle(ix, lambda: _np(ix.exact_query(yy, alias=alias)), Q, tg, pred=FOUR)
                        _eq(_np(ix.exact_query(yy, alias=alias, where=w)), want, (what, "exact"))
    finally:
        ix.close()
