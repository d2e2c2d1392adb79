"""GPU: the hashed tail's kernel at a row length of every layout code (tests/test_gpu_exact_knn.py::SWEEP; tests/
test_layout_table.py proves the list complete), as tests/test_gpu_layout_sweep.py sweeps the exact tail.
tail_hash_merge_kernel is instantiated once per code and validity form -- its own lane map, chunk count, wave count and LDS
carve-up -- and the generic form serves the codes without a register layout.

Per row length one index (n = 1500, kg = 6, T = 2), 24 fresh and 24 aliased queries, 700 appended rows of which the first
500 are hashed; probe 0 and 3 x none / allow list / where= / both, at k = kg, 1 and 100.  R(q) is what the index itself
returns BEFORE the rows are appended (tests/test_gpu_layout_sweep.py verifies those rows against numpy at every code); the
tail side is the numpy expectation of tests/test_gpu_tail_hash.py.  Rows longer than 4096 bytes take their tables from the
oracle's host precomp (tests/test_gpu_probe.py::_build_host).  Bit-exact on ids and distance bytes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_exact_knn import SWEEP_CASES
from tests.test_gpu_probe import _build_host, pts_bytes
from tests.test_gpu_query_k import _build, _np, _tenants
from tests.test_gpu_tail_hash import Expect, _eq, _nonvacuous, _valid, _want

pytestmark = pytest.mark.gpu

N, KG, T, Q, M, MH = 1500, 6, 2, 24, 700, 500
KS = (KG, 1, 100)
FORMS = ("plain", "allow", "where", "allow+where")


def _settings(ix, form, allow, tags):
    ix.set_tags(tags)
    ix.set_filter(allow if form.startswith("allow") else None)


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_the_hashed_tail_at_every_layout(prec, d):
    orc, pts, tp, ix = (_build_host if d * pts_bytes(prec) > 4096 else _build)(prec, N, d, KG, T, 9100 + d)
    try:
        rng = np.random.default_rng(9400 + d)
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))).cuda()
        ta = tp[:Q].contiguous()
        ix.set_fixed(True)
        allow = rng.random(N + M) < 0.4
        tags, where = _tenants(N + M, Q, 9500 + d)
        batches = ((ty, False), (ta, True))

        def calls(form, alias):
            return dict(alias=alias, **(dict(where=where) if form.endswith("where") else {}))

        base = {}
        for yy, alias in batches:
            for probe in (0, 3):
                ix.set_probe(probe)
                for form in FORMS:
                    _settings(ix, form, allow[:N], tags[:N])
                    for k in KS:
                        base[(alias, probe, form, k)] = _np(ix.query(yy, k=k, **calls(form, alias)))
        ix.set_filter(None), ix.set_tags(None)

        tail = np.ascontiguousarray(rng.standard_normal((M, d)).astype(pts.dtype))
        tail[5] = pts[7]  # a duplicate of a built row
        ttail = torch.from_numpy(tail).cuda()
        assert ix.append(ttail[:MH].contiguous()) == N
        ix.hash_tail()
        ix.append(ttail[MH:].contiguous())
        assert ix.tail == M and ix.tail_hashed == MH
        for yy, alias in batches:
            for probe in (0, 3):
                ix.set_probe(probe)
                exp = Expect(ix, ttail, yy, MH)
                for form in FORMS:
                    _settings(ix, form, allow, tags)
                    valid = _valid(Q, M, N, allow if form.startswith("allow") else None,
                                   *((tags, where) if form.endswith("where") else (None, None)))
                    knn = exp.knn(max(KS), valid)
                    for k in KS:
                        what = "%s d=%d probe=%d %s alias=%d k=%d" % (prec, d, probe, form, alias, k)
                        want = _want(exp, base[(alias, probe, form, k)], N, k, knn)
                        _eq(_np(ix.query(yy, k=k, **calls(form, alias))), want, what)
                        if k == KG:
                            _eq(_np(ix.query(yy, **calls(form, alias))), want, what + " plain call")
                            if form == "plain":
                                _nonvacuous(exp, want, N, base[(alias, probe, form, k)])
    finally:
        ix.close()
