"""GPU: stage1_radius_kernel at a row length of every layout code (tests/test_gpu_exact_knn.py::SWEEP; tests/
test_layout_table.py proves the list complete), as tests/test_gpu_tail_hash_layouts.py sweeps the hashed tail.  The family
is instantiated once per code, segment form and row type -- its own lane map, chunk count and LDS carve-up.

Per row length one index (n = 1500, kg = 6, T = 2), 24 free and 24 aliased queries.  The +inf equality against
query(k=kcap): probe 0 and 3 x plain / allow list / where= / both, at kcap = kg, 1 and 100 (tests/test_gpu_layout_sweep.py
verifies those rows against numpy at every code).  Finite radii against the oracle of tests/test_gpu_radius.py: the plain
form, kcap = 100, both probe settings.  Rows longer than 4096 bytes take their tables from the oracle's host precomp
(tests/test_gpu_probe.py::_build_host).  Bit-exact on ids and distance bytes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_exact_knn import SWEEP_CASES
from tests.test_gpu_probe import _build_host, pts_bytes
from tests.test_gpu_query_k import Oracle, _build, _dict, _np, _same_bits, _tenants
from tests.test_gpu_radius import _eq3, _np3, cycle_radii, radius_rows, stage1_dists

pytestmark = pytest.mark.gpu

N, KG, T, Q = 1500, 6, 2, 24
KS = (KG, 1, 100)
FORMS = ("plain", "allow", "where", "allow+where")


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_the_radius_family_at_every_layout(prec, d):
    orc, pts, tp, ix = (_build_host if d * pts_bytes(prec) > 4096 else _build)(prec, N, d, KG, T, 9600 + d)
    try:
        rng = np.random.default_rng(9700 + d)
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))).cuda()
        ta = tp[:Q].contiguous()
        sd = _dict(ix)
        ix.set_fixed(True)
        allow = rng.random(N) < 0.4
        tags, where = _tenants(N, Q, 9800 + d)
        ix.set_tags(tags)
        inf = float("inf")
        partial = 0
        for yy, alias in ((ty, False), (ta, True)):
            for probe in (0, 3):
                ix.set_probe(probe)
                for form in FORMS:
                    ix.set_filter(allow if form.startswith("allow") else None)
                    kw = dict(alias=alias, **(dict(where=where) if form.endswith("where") else {}))
                    for kcap in KS:
                        what = "%s d=%d probe=%d %s alias=%d kcap=%d" % (prec, d, probe, form, alias, kcap)
                        base = _np(ix.query(yy, k=kcap, **kw))
                        got = _np3(ix.query_radius(yy, inf, k=kcap, **kw))
                        assert _same_bits(got[:2], base), what
                        assert np.array_equal(got[2], (base[0] != N).sum(axis=1)), what
                ix.set_filter(None)
                orac = Oracle(ix, sd, tp, yy, alias)
                rad = cycle_radii(stage1_dists(orac, 41))
                want = radius_rows(orac, 100, rad)
                partial += int(((want[2] > 0) & (want[2] < 100)).sum())
                assert (want[2] == 0).any()
                _eq3(_np3(ix.query_radius(yy, rad, k=100, alias=alias)), want, (prec, d, probe, alias))
        assert partial > 0
    finally:
        ix.close()
