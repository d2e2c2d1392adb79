"""GPU: the pruned stage 1 at a row length of every layout code (tests/test_gpu_exact_knn.py::SWEEP; tests/
test_layout_table.py proves the list complete).  prune_rescore_kernel<D> is instantiated for every register layout, and
the narrow preselection keeps K' > k + 1 keys at the same codes; a row length whose code is generic (0 and the two
generic fold codes) has no pruned path and must say so.  The data are the trap data of tests/prune_model.py, so every
register layout is run where the certificate has to refuse: pruned = native = oracle on ids and distance bits, and the
count of refused queries is the exact model's."""
import numpy as np
import pytest
import torch

from approximatenn_amd import _lib
from tests import prune_model as M
from tests.test_gpu_exact_knn import SWEEP
from tests.test_gpu_prune_certificate import _index, _np, _prune_on, _run, _same
from tests.test_layout_table import FOLD4G, FOLD5G

pytestmark = pytest.mark.gpu

N, K, T, Q = 2000, 10, 3, 96
GENERIC = (0, FOLD4G, FOLD5G)  # no register layout: layout_is_generic (ann_host.hip)


def test_the_sweep_has_both_kinds():
    codes = {d: _lib.load("f32").annhip_layout_code(d) for d in SWEEP["f32"]}
    assert {c for c in codes.values() if c in GENERIC} == set(GENERIC)
    assert len({c for c in codes.values() if c not in GENERIC}) >= 20


@pytest.mark.parametrize("d", SWEEP["f32"])
def test_every_layout(d):
    code = _lib.load("f32").annhip_layout_code(d)
    c, dec_np = M.trap_case(N, d, K, T, Q, ladder=False)
    ix, tp = _index(c)
    try:
        ty = torch.from_numpy(np.array(c.y)).cuda()
        assert not ix.prune
        _same(_np(ix.query(ty)), c.want, "native d=%d" % d)
        if code in GENERIC:
            with pytest.raises(ValueError):
                ix.set_prune("on")
            assert not ix.prune and ix.prune_bound is None
            ix.set_prune("auto")
            assert not ix.prune and ix.prune_bound is None
            got, unc = _run(ix, ty)
            _same(got, c.want, "d=%d (code %d) after the refusal" % (d, code))
            assert unc == 0
            return
        E, kp = _prune_on(ix, M.default_keys(K), c.pts)
        dec = c.model.decide(c.cands, kp, E)
        dec.check("d=%d at the device's E" % d)
        got, unc = _run(ix, ty)
        print("d=%d code=%d: %r; device uncertified %d" % (d, code, dec, unc))
        _same(got, c.want, "pruned d=%d (code %d)" % (d, code))
        assert unc == dec.uncertified, "d=%d (code %d): the device refused %d queries, the model %d" % (
            d, code, unc, dec.uncertified)
    finally:
        ix.close()
