"""GPU: the stand-alone rerank (annhip_rerank) over one row length per layout code -- every rerank_kernel<D> instance and
rerank_generic_kernel (ann_rerank_kernels.h).  SWEEP_CASES of tests/test_gpu_exact_knn.py has a row length for every code,
which tests/test_layout_table.py proves.  Bit-exact against the numpy expectation of tests/test_gpu_rerank.py; no index is
built, so rows of more than 4096 bytes are served too."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from tests.test_gpu_exact_knn import SWEEP_CASES, normal, np_dists
from tests.test_gpu_rerank import expect, same

pytestmark = pytest.mark.gpu

N, QN, CN = 1500, 24, 100


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_every_layout(prec, d):
    pts, y = normal(prec, N, d, QN, 8100 + d)
    dist = np_dists(pts, y)
    rng = np.random.default_rng(8101 + d)
    cand = rng.integers(0, N, size=(QN, CN)).astype(np.int64)
    hit = rng.random((QN, CN)) < 0.1
    cand[hit] = np.array([N, -1, 2 ** 32 + 5], dtype=np.int64)[rng.integers(0, 3, size=int(hit.sum()))]
    cand[:, 70] = cand[:, 3]  # a duplicate for every query, in another 64-entry block
    cand[:, 4] = cand[:, 3]   # and one beside it
    cand[0, 7:] = N           # fewer than 10 distinct ids
    assert (cand == N).any() and (cand == -1).any() and (cand == 2 ** 32 + 5).any()
    tp, ty, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(cand).cuda()
    want = expect(dist, cand, 10, N)
    assert (want[0][0] == N).any() and (want[0][1:] < N).all()
    same(A.rerank(tp, ty, tc, 10), want, "%s d=%d k=10" % (prec, d))
    same(A.rerank(tp, ty, tc, 1), (want[0][:, :1], want[1][:, :1]), "%s d=%d k=1" % (prec, d))
