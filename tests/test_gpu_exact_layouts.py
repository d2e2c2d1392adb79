"""GPU: the filtered and tagged exact scans (annhip_exact_knn_filtered, annhip_exact_knn_tagged; the EX_BITS and EX_TAGS
instances of exact_scan_kernel and exact_scan_generic_kernel) at a row length of every layout code, as tests/test_gpu_exact_knn.py::
test_every_layout does for the unfiltered scan.  The other bit-exact oracles of the suite (tests/test_gpu_query_k.py,
tests/test_gpu_tail.py) use these scans as their ground truth at whatever row length they run.

The expected answer is numpy alone: np_dists (the reference's halving tree, tied to the oracle's in
test_numpy_tree_is_the_oracles_tree), the columns a query may not see removed, then np.lexsort((ids, distance bits)).
Every comparison is on ids and distance bytes, every query.  Each case runs once as one row range and once split into
three (range starts 1001 and 2002: no multiple of 32, none of a tile), so a tile's first bitmap and tag word is met at an
offset inside a word."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from tests.test_gpu_exact_knn import SWEEP_CASES, normal, np_dists, ranges, same
from tests.test_gpu_query_k import _tenants

pytestmark = pytest.mark.gpu

N, Q, K = 3001, 53, 10  # Q: a ragged last group of 4 queries, a second workgroup with whole waves beyond the batch


def _bits(d):
    return d.view(np.uint32 if d.dtype == np.float32 else np.uint64)


def _expect(dist, valid, k):
    """The k smallest (distance bits, id) of every query among its valid columns."""
    ids = np.empty((dist.shape[0], k), dtype=np.int64)
    dd = np.empty((dist.shape[0], k), dtype=dist.dtype)
    for q in range(dist.shape[0]):
        cols = np.flatnonzero(valid[q])
        assert cols.size >= k  # the cases below leave every query at least k rows: no pads here
        o = cols[np.lexsort((cols, _bits(dist[q, cols])))[:k]]
        ids[q], dd[q] = o, dist[q, o]
    return ids, dd


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_filtered_and_tagged_scan_at_every_layout(prec, d):
    pts, y = normal(prec, N, d, Q, 2000 + d)
    tp = torch.from_numpy(pts).cuda()
    allow = np.random.default_rng(3000 + d).random(N) < 0.4
    tallow = torch.from_numpy(allow).cuda()
    tags, where = _tenants(N, Q, 4000 + d)  # a mixed-tenant batch: tenants 0, 1, 2 and "everything" in turn
    tagged = (tags[None, :] & where[0][:, None]) == where[1][:, None]
    forms = [("allow", dict(allow=tallow), np.broadcast_to(allow, (Q, N))),
             ("tags", dict(tags=tags, where=where), tagged),
             ("allow+tags", dict(allow=tallow, tags=tags, where=where), tagged & allow[None, :])]
    for yy, alias in ((y, False), (np.ascontiguousarray(pts[:Q]), True)):
        ty = torch.from_numpy(yy).cuda()
        dist = np_dists(pts, yy)
        everything = np.ones((Q, N), dtype=bool)
        if alias:
            everything[np.arange(Q), np.arange(Q)] = False
        plain = _expect(dist, everything, K)
        for name, kw, valid in forms:
            want = _expect(dist, valid & everything, K)
            changed = int((want[0] != plain[0]).any(axis=1).sum())
            assert 2 * changed >= Q, (name, changed)  # the filter decides the answer of at least half the queries
            for r in (None, 3):
                what = "%s d=%d %s alias=%d ranges=%s" % (prec, d, name, alias, r)
                if r is None:
                    got10 = A.exact_knn(tp, ty, K, self_exclude=alias, **kw)
                    got1 = A.exact_knn(tp, ty, 1, self_exclude=alias, **kw)
                else:
                    with ranges(r):
                        got10 = A.exact_knn(tp, ty, K, self_exclude=alias, **kw)
                        got1 = A.exact_knn(tp, ty, 1, self_exclude=alias, **kw)
                same((got10[0].cpu().numpy(), got10[1].cpu().numpy()), want, what + " k=10")
                same((got1[0].cpu().numpy(), got1[1].cpu().numpy()), (want[0][:, :1], want[1][:, :1]), what + " k=1")
