"""GPU: stage 1's running selection on free-standing key streams (annhip_test_select, include/ann_hip.h): the kernel
behind the hook calls the device functions stage1_select_kernel calls -- the offer of one gather pass and wave 0's merge
of the W waves' results -- in the register form (K1 <= 128) and in the LDS form.  The contract is exact: the K1 smallest
DISTINCT (distance, id) keys of the stream, ascending, padded with (+inf, 0xFFFFFFFF).  numpy says what they are:
np.unique over the (distance bits, id) pairs sorts them in the kernels' key order (distances are >= +0, so their bit
patterns order like the values).  Both libraries: a key is one u64 in f32 and a struct of two in f64."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A

pytestmark = pytest.mark.gpu

PAD_ID = 0xFFFFFFFF
ORDERS = ("ascending", "descending", "identical", "repeated", "equal_dist", "inf")


def _ft(prec):
    return (np.float32, np.uint32) if prec == "f32" else (np.float64, np.uint64)


def _stream(order, cnt, ft, rng):
    """cnt keys: (dist [cnt] ft, id [cnt] uint32)."""
    ids = rng.permutation(4 * cnt + 8)[:cnt].astype(np.uint32)
    dist = np.sort(rng.random(cnt) + 0.25).astype(ft)
    if order == "ascending":        # distinct after rounding or not: the ids are distinct, so the keys are
        pass                        # nothing after the first K1 keys passes the threshold
    elif order == "descending":     # every key enters the list
        dist = dist[::-1].copy()
    elif order == "identical":      # one key, cnt times
        dist[:] = 1.5
        ids[:] = 7
    elif order == "repeated":       # every key occurs 1..4 times, shuffled
        src = np.repeat(np.arange(cnt), rng.integers(1, 5, size=cnt))[:cnt]
        src = rng.permutation(src)
        dist, ids = dist[src], ids[src]
    elif order == "equal_dist":     # one distance, distinct ids: the id half of the key decides
        dist[:] = 2.0
    elif order == "inf":            # +inf is an ordinary distance for the selection: (inf, id) keys sort by id, after the finite ones
        dist[rng.random(cnt) < 0.7] = np.inf
    return np.ascontiguousarray(dist), np.ascontiguousarray(ids)


def _want(dist, ids, K1, ft, bt):
    keys = np.stack([dist.view(bt).astype(np.uint64), ids.astype(np.uint64)], axis=1)
    keys = np.unique(keys, axis=0)[:K1]          # lexicographic (distance bits, id), distinct
    wd = np.full(K1, np.inf, dtype=ft)
    wi = np.full(K1, PAD_ID, dtype=np.uint32)
    wd[:len(keys)] = keys[:, 0].astype(bt).view(ft)
    wi[:len(keys)] = keys[:, 1].astype(np.uint32)
    return wd, wi


def _cases(K1, ft, seed):
    rng = np.random.default_rng(seed)
    cnts = sorted({0, 1, K1 - 1, K1, K1 + 1, 63, 64, 65, 1000})
    return [(order, cnt) + _stream(order, cnt, ft, rng) for order in ORDERS for cnt in cnts]


def _run(lib, cases, K1, W, lds, ft):
    off = np.zeros(len(cases) + 1, dtype=np.int64)
    off[1:] = np.cumsum([c[1] for c in cases])
    dist = np.concatenate([c[2] for c in cases] + [np.zeros(1, dtype=ft)])   # (never empty)
    ids = np.concatenate([c[3] for c in cases] + [np.zeros(1, dtype=np.uint32)])
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    t_d, t_i = torch.from_numpy(dist).cuda(), torch.from_numpy(ids.view(np.int32)).cuda()
    od = torch.zeros((len(cases), K1), dtype=t_d.dtype, device="cuda")
    oi = torch.zeros((len(cases), K1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.annhip_test_select(len(cases), t_off.data_ptr(), t_d.data_ptr(), t_i.data_ptr(), K1, W, lds, od.data_ptr(), oi.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return od.cpu().numpy(), oi.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("K1", [1, 11, 16, 63, 64, 65, 128])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_selection_equals_numpy(prec, K1):
    lib = A._lib.load(prec)
    ft, bt = _ft(prec)
    cases = _cases(K1, ft, 100 + K1)
    want = [_want(c[2], c[3], K1, ft, bt) for c in cases]
    for lds in (0, 1):          # the register list, and the LDS buffer the other layouts and K1 > 128 keep
        for W in (1, 2, 4):
            gd, gi = _run(lib, cases, K1, W, lds, ft)
            for x, (c, (wd, wi)) in enumerate(zip(cases, want)):
                what = "%s K1=%d W=%d lds=%d %s cnt=%d" % (prec, K1, W, lds, c[0], c[1])
                assert np.array_equal(gi[x], wi), (what, gi[x], wi)
                assert np.array_equal(gd[x].view(bt), wd.view(bt)), (what, gd[x], wd)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lds_form_beyond_the_register_range_and_refusals(prec):
    lib = A._lib.load(prec)
    ft, bt = _ft(prec)
    K1 = 129                    # the first K1 the register list does not hold
    cases = _cases(K1, ft, 300)
    gd, gi = _run(lib, cases, K1, 4, 1, ft)
    for x, c in enumerate(cases):
        wd, wi = _want(c[2], c[3], K1, ft, bt)
        assert np.array_equal(gi[x], wi) and np.array_equal(gd[x].view(bt), wd.view(bt)), (c[0], c[1])
    assert lib.annhip_test_select(1, None, None, None, 129, 4, 0, None, None) == -1    # registers: K1 <= 128
    assert lib.annhip_test_select(1, None, None, None, 0, 4, 0, None, None) == -1
    assert lib.annhip_test_select(1, None, None, None, 16, 5, 0, None, None) == -1
    assert lib.annhip_test_select(1, None, None, None, 257, 4, 1, None, None) == -1
