"""GPU: exact brute-force k nearest neighbours (annhip_exact_knn, include/ann_hip.h; kernels in ann_exact_kernels.h).

The expected answer is computed here with numpy: squared differences in the test's dtype, the reference's in-place halving
tree written as whole-array operations over the last axis, then np.lexsort((ids, dist))[:k] -- the order (distance, id).
The numpy tree is tied to the oracle's oracle_tree_sum (CpuBackend.tree_sum) pair by pair in the first test.  Every
comparison is on bits, ids and distances, every query."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests.util import bits_equal, load_golden

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
# a row length for every code annhip_layout_code(d) returns (the lists of tests/test_gpu_rows_f16.py::LAYOUTS and
# tests/test_layout_table.py::F64), plus 100 and 131; 40 in f32 is code -82 (5 lanes x 2 chunks), which those lists lack
D_F32 = [128, 80, 96, 160, 192, 320, 384, 24, 48, 28, 280, 112, 224, 100, 70, 50, 36, 150, 30, 260, 300, 2084, 131, 40]
D_F64 = [128, 512, 1024, 40, 80, 48, 96, 160, 192, 12, 24, 20, 14, 28, 56, 112, 100, 36, 33, 150, 300, 2084, 131]
LAYOUT_CASES = [("f32", d) for d in D_F32] + [("f64", d) for d in D_F64]
# the lists above plus every power of two the layout table holds (RowLay<D>): the row lengths the filtered and tagged
# scans, the fixed-mode query families and the tail are swept over.  tests/test_layout_table.py proves that no row
# length in 1..4096 has a code that SWEEP lacks.
SWEEP = {"f32": D_F32 + [16, 32, 64, 256, 512, 1024], "f64": D_F64 + [16, 32, 64, 256]}
SWEEP_CASES = [(p, d) for p in ("f32", "f64") for d in SWEEP[p]]


def np_tree(m):
    """oracle_tree_sum over the last axis of m (consumed): halves at every level, the odd element folded into z == 0."""
    s = m.shape[-1]
    while s >> 1:
        h = s >> 1
        g = np.zeros(m.shape[:-1] + (h,), dtype=m.dtype)
        if s & 1:
            g[..., 0] = m[..., s - 1]
        m[..., :h] = m[..., :h] + (m[..., h:2 * h] + g)
        s = h
    return m[..., 0].copy()


def np_dists(points, y):
    """[Q, n] squared distances in the arrays' dtype, by the tree"""
    out = np.empty((y.shape[0], points.shape[0]), dtype=points.dtype)
    step = max(1, 20_000_000 // (points.shape[0] * points.shape[1]))
    with np.errstate(over="ignore", invalid="ignore"):
        for q0 in range(0, y.shape[0], step):
            df = y[q0:q0 + step, None, :] - points[None, :, :]
            out[q0:q0 + step] = np_tree(df * df)
    return out


def np_exact(points, y, k, self_exclude=False):
    dist = np_dists(points, y)
    n = points.shape[0]
    ids = np.arange(n)
    want_i = np.empty((y.shape[0], k), dtype=np.int64)
    want_d = np.empty((y.shape[0], k), dtype=points.dtype)
    for q in range(y.shape[0]):
        order = np.lexsort((ids, dist[q]))
        if self_exclude:
            order = order[order != q]
        want_i[q] = order[:k]
        want_d[q] = dist[q][order[:k]]
    return want_i, want_d


def gpu_exact(points, y, k, self_exclude=False):
    ids, dd = A.exact_knn(torch.from_numpy(points).cuda(), torch.from_numpy(y).cuda(), k, self_exclude=self_exclude)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (y.shape[0], k) and tuple(dd.shape) == (y.shape[0], k)
    return ids.cpu().numpy(), dd.cpu().numpy()


def same(got, want, what):
    bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
    assert bad.size == 0, "%s: ids differ for %d queries, first %d: got %s want %s" % (
        what, bad.size, bad[0], got[0][bad[0]][:12], want[0][bad[0]][:12])
    assert bits_equal(got[1], want[1]), "%s: distances not bit-identical" % what


def normal(prec, n, d, Q, seed):
    rng = np.random.default_rng(seed)
    return (np.ascontiguousarray(rng.standard_normal((n, d)).astype(NP[prec])),
            np.ascontiguousarray(rng.standard_normal((Q, d)).astype(NP[prec])))


def lattice(prec, n, d, Q, seed):
    rng = np.random.default_rng(seed)
    return (np.ascontiguousarray(rng.integers(-2, 3, (n, d)).astype(NP[prec])),
            np.ascontiguousarray(rng.integers(-2, 3, (Q, d)).astype(NP[prec])))


class ranges:
    """ANN_HIP_EXACT_RANGES: the number of row ranges the scan is split into (a test switch of the library)"""

    def __init__(self, r):
        self.r = r

    def __enter__(self):
        os.environ["ANN_HIP_EXACT_RANGES"] = str(self.r)
        A._lib.reload_env()

    def __exit__(self, *a):
        os.environ.pop("ANN_HIP_EXACT_RANGES", None)
        A._lib.reload_env()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_numpy_tree_is_the_oracles_tree(prec):
    orc = O.CpuBackend(prec, "oracle")
    rng = np.random.default_rng(5)
    for d in (1, 2, 3, 5, 7, 32, 80, 100, 128, 131, 256):
        v = (rng.standard_normal((30, d)) ** 2).astype(NP[prec])
        got = np_tree(v.copy())
        want = np.array([orc.tree_sum(row) for row in v], dtype=NP[prec])
        assert bits_equal(got, want), d


@pytest.mark.parametrize("prec,d", LAYOUT_CASES, ids=["%s-d%d" % c for c in LAYOUT_CASES])
def test_every_layout(prec, d):
    pts, y = normal(prec, 3001, d, 37, 1000 + d)
    dist = np_dists(pts, y)
    order = np.stack([np.lexsort((np.arange(pts.shape[0]), dist[q]))[:10] for q in range(y.shape[0])])
    want = (order, np.take_along_axis(dist, order, axis=1))
    same(gpu_exact(pts, y, 10), want, "%s d=%d k=10" % (prec, d))
    same(gpu_exact(pts, y, 1), (want[0][:, :1], want[1][:, :1]), "%s d=%d k=1" % (prec, d))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("d", [1, 2, 3, 5, 7, 16])
def test_small_d(prec, d):
    pts, y = normal(prec, 777, d, 21, 50 + d)
    same(gpu_exact(pts, y, 10), np_exact(pts, y, 10), "%s d=%d" % (prec, d))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ties_on_the_integer_lattice(prec):
    pts, y = lattice(prec, 2000, 32, 64, 9)
    pts[900] = pts[5]
    pts[1999] = pts[5]  # the same row at ids 5, 900 and 1999
    y[0] = pts[5]
    want = np_exact(pts, y, 10)
    tied = sum(len(set(row.tolist())) < 10 for row in want[1])
    assert tied >= 60, tied  # nearly every query has equal distances inside its top 10: a wrong tie order cannot pass
    assert want[0][0][:3].tolist() == [5, 900, 1999]
    same(gpu_exact(pts, y, 10), want, "lattice")
    # a tie exactly at rank k: query 0 has three rows at distance 0; k = 1 and k = 2 cut through them
    for k in (1, 2):
        got = gpu_exact(pts, y, k)
        same(got, (want[0][:, :k], want[1][:, :k]), "lattice k=%d" % k)
        assert got[0][0].tolist() == [5, 900][:k]
    # and a tie at rank k for every query that has one at rank 10
    full = np_exact(pts, y, 11)
    assert (full[1][:, 9] == full[1][:, 10]).sum() > 10


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_self_exclude(prec):
    pts, _ = normal(prec, 1500, 80, 1, 77)
    Q = 200
    y = np.ascontiguousarray(pts[:Q])
    got = gpu_exact(pts, y, 10, self_exclude=True)
    same(got, np_exact(pts, y, 10, self_exclude=True), "self")
    assert not (got[0] == np.arange(Q)[:, None]).any()
    plain = gpu_exact(pts, y, 10)
    same(plain, np_exact(pts, y, 10), "no self")
    assert (plain[0][:, 0] == np.arange(Q)).all() and (plain[1][:, 0] == 0).all()


def test_k100_f64_d256_cfg5_shape():
    pts, y = normal("f64", 20000, 256, 24, 3)
    same(gpu_exact(pts, y, 100), np_exact(pts, y, 100), "k=100")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_k1024(prec):
    pts, y = normal(prec, 1500, 32, 9, 4)
    same(gpu_exact(pts, y, 1024), np_exact(pts, y, 1024), "k=1024")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_k_equals_n(prec):
    pts, _ = normal(prec, 40, 24, 1, 6)
    y = np.ascontiguousarray(pts[:13])
    same(gpu_exact(pts, y, 40), np_exact(pts, y, 40), "k=n")
    same(gpu_exact(pts, y, 39, self_exclude=True), np_exact(pts, y, 39, self_exclude=True), "k=n-1 self")


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [70, 100003])
def test_row_ranges_by_size(prec, n):
    pts, y = normal(prec, n, 16, 5, n)
    same(gpu_exact(pts, y, 10), np_exact(pts, y, 10), "n=%d" % n)


@pytest.mark.parametrize("prec,d", [("f32", 128), ("f32", 80), ("f64", 100), ("f32", 2084), ("f64", 3)])
def test_forced_row_ranges_agree(prec, d):
    pts, y = lattice(prec, 2503, d, 19, d)  # ties across the range boundaries
    want = np_exact(pts, y, 10)
    for r in (1, 2, 7, 33):
        with ranges(r):
            same(gpu_exact(pts, y, 10), want, "ranges=%d" % r)
            same(gpu_exact(pts, np.ascontiguousarray(pts[:19]), 10, self_exclude=True),
                 np_exact(pts, np.ascontiguousarray(pts[:19]), 10, self_exclude=True), "ranges=%d self" % r)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("Q", [1, 10007])
def test_batch_sizes(prec, Q):
    pts, y = normal(prec, 300, 16, Q, Q)
    same(gpu_exact(pts, y, 10), np_exact(pts, y, 10), "Q=%d" % Q)


def test_overflow_to_inf_sorts_last_by_id():
    pts, y = normal("f32", 500, 32, 6, 8)
    far = [3, 17, 200, 499]
    pts[far] = np.float32(3e19)
    pts[far, ::2] = np.float32(-3e19)
    want = np_exact(pts, y, 500)
    assert np.isinf(want[1][:, -4:]).all() and (want[0][:, -4:] == np.array(far)).all()
    same(gpu_exact(pts, y, 500), want, "inf")
    y[2] = np.float32(3e19)  # every distance of this query overflows: ids ascending
    want = np_exact(pts, y, 20)
    assert np.isinf(want[1][2]).sum() >= 15
    same(gpu_exact(pts, y, 20), want, "inf query")


def test_refusals_leave_the_outputs_untouched():
    pts, y = normal("f32", 50, 16, 4, 1)
    tp, ty = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda()
    for k, se in ((0, False), (1025, False), (51, False), (50, True)):
        ids = torch.full((4, max(k, 1)), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((4, max(k, 1)), -7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError):
            A.exact_knn(tp, ty, k, self_exclude=se, out_ids=ids, out_dists=dd)
        torch.cuda.synchronize()
        assert (ids == -7).all() and (dd == -7.0).all()
    with pytest.raises(ValueError):
        A.exact_knn(tp, ty.double(), 5)
    with pytest.raises(ValueError):
        A.exact_knn(tp.double(), ty, 5)
    A.exact_knn(tp, ty, 50)  # k = n is served
    A.exact_knn(tp, ty, 49, self_exclude=True)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_host_call_equals_the_device_call(prec):
    pts, y = normal(prec, 999, 80, 33, 12)
    lib = A._lib.load(prec)
    for se, yy in ((0, y), (1, np.ascontiguousarray(pts[:33]))):
        ids = np.zeros((33, 7), dtype=np.uint64)
        dd = np.zeros((33, 7), dtype=NP[prec])
        assert lib.annhip_exact_knn_host(999, 80, 7, pts.ctypes.data, 33, yy.ctypes.data, se, ids.ctypes.data, dd.ctypes.data) == 0
        dev = gpu_exact(pts, yy, 7, self_exclude=bool(se))
        same((ids.astype(np.int64), dd), dev, "host call")
        same(dev, np_exact(pts, yy, 7, self_exclude=bool(se)), "device call")
    before = ids.copy()
    assert lib.annhip_exact_knn_host(999, 80, 0, pts.ctypes.data, 33, y.ctypes.data, 0, ids.ctypes.data, dd.ctypes.data) != 0
    assert np.array_equal(ids, before)


@pytest.mark.parametrize("prec,narrow", [("f32", "f16"), ("f64", "f32")])
def test_index_exact_query(prec, narrow):
    pts, y = normal(prec, 2000, 64, 50, 21)
    tp, ty = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda()
    O.srandom(5)
    ix = A.Index.precomp(tp, 7, 4)
    try:
        for alias, yy in ((False, ty), (True, tp[:50].contiguous())):
            want = A.exact_knn(tp, yy, 7, self_exclude=alias)
            got = ix.exact_query(yy, alias=alias)
            assert torch.equal(got[0], want[0]) and bits_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
            same((got[0].cpu().numpy(), got[1].cpu().numpy()), np_exact(pts, yy.cpu().numpy(), 7, self_exclude=alias), "index")
        ix.set_rows(narrow)  # exact_query reads the native rows whatever the query path is set to
        got = ix.exact_query(ty)
        want = A.exact_knn(tp, ty, 7)
        assert torch.equal(got[0], want[0]) and bits_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
        ix.set_rows("native")
        shard = tp[500:1500].contiguous()
        ix.reshard(shard, 500, 1500)
        with pytest.raises(ValueError):
            ix.exact_query(ty)
    finally:
        ix.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_recall_ranks_of_the_exact_ids(prec):
    pts, y = normal(prec, 5000, 128, 40, 31)
    lat_p, lat_y = lattice(prec, 2000, 32, 40, 32)
    for p, q in ((pts, y), (lat_p, lat_y)):
        tp, ty = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
        ids, dd = A.exact_knn(tp, ty, 10)
        ranks = A.recall_ranks(tp, ty, ids).cpu().numpy()
        j = np.arange(10)[None, :]
        assert (ranks <= j).all()
        dn = dd.cpu().numpy()
        distinct = np.array([len(set(r.tolist())) == 10 for r in dn])
        assert (ranks[distinct] == j).all()
    assert distinct.sum() < 40  # the lattice has tied rows, the normal data (checked first) has none


def test_against_the_query_path_on_a_golden_index():
    g = load_golden("pow2_d32_f32")
    save = A.Save.from_dict("f32", g["save"])
    pts, y = np.ascontiguousarray(g["points"]), np.ascontiguousarray(g["y"])
    tp, ty = torch.from_numpy(pts).cuda(), torch.from_numpy(y).cuda()
    ix = A.Index.from_save(save, tp)
    try:
        k = ix.k
        q_ids, q_d, _ = ix.query(ty)
        e_ids, e_d = ix.exact_query(ty)
        same((e_ids.cpu().numpy(), e_d.cpu().numpy()), np_exact(pts, y, k), "golden")
        qd = np.sort(q_d.cpu().numpy(), axis=1)
        assert (qd >= e_d.cpu().numpy()).all()  # any k distinct rows are, rank by rank, no closer than the k nearest
        # where the query path found a true neighbour it reports the exact path's distance bits
        qi, ei = q_ids.cpu().numpy(), e_ids.cpu().numpy()
        qdn, edn = q_d.cpu().numpy(), e_d.cpu().numpy()
        overlap = 0
        for r in range(qi.shape[0]):
            for c, i in enumerate(ei[r]):
                hit = np.nonzero(qi[r] == i)[0]
                if hit.size:
                    overlap += 1
                    assert qdn[r][hit[0]].view(np.uint32) == edn[r][c].view(np.uint32)
        assert A.recall_at_k(q_ids, e_ids) == pytest.approx(overlap / ei.size, abs=1e-12)
        assert overlap > 0
    finally:
        ix.close()
        save.free()
