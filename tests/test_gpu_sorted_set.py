"""GPU: sets of intervals per query and runs split over workgroups (annhip_tag_runs_set, annhip_query_sorted_set;
include/ann_hip.h, the end of ann_sorted_kernels.h).

The ground truth never runs the new kernels: for each interval rank r of the numpy-normalised sets
(A.normalize_intervals), Index.exact_query(y, k=kq, alias=..., where=(M, lo_r, hi_r)) -- an empty interval where a set is
shorter --, the non-pad entries merged on the CPU by (distance bits, id) to the first kq and padded with (n_total, +inf);
with a radius, A.radius_trim of that.  Every comparison is on ids and distance bytes, with no tolerance.

Shapes, the value column (run lengths 1, tile - 1, tile, tile + 1, 3 * tile + 5, 3 and the rest) and the helpers are those
of tests/test_gpu_sorted.py.  A split S below 64 is refused: where tile - 1, tile or tile + 1 fall below it the test
asserts the refusal, and the split tests include the shapes whose tile is large enough for every S to be served."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from tests.test_gpu_query_k import _np, _same_bits
from tests.test_gpu_sorted import FULL, _built, _index, _intervals, _queries, _runs_numpy, _scan_tile, _triple, _u32, _values
from tests.test_gpu_tail import SHAPES, Q, _rows

pytestmark = pytest.mark.gpu

IDS = ["%s-n%d-d%d-k%d-T%d" % s for s in SHAPES]


def _sets(Qn):
    """Per-query sets, cycled to Qn queries: 0, 1, 2, 3 or 7 items drawn from disjoint values, touching values (neighbours
    touch in the order), duplicates, nested and overlapping windows, an empty interval, (0, 0xFFFFFFFF) followed by
    others, a value nobody has (7, 8, 9), and the 0xFFFFFFFF edge."""
    base = [[], [5], [1, 3], [2, 3], [4, 4, 4], [(2, 5), (3, 4)], [(3, 12), (10, 15), (12, 19)], [(9, 8), 6, (7, 7)],
            [(0, FULL), 5, (3, 4)], [1, 2, 3, 4, 5, 6, (10, 19)], [(12, 19), (4, 12), 6, (6, 6), (9, 8), (2, 3), 7],
            [5], [5, 5], [(5, 5), 8], [5, (9, 8)], [(10, FULL), (FULL, FULL), (19, 19)], [(0, 0), (FULL, FULL)], [(7, 9)],
            [6, 1], [(1, 6)], [11, 13, 19], [(4, 5), (5, 6), (1, 2)], [(16, FULL), (0, 3), (2, 17), 1, 19, (9, 8), (5, 5)]]
    return (base * (Qn // len(base) + 1))[:Qn]


def _singles(qlo, qhi):
    return A.where_in(FULL, [[(int(a), int(b))] for a, b in zip(qlo, qhi)])


def _host(where):
    return tuple(w.cpu().numpy().view(np.uint32) if isinstance(w, torch.Tensor) else w for w in where)


def _set_runs_numpy(tags, where):
    """the runs of the normalised intervals: normalize_intervals plus numpy.searchsorted"""
    M, off, lo, hi = _host(where)
    nlo, nhi = A.normalize_intervals(off, lo, hi)
    return _runs_numpy(tags, M, nlo, nhi)


def _truth(ix, y, where, k=None, alias=False, radius=None):
    M, off, lo, hi = _host(where)
    off = np.asarray(off, dtype=np.int64)
    nlo, nhi = A.normalize_intervals(off, lo, hi)
    Qn, cnt, kq, nt = off.size - 1, np.diff(off), ix.k if k is None else k, ix.n_total
    dt = np.float32 if y.dtype == torch.float32 else np.float64
    I, D = [np.full((Qn, kq), nt, dtype=np.int64)], [np.full((Qn, kq), np.inf, dtype=dt)]
    for r in range(int(cnt.max()) if Qn else 0):
        rlo, rhi = np.ones(Qn, dtype=np.uint32), np.zeros(Qn, dtype=np.uint32)
        has = cnt > r
        rlo[has], rhi[has] = nlo[off[:-1][has] + r], nhi[off[:-1][has] + r]
        gi, gd = _np(ix.exact_query(y, k=kq, alias=alias, where=(np.full(Qn, M, dtype=np.uint32), rlo, rhi)))
        I.append(gi.astype(np.int64)), D.append(gd)
    I, D = np.concatenate(I, axis=1), np.ascontiguousarray(np.concatenate(D, axis=1))
    bits = D.view(np.uint32 if dt == np.float32 else np.uint64)  # distances are >= +0: their bits order like the values
    order = np.lexsort((I, bits), axis=1)[:, :kq]  # the pads (n_total, +inf) come last
    ids, dists = np.take_along_axis(I, order, axis=1), np.take_along_axis(D, order, axis=1)
    if radius is None:
        return ids, dists
    ti, td = torch.from_numpy(ids).cuda(), torch.from_numpy(dists).cuda()
    counts = A.radius_trim(ti, td, radius, nt)
    return ti.cpu().numpy(), td.cpu().numpy(), counts.cpu().numpy()


def _check(ix, y, where, what, want=None, **kw):
    """query_sorted_set against the truth (or against `want`) -> ((ids, dists), entries)"""
    got = ix.query_sorted_set(y, where, **kw)
    g = _np(got)
    w = want if want is not None else _truth(ix, y, where, k=kw.get("k"), alias=kw.get("alias", False))
    bad = np.nonzero((g[0] != w[0]).any(axis=1))[0]
    assert bad.size == 0, "%s: ids differ for queries %s, first: got %s want %s" % (what, bad[:8], g[0][bad[0]][:8], w[0][bad[0]][:8])
    assert _same_bits(g, w), "%s: distances not bit-identical" % what
    return g, int(got[-1])


def _splits(prec, d, n_total):
    t = _scan_tile(prec, d)
    return [64, t - 1, t, t + 1, 3 * t + 5, n_total + 11]


def _setup(shape):
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    tags, counts = _values(prec, n, d, 7300 + d)
    ix.set_tags(tags)
    ix.sort_tags()
    return tp, ix, tags, counts


# ------------------------------------------------------------------------------------------ 1: identity
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_interval_per_query_is_query_sorted(shape):
    prec, n, d, kg, T = shape
    tp, ix, tags, _ = _setup(shape)
    qlo, qhi = _intervals(Q)
    y = _queries(prec, Q, d, 7400 + d)
    where = _singles(qlo, qhi)
    wl = _runs_numpy(tags, FULL, qlo, qhi)[1]
    assert (wl == 0).any() and (qlo > qhi).any()
    for k in (None, 1, 256, 1024):
        want = _np(ix.query_sorted(y, _triple(FULL, qlo, qhi), k=k))
        _, entries = _check(ix, y, where, "%s k=%s" % (shape, k), want=want, k=k)
        assert entries == int((wl > 0).sum()), (k, entries)


# ------------------------------------------------------------------------------------------ 2: sets
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sets_of_intervals(shape):
    prec, n, d, kg, T = shape
    tp, ix, tags, _ = _setup(shape)
    sets = _sets(Q)
    assert {len(s) for s in sets} == {0, 1, 2, 3, 7}
    where = A.where_in(FULL, sets)
    y = _queries(prec, Q, d, 7400 + d)
    start, length = ix.tag_runs_set(where)
    ws, wl = _set_runs_numpy(tags, where)
    assert np.array_equal(_u32(start), ws) and np.array_equal(_u32(length), wl)
    nlo, nhi = A.normalize_intervals(*where[1:])
    assert ((nlo > nhi) & (where[2] <= where[3])).any()  # the normalisation emptied a slot that was not empty
    for k in (None, 1, 1024):
        g, entries = _check(ix, y, where, "%s sets k=%s" % (shape, k), k=k)
        assert entries == int((wl > 0).sum())
        none = [q for q, s in enumerate(sets) if not s]
        assert none and (g[0][none] == n).all() and np.isinf(g[1][none]).all()  # no interval: all pads
    dev = (FULL, where[1], torch.from_numpy(where[2].view(np.int32)).cuda(), torch.from_numpy(where[3].view(np.int32)).cuda())
    assert _same_bits(_np(ix.query_sorted_set(y, dev)), _np(ix.query_sorted_set(y, where)))  # device arrays


def test_a_set_of_256_values_and_257_refused():
    shape = SHAPES[0]
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    rng = np.random.default_rng(8100)
    tags = rng.integers(0, 400, size=n).astype(np.uint32)
    ix.set_tags(tags)
    ix.sort_tags()
    Qn = 5
    y = _queries(prec, Qn, d, 8101)
    vals = rng.permutation(400)[:257]
    sets = [list(vals[:256]), [3], list(vals[:256][::-1]), [], list(vals[100:356 - 100]) + [(0, 50)]]
    where = A.where_in(FULL, sets)
    start, length = ix.tag_runs_set(where)
    ws, wl = _set_runs_numpy(tags, where)
    assert np.array_equal(_u32(start), ws) and np.array_equal(_u32(length), wl)
    for S in (0, 64):
        _check(ix, y, where, "256 values S=%d" % S, k=kg, split=S)
    with pytest.raises(ValueError):
        A.where_in(FULL, [list(vals)])
    off = np.array([0, 257], dtype=np.int64)
    lo = np.ascontiguousarray(vals.astype(np.uint32))
    with pytest.raises(ValueError):
        ix.query_sorted_set(y[:1].contiguous(), (FULL, off, lo, lo))
    with pytest.raises(ValueError):
        ix.tag_runs_set((FULL, off, lo, lo))


# ------------------------------------------------------------------------------------------ 3: split
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[5]], ids=[IDS[0], IDS[3], IDS[4], IDS[5]])
def test_split_runs_give_the_unsplit_bytes(shape):
    """Q = 150: the pieces of one query straddle workgroups and one workgroup holds several pieces of one query."""
    prec, n, d, kg, T = shape
    tp, ix, tags, _ = _setup(shape)
    Qn = 150
    y = _queries(prec, Qn, d, 7700 + d)
    qlo, qhi = _intervals(Qn)
    served = 0
    for name, where in (("intervals", _singles(qlo, qhi)), ("sets", A.where_in(FULL, _sets(Qn)))):
        ws, wl = _set_runs_numpy(tags, where)
        for k in (None, 1024):
            base, e0 = _check(ix, y, where, "%s %s k=%s S=0" % (shape, name, k), k=k)
            assert e0 == int((wl > 0).sum())
            for S in _splits(prec, d, n):
                if S < 64:
                    with pytest.raises(ValueError):
                        ix.query_sorted_set(y, where, k=k, split=S)
                    continue
                slot, ps, pe = A.set_pieces(ws, wl, S)
                _, entries = _check(ix, y, where, "%s %s k=%s S=%d" % (shape, name, k, S), want=base, k=k, split=S)
                print("%s %s k=%s S=%d: %d entries" % (shape, name, k, S, entries))
                assert entries == slot.size, (S, entries, slot.size)
                served += 1
                if S > n:
                    assert entries == e0
                if S == 64:  # a run of fewer than 1024 rows in several pieces: pads have to merge
                    per = np.bincount(slot, minlength=wl.size)
                    assert ((per > 1) & (wl < 1024)).any()
    assert served >= 8


def test_staging_beyond_one_scan_chunk_and_one_lane_per_list():
    """T = 1 100 interval slots cross tsort_scan_kernel's chunk of 1 024 words in the piece offsets, E > 8 192 entries
    cross it in the sort's histogram (256 words per 2 048 entries), and a query with more than 64 pieces gives the lanes
    of sorted_set_merge_kernel two lists each."""
    shape = SHAPES[0]
    prec, n, d, kg, T = shape
    tp, ix, tags, _ = _setup(shape)
    Qn, S = 1100, 64
    y = _queries(prec, Qn, d, 8300)
    where = A.where_in(FULL, [[(0, FULL)] if q % 3 == 0 else [5, 10 + q % 10] for q in range(Qn)])
    ws, wl = _set_runs_numpy(tags, where)
    slot = A.set_pieces(ws, wl, S)[0]
    assert int(where[1][-1]) > 1024 and slot.size > 8192 and np.bincount(slot).max() > 64
    _, entries = _check(ix, y, where, "many entries", split=S)
    assert entries == slot.size


# ------------------------------------------------------------------------------------------ 4: the sharing
def _fetched_model(start, length, S, G):
    """rows fetched when the entries, ordered by start (ties in creation order), go to workgroups of G entries that
    stream every span of touching or overlapping runs once"""
    _, ps, pe = A.set_pieces(start, length, S)
    order = np.argsort(ps, kind="stable")
    ps, pe = ps[order], pe[order]
    total = 0
    for g0 in range(0, ps.size, G):
        lo = hi = None
        for s, e in zip(ps[g0:g0 + G].tolist(), pe[g0:g0 + G].tolist()):
            if lo is None or s > hi:
                total += (hi - lo) if lo is not None else 0
                lo, hi = s, e
            else:
                hi = max(hi, e)
        total += (hi - lo) if lo is not None else 0
    return total


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_rows_fetched_show_the_sharing(shape):
    prec, n, d, kg, T = shape
    tp, ix, tags, counts = _setup(shape)
    t = _scan_tile(prec, d)
    assert t >= 64
    y = _queries(prec, Q, d, 7400 + d)
    ix.profile(True)

    def fetched(yy, where, S, k=None):
        before = ix.stats()["other_rows"]
        ix.query_sorted_set(yy, where, k=k, split=S)
        torch.cuda.synchronize()
        return int(ix.stats()["other_rows"] - before)

    # six queries on the run of 3 * tile + 5 rows, cut at the global multiples of the tile: aligned pieces, one fetch
    six = A.where_in(FULL, [[5]] * 6)
    L = counts[5]
    ws, wl = _set_runs_numpy(tags, six)
    got = fetched(y[:6].contiguous(), six, t)
    few, many = _fetched_model(ws, wl, t, 48), _fetched_model(ws, wl, t, 4)
    print("six queries on %d rows, S = tile = %d: fetched %d rows (model: %d with 48 entries per workgroup, %d with 4)" % (L, t, got, few, many))
    assert few == L and L <= got <= many
    generic = A._lib.load(prec).annhip_layout_code(d) in (0, -246, -247)
    if not generic:
        assert got == L
    else:  # the any-d form: 4 waves, 16 entries per workgroup
        assert got == _fetched_model(ws, wl, t, 16)
    # pairwise disjoint sets fetch the sum of the run lengths, for every S
    vals = [[1, 3], [2], [4, 6, 10], [5], [(11, 12)], [13, 15, 17, 19], [(7, 9)], [14], [16, 18]]
    dis = A.where_in(FULL, vals)
    ws, wl = _set_runs_numpy(tags, dis)
    yd = y[:len(vals)].contiguous()
    for S in [0] + [S for S in _splits(prec, d, n) if S >= 64]:  # (a smaller S is refused: test_split_runs_...)
        for k in (None, 1024):
            got = fetched(yd, dis, S, k)
            print("disjoint sets S=%d k=%s: fetched %d rows, sum of the run lengths %d" % (S, k, got, wl.sum()))
            assert got == wl.sum()
    ix.profile(False)


# ------------------------------------------------------------------------------------------ 5: composition
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3], SHAPES[5]], ids=[IDS[0], IDS[1], IDS[3], IDS[5]])
def test_sets_compose_with_the_other_features(shape):
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    rng = np.random.default_rng(8200 + d)
    m1, m2 = 41, 23  # rows appended before the sort and after it
    tags, _ = _values(prec, n, d, 7300 + d, rows=n + m1)
    sets = _sets(Q)
    where = A.where_in(FULL, sets)
    y = _queries(prec, Q, d, 7400 + d)
    ya = tp[:Q].contiguous()
    what = "%s " % (shape,)
    S = max(64, _scan_tile(prec, d))
    ix.set_tags(tags[:n])
    ix.sort_tags()
    _check(ix, ya, where, what + "alias", alias=True)
    _check(ix, ya, where, what + "alias k=1 split", alias=True, k=1, split=S)
    plain, _ = _check(ix, y, where, what + "plain")
    ix.set_rows("f16" if prec == "f32" else "f32")
    assert _same_bits(_np(ix.query_sorted_set(y, where, split=S)), plain), what + "narrow rows"
    ix.set_rows("native")
    allow = rng.random(n) < 0.4
    ix.set_filter(allow)
    ga, _ = _check(ix, y, where, what + "allow", split=S)
    assert allow[ga[0][ga[0] < n]].all() and not _same_bits(ga, plain)
    _check(ix, ya, where, what + "allow alias k=256", alias=True, k=256)
    ix.set_filter(None)
    # rows appended before the sort are inside the order, a hashed tail changes nothing ...
    ix.append(_rows(prec, m1, d, 7900 + d), tags=tags[n:])
    _check(ix, y, where, what + "fresh only", split=S)
    ix.hash_tail()
    ix.sort_tags()
    assert ix.tag_order == (FULL, n + m1)
    g1, _ = _check(ix, y, where, what + "tail inside the order k=64", k=64, split=S)
    assert (g1[0][g1[0] < n + m1] >= n).any()
    # ... rows appended after it compete exactly once: a copy of query qa that matches its SECOND interval only, and a copy
    # of query qb that matches all three of its raw, overlapping intervals
    qa, qb = sets.index([1, 3]), sets.index([(3, 12), (10, 15), (12, 19)])
    tail2 = _rows(prec, m2, d, 8000 + d)
    ftags = rng.integers(10, 20, size=m2).astype(np.uint32)
    tail2[0], ftags[0] = y[qa].cpu().numpy(), 3
    tail2[1], ftags[1] = y[qb].cpu().numpy(), 12
    ix.append(tail2, tags=ftags)
    assert ix.tag_order == (FULL, n + m1) and ix.n_total == n + m1 + m2
    for SS in (0, S):
        g2, _ = _check(ix, y, where, what + "fresh rows S=%d" % SS, split=SS, k=64)
        for q, j in ((qa, 0), (qb, 1)):
            assert g2[0][q, 0] == n + m1 + j and g2[1][q, 0] == 0 and (g2[0][q] == n + m1 + j).sum() == 1
    allow = rng.random(n + m1 + m2) < 0.4
    allow[n + m1:n + m1 + 2] = True
    ix.set_filter(allow)
    _check(ix, y, where, what + "tail, fresh rows and allow list", split=S)
    _check(ix, ya, where, what + "tail, fresh rows, allow list, alias, k=1024", alias=True, k=1024, split=S)
    # a workspace and a stream give the null stream's bits
    null, _ = _check(ix, y, where, what + "k=20", k=20)
    st, ws = torch.cuda.Stream(), ix.workspace()
    for SS in (0, S):
        on = ix.query_sorted_set(y, where, k=20, split=SS, ws=ws, stream=st)
        st.synchronize()
        assert _same_bits(_np(on), null), what + "stream S=%d" % SS
    # radius: a finite one from the data, and +inf, with counts
    fin = np.where(np.isfinite(null[1]), null[1], 0)
    rad = np.ascontiguousarray(fin.max(axis=1) * 0.5).astype(null[1].dtype)
    res = {}
    for r, tag in ((rad, "finite"), (float("inf"), "inf")):
        wi, wd, wc = _truth(ix, y, where, k=20, radius=r)
        for SS in (0, S):
            gi, gd, gc, _ = ix.query_sorted_set(y, where, k=20, radius=r, split=SS)
            assert _same_bits(_np((gi, gd)), (wi, wd)), what + "radius %s S=%d" % (tag, SS)
            assert np.array_equal(gc.cpu().numpy(), wc), what + "radius counts %s S=%d" % (tag, SS)
        res[tag] = ((wi, wd), wc)
    assert _same_bits(res["inf"][0], null)
    assert (res["finite"][1] > 0).any() and (res["finite"][1] < res["inf"][1]).any()
    on_r = ix.query_sorted_set(y, where, k=20, radius=rad, split=S, ws=ws, stream=st)
    st.synchronize()
    assert _same_bits(_np(on_r), res["finite"][0]) and np.array_equal(on_r[2].cpu().numpy(), res["finite"][1])


# ------------------------------------------------------------------------------------------ 6: refusals
def _raw(ix, y, kq, off, lo, hi, ids, dists, S=0, alias=0, ycnt=None):
    return ix.lib.annhip_query_sorted_set(ix.h, None, None, y.shape[0] if ycnt is None else ycnt, y.data_ptr(), alias, kq, None,
                                          off.ctypes.data if off is not None else None, lo.data_ptr() if lo is not None else None,
                                          hi.data_ptr() if hi is not None else None, S, ids.data_ptr(), dists.data_ptr(), None)


def test_refusals_leave_the_outputs_untouched():
    shape = SHAPES[2]
    prec, n, d, kg, T = shape
    tp, ix = _index(shape)
    tags, _ = _values(prec, n, d, 7300 + d)
    Qb = 3000  # enough queries for more than 2^27 partial slots at kq = 1024
    y = _queries(prec, Qb, d, 7400 + d)
    M, off64, lo, hi = A.where_in(FULL, _sets(Q))
    off = off64.astype(np.uint32)
    dlo, dhi = torch.from_numpy(lo.view(np.int32)).cuda(), torch.from_numpy(hi.view(np.int32)).cuda()
    ids = torch.full((Qb, 1024), -7, dtype=torch.int64, device="cuda")
    dists = torch.full((Qb, 1024), -3.0, dtype=y.dtype, device="cuda")
    yq = y[:Q].contiguous()

    def untouched():
        torch.cuda.synchronize()
        return bool((ids == -7).all().item()) and bool((dists == -3.0).all().item())

    # no order
    ix.set_tags(tags)
    with pytest.raises(ValueError):
        ix.query_sorted_set(yq, (M, off64, lo, hi))
    with pytest.raises(ValueError):
        ix.tag_runs_set((M, off64, lo, hi))
    assert _raw(ix, yq, kg, off, dlo, dhi, ids, dists) == -2 and untouched()
    runs = torch.full((lo.size,), -5, dtype=torch.int32, device="cuda")
    assert ix.lib.annhip_tag_runs_set(ix.h, None, Q, off.ctypes.data, dlo.data_ptr(), dhi.data_ptr(), runs.data_ptr(), runs.data_ptr()) == -1
    ix.sort_tags()
    assert _raw(ix, yq, kg, off, dlo, dhi, ids, dists, S=64) >= 0  # the arguments are good
    ids.fill_(-7), dists.fill_(-3.0)
    # NULL arrays
    assert _raw(ix, yq, kg, None, dlo, dhi, ids, dists) == -2 and untouched()
    assert _raw(ix, yq, kg, off, None, dhi, ids, dists) == -2 and untouched()
    assert _raw(ix, yq, kg, off, dlo, None, ids, dists) == -2 and untouched()
    # offsets that decrease or do not start at 0; a set of 257
    down = off.copy()
    down[5] = down[6] + 1
    up = off.copy()
    up[0] = 1
    for bad in (down, up):
        assert _raw(ix, yq, kg, bad, dlo, dhi, ids, dists) == -2 and untouched()
        assert ix.lib.annhip_tag_runs_set(ix.h, None, Q, bad.ctypes.data, dlo.data_ptr(), dhi.data_ptr(), runs.data_ptr(), runs.data_ptr()) == -1
        with pytest.raises(ValueError):
            ix.query_sorted_set(yq, (M, bad, lo, hi))
    big = np.array([0, 257], dtype=np.uint32)
    blo = torch.arange(257, dtype=torch.int32, device="cuda")
    assert _raw(ix, yq, kg, big, blo, blo, ids, dists, ycnt=1) == -2 and untouched()
    torch.cuda.synchronize()
    assert bool((runs == -5).all().item())
    # 0 < S < 64, kq of 0 and 1025, kq above the rows on offer
    for S in (1, 63):
        assert _raw(ix, yq, kg, off, dlo, dhi, ids, dists, S=S) == -2 and untouched(), S
        with pytest.raises(ValueError):
            ix.query_sorted_set(yq, (M, off64, lo, hi), split=S)
    for kq in (0, 1025):
        assert _raw(ix, yq, kq, off, dlo, dhi, ids, dists) == -2 and untouched(), kq
    for k in (0, 1025, True, 2.0):
        with pytest.raises(ValueError):
            ix.query_sorted_set(yq, (M, off64, lo, hi), k=k)
    for split in (True, 1.5, -1, 1 << 32):
        with pytest.raises(ValueError):
            ix.query_sorted_set(yq, (M, off64, lo, hi), split=split)
    # malformed Python input: a wrong mask, arrays of wrong length or dtype, off of wrong length
    for bad in ((0xFF, off64, lo, hi), (M, off64, lo[:-1], hi), (M, off64, lo.astype(np.int64), hi), (M, off64[:-1], lo, hi),
                (M, list(off64), lo, hi), (M, off64.astype(np.float64), lo, hi), (M, off64, lo)):
        with pytest.raises(ValueError):
            ix.query_sorted_set(yq, bad)
    for bad in ([[(1, 2, 3)]], [[-1]], [[1 << 32]], [[1.5]], [[True]]):
        with pytest.raises(ValueError):
            A.where_in(FULL, bad)
    with pytest.raises(ValueError):
        A.where_in(1 << 32, [[1]])
    # more than 2^27 partial slots: known before anything runs with S = 0 (interval slots) ...
    many = A.where_in(FULL, [list(range(80))] * Qb)
    mlo, mhi = torch.from_numpy(many[2].view(np.int32)).cuda(), torch.from_numpy(many[3].view(np.int32)).cuda()
    moff = many[1].astype(np.uint32)
    assert int(moff[-1]) * 1024 > 1 << 27
    assert _raw(ix, y, 1024, moff, mlo, mhi, ids, dists) == -2 and untouched()
    # ... and after the runs are known with S > 0 (pieces): the whole index, cut every 64 rows
    whole = A.where_in(FULL, [[(0, FULL)]] * Qb)
    wlo, whi = torch.from_numpy(whole[2].view(np.int32)).cuda(), torch.from_numpy(whole[3].view(np.int32)).cuda()
    pieces = (n + 63) // 64 * Qb
    assert pieces * 1024 > 1 << 27 and Qb * 1024 <= 1 << 27
    assert _raw(ix, y, 1024, whole[1].astype(np.uint32), wlo, whi, ids, dists, S=64) == -2 and untouched()
    with pytest.raises(ValueError):
        ix.query_sorted_set(y, whole, k=1024, split=64)
    assert _raw(ix, y, 1, whole[1].astype(np.uint32), wlo, whi, ids, dists, S=64) == pieces  # kq = 1 fits
    # a resharded index refuses
    ns = 600
    small = tp[:ns].contiguous()
    lone = A.Index.precomp(small, kg, T)
    try:
        lone.set_tags(tags[:ns])
        lone.sort_tags()
        ids.fill_(-7), dists.fill_(-3.0)
        for kq, alias in ((ns + 1, 0), (ns, 1)):
            assert _raw(lone, small[:Q].contiguous(), kq, off, dlo, dhi, ids, dists, alias=alias) == -2 and untouched(), (kq, alias)
        lone.reshard(tp[: ns // 2].contiguous(), 0, ns // 2)
        assert _raw(lone, yq, kg, off, dlo, dhi, ids, dists) == -2 and untouched()
    finally:
        lone.close()


def test_zz_close_the_shared_indexes():
    for tp, ix in _built.values():
        ix.close()
    _built.clear()
