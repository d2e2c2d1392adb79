"""GPU: per-query tag predicates of fixed mode and of the exact scan (annhip_index_set_tags, annhip_query_tagged,
annhip_exact_knn_tagged; include/ann_hip.h).  Row i competes for query q iff (tags[i] & qmask[q]) == qvalue[q].  The oracle
is the allow-list bitmap path (tests/test_gpu_filter.py checks that one against brute force): in fixed mode a query's answer
depends on nothing but its own row, codes and ranked bits, so for every predicate g of a batch the tagged batch's rows with
predicate g must equal -- ids and distance bytes, no tolerance -- the same rows of the whole batch queried under
set_filter(allow_g), allow_g = (tags & mask_g) == value_g.  Helpers follow tests/test_gpu_filter.py."""
import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

SHAPES = [("f64", 3000, 32, 5, 4), ("f32", 5000, 64, 10, 6), ("f64", 2500, 80, 8, 3), ("f64", 2000, 16, 33, 2),
          ("f32", 2500, 33, 6, 3), ("f32", 2000, 100, 6, 3), ("f64", 1500, 300, 5, 2)]  # + unaligned, folded, any-d hash

# (mask, value), dealt round-robin over the queries of every batch
PRED = [(0xFF, 0), (0xFF, 1), (0xFF, 2), (0xFF, 3),  # tenant equality
        (0x1FF, 1 | 0x100),                          # tenant 1 with bit 8 set
        (0x100, 0x100),                              # bit 8 set
        (0, 0),                                      # everything
        (0xFF, 200),                                 # nobody
        (0xFF, 1 << 20),                             # value outside mask: nobody
        (0xFF, 7)]                                   # fewer than k rows
NOBODY, FEW = (7, 8), 9


def _build(prec, n, d, k, T, seed):
    orc = O.CpuBackend(prec, "oracle")
    O.srandom(seed)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    O.srandom(seed + 1)
    tp = torch.from_numpy(pts).cuda()
    ix = A.Index.precomp(tp, k, T)
    return orc, pts, tp, ix


def _tags(n, k, seed):
    """tenant = uniform 0..3 in bits 0-7, bit 8 with probability 0.5, then tenant 7 on exactly max(1, k - 2) rows."""
    rng = np.random.default_rng(seed)
    tags = rng.integers(0, 4, size=n).astype(np.uint32)
    tags |= (rng.random(n) < 0.5).astype(np.uint32) << np.uint32(8)
    rows = rng.choice(n, size=max(1, k - 2), replace=False)
    tags[rows] = (tags[rows] & ~np.uint32(0xFF)) | np.uint32(7)
    return tags


def _where(Q):
    qm = np.array([PRED[q % len(PRED)][0] for q in range(Q)], dtype=np.uint32)
    qv = np.array([PRED[q % len(PRED)][1] for q in range(Q)], dtype=np.uint32)
    return qm, qv


def _groups(Q):
    return [np.arange(g, Q, len(PRED)) for g in range(len(PRED))]


def _allow(tags, g):
    return (tags & np.uint32(PRED[g][0])) == np.uint32(PRED[g][1])


def _np(t):
    return tuple(v.cpu().numpy() for v in t[:2])


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def _bitmap_oracle(ix, y, alias, tags, base=None):
    """Rows of group g from the WHOLE batch queried under set_filter(allow_g [& base]).  Leaves the filter at `base`."""
    Q = y.shape[0]
    out = None
    for g, rows in enumerate(_groups(Q)):
        allow = _allow(tags, g)
        ix.set_filter(allow if base is None else allow & base)
        r = _np(ix.query(y, alias=alias))
        if out is None:
            out = (np.empty_like(r[0]), np.empty_like(r[1]))
        out[0][rows], out[1][rows] = r[0][rows], r[1][rows]
    ix.set_filter(base)
    return out


def _check_pads(got, n, Q):
    gr = _groups(Q)
    for g in NOBODY:
        assert np.all(got[0][gr[g]] == n) and np.all(np.isinf(got[1][gr[g]])), g
    assert np.all(got[0][gr[FEW]][:, -1] == n) and np.all(np.isinf(got[1][gr[FEW]][:, -1]))


# ------------------------------------------------------------------------------------------ 1: mixed batch, group by group
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_mixed_batch_equals_the_bitmap_path_group_by_group(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 7100 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        tags = _tags(n, k, 71)
        ix.set_fixed(True)
        ix.set_tags(tags)
        assert ix.has_tags
        for b in (0, 3, "all"):
            ix.set_probe(b)
            for yy, alias in ((ty, False), (ta, True)):
                Q = yy.shape[0]
                want = _bitmap_oracle(ix, yy, alias, tags)
                got = _np(ix.query(yy, alias=alias, where=_where(Q)))
                for g, rows in enumerate(_groups(Q)):
                    assert _same_bits((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows])), (b, alias, PRED[g])
                _check_pads(got, n, Q)
                if alias:
                    for x in range(Q):
                        assert x not in got[0][x].tolist()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 2: (0, 0) is a no-op
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_everything_predicate_returns_the_unfiltered_bits_and_row_count(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 7200 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        ix.set_fixed(True)
        ix.set_tags(_tags(n, k, 72))
        ix.profile(1)
        zero80, zero60 = np.zeros(80, dtype=np.uint32), np.zeros(60, dtype=np.uint32)
        for b in (0, 3, "all"):
            ix.set_probe(b)
            ix.stats(reset=True)
            plain = _np(ix.query(ty))
            torch.cuda.synchronize()
            rows_plain = ix.stats(reset=True)["s1_rows"]
            plain_a = _np(ix.query(ta, alias=True))
            ix.stats(reset=True)
            got = _np(ix.query(ty, where=(zero80, zero80)))
            torch.cuda.synchronize()
            rows_tag = ix.stats(reset=True)["s1_rows"]
            assert _same_bits(got, plain), b
            assert _same_bits(_np(ix.query(ta, alias=True, where=(zero60, zero60))), plain_a), b
            assert rows_tag == rows_plain, (b, rows_tag, rows_plain)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 3: gathered rows
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_gathered_row_count_is_the_sum_over_the_groups(prec, n, d, k, T):
    """The test happens before a row is fetched: stage 1 of a mixed batch gathers exactly the rows that the bitmap path
    gathers for every group's own sub-batch; a batch in which nobody matches gathers none."""
    orc, pts, tp, ix = _build(prec, n, d, k, T, 7300 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        tags = _tags(n, k, 73)
        ix.set_fixed(True)
        ix.set_tags(tags)
        ix.profile(1)
        for b in (0, 3):
            ix.set_probe(b)
            ix.stats(reset=True)
            ix.query(ty, where=_where(80))
            torch.cuda.synchronize()
            rows_tag = ix.stats(reset=True)["s1_rows"]
            want = 0
            for g, rows in enumerate(_groups(80)):
                ix.set_filter(_allow(tags, g))
                ix.stats(reset=True)
                ix.query(ty[torch.from_numpy(rows).cuda()].contiguous())
                torch.cuda.synchronize()
                want += ix.stats(reset=True)["s1_rows"]
            ix.set_filter(None)
            print("%s n %d d %d b %r: stage-1 rows tagged %d, bitmap path summed over the groups %d" % (prec, n, d, b, rows_tag, want))
            assert rows_tag == want, (b, rows_tag, want)
            qm = np.full(80, 0xFF, dtype=np.uint32)
            for qv in (np.full(80, 200, dtype=np.uint32), np.full(80, 1 << 20, dtype=np.uint32)):
                ix.stats(reset=True)
                got = _np(ix.query(ty, where=(qm, qv)))
                torch.cuda.synchronize()
                assert ix.stats(reset=True)["s1_rows"] == 0
                assert np.all(got[0] == n) and np.all(np.isinf(got[1]))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 4: tags AND bitmap
@pytest.mark.parametrize("prec,n,d,k,T", SHAPES)
def test_tag_test_and_index_bitmap_both_apply(prec, n, d, k, T):
    orc, pts, tp, ix = _build(prec, n, d, k, T, 7400 + d)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        tags = _tags(n, k, 74)
        m = np.random.default_rng(740).random(n) < 0.5
        ix.set_fixed(True)
        ix.set_tags(tags)
        for b in (0, 3, "all"):
            ix.set_probe(b)
            for yy, alias in ((ty, False), (ta, True)):
                Q = yy.shape[0]
                want = _bitmap_oracle(ix, yy, alias, tags, base=m)  # leaves set_filter(m) in place
                got = _np(ix.query(yy, alias=alias, where=_where(Q)))
                for g, rows in enumerate(_groups(Q)):
                    assert _same_bits((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows])), (b, alias, PRED[g])
                _check_pads(got, n, Q)
                assert m[got[0][got[0] < n]].all()
            ix.set_filter(None)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 5: other kernel forms
@pytest.mark.parametrize("prec,d", [("f32", 64), ("f64", 32), ("f32", 80)])
def test_other_kernel_forms_give_the_same_tagged_results(prec, d, monkeypatch):
    """A table scanned without segment words (ANN_HIP_SLOT_SCAN, read when the index is made) and other wave counts per
    query (ANN_HIP_S1_WAVES): the tagged results and the gathered-row counter are the same, bit for bit, with and without
    an index bitmap."""
    n, k, T = 4000, 9, 5
    tags = _tags(n, k, 75)
    m = np.random.default_rng(750).random(n) < 0.5

    def run():
        orc, pts, tp, ix = _build(prec, n, d, k, T, 7500 + d)
        try:
            ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(150 * d).reshape(150, d))).cuda()
            ix.set_fixed(True)
            ix.set_tags(tags)
            ix.profile(1)
            out = []
            for b in (0, 4):
                ix.set_probe(b)
                for base in (None, m):
                    ix.set_filter(base)
                    ix.stats(reset=True)
                    out.append(_np(ix.query(ty, where=_where(150))))
                    out.append(_np(ix.query(tp[:100].contiguous(), alias=True, where=_where(100))))
                    torch.cuda.synchronize()
                    out.append(ix.stats(reset=True)["s1_rows"])
            return out
        finally:
            ix.close()
    want = run()
    for env in ({"ANN_HIP_SLOT_SCAN": "1"}, {"ANN_HIP_S1_WAVES": "1"}, {"ANN_HIP_S1_WAVES": "3"}):
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        A._lib.reload_env()
        try:
            got = run()
        finally:
            for kk in env:
                monkeypatch.delenv(kk)
            A._lib.reload_env()
        for g, w in zip(got, want):
            assert (g == w) if not isinstance(w, tuple) else _same_bits(g, w), env


@pytest.mark.parametrize("prec,n,d,k,T", [SHAPES[1], SHAPES[2]])
def test_tables_without_the_sorted_prefix_layout_give_the_same_tagged_results(prec, n, d, k, T):
    """An index made from a save in which an arbitrary mask's ids were replaced by the sentinel n: its tables have no
    sorted-prefix layout, so a tagged query of it runs the slot-scan form of stage 1.  Its answers must be those of the
    default form on the original index under set_filter(mask) (test 4 ties that one to the bitmap path)."""
    orc, pts, tp, ix = _build(prec, n, d, k, T, 7550 + d)
    ix2 = None
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(80 * d).reshape(80, d))).cuda()
        ta = tp[:60].contiguous()
        tags = _tags(n, k, 755)
        save = ix.export()
        sd = save.to_dict()
        save.free()
        mask = np.random.default_rng(756).random(n) < 0.7
        ed = dict(sd)
        lut = np.where(mask, np.arange(n, dtype=np.uint64), np.uint64(n))
        lut = np.concatenate([lut, np.full(1, n, dtype=np.uint64)])
        ed["which_par"] = [lut[np.minimum(np.asarray(w), n).astype(np.int64)] for w in sd["which_par"]]
        ed["graph"] = lut[np.minimum(np.asarray(sd["graph"]), n).astype(np.int64)]
        ix2 = A.Index.from_save(A.Save.from_dict(prec, ed), tp)
        for i in (ix, ix2):
            i.set_fixed(True)
            i.set_tags(tags)
        ix.set_filter(mask)
        for b in (0, 3, "all"):
            ix.set_probe(b), ix2.set_probe(b)
            for yy, alias in ((ty, False), (ta, True)):
                w = _where(yy.shape[0])
                want = _np(ix.query(yy, alias=alias, where=w))
                assert _same_bits(_np(ix2.query(yy, alias=alias, where=w)), want), (b, alias)
                ix2.set_filter(mask)  # the same mask as an index bitmap removes nothing more
                assert _same_bits(_np(ix2.query(yy, alias=alias, where=w)), want), (b, alias, "bitmap")
                ix2.set_filter(None)
    finally:
        if ix2 is not None:
            ix2.close()
        ix.close()


# ------------------------------------------------------------------------------------------ 6: exact scan
def _exact_groups_equal(got, pts, y, k, tags, Q, self_exclude=False, base=None):
    for g, rows in enumerate(_groups(Q)):
        allow = _allow(tags, g) if base is None else _allow(tags, g) & base
        want = A.exact_knn(pts, y, k, self_exclude=self_exclude, allow=torch.from_numpy(allow).cuda())
        r = torch.from_numpy(rows).cuda()
        assert torch.equal(got[0][r], want[0][r]) and torch.equal(got[1][r].view(torch.uint8), want[1][r].view(torch.uint8)), (k, PRED[g])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("d", [128, 80, 100, 300])
def test_exact_knn_with_tag_predicates(prec, d, monkeypatch):
    n, Q = 3000, 70
    dt = torch.float32 if prec == "f32" else torch.float64
    gen = torch.Generator().manual_seed(760 + d)
    pts = torch.randn((n, d), generator=gen, dtype=torch.float64).to(dt).cuda()
    y = torch.randn((Q, d), generator=gen, dtype=torch.float64).to(dt).cuda()
    tags = _tags(n, 10, 76)  # tenant 7 on 8 rows
    where = _where(Q)
    gr = _groups(Q)
    for k in (1, 10, 100):
        got = A.exact_knn(pts, y, k, tags=tags, where=where)
        _exact_groups_equal(got, pts, y, k, tags, Q)
        for g in NOBODY:
            assert torch.all(got[0][gr[g]] == n) and torch.all(torch.isinf(got[1][gr[g]]))
        if k > 8:
            few = got[0][gr[FEW]]
            assert torch.all(few[:, 8:] == n) and torch.all(few[:, :8] < n) and torch.all(torch.isinf(got[1][gr[FEW]][:, 8:]))
        monkeypatch.setenv("ANN_HIP_EXACT_RANGES", "3")  # another split of the rows changes nothing
        A._lib.reload_env()
        try:
            r = A.exact_knn(pts, y, k, tags=tags, where=where)
        finally:
            monkeypatch.delenv("ANN_HIP_EXACT_RANGES")
            A._lib.reload_env()
        assert torch.equal(r[0], got[0]) and torch.equal(r[1].view(torch.uint8), got[1].view(torch.uint8)), k
    # tags and where as device tensors give the same bits
    dev = A.exact_knn(pts, y, 10, tags=torch.from_numpy(tags.view(np.int32)).cuda(),
                      where=tuple(torch.from_numpy(w.view(np.int32)).cuda() for w in where))
    ref = A.exact_knn(pts, y, 10, tags=tags, where=where)
    assert torch.equal(dev[0], ref[0]) and torch.equal(dev[1].view(torch.uint8), ref[1].view(torch.uint8))
    # self_exclude with y = points
    yq = pts[:Q].contiguous()
    got = A.exact_knn(pts, yq, 10, self_exclude=True, tags=tags, where=where)
    _exact_groups_equal(got, pts, yq, 10, tags, Q, self_exclude=True)
    for q in range(Q):
        assert q not in got[0][q].tolist()
    # allow= given as well: ANDed with the tag test
    m = np.random.default_rng(761).random(n) < 0.5
    got = A.exact_knn(pts, y, 10, tags=tags, where=where, allow=torch.from_numpy(m).cuda())
    _exact_groups_equal(got, pts, y, 10, tags, Q, base=m)
    # (0, 0) for every query is the plain scan
    z = np.zeros(Q, dtype=np.uint32)
    a, b = A.exact_knn(pts, y, 10), A.exact_knn(pts, y, 10, tags=tags, where=(z, z))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.uint8), b[1].view(torch.uint8))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_index_exact_query_with_tag_predicates(prec):
    n = 4000
    orc, pts, tp, ix = _build(prec, n, 64, 10, 4, 7650)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(90 * 64).reshape(90, 64))).cuda()
        tags = _tags(n, 10, 765)
        m = np.random.default_rng(766).random(n) < 0.5
        ix.set_tags(tags)  # tags are row attributes: no fixed mode needed for the exact scan
        for alias, yy in ((False, ty), (True, tp[:90].contiguous())):
            w = _where(90)
            got = ix.exact_query(yy, alias=alias, where=w)
            want = A.exact_knn(tp, yy, 10, self_exclude=alias, tags=tags, where=w)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.uint8), want[1].view(torch.uint8))
            _exact_groups_equal(got, tp, yy, 10, tags, 90, self_exclude=alias)
        ix.set_fixed(True)
        ix.set_filter(m)
        for alias, yy in ((False, ty), (True, tp[:90].contiguous())):
            got = ix.exact_query(yy, alias=alias, where=_where(90))
            _exact_groups_equal(got, tp, yy, 10, tags, 90, self_exclude=alias, base=m)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7: the other knobs
@pytest.mark.parametrize("prec,rows", [("f32", "f16"), ("f64", "f32")])
def test_tags_compose_with_narrow_rows(prec, rows):
    n, d, k, T = 4000, 64, 7, 4
    orc, pts, tp, ix = _build(prec, n, d, k, T, 7700)
    try:
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(60 * d).reshape(60, d))).cuda()
        tags = _tags(n, k, 77)
        ix.set_fixed(True)
        ix.set_tags(tags)
        native = None
        for b in (0, 4):
            ix.set_probe(b)
            for setting in (rows, "native"):
                ix.set_rows(setting)
                want = _bitmap_oracle(ix, ty, False, tags)
                got = _np(ix.query(ty, where=_where(60)))
                assert _same_bits(got, want), (b, setting)
                if setting == "native":
                    native = got
                else:
                    narrow = got
            assert not np.array_equal(narrow[1].view(np.uint8), native[1].view(np.uint8))  # the narrow rows were read
    finally:
        ix.close()


def test_tags_on_workspaces_and_streams():
    n = 6000
    orc, pts, tp, ix = _build("f32", n, 64, 10, 6, 7800)
    try:
        ta = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(700 * 64).reshape(700, 64))).cuda()
        tb = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(300 * 64).reshape(300, 64))).cuda()
        ix.set_fixed(True)
        ix.set_tags(_tags(n, 10, 78))
        wa = _where(700)
        wb = tuple(np.roll(w, 3) for w in _where(300))  # another dealing of the predicates
        for b in (0, 5):
            ix.set_probe(b)
            serial_a, serial_b = _np(ix.query(ta, where=wa)), _np(ix.query(tb, where=wb))
            torch.cuda.synchronize()
            w1, w2, s1, s2 = ix.workspace(), ix.workspace(), torch.cuda.Stream(), torch.cuda.Stream()
            with torch.cuda.stream(s1):
                ga = ix.query(ta, ws=w1, stream=s1, where=wa)
            with torch.cuda.stream(s2):
                gb = ix.query(tb, ws=w2, stream=s2, where=wb)
            s1.synchronize(), s2.synchronize()
            assert _same_bits(_np(ga), serial_a) and _same_bits(_np(gb), serial_b)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 8: refusals and lifecycle
def test_refusals_and_lifecycle():
    n, Q = 5000, 120
    orc, pts, tp, ix = _build("f32", n, 64, 10, 6, 7900)
    try:
        y = np.ascontiguousarray(orc.gen_rand(Q * 64).reshape(Q, 64))
        ty = torch.from_numpy(y).cuda()
        save = ix.export()
        sd = save.to_dict()
        save.free()
        parity = orc.query(sd, pts, y)
        tags, where = _tags(n, 10, 79), _where(Q)
        ids = torch.full((Q, 10), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((Q, 10), -7.0, dtype=torch.float32, device="cuda")

        def refused(**kw):
            with pytest.raises(ValueError):
                ix.query(ty, out_ids=ids, out_dists=dd, **kw)
            torch.cuda.synchronize()
            assert torch.all(ids == -7) and torch.all(dd == -7.0)  # nothing was launched

        assert not ix.has_tags
        ix.set_tags(tags)                # tags are row attributes: parity mode takes them
        assert ix.has_tags
        refused(where=where)             # ... but a predicate needs fixed mode
        ix.set_fixed(True)
        ix.set_tags(None)
        assert not ix.has_tags
        refused(where=where)             # no tags
        for bad in (tags[:-1], np.ones(n + 1, dtype=np.uint32), tags.astype(np.int64), tags.astype(np.int32), tags.tolist(),
                    torch.from_numpy(tags.view(np.int32)), torch.from_numpy(tags.astype(np.int64)).cuda(),
                    torch.zeros(n - 1, dtype=torch.int32, device="cuda")):
            with pytest.raises(ValueError):
                ix.set_tags(bad)
            assert not ix.has_tags
        ix.set_tags(tags)
        for bad in ((where[0][:-1], where[1]), (where[0], where[1][:-1]), (where[0].astype(np.int32), where[1]),
                    (where[0], where[1].astype(np.int64)), where[0], (where[0],), (where[0], None),
                    (torch.from_numpy(where[0].view(np.int32)), torch.from_numpy(where[1].view(np.int32)))):
            refused(where=bad)
            with pytest.raises(ValueError):
                ix.exact_query(ty, where=bad)
        # the library's own refusal of NULL arrays: -2, nothing launched
        lib = ix.lib
        assert lib.annhip_query_tagged(ix.h, None, None, Q, ty.data_ptr(), 0, None, None, ids.data_ptr(), dd.data_ptr()) == -2
        torch.cuda.synchronize()
        assert torch.all(ids == -7) and torch.all(dd == -7.0)
        assert lib.annhip_index_has_tags(ix.h) == 1
        # exact_knn: tags and where go together
        with pytest.raises(ValueError):
            A.exact_knn(tp, ty, 10, tags=tags)
        with pytest.raises(ValueError):
            A.exact_knn(tp, ty, 10, where=where)
        with pytest.raises(ValueError):
            A.exact_knn(tp, ty, 10, tags=tags[:-1], where=where)
        with pytest.raises(ValueError):
            A.exact_knn(tp, ty, 10, tags=tags, where=(where[0][:-1], where[1][:-1]))
        # a numpy tag array and the same words as a device tensor give the same results
        from_numpy = _np(ix.query(ty, where=where))
        plain = _np(ix.query(ty))
        assert not _same_bits(from_numpy, plain)
        ix.set_tags(torch.from_numpy(tags.view(np.int32)).cuda())
        assert _same_bits(_np(ix.query(ty, where=where)), from_numpy)
        dev_where = tuple(torch.from_numpy(w.view(np.int32)).cuda() for w in where)
        assert _same_bits(_np(ix.query(ty, where=dev_where)), from_numpy)
        with pytest.raises(ValueError):  # a refused call leaves the setting as it was
            ix.set_tags(tags[:-1])
        assert ix.has_tags and _same_bits(_np(ix.query(ty, where=where)), from_numpy)
        assert _same_bits(_np(ix.query(ty)), plain)  # no untagged call reads the tags
        # set_tags(None), then a tagged query is refused
        ix.set_tags(None)
        refused(where=where)
        with pytest.raises(ValueError):
            ix.exact_query(ty, where=where)
        # leaving fixed mode keeps the tags; a plain query then returns the reference's bytes
        ix.set_tags(tags)
        ix.set_fixed(False)
        assert ix.has_tags
        ids0, dd0, _ = ix.query(ty)
        assert np.array_equal(ids0.cpu().numpy().astype(np.uint64), parity[0])
        assert np.array_equal(dd0.cpu().numpy().view(np.uint8), parity[1].view(np.uint8))
        refused(where=where)
        ix.set_fixed(True)
        assert _same_bits(_np(ix.query(ty, where=where)), from_numpy)
        # a resharded index drops the tags and refuses new ones
        half = tp[: n // 2].contiguous()
        ix.reshard(half, 0, n // 2)
        assert not ix.has_tags
        with pytest.raises(ValueError):
            ix.set_tags(tags)
        ix.set_tags(None)                # clearing is always accepted
    finally:
        ix.close()
