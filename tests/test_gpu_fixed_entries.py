"""GPU: the four entries of fixed mode beside annhip_query -- annhip_query_tagged, annhip_query_k, annhip_query_radius and
annhip_query_between (include/ann_hip.h) -- held against each other.  Every one of them runs the same sequence on the host
(hash, stage 1, finalize, a stage 2, the appended rows, a radius call's trim), and where two of them are given the same
question they must give the same bytes, whatever the index is set to and wherever the call runs.  No feature's own test
owns these cells: each is about one entry.  Here: both precisions, a power-of-two row layout (d = 32) and two without
lanes of a power of two (d = 9, d = 257), Q = 257 (one past a tile of 256), tags, an allow list, pair bits, and appended
rows of both kinds (200 hashed, 100 scanned).  Also pinned: the stage segments every entry reports in profile mode, and every refusal of the four entries
with its text, through the library itself."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tags import _build

pytestmark = pytest.mark.gpu

N, K, T, Q, EXTRA, HASHED = 3000, 8, 4, 257, 300, 200
KQS = (1, K, 40)
# (mask, value), dealt round-robin over the queries: tenant equality, tenant with bit 8, bit 8, everything, nobody, few rows
PAIRS = [(0xFF, 0), (0xFF, 1), (0x1FF, 0x102), (0x100, 0x100), (0, 0), (0xFF, 200), (0xFF, 7)]


def _tags(rows, seed):
    """tenant = uniform 0..3 in bits 0-7, bit 8 on a random half, tenant 7 on exactly five rows"""
    rng = np.random.default_rng(seed)
    tags = rng.integers(0, 4, size=rows).astype(np.uint32) | ((rng.random(rows) < 0.5).astype(np.uint32) << np.uint32(8))
    few = rng.choice(rows, size=5, replace=False)
    tags[few] = (tags[few] & ~np.uint32(0xFF)) | np.uint32(7)
    return tags


# Row layouts (annhip_layout_code): 32 = a power of two; 9 = the smallest odd d an index can be built with (the library
# refuses d <= 8, where the reference's transform reads out of bounds, so there is no index with d = 7): element-wise
# loads, a tree of length d; 257 = no lanes-per-row layout in either precision, the any-d code everywhere.
LAYOUTS = {32: 32, 9: -241, 257: -246}


@pytest.fixture(scope="module", params=[(p, d) for d in LAYOUTS for p in ("f32", "f64")], ids=lambda p: "%s-d%d" % p)
def setup(request):
    """One index per precision and layout for the whole module: fixed mode, tags, 300 appended rows of which the first 200
    are hashed.  Tests leave the filter off, the probe at 0 and profiling off."""
    prec, d = request.param
    orc, pts, tp, ix = _build(prec, N, d, K, T, 9900 + d)
    assert ix.lib.annhip_layout_code(d) == LAYOUTS[d]
    more = np.ascontiguousarray(orc.gen_rand((EXTRA + Q) * d).reshape(EXTRA + Q, d))
    tags = _tags(N + EXTRA, 99)
    ix.set_fixed(True)
    ix.set_tags(tags[:N])
    ix.append(more[:HASHED], tags=tags[N:N + HASHED])
    ix.hash_tail()
    ix.append(more[HASHED:EXTRA], tags=tags[N + HASHED:])
    assert ix.n_total == N + EXTRA and ix.tail_hashed == HASHED and ix.max_query_k >= max(KQS)
    ty = torch.from_numpy(more[EXTRA:]).cuda()
    qm = np.array([PAIRS[q % len(PAIRS)][0] for q in range(Q)], dtype=np.uint32)
    qv = np.array([PAIRS[q % len(PAIRS)][1] for q in range(Q)], dtype=np.uint32)
    allow = np.random.default_rng(7).random(N + EXTRA) < 0.6
    torch.cuda.synchronize()
    yield ix, ty, (qm, qv), (qm, qv, qv.copy()), allow
    ix.close()


def _bits(r):
    """(ids, dists[, counts or rc]) -> comparable bytes; the third member counts only where it is an array"""
    out = [r[0].cpu().numpy().tobytes(), r[1].cpu().numpy().tobytes()]
    if len(r) > 2 and isinstance(r[2], torch.Tensor):
        out.append(r[2].cpu().numpy().tobytes())
    return out


def _radii(dists, kq):
    """Finite radii from a [Q,kq] result: a distance out of the middle of each row (+inf where the row is short), every
    fifth query a negative radius, every seventh zero."""
    rad = dists[:, kq // 3].clone()
    rad[::5] = -1.0
    rad[3::7] = 0.0
    return rad


# ------------------------------------------------------------------------------------------ 1: the same question, two entries
# tests/test_gpu_between.py::test_lo_equal_hi_gives_the_pair_form_bits asserts (a), (b) and (d) on the index's own
# workspace and the null stream, without appended rows or an allow list, at probe 0 and 3 and Q = 80.  What is left for
# this test: the appended rows, the allow list, probe 2, a private workspace on a stream of its own, Q past a tile, the
# generic layout in both precisions -- and (c), which sets annhip_query_radius against annhip_query_k.
@pytest.mark.parametrize("where_runs", ["own workspace, null stream", "private workspace, own stream"])
@pytest.mark.parametrize("variant", ["plain", "filter", "probe2"])
def test_two_entries_one_question_same_bytes(setup, variant, where_runs):
    ix, ty, pair, tri, allow = setup
    private = where_runs.startswith("private")
    kw = dict(ws=ix.workspace(), stream=torch.cuda.Stream()) if private else {}

    def run(call, **args):
        r = call(ty, **args, **kw)
        if private:
            kw["stream"].synchronize()
        return r

    try:
        if variant == "filter":
            ix.set_filter(allow)
        if variant == "probe2":
            ix.set_probe(2)
        # (a) annhip_query_tagged and annhip_query_between with the index's own k
        assert _bits(run(ix.query, where=pair)) == _bits(run(ix.query, where=tri)), "a"
        for kq in KQS:
            # (b) annhip_query_k and annhip_query_between (stage2_kq_kernel in both, also at kq == k)
            by_k = run(ix.query, k=kq, where=pair)
            assert _bits(by_k) == _bits(run(ix.query, k=kq, where=tri)), ("b", kq)
            # (c) annhip_query_radius with +inf and annhip_query_k: ids and distance bytes
            plain = run(ix.query, k=kq)
            assert _bits(run(ix.query_radius, radius=float("inf"), k=kq))[:2] == _bits(plain)[:2], ("c", kq)
            # (d) annhip_query_radius and annhip_query_between with a radius, counts included
            rad = _radii(by_k[1], kq)
            got_pair, got_tri = run(ix.query_radius, radius=rad, k=kq, where=pair), run(ix.query_radius, radius=rad, k=kq, where=tri)
            assert len(_bits(got_pair)) == 3 and _bits(got_pair) == _bits(got_tri), ("d", kq)
            assert (got_pair[2] == 0).any() and (got_pair[2] > 0).any()  # (the radii cut somewhere)
    finally:
        ix.set_filter(None)
        ix.set_probe(0)


# ------------------------------------------------------------------------------------------ 2: the stage segments of a call
def test_every_entry_reports_the_segments_of_a_plain_query(setup):
    """annhip_stage_ms after one call in profile mode: every entry takes seven marks, so it fills the same six segments as
    annhip_query does in fixed mode ("widen" lies between two marks with nothing between them: it is there only while the
    seventh mark is), none is negative, and hash, stage 1, finalize, stage 2 and the appended rows all took time."""
    ix, ty, pair, tri, allow = setup
    rad = _radii(ix.query(ty, k=K)[1], K)
    calls = {"annhip_query": lambda: ix.query(ty),
             "annhip_query_tagged": lambda: ix.query(ty, where=pair),
             "annhip_query_between, own k": lambda: ix.query(ty, where=tri),
             "annhip_query_k": lambda: ix.query(ty, k=K),
             "annhip_query_k, 40": lambda: ix.query(ty, k=40, where=pair),
             "annhip_query_between, k=": lambda: ix.query(ty, k=40, where=tri),
             "annhip_query_radius": lambda: ix.query_radius(ty, rad, k=K, where=pair),
             "annhip_query_between, radius": lambda: ix.query_radius(ty, rad, k=K, where=tri)}
    ix.profile(True)
    try:
        seen = {}
        for name, call in calls.items():
            ix.stats(reset=True)
            call()
            torch.cuda.synchronize()
            ms = ix.stage_ms()
            print(name, ms)
            assert all(v >= 0 for v in ms.values()), (name, ms)
            for seg in ("codes", "stage1", "finalize_fallback", "stage2_rows", "stage2_network"):
                assert ms[seg] > 0, (name, seg, ms)
            seen[name] = {seg for seg, v in ms.items() if v > 0}
            assert ix.stats()["queries"] == Q, name
        for name, segs in seen.items():
            assert segs == seen["annhip_query"], (name, segs, seen["annhip_query"])
    finally:
        ix.profile(False)
        ix.stats(reset=True)


# ------------------------------------------------------------------------------------------ 3: refusals, through the library
FIXED_OFF = "fixed mode is off (annhip_index_set_fixed)"
RESHARDED = "the index does not hold rows [0, n) on this device (resharded)"
NO_TAGS = "the index has no tags (annhip_index_set_tags)"
PAIR = "qmask_dev and qvalue_dev must both be given, or neither"
KQ = "kq outside 1..annhip_index_max_query_k"


def test_every_refusal_of_the_four_entries(capfd):
    """Each entry returns -2 for each of its reasons, says "entry: reason" on stderr and leaves pre-filled outputs as they
    were.  The resharded index comes last.  annhip_query_tagged is not called on it: that entry does not test for it and
    ends the process there by design."""
    d, Qr = 32, 50
    orc, pts, tp, ix = _build("f32", N, d, K, T, 9950)
    try:
        lib, h = ix.lib, ix.h
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Qr * d).reshape(Qr, d))).cuda()
        kmax_k = 64
        ids = torch.full((Qr, kmax_k), -7, dtype=torch.int64, device="cuda")
        dd = torch.full((Qr, kmax_k), -7.0, dtype=torch.float32, device="cuda")
        cc = torch.full((Qr,), -7, dtype=torch.int32, device="cuda")
        w = torch.zeros((Qr,), dtype=torch.int32, device="cuda")
        rad = torch.full((Qr,), 1e30, dtype=torch.float32, device="cuda")
        y, m, i, o, c, r = ty.data_ptr(), w.data_ptr(), ids.data_ptr(), dd.data_ptr(), cc.data_ptr(), rad.data_ptr()
        torch.cuda.synchronize()

        def refused(entry, why, *args):
            capfd.readouterr()
            assert getattr(lib, entry)(h, None, None, Qr, y, 0, *args) == -2, (entry, why)
            assert capfd.readouterr().err == "%s: %s\n" % (entry, why)
            torch.cuda.synchronize()
            assert torch.all(ids == -7) and torch.all(dd == -7.0) and torch.all(cc == -7), (entry, why)

        ix.set_fixed(True)
        ix.set_tags(_tags(N, 98))
        big = ix.max_query_k + 1
        # what the arguments alone decide
        for qm, qv in ((None, m), (m, None), (None, None)):
            refused("annhip_query_tagged", "qmask_dev and qvalue_dev must both be given", qm, qv, i, o)
        for qm, qv in ((None, m), (m, None)):
            refused("annhip_query_k", PAIR, 4, qm, qv, i, o)
            refused("annhip_query_radius", PAIR, 4, r, qm, qv, i, o, c)
        for kq in (0, big):
            refused("annhip_query_k", KQ, kq, None, None, i, o)
            refused("annhip_query_k", KQ, kq, m, m, i, o)
            refused("annhip_query_radius", "kcap outside 1..annhip_index_max_query_k", kq, r, None, None, i, o, c)
            refused("annhip_query_between", KQ, kq, None, m, m, m, i, o, c)
            refused("annhip_query_between", KQ, kq, r, m, m, m, i, o, c)
        refused("annhip_query_radius", "radius_dev must be given", 4, None, None, None, i, o, c)
        refused("annhip_query_radius", "ids_dev must be given", 4, r, None, None, None, o, c)
        refused("annhip_query_radius", "radius_dev must be given", 0, None, None, m, None, o, c)  # the first reason that holds
        for qm, ql, qh in ((None, m, m), (m, None, m), (m, m, None)):
            refused("annhip_query_between", "qmask_dev, qlo_dev and qhi_dev must all be given", 4, None, qm, ql, qh, i, o, c)
        refused("annhip_query_between", "ids_dev must be given", 4, r, m, m, m, None, o, c)
        # an index without tags
        ix.set_tags(None)
        refused("annhip_query_tagged", NO_TAGS, m, m, i, o)
        refused("annhip_query_tagged", NO_TAGS, None, None, i, o)  # ... which this entry tests before its arrays
        refused("annhip_query_k", NO_TAGS, 4, m, m, i, o)
        refused("annhip_query_radius", NO_TAGS, 4, r, m, m, i, o, c)
        refused("annhip_query_between", NO_TAGS, 4, None, m, m, m, i, o, c)
        refused("annhip_query_between", NO_TAGS, K, None, m, m, m, i, o, c)
        refused("annhip_query_between", "qmask_dev, qlo_dev and qhi_dev must all be given", 4, None, None, m, m, i, o, c)
        # fixed mode off: before everything else
        ix.set_fixed(False)
        refused("annhip_query_tagged", FIXED_OFF, None, None, i, o)
        refused("annhip_query_k", FIXED_OFF, 0, None, m, i, o)
        refused("annhip_query_radius", FIXED_OFF, 0, None, None, m, None, o, c)
        refused("annhip_query_between", FIXED_OFF, 0, r, None, None, None, None, o, c)
        # a resharded index: after fixed mode, before everything else
        ix.set_fixed(True)
        ix.reshard(tp[: N // 2].contiguous(), 0, N // 2)
        refused("annhip_query_k", RESHARDED, 4, None, None, i, o)
        refused("annhip_query_k", RESHARDED, 0, None, m, i, o)
        refused("annhip_query_radius", RESHARDED, 4, r, None, None, i, o, c)
        refused("annhip_query_radius", RESHARDED, 0, None, None, m, None, o, c)
        refused("annhip_query_between", RESHARDED, K, None, m, m, m, i, o, c)
        refused("annhip_query_between", RESHARDED, 0, r, None, None, None, None, o, c)
    finally:
        ix.close()
