"""GPU: the device code that only a launch-shape knob or an A/B environment switch selects ("Environment
switches": each switch leaves the answer unchanged), against the CPU oracle.

  A  stage1_select_kernel as a PERSISTENT grid on one device (ANN_HIP_S1_SLOTS): min(Q, CUs*4*slots/W) workgroups walk the
     batch with `for (xi = blockIdx.x; xi < P.qn; xi += gridDim.x)`.  Q = 2 G + 37: some workgroups make three passes, some
     two, the last stride is ragged.  Every kernel family, both precisions, both scans, narrow rows, the pruned preselection.
  B  the same grid for annhip_sh_stage1 (ShardedQuery.configure(..., slots=)), whole and in two pieces (P.q0 > 0), with
     segment words (world 2) and inline records (world 4), both exchanges
  C  ANN_HIP_S2_THREADS, ANN_HIP_FIN_TAIL, ANN_HIP_S2_MULTI, ANN_HIP_POINT_PRECOMP, ANN_HIP_PRECOMP_ALL_TRIES, ANN_HIP_SEGX

Every comparison is exact (ids, distance bytes, every query) and the expectation is always oracle_py.CpuBackend(prec, "oracle"):
precomp and query on the same rows.  A run of the library with the switch off is at most an extra assertion.  As in
tests/test_gpu_size_steps.py every test first asserts, from the host's rules restated below, that its input reaches the path.

What fails if a later pass of the persistent grid is wrong (tried on scratch builds):
  x = xi without P.q0      B's two-piece schedule: the second piece answers the first piece's queries again and leaves its
                           own keys unwritten; the merge flags all of them and the exact path repairs them, so the answers
                           are right and the flagged count (296 against the default launch's 0) is what fails
  cnts[] zeroed once       a later pass adds its valid-slot count to the earlier one's, finalize's prefix test
                           (L1 > P1 && valid >= P1) flags queries it should not: exact_queries differs from the default run's
  yq loaded once           code 0 (d = 2084; the *G folds read the query from global memory) measures every later query
                           against the first query's row: ids and bytes differ
"""
import contextlib

import numpy as np
import pytest
import torch

import approximatenn_amd as A
from oracle import oracle_py as O
from tests.test_gpu_exact_knn import SWEEP
from tests.test_gpu_sharded import _run_sharded
from tests.util import assert_save_equal, bits_equal, load_golden

pytestmark = pytest.mark.gpu

# ---- the host's rules, restated (ann_host.hip, ann_query_kernels.h, ann_device.h)
UNALIGNED, FOLD2, FOLD3, FOLD4, FOLD4G, FOLD5G = -241, -243, -244, -245, -246, -247  # ANN_D_UNALIGNED, ANN_D_FOLD*
SEL_REGS_KMAX = 128   # ANN_SEL_REGS_KMAX: K1 = k + 1 above it keeps the running selection in the LDS buffer kbuf
S2_FUSED_MAX = 1024   # stage2_fused_kernel serves P.Lc2 <= 1024
S2M_CAP = 2048        # ANN_S2M_CAP: stage2_dist_multi_kernel serves Lc2 - k <= 2048 at a power-of-two d
SEGX_SHARE = 0.3      # build_segments: inline records for shards of at most 30 % of the rows ...
SEGX_PM = 255         # ... whose tables have par_maxes <= 255
NP = {"f32": np.float32, "f64": np.float64}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count  # device_cus() reads the same property


def grid_cap(slots, waves):
    """launch_stage1: max_grid = max(1, CUs * 4 * slots / W) workgroups; slots as load_env clamps the switch."""
    slots = max(0, min(8, slots))
    return max(1, cus() * 4 * slots // waves) if slots > 0 else None


def family(prec, d):
    """The kernel family of a row length, through annhip_layout_code: pow2 (RowLay), oc (lanes per row, register
    selection), noregs (the folds, sel_regs_code false), generic (yq in LDS: code 0 and the two *G folds)."""
    code = A._lib.load(prec).annhip_layout_code(d)
    if code > 0:
        return "pow2"
    if code in (0, FOLD4G, FOLD5G):
        return "generic"
    return "noregs" if code in (FOLD2, FOLD3, FOLD4) else "oc"


def need_len(L, k):
    """ann_need_len (ann_device.h)"""
    if L < 16:
        return L
    P = 1 << (L.bit_length() - 1)
    return min(max(P, k) + 1, L)


@contextlib.contextmanager
def switches(monkeypatch, **kv):
    for name, v in kv.items():
        assert name.startswith("ANN_HIP_")
        monkeypatch.setenv(name, str(v))
    A._lib.reload_env()
    try:
        yield
    finally:
        for name in kv:
            monkeypatch.delenv(name, raising=False)
        A._lib.reload_env()
        for prec in ("f32", "f64"):
            A._lib.load(prec).annhip_cache_clear()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ix, ty, alias=False):
    """One batch on a resident index -> ((ids, dists), the call's statistics)."""
    ix.stats(reset=True)
    ids, dd, _ = ix.query(ty, alias=alias)
    torch.cuda.synchronize()
    return (ids.cpu().numpy().astype(np.uint64), dd.cpu().numpy()), ix.stats(reset=True)


def _same(got, want, what):
    bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
    assert bad.size == 0, "%s: ids differ for %d of %d queries, first at batch position %d" % (what, bad.size, len(want[0]), bad[0])
    assert bits_equal(got[1], want[1]), "%s: distances not bit-identical" % (what,)


# ------------------------------------------------------------------------------------------ the data, built once per shape
_cases = {}


class Case:
    """n rows of which every fourth exists twice (twins share a bucket and a distance: a fair share of the queries fails
    finalize's tie test, the others pass it), the oracle's index of them, a fresh batch and the alias batch rows[:Q] with the
    oracle's answers.  narrow: the oracle answers on the rows rounded to that type, as annhip_index_set_rows promises."""

    def __init__(self, prec, d, k, T, Q, n_base=1792, narrow=None, alias=True):
        self.prec, self.d, self.k, self.T, self.Q = prec, d, k, T, Q
        orc = O.CpuBackend(prec, "oracle")
        O.srandom(7000 + d + k)
        orc.rand_norm_reset()
        base = orc.gen_rand(n_base * d).reshape(n_base, d)
        self.pts = np.ascontiguousarray(np.concatenate([base, base[::4]]))
        self.y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
        assert not alias or Q <= n_base
        O.srandom(17)
        _, _, self.save = orc.precomp(self.pts, k, T)
        rows = self.pts
        if narrow:
            with np.errstate(over="ignore"):
                rows = np.ascontiguousarray(self.pts.astype({"f16": np.float16, "f32": np.float32}[narrow]).astype(NP[prec]))
        self.rows = rows
        ids, dd, self.ostats = orc.query(self.save, rows, self.y, stats=True)
        self.want = (ids, dd)
        self.want_alias = orc.query(self.save, rows, Q, alias=True) if alias else None  # query x is row x and leaves it out
        self.tp, self.ty, self.ta = _cuda(self.pts), _cuda(self.y), _cuda(rows[:Q]) if alias else None

    def index(self):
        save = A.Save.from_dict(self.prec, self.save)
        ix = A.Index.from_save(save, self.tp)
        ix._save = save
        return ix


def case(*key, **kw):
    full = key + tuple(sorted(kw.items()))
    if full not in _cases:
        _cases[full] = Case(*key, **kw)
    return _cases[full]


def persistent_q(full=2):
    """Q = full G + 37 for the grid of ANN_HIP_S1_SLOTS=1 with four waves per workgroup (G = CUs: 256 on an MI355X)."""
    return full * grid_cap(1, 4) + 37


# ------------------------------------------------------------------------------------------ A: persistent grid, one device
def _persistent(monkeypatch, c, what, build_env=None, after_build=None, check_stats=None, some_pass=True, full=2):
    """The batch of c, fresh and alias, through the one-workgroup-per-query launch (the default), through the persistent grid
    in full + 1 / full passes (slots = 1, W = 4) and through the grid clamped to Q (slots = 8, W = 1); all against the
    oracle, and the flagged-query count against the default launch's."""
    Q, G = c.Q, grid_cap(1, 4)
    assert G == cus() and Q == full * G + 37 and Q > 2 * G and Q % G != 0  # passes 0 .. full - 1 and a ragged last one
    assert grid_cap(8, 1) == cus() * 32 > Q  # the clamp min(qn, max_grid) decides the grid: one pass
    build_env = dict(build_env or {})
    batches = [(c.ty, False, c.want, "")] + ([(c.ta, True, c.want_alias, ", alias")] if c.want_alias is not None else [])
    with switches(monkeypatch, ANN_HIP_FUSE="0", ANN_HIP_S1_WAVES="4", **build_env):  # the fused launch passes no slots
        ix = c.index()
        if after_build:
            after_build(ix)
        assert ix.L1 > ix.P1  # finalize's prefix test reads the valid-slot count cnts[0]: a stale count can flag a query
        base = [_run(ix, t, alias=al) for t, al, _, _ in batches]
    try:
        for (got, st0), (_, _, want, tag) in zip(base, batches):
            _same(got, want, what + ": default launch" + tag)
            # more flagged queries than the grid has workgroups: at least that many more were flagged in a pass after the
            # first, where F.flist[atomicAdd(F.fcount, 1)] = x is written with the x of that pass
            # Where Lc2 > 1024 stage 2 runs by selection (stage2_select_with_fallback) and adds the rows IT flags, at most Q,
            # to the same counter: stage 1 flagged at least count - Q queries.
            s2 = Q if ix.Lc2 > S2_FUSED_MAX else 0
            print("%s%s: %d flagged of Q = %d (stage 2 adds at most %d), G = %d" % (what, tag, st0["exact_queries"], Q, s2, G))
            assert G < st0["exact_queries"] - s2 and st0["exact_queries"] <= Q + s2, (st0["exact_queries"], G, Q, s2)
            # ... and some queries pass the test (some_pass=False: k = 130 with twin rows, where next to none does)
            assert not some_pass or st0["exact_queries"] < Q
        if check_stats:
            check_stats(base[0][1])
        for slots, waves in (("1", "4"), ("8", "1")):
            with switches(monkeypatch, ANN_HIP_FUSE="0", ANN_HIP_S1_WAVES=waves, ANN_HIP_S1_SLOTS=slots, **build_env):
                runs = [_run(ix, t, alias=al) for t, al, _, _ in batches]
            for (got, st), (_, st0), (_, _, want, tag) in zip(runs, base, batches):
                tag = "%s: slots=%s waves=%s%s" % (what, slots, waves, tag)
                _same(got, want, tag)  # (alias: `id == x` of the self exclusion is the global query index)
                assert st["exact_queries"] == st0["exact_queries"], (tag, st["exact_queries"], st0["exact_queries"])
                assert st["uncertified_queries"] == st0["uncertified_queries"], tag
    finally:
        ix.close()


# (precision, row length, the family annhip_layout_code must put it in); row lengths from SWEEP, plus the issue's 9 and 257
A_LAYOUTS = [("f32", 32, "pow2"), ("f32", 80, "oc"), ("f32", 100, "noregs"), ("f32", 260, "generic"), ("f32", 2084, "generic"),
             ("f64", 32, "pow2"), ("f64", 40, "oc"), ("f64", 100, "noregs"), ("f64", 150, "generic"), ("f64", 300, "generic"),
             ("f64", 2084, "generic")]  # (2084 is code 0, the one layout whose stage 1 reads the LDS copy yq of the query)
A_ODD = [("f32", 9, "oc"), ("f32", 257, "generic"), ("f64", 9, "oc"), ("f64", 257, "generic")]


@pytest.mark.parametrize("prec,d,fam", A_LAYOUTS, ids=["%s-d%d-%s" % c for c in A_LAYOUTS])
def test_persistent_grid_every_kernel_family(prec, d, fam, monkeypatch):
    assert d in SWEEP[prec] and family(prec, d) == fam
    codes = {A._lib.load(prec).annhip_layout_code(d)}
    assert fam != "generic" or codes <= {0, FOLD4G, FOLD5G}  # yq is loaded into LDS at the top of every pass
    c = case(prec, d, 6, 3, persistent_q())
    _persistent(monkeypatch, c, "%s d=%d (%s)" % (prec, d, fam))


@pytest.mark.parametrize("prec,d,fam", A_ODD, ids=["%s-d%d-%s" % c for c in A_ODD])
def test_persistent_grid_odd_row_lengths(prec, d, fam, monkeypatch):
    """d = 9 and d = 257, rows that are no whole number of 16-byte chunks: the table gives 9 the element-wise lanes-per-row
    layout (ANN_D_UNALIGNED, register selection) and 257 the generic code ANN_D_FOLD4G, in both libraries."""
    assert family(prec, d) == fam and A._lib.load(prec).annhip_layout_code(d) == (UNALIGNED if d == 9 else FOLD4G)
    c = case(prec, d, 6, 3, persistent_q())
    _persistent(monkeypatch, c, "%s d=%d (%s)" % (prec, d, fam))


def test_persistent_grid_selection_in_the_lds_buffer(monkeypatch):
    """k = 130: K1 = 131 > ANN_SEL_REGS_KMAX, the running selection lives in kbuf, which every pass reuses.  The oracle
    sorts a row of k (k + 1) = 17 030 entries per point and per query: 400 rows and no alias batch keep it to seconds."""
    k = 130
    assert family("f32", 32) == "pow2" and k + 1 > SEL_REGS_KMAX
    c = case("f32", 32, k, 2, persistent_q(), n_base=320, alias=False)
    _persistent(monkeypatch, c, "f32 k=130", some_pass=False)


def test_persistent_grid_six_passes(monkeypatch):
    """Q = 5 G + 37.  A query sees about a third of P1 valid slots, so a valid-slot count that was carried over from
    earlier passes reaches P1 -- and trips finalize's prefix test -- from the fourth pass on at the latest: asserted from
    the oracle's own count of valid slots.  The flagged-query count must still equal the default launch's."""
    c = case("f32", 32, 6, 3, persistent_q(5))
    per_query = c.ostats["valid1"] / c.Q
    assert c.ostats["L1"] > c.ostats["P1"] and per_query < c.ostats["P1"] / 2 and 4 * per_query >= 1.25 * c.ostats["P1"]
    _persistent(monkeypatch, c, "f32 d=32 six passes", full=5)


@pytest.mark.parametrize("prec,d", [("f32", 32), ("f64", 150)], ids=["f32-d32", "f64-d150"])
def test_persistent_grid_slot_scan(prec, d, monkeypatch):
    """ANN_HIP_SLOT_SCAN=1 at index creation: build_segments leaves use_seg = 0, stage 1 reads every slot (SEG = 0)."""
    c = case(prec, d, 6, 3, persistent_q())
    _persistent(monkeypatch, c, "%s d=%d slot scan" % (prec, d), build_env={"ANN_HIP_SLOT_SCAN": "1"})


@pytest.mark.parametrize("prec,narrow,d", [("f32", "f16", 32), ("f32", "f16", 260), ("f64", "f32", 32), ("f64", "f32", 150)],
                         ids=["f32-f16-d32", "f32-f16-d260", "f64-f32-d32", "f64-f32-d150"])
def test_persistent_grid_narrow_rows(prec, narrow, d, monkeypatch):
    """Index.set_rows: the RT = RN instances; the oracle answers on the rounded rows."""
    c = case(prec, d, 6, 3, persistent_q(), narrow=narrow)

    def narrow_rows(ix):
        ix.set_rows(narrow)
        assert ix.rows == narrow
    _persistent(monkeypatch, c, "%s rows %s d=%d" % (prec, narrow, d), after_build=narrow_rows)


def test_persistent_grid_pruned_preselection(monkeypatch):
    """ANN_HIP_PRUNE=1 on an eligible f32 index: the preselection is the stage-1 launch that gets `slots`; keys = kp."""
    c = case("f32", 32, 6, 3, persistent_q())

    def pruned(ix):
        assert ix.prune and ix.prune_bound is not None and ix.prune_bound[1] >= c.k + 1

    def mostly_certified(st0):
        assert st0["uncertified_queries"] <= st0["exact_queries"] and st0["uncertified_queries"] < c.Q / 2
    _persistent(monkeypatch, c, "f32 pruned", build_env={"ANN_HIP_PRUNE": "1"}, after_build=pruned, check_stats=mostly_certified)


@pytest.mark.parametrize("value", ["0", "-3", "99"])
def test_slots_switch_is_clamped(value, monkeypatch):
    """load_env clamps ANN_HIP_S1_SLOTS to 0..8: 0 and -3 are the default launch, 99 is 8 (grid CUs * 8 > Q: one pass)."""
    c = case("f32", 32, 6, 3, persistent_q())
    assert grid_cap(int(value), 4) in (None, cus() * 8) and cus() * 8 > c.Q
    with switches(monkeypatch, ANN_HIP_FUSE="0", ANN_HIP_S1_WAVES="4"):
        ix = c.index()
        base, st0 = _run(ix, c.ty)
    try:
        with switches(monkeypatch, ANN_HIP_FUSE="0", ANN_HIP_S1_WAVES="4", ANN_HIP_S1_SLOTS=value):
            got, st = _run(ix, c.ty)
        _same(got, c.want, "slots=" + value)
        assert bits_equal(got[1], base[1]) and np.array_equal(got[0], base[0]) and st["exact_queries"] == st0["exact_queries"]
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ B: persistent grid, sharded
_heavy = {}


def heavy(prec, Q):
    """The rows of tests/test_gpu_sharded.py::test_small_shards_with_a_heavy_bucket (a cluster of 120 near-identical points:
    buckets with far more owned ids than the 7 an inline record holds) with a batch of Q queries, 32 of them at the cluster."""
    if (prec, Q) not in _heavy:
        orc = O.CpuBackend(prec, "oracle")
        O.srandom(2025)
        orc.rand_norm_reset()
        n, d, k, T = 4000, 32, 5, 3
        pts = orc.gen_rand(n * d).reshape(n, d)
        rng = np.random.default_rng(3)
        hv = rng.choice(n, size=120, replace=False)
        pts[hv] = pts[hv[0]] + (1e-3 * orc.gen_rand(120 * d).reshape(120, d)).astype(pts.dtype)
        y = orc.gen_rand(Q * d).reshape(Q, d)
        late = Q - 40  # the cluster's queries sit in the last stride of the grid and in the second piece
        y[late:late + 32] = pts[hv[0]] + (1e-2 * orc.gen_rand(32 * d).reshape(32, d)).astype(pts.dtype)
        pts, y = np.ascontiguousarray(pts), np.ascontiguousarray(y)
        O.srandom(8)
        _, _, save = orc.precomp(pts, k, T)
        pm = max(int(v) for v in save["par_maxes"])
        assert 60 < pm <= SEGX_PM
        rev = np.ascontiguousarray(y[::-1])  # the same queries in reverse order: another batch, position by position
        assert not (rev == y).all(axis=1)[-(-Q // 2):].any()  # (an odd Q's middle query, in the first piece, is its own mirror)
        _heavy[(prec, Q)] = dict(pts=pts, y=y, rev=rev, save=save, want=orc.query(save, pts, y), want_rev=orc.query(save, pts, rev),
                                 want_alias=orc.query(save, pts, Q, alias=True))
    return _heavy[(prec, Q)]


def sharded_q():
    return 2 * cus() + cus() * 3 // 10 + 5  # about 2.3 G


def expected_seg(world, save, segx=None):
    """build_segments restated: 2 (inline records) for a shard of <= 30 % of the rows with par_maxes <= 255, unless
    ANN_HIP_SEGX=0; else 1 (segment words).  ANN_HIP_SEGX=1 does not waive either condition."""
    small = 1.0 / world <= SEGX_SHARE and max(int(v) for v in save["par_maxes"]) <= SEGX_PM
    return 2 if small and segx != 0 else 1


B_SCHEDULES = [(2, False, 0, 1, 1), (3, True, 0, 2, 1)]  # (lanes, two-half issue, reserved CUs, pieces, slots)


@pytest.mark.parametrize("schedule", B_SCHEDULES, ids=["whole", "two-pieces"])
@pytest.mark.parametrize("prec,world,fast,alias", [("f32", 2, True, False), ("f64", 2, False, False), ("f32", 4, True, False),
                                                   ("f64", 4, False, False), ("f32", 4, True, True), ("f32", 2, False, True)],
                         ids=["f32-w2-a2a", "f64-w2-ag", "f32-w4-a2a", "f64-w4-ag", "f32-w4-alias", "f32-w2-alias"])
def test_persistent_grid_sharded(prec, world, fast, alias, schedule, monkeypatch):
    """A fresh batch takes turns with its reverse, so that every lane's key and count buffers serve both in alternation
    (_run_sharded, other=): a piece that writes the wrong queries' entries leaves its own holding the OTHER batch's keys,
    which belong to other query vectors at every position -- wrong by construction, whatever the allocator handed out.
    Such queries fail the merge's test and are answered by the exact path, so the flagged count is what gives them away."""
    pieces = schedule[3]
    Q, G = sharded_q(), grid_cap(schedule[4], 4)
    assert G == cus() and -(-Q // pieces) > G  # every piece makes a second pass; with two pieces one of them at P.q0 > 0
    assert pieces == 1 or (Q - -(-Q // pieces)) > G
    h = heavy(prec, Q)
    assert expected_seg(world, h["save"]) == (2 if world == 4 else 1)
    y, want, other = (h["pts"][:Q], h["want_alias"], None) if alias else (h["y"], h["want"], h["rev"])
    last, want_last = (y, want) if other is None else (other, h["want_rev"])  # the batch a rank's last_exact belongs to
    with switches(monkeypatch, ANN_HIP_S1_WAVES="4"):  # W = 4 keeps the grid at CUs workgroups (own_frac alone gives W = 1)
        base = _run_sharded(prec, h["save"], h["pts"], last, world, alias=alias, fast=fast)  # one workgroup per query
        res = _run_sharded(prec, h["save"], h["pts"], y, world, alias=alias, fast=fast, schedule=schedule, other=other)
    for rank, (r, b) in enumerate(zip(res, base)):
        what = "%s world %d rank %d schedule %s" % (prec, world, rank, schedule)
        _same(b[:2], want_last, what + ", default launch")
        _same(r[:2], want, what)
        if other is not None:
            _same(r[3], h["want_rev"], what + ", reversed batch")
        # The owner protocol repairs what it flags: queries whose keys a piece never wrote come out right, through the exact
        # path.  The count of flagged queries shows them, against the default launch's for the same batch.
        assert r[2] == b[2], (what, "flagged queries", r[2], "default launch", b[2])


# ------------------------------------------------------------------------------------------ C: the other switches
@pytest.mark.parametrize("k", [6, 17])
@pytest.mark.parametrize("prec,d", [("f32", 32), ("f32", 260), ("f64", 32), ("f64", 150)], ids=["f32-d32", "f32-d260", "f64-d32", "f64-d150"])
def test_stage2_with_128_threads(prec, d, k, monkeypatch):
    """ANN_HIP_S2_THREADS=128: stage2_fused_kernel with two waves; any other value is 64."""
    c = case(prec, d, k, 3, 301)
    assert family(prec, d) == ("pow2" if d == 32 else "generic")
    for threads in ("128", "96"):
        with switches(monkeypatch, ANN_HIP_FUSE="0", ANN_HIP_S2_THREADS=threads):
            ix = c.index()
            try:
                assert ix.Lc2 == need_len(k * (k + 1), k) <= S2_FUSED_MAX and ix.n == c.pts.shape[0]  # whole index: the fused stage 2
                _same(_run(ix, c.ty)[0], c.want, "%s d=%d k=%d threads=%s" % (prec, d, k, threads))
                _same(_run(ix, c.ta, alias=True)[0], c.want_alias, "%s d=%d k=%d threads=%s alias" % (prec, d, k, threads))
            finally:
                ix.close()


@pytest.mark.parametrize("prec,d", [("f32", 32), ("f64", 100)], ids=["f32-d32", "f64-d100"])
def test_finalize_as_its_own_launch(prec, d, monkeypatch):
    """ANN_HIP_FIN_TAIL=0 with ANN_HIP_FUSE=0: stage 1 runs with F.enabled = 0 and finalize1_kernel tests the candidates."""
    c = case(prec, d, 6, 3, 301)
    with switches(monkeypatch, ANN_HIP_FUSE="0"):
        ix = c.index()
        base, st0 = _run(ix, c.ty)
    try:
        _same(base, c.want, "in the tail")
        assert 0 < st0["exact_queries"] < c.Q  # both outcomes of the test occur
        with switches(monkeypatch, ANN_HIP_FUSE="0", ANN_HIP_FIN_TAIL="0"):
            got, st = _run(ix, c.ty)
            got_a, _ = _run(ix, c.ta, alias=True)
        _same(got, c.want, "own launch")
        _same(got_a, c.want_alias, "own launch, alias")
        assert st["exact_queries"] == st0["exact_queries"]
    finally:
        ix.close()


@pytest.mark.parametrize("name,world", [("pow2_d32_f32", 2), ("pow2_d128_f32", 3), ("pow2_d128_f64", 2), ("pow2_d32_f64", 3)])
def test_sharded_stage2_one_workgroup_per_query(name, world, monkeypatch):
    """ANN_HIP_S2_MULTI=0 at a power-of-two d, where annhip_sh_stage2 otherwise takes stage2_dist_multi_kernel."""
    g = load_golden(name)
    c, prec = g["cfg"], g["prec"]
    assert family(prec, c["d"]) == "pow2" and 0 < need_len(c["k"] * (c["k"] + 1), c["k"]) - c["k"] <= S2M_CAP
    orc = O.CpuBackend(prec, "oracle")
    pts, y = np.ascontiguousarray(g["points"]), np.ascontiguousarray(g["y"])
    want = orc.query(g["save"], pts, y)
    with switches(monkeypatch, ANN_HIP_S2_MULTI="0"):
        for fast in (True, False):
            for rank, (ids, dd, _) in enumerate(_run_sharded(prec, g["save"], pts, y, world, fast=fast)):
                _same((ids, dd), want, "%s world %d rank %d" % (name, world, rank))


def tries_scored(k, T):
    """annhip_precomp_begin: min(T, ceil(ann_need_len(k T, k) / k))"""
    return min(T, -(-need_len(k * T, k) // k))


def _precomp_equals_the_oracles(prec, d, k, T, what):
    orc = O.CpuBackend(prec, "oracle")
    O.srandom(7500 + d)
    orc.rand_norm_reset()
    n, Q = 2000, 150
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    y = np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))
    O.srandom(29)
    o_ids, o_d, o_save = orc.precomp(pts, k, T)
    O.srandom(29)
    ids, dd, save = A.precomp(pts, k, T)
    try:
        assert np.array_equal(ids, o_ids) and bits_equal(dd, o_d), what + ": graph"
        assert_save_equal(save.to_dict(), o_save)
        _same(A.query(save, pts, y), orc.query(o_save, pts, y), what + ": query")
    finally:
        A._lib.load(prec).annhip_cache_clear()
        save.free()


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_precomp_per_point_at_a_power_of_two(prec, d, monkeypatch):
    """ANN_HIP_POINT_PRECOMP=1: launch_stage1_bucket declines, precomp's stage 1 runs per point at a d that otherwise takes
    the bucket kernel (d_is_fast)."""
    assert family(prec, d) == "pow2"
    with switches(monkeypatch, ANN_HIP_POINT_PRECOMP="1"):
        _precomp_equals_the_oracles(prec, d, 6, 4, "%s d=%d per point" % (prec, d))


@contextlib.contextmanager
def precomp_infos(prec):
    """What annhip_precomp_info reports to approximatenn_amd.sharded.precomp_sharded while the block runs: a list of
    [d_short, Wn, tries scored, tries, n, k], one entry per build (rank threads append side by side)."""
    lib, seen = A._lib.load(prec), []
    real = lib.annhip_precomp_info

    def spy(h, ref):
        real(h, ref)
        seen.append([int(v) for v in ref._obj])
    lib.annhip_precomp_info = spy
    try:
        yield seen
    finally:
        lib.annhip_precomp_info = real


def _device_build(prec, pts, k, T, seed):
    """precomp_sharded on one rank -- annhip_precomp_index's own sequence -- -> (save dict, graph distances, info)."""
    from approximatenn_amd.sharded import precomp_sharded
    with precomp_infos(prec) as seen:
        O.srandom(seed)
        ix = precomp_sharded(_cuda(pts), k, T, want_dists=True)
    try:
        save = ix.export()
        sd = save.to_dict()
        save.free()
        torch.cuda.synchronize()
        assert len(seen) == 1
        return sd, ix.graph_dists.cpu().numpy(), seen[0]
    finally:
        ix.close()


@pytest.mark.parametrize("prec,d", [("f32", 32), ("f64", 64), ("f32", 80)], ids=["f32-d32", "f64-d64", "f32-d80"])
def test_precomp_scores_every_try(prec, d, monkeypatch):
    """ANN_HIP_PRECOMP_ALL_TRIES=1: no try skips its distance pass and the merged rows have the stride T k.  That the switch
    took effect is read from annhip_precomp_info: tries scored == tries and Wn = T k with it, fewer and shorter without."""
    k, T, n = 5, 6, 1500
    assert tries_scored(k, T) == 4 < T  # by default the last two tries are never scored
    orc = O.CpuBackend(prec, "oracle")
    O.srandom(7600 + d)
    orc.rand_norm_reset()
    pts = np.ascontiguousarray(orc.gen_rand(n * d).reshape(n, d))
    O.srandom(31)
    _, o_d, o_save = orc.precomp(pts, k, T)
    sd, gd, info = _device_build(prec, pts, k, T, 31)
    assert info[2] == tries_scored(k, T) < info[3] == T and info[1] == info[2] * k, info
    assert_save_equal(sd, o_save)
    assert bits_equal(gd, o_d)
    with switches(monkeypatch, ANN_HIP_PRECOMP_ALL_TRIES="1"):
        sd, gd, info = _device_build(prec, pts, k, T, 31)
        assert info[2] == info[3] == T and info[1] == T * k, info
        assert_save_equal(sd, o_save)
        assert bits_equal(gd, o_d)
        _precomp_equals_the_oracles(prec, d, k, T, "%s d=%d every try" % (prec, d))  # precomp_gpu, then query_gpu


def test_sharded_precomp_scores_every_try(monkeypatch):
    """The same through precomp_sharded on two ranks, on a golden case: the oracle's precomp gives the golden index, and
    every rank's build reports all tries scored and gives that index (tests/test_gpu_sharded.py's check)."""
    from tests.test_gpu_sharded import sharded_precomp_matches_golden
    g = load_golden("pow2_d64_f32")
    c = g["cfg"]
    assert tries_scored(c["k"], c["tries"]) < c["tries"]
    orc = O.CpuBackend("f32", "oracle")
    O.srandom(c["seed"])  # the libc stream as the golden generator had it after drawing the points
    orc.rand_norm_reset()
    orc.gen_rand(c["n"] * c["d"] + (c["n"] * c["d"]) % 2)
    o_ids, o_d, o_save = orc.precomp(np.ascontiguousarray(g["points"]), c["k"], c["tries"], c["rb"], c["rlb"], c["ra"], c["rla"])
    assert_save_equal(o_save, g["save"])
    assert bits_equal(o_d, g["precomp_dists"])
    with switches(monkeypatch, ANN_HIP_PRECOMP_ALL_TRIES="1"), precomp_infos("f32") as seen:
        sharded_precomp_matches_golden("pow2_d64_f32", 2)
    assert len(seen) == 2 and all(i[2] == i[3] == c["tries"] and i[1] == c["tries"] * c["k"] for i in seen), seen


@pytest.mark.parametrize("segx,world", [(0, 4), (0, 8), (1, 4)])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_inline_records_forced_off_and_on(prec, segx, world, monkeypatch):
    """ANN_HIP_SEGX at shards that qualify for the inline records (1/4 and 1/8 of the rows, par_maxes <= 255): 0 -> use_seg = 1,
    the segment words the automatic choice never takes here; 1 -> use_seg = 2, as the automatic choice."""
    h = heavy(prec, 96)
    assert expected_seg(world, h["save"]) == 2 and expected_seg(world, h["save"], segx) == (1 if segx == 0 else 2)
    with switches(monkeypatch, ANN_HIP_SEGX=str(segx)):
        for rank, (ids, dd, _) in enumerate(_run_sharded(prec, h["save"], h["pts"], h["y"], world)):
            _same((ids, dd), h["want"], "%s segx=%d world %d rank %d" % (prec, segx, world, rank))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_inline_records_are_refused_on_a_whole_index(prec, monkeypatch):
    """ANN_HIP_SEGX=1 on a single-device index: the shard holds all rows (> 30 %), so use_seg stays 1 -- the switch lifts
    neither that rule nor par_maxes <= 255; the records would be wrong for ids outside the shard, the answer shows it is not."""
    h = heavy(prec, 96)
    assert expected_seg(1, h["save"], 1) == 1
    with switches(monkeypatch, ANN_HIP_SEGX="1"):
        save = A.Save.from_dict(prec, h["save"])
        ix = A.Index.from_save(save, _cuda(h["pts"]))
        try:
            for fuse in ("0", "1"):
                with switches(monkeypatch, ANN_HIP_SEGX="1", ANN_HIP_FUSE=fuse):
                    _same(_run(ix, _cuda(h["y"]))[0], h["want"], "%s whole index, fuse=%s" % (prec, fuse))
        finally:
            ix.close()


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_data():
    yield
    _cases.clear()
    _heavy.clear()
