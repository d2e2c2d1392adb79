"""GPU: the fixed-mode query families and the tail at a row length of every layout code (tests/test_gpu_exact_knn.py::
SWEEP; tests/test_layout_table.py proves the list complete).  Every kernel that reads point rows is instantiated once per
code -- its own lane map, chunk count, wave count and LDS carve-up -- so each family runs here at each code:
stage1_probe / codes_probe (ann_probe_kernels.h), the filter and tag forms of stage 1 and stage 2 (ann_filter_kernels.h,
ann_tag_kernels.h), stage2_kq (ann_kq_kernels.h), tail_merge in its three validity forms and its generic form
(ann_tail_kernels.h), and Index.exact_query over built rows plus tail.

The expectation is the contract of tests/test_gpu_query_k.py::Oracle with both scans done in numpy: np_dists (the
reference's halving tree) gives the [Q, n] distances once per batch, np.lexsort((ids, distance bits)) selects.  No kernel
of the library produces a distance or a selection of the expectation; the library contributes its hash codes, asserted
equal to the CPU oracle's, and its ranked probe bits (tests/test_gpu_probe.py checks those at every code).  Every
comparison is on ids and distance bytes, every query.

One index per row length serves both parts: the query families first, then 700 rows are appended and the same variants
must return the merge of the rows just verified and the tail's exact neighbours."""
import numpy as np
import pytest
import torch

from approximatenn_amd.sharded import HipEngine
from tests.test_gpu_exact_knn import SWEEP_CASES, np_dists
from tests.test_gpu_probe import _build_host, pts_bytes
from tests.test_gpu_query_k import _build, _codes_of, _dict, _masks, _np, _ranked, _tenants
from tests.test_gpu_tail import _tile_rows

pytestmark = pytest.mark.gpu

N, KG, T, Q, M = 1500, 6, 2, 24, 700
KS = (1, KG, KG + 7, 100)
FORMS = ("plain", "allow", "where", "allow+where")


def _bits(d):
    return d.view(np.uint32 if d.dtype == np.float32 else np.uint64)


def _top(ids, dist_row, k):
    """The k smallest of ids by (distance bits, id)."""
    return ids[np.lexsort((ids, _bits(dist_row[ids])))[:k]]


def _padded(ids, dist_row, k, pad):
    out_i = np.full(k, pad, dtype=np.int64)
    out_d = np.full(k, np.inf, dtype=dist_row.dtype)
    out_i[:ids.size], out_d[:ids.size] = ids, dist_row[ids]
    return out_i, out_d


class Batch:
    """One query batch against the built rows: distances, raw candidate sets per probe setting, validity per form."""

    def __init__(self, ix, sd, orc, pts, ty, alias, allow, tags, where):
        self.ty, self.alias, self.where = ty, alias, where
        y = ty.cpu().numpy()
        n, ds = pts.shape[0], sd["d_short"]
        self.dist = np_dists(pts, y)
        codes = _codes_of(HipEngine(ix), ty, T)
        assert np.array_equal(codes.reshape(-1), orc.query_codes(sd, y).astype(np.int64)), "hash codes differ from the oracle's"
        tabs = [np.asarray(sd["which_par"][t]).reshape(1 << ds, -1) for t in range(T)]
        self.raw = {}
        for probe in (0, 3):
            ix.set_probe(probe)
            ranked = _ranked(ix, ty)
            raw = np.zeros((Q, n), dtype=bool)
            for x in range(Q):
                for t in range(T):
                    for m in _masks(ds, ranked[x][t]):
                        row = tabs[t][int(codes[x, t]) ^ m]
                        raw[x, row[row < n].astype(np.int64)] = True
            self.raw[probe] = raw
        ix.set_probe(0)
        base = np.ones((Q, n), dtype=bool)
        if alias:
            base[np.arange(Q), np.arange(Q)] = False
        tagged = (tags[None, :n] & where[0][:, None]) == where[1][:, None]
        self.valid = {"plain": base, "allow": base & allow[None, :n], "where": base & tagged,
                      "allow+where": base & tagged & allow[None, :n]}

    def stages(self, graph, probe, form, x, k):
        """(stage-1 ids, stage-2 set) of query x: the k best valid candidates, then those plus their valid graph neighbours."""
        valid = self.valid[form][x]
        s1 = _top(np.flatnonzero(self.raw[probe][x] & valid), self.dist[x], k)
        nb = graph[s1].reshape(-1)
        nb = nb[nb < valid.size]
        return s1, np.union1d(s1, nb[valid[nb]])

    def rows(self, graph, probe, form, k):
        """The expected [Q, k] ids and distances, (n, +inf) where fewer than k candidates exist."""
        n = self.dist.shape[1]
        out = [_padded(_top(self.stages(graph, probe, form, x, k)[1], self.dist[x], k), self.dist[x], k, n) for x in range(Q)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _same(got, want, what):
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert bad.size == 0, "%s: ids differ for %d queries, first %d: got %s want %s" % (
        what, bad.size, bad[0], got[0][bad[0]][:12], want[0][bad[0]][:12])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), "%s: distances not bit-identical" % (what,)


def _settings(ix, form, allow, tags):
    """Tags are row attributes that only where= reads; the allow list is set for the forms that name it."""
    ix.set_tags(tags)
    ix.set_filter(allow if form.startswith("allow") else None)


@pytest.mark.parametrize("prec,d", SWEEP_CASES, ids=["%s-d%d" % c for c in SWEEP_CASES])
def test_query_families_then_the_tail_at_every_layout(prec, d):
    # rows of more than 4096 bytes: built on the host, the device precomp's hashing has no room for them
    orc, pts, tp, ix = (_build_host if d * pts_bytes(prec) > 4096 else _build)(prec, N, d, KG, T, 9100 + d)
    try:
        rng = np.random.default_rng(9200 + d)
        ty = torch.from_numpy(np.ascontiguousarray(orc.gen_rand(Q * d).reshape(Q, d))).cuda()
        ta = tp[:Q].contiguous()
        sd = _dict(ix)
        graph = np.asarray(sd["graph"]).reshape(N, KG).astype(np.int64)
        ix.set_fixed(True)
        assert ix.max_query_k >= max(KS)
        allow = rng.random(N + M) < 0.4              # full length: the first N serve the built rows
        tags, where = _tenants(N + M, Q, 9300 + d)    # the queries ask for tenant 0, 1, 2 and for everything, in turn
        batches = [Batch(ix, sd, orc, pts, yy, alias, allow, tags, where) for yy, alias in ((ty, False), (ta, True))]

        # ---- preconditions, on the expectation: a vacuous case fails here
        for b in batches:
            grew = sum(int(b.raw[3][x].sum() > b.raw[0][x].sum()) for x in range(Q))
            assert 2 * grew >= Q, ("probe 3 enlarges too few candidate sets", b.alias, grew)
            added = sum(int(np.setdiff1d(b.stages(graph, 0, "plain", x, KG)[1], np.flatnonzero(b.raw[0][x])).size > 0)
                        for x in range(Q))
            assert 2 * added >= Q, ("stage 2 adds an id beyond stage 1's candidates for too few queries", b.alias, added)
            plain_i = b.rows(graph, 0, "plain", KG)[0]
            cut = sum(int((~allow[plain_i[x][plain_i[x] < N]]).any()) for x in range(Q))
            assert 2 * cut >= Q, ("the allow list removes an id from too few unfiltered rows", b.alias, cut)

        # ---- the query families on the built rows
        recorded = {}
        for b in batches:
            for probe in (0, 3):
                ix.set_probe(probe)
                for form in FORMS:
                    _settings(ix, form, allow[:N], tags[:N])
                    kw = dict(alias=b.alias, **(dict(where=where) if form.endswith("where") else {}))
                    what = "%s d=%d probe=%d %s alias=%d" % (prec, d, probe, form, b.alias)
                    today = _np(ix.query(b.ty, **kw))
                    assert today[0].shape == (Q, KG)
                    for k in KS:
                        want = b.rows(graph, probe, form, k)
                        got = _np(ix.query(b.ty, k=k, **kw))
                        _same(got, want, what + " k=%d" % k)
                        if k == KG:
                            _same(today, got, what + " plain call against k=kg")
                        if probe == 0:
                            recorded[(b.alias, form, k)] = want
        ix.set_probe(0)

        # ---- the tail: one append of several LDS tiles (384 rows at d = 16 f32 down to one row at d = 2084); the last
        # tile is ragged except where the tile divides 700 (2, 10 or 20 rows: d = 384 f32; d = 100, 192, 1024 f64)
        assert M > _tile_rows(prec, d, KG)
        tail = np.ascontiguousarray(rng.standard_normal((M, d)).astype(pts.dtype))
        tail[5] = pts[7]  # a duplicate of a built row
        ix.set_filter(None), ix.set_tags(None)
        assert ix.append(torch.from_numpy(tail).cuda()) == N and ix.tail == M and ix.n_total == N + M
        tagged = (tags[None, N:] & where[0][:, None]) == where[1][:, None]
        tvalid = {"plain": np.ones((Q, M), dtype=bool), "allow": np.broadcast_to(allow[N:], (Q, M)), "where": tagged,
                  "allow+where": tagged & allow[None, N:]}
        for b in batches:
            tdist = np_dists(tail, b.ty.cpu().numpy())  # an aliased query is a built row: it skips no tail row
            both = np.concatenate([b.dist, tdist], axis=1)

            def merged(form, k):
                """The k best of the recorded row (pads dropped) and the tail's k exact neighbours (ids + N)."""
                base, out = recorded[(b.alias, form, k)][0], []
                for x in range(Q):
                    theirs = N + _top(np.flatnonzero(tvalid[form][x]), tdist[x], k)
                    out.append(_top(np.concatenate([base[x][base[x] < N], theirs]), both[x], k))
                return out

            def exact(form, k):
                valid = np.concatenate([b.valid[form], tvalid[form]], axis=1)
                return [_top(np.flatnonzero(valid[x]), both[x], k) for x in range(Q)]

            def padded(ids, k):
                rows = [_padded(ids[x], both[x], k, N + M) for x in range(Q)]
                return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])

            plain = merged("plain", KG)
            kept, gained = sum(int((r < N).any()) for r in plain), sum(int((r >= N).any()) for r in plain)
            assert 4 * kept >= Q and 4 * gained >= Q, ("the merge is one-sided", b.alias, kept, gained)
            for form in FORMS:
                _settings(ix, form, allow, tags)
                kw = dict(alias=b.alias, **(dict(where=where) if form.endswith("where") else {}))
                for k in (KG, 1, 100):
                    what = "%s d=%d tail %s alias=%d k=%d" % (prec, d, form, b.alias, k)
                    want = padded(merged(form, k), k)
                    _same(_np(ix.query(b.ty, k=k, **kw)), want, what)
                    if k == KG:
                        _same(_np(ix.query(b.ty, **kw)), want, what + " plain call")
                    want = padded(exact(form, k), k)
                    _same(_np(ix.exact_query(b.ty, k=k, **kw)), want, what + " exact_query")
                    if k == KG:
                        _same(_np(ix.exact_query(b.ty, **kw)), want, what + " exact_query plain call")
    finally:
        ix.close()
