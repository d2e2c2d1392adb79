"""numpy model of the pruned stage 1 (approximatenn_amd/csrc/ann_prune_kernels.h): preselect K' keys on the binary16
copy of the rows, rescore them on the float rows, certify.  Shared by tests/test_prune_model.py (CPU) and
tests/test_gpu_prune.py (which uses it to choose a data set where both outcomes occur).

The second half is the EXACT model (DeviceModel: the device's candidates, distance bits, order and certificate, query by
query) and the trap data (trap_case) that tests/test_gpu_prune_certificate.py and tests/test_gpu_prune_layouts.py compare
the device's decisions with."""
import numpy as np

GAMMA = 2.0 ** -16


def h(p):
    """The rows rounded to binary16 and widened back (what annhip_index_set_rows stores)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(p, dtype=np.float32).astype(np.float16).astype(np.float32))


def row_error(p):
    """E >= max over the rows of ||p - h(p)||_2, in double, rounded up; inf where a row does not survive binary16."""
    df = np.asarray(p, dtype=np.float64) - h(p).astype(np.float64)
    with np.errstate(invalid="ignore"):
        worst = np.max(np.sum(df * df, axis=1))
    if not np.isfinite(worst):
        return np.inf
    return float(np.sqrt(worst) * (1.0 + 2.0 ** -20))


def row_error_true(p):
    """max over the rows of ||p - h(p)||_2 in double, not rounded up: what the device's E must lie just above."""
    df = np.asarray(p, dtype=np.float64) - h(p).astype(np.float64)
    return float(np.sqrt(np.max(np.sum(df * df, axis=1))))


def sqdist32(y, rows):
    """Squared distances in float32 (a float tree of non-negative terms: within (1 + 2^-24)^(few) of the real sum)."""
    df = (rows - y[None, :]).astype(np.float32)
    return np.sum(df * df, axis=1, dtype=np.float32)


def keys_sorted(dist, ids):
    """Indices that order (distance bits, id) ascending: the selection path's total order."""
    return np.lexsort((ids, dist.view(np.uint32)))


def certify(B, tau, E):
    """The certificate of one query whose preselection is full: LB > tau, written so that everything odd fails."""
    B, tau = np.float64(B), np.float64(tau)
    g1 = 1.0 - GAMMA
    with np.errstate(invalid="ignore"):
        r = np.sqrt(B * g1) - E
    if not (B >= 2.0 ** -100 and r > 0.0):
        return False
    LB = (r * r) * g1 * (1.0 - 2.0 ** -40)
    return bool(LB > tau)


def prune_query(y, rows, rows_h, ids, k, kp, E):
    """One query against the candidate rows `rows` (ids `ids`, distinct).  Returns (certified, rescored, truth):
    rescored = the k+1 smallest exact keys among the preselection, truth = among ALL candidates, as (dist, id) arrays."""
    K1 = k + 1
    dh = sqdist32(y, rows_h)
    pre = keys_sorted(dh, ids)[:kp]
    m = pre.size
    dx = sqdist32(y, rows[pre])
    o = keys_sorted(dx, ids[pre])[:K1]
    rescored = (dx[o], ids[pre][o])
    dall = sqdist32(y, rows)
    oa = keys_sorted(dall, ids)[:K1]
    truth = (dall[oa], ids[oa])
    if m < kp:
        cert = True
    elif o.size < K1:
        cert = False
    else:
        cert = certify(dh[pre[-1]], rescored[0][K1 - 1], E)
    return cert, rescored, truth


def default_keys(k):
    return min(64, max(16, 3 * (k + 1) // 2))


def clamp_keys(k, asked):
    """K' of an index with this k under ANN_HIP_PRUNE_K=asked (0: unset): clamped to k + 1 ... 64 (prune_keys)."""
    return min(64, max(asked if asked > 0 else default_keys(k), k + 1))


# ------------------------------------------------------------------------------------------------------------------
# The exact model of the device's decision.  Nothing below calls a kernel of the library: the candidate ids come from the
# oracle's hash codes and the saved bucket tables (CpuShardEngine._row_ids), the distances from the numpy halving tree
# that tests/test_gpu_exact_knn.py ties to the oracle's tree pair by pair (the query path's bits), the order is
# (distance bits, id) and the certificate is certify() above.

def margin_of(B, tau, E):
    """How far the certificate's comparison is from flipping, relative: |LB - tau| / tau where the root clears E,
    |root - E| / E where it does not.  inf where nothing finite is compared."""
    B, tau = np.float64(B), np.float64(tau)
    g1 = 1.0 - GAMMA
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(B * g1) - E
        if not np.isfinite(r) or not B >= 2.0 ** -100:
            return np.inf
        if not r > 0.0:
            return float(abs(r) / E) if E > 0 else np.inf
        LB = (r * r) * g1 * (1.0 - 2.0 ** -40)
        return float(abs(LB - tau) / tau) if tau > 0 else np.inf


def decide(dh, dx, ids, k, kp, E):
    """One query: dh / dx = the distances of its distinct candidates `ids` on the narrow and on the native rows.
    Returns (certified, trap, margin): trap = the k+1 smallest exact keys of the preselection are not the k+1 smallest
    exact keys of all candidates."""
    K1 = k + 1
    pre = keys_sorted(dh, ids)[:kp]
    o = keys_sorted(dx[pre], ids[pre])[:K1]
    oa = keys_sorted(dx, ids)[:K1]
    got, want = pre[o], oa
    trap = not (np.array_equal(ids[got], ids[want]) and np.array_equal(dx[got].view(np.uint32), dx[want].view(np.uint32)))
    if pre.size < kp:
        return True, trap, np.inf
    B, tau = dh[pre[-1]], dx[got[K1 - 1]]
    return certify(B, tau, E), trap, margin_of(B, tau, E)


class Decisions:
    def __init__(self, rows):
        self.certified = np.array([r[0] for r in rows], dtype=bool)
        self.trap = np.array([r[1] for r in rows], dtype=bool)
        self.margin = np.array([r[2] for r in rows], dtype=np.float64)
        self.Q = len(rows)
        self.uncertified = int(np.sum(~self.certified))
        self.wrong = int(np.sum(self.certified & self.trap))

    def __repr__(self):
        return "traps=%d certified=%d uncertified=%d wrong=%d min margin=%.3g" % (
            int(self.trap.sum()), int(self.certified.sum()), self.uncertified, self.wrong, float(self.margin.min()))

    def check(self, what):
        """The conditions a trap data set must meet before it is worth a device run (conditions on the inputs)."""
        assert int(self.trap.sum()) >= 3, "%s: only %d trap queries" % (what, int(self.trap.sum()))
        assert self.wrong == 0, "%s: the model certifies %d trap queries" % (what, self.wrong)
        assert 0 < self.uncertified < self.Q, "%s: one outcome only (%r)" % (what, self)
        assert float(self.margin.min()) >= 2.0 ** -30, "%s: a decision hangs on the last bits (%r)" % (what, self)


class DeviceModel:
    """The pruned stage 1 of one index (its save as a dict, its rows), restated."""

    def __init__(self, sd, pts):
        from tests.cpu_engine import CpuShardEngine
        self.pts = np.ascontiguousarray(pts, dtype=np.float32)
        self.hp = h(self.pts)
        self.eng = CpuShardEngine(sd, self.pts, 0, int(sd["n"]), "f32")
        self.k, self.n, self.P1 = self.eng.k, self.eng.n, self.eng.P1

    def gather(self, y, alias=False):
        """Per query of the batch y: (ids, distances on h(rows), distances on the rows) of the distinct valid ids in the
        first P1 slots of its candidate row.  The hash codes are read as the query path reads them, which depends on
        the batch's size: a query asked alone has another candidate row than the same query inside a batch."""
        from tests.test_gpu_exact_knn import np_tree
        y = np.ascontiguousarray(y, dtype=np.float32)
        Q = y.shape[0]
        codes = self.eng.orc.query_codes(self.eng.hs, y)
        out = []
        for x in range(Q):
            ids = self.eng._row_ids(x, Q, codes, self.P1)
            ids = np.unique(ids[ids < self.n])
            if alias:
                ids = ids[ids != x]
            with np.errstate(over="ignore", invalid="ignore"):
                dfh, dfx = y[x][None, :] - self.hp[ids], y[x][None, :] - self.pts[ids]
                dh, dx = np_tree(dfh * dfh), np_tree(dfx * dfx)
            out.append((ids.astype(np.uint32), dh.reshape(-1), dx.reshape(-1)))
        return out

    def decide(self, cands, kp, E):
        return Decisions([decide(dh, dx, ids, self.k, kp, E) for ids, dh, dx in cands])


def trap_points(n, d, Q, seed, clusters=12, size=100, spread=3e-4, ladder=True):
    """iid N(0,1) rows with `clusters` clusters of `size` rows written over the first rows, cluster j in the rows j,
    j + clusters, ...: a centre plus noise of spread * 2^(j/2) (ladder: from well below binary16's resolution at
    magnitude 1 to well above it) or of `spread` throughout.  Two thirds of the queries sit at a centre plus noise of
    twice its cluster's spread, the rest are iid.  Rows of one cluster tie on the narrow copy, ties go to the lowest
    ids, and the true neighbours are elsewhere in the cluster.  The first Q rows make an aliased batch that covers
    every cluster."""
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.standard_normal((Q, d)).astype(np.float32)
    centres = rng.standard_normal((clusters, d)).astype(np.float32)
    s = (spread * 2.0 ** (np.arange(clusters) / 2.0 if ladder else np.zeros(clusters))).astype(np.float32)
    cj = np.arange(clusters * size) % clusters
    pts[:clusters * size] = centres[cj] + rng.standard_normal((clusters * size, d)).astype(np.float32) * s[cj, None]
    nq = 2 * Q // 3
    qj = np.arange(nq) % clusters
    y[:nq] = centres[qj] + rng.standard_normal((nq, d)).astype(np.float32) * (2 * s[qj, None])
    return np.ascontiguousarray(pts), np.ascontiguousarray(y), nq


_TRAPS = {}
# n = 3000, k = 10, T = 3, Q = 192 on the ladder: the seed per row length at which the model's certified counts at E,
# E / 2 and 2 E are three different numbers (d = 64: 147 / 152 / 143, d = 80: 153 / 155 / 152, d = 128: 161 / 162 / 158)
MAIN_SEED = {64: 2, 80: 1, 128: 1}


def trap_case(n, d, k, T, Q, seed=1, ladder=True, alias=False, kp=None, three_counts=False):
    """The trap data of one shape with its index (built by the oracle), its exact model and the model's decisions at
    the numpy E, checked: made once per shape and shared, everything in it read-only.  three_counts: the model's
    certified counts at E, E / 2 and 2 E must differ, so that a bound off by a factor of two shows in the count."""
    key = (n, d, k, T, Q, seed, ladder, alias)
    c = _TRAPS.get(key)
    if c is None:
        from types import SimpleNamespace
        from oracle import oracle_py as O
        pts, y, nq = trap_points(n, d, Q, seed, ladder=ladder)
        if alias:
            y, nq = pts[:Q], Q
        orc = O.CpuBackend("f32", "oracle")
        O.srandom(1000 + seed)
        _, _, sd = orc.precomp(pts, k, T)
        model = DeviceModel(sd, pts)
        for a in (pts, y):
            a.setflags(write=False)
        c = SimpleNamespace(orc=orc, pts=pts, y=y, sd=sd, model=model, k=k, Q=Q, nq=nq, alias=alias, d=d,
                            E=row_error(pts), cands=model.gather(y, alias), want=orc.query(sd, pts, Q if alias else y, alias=alias))
        for a in c.want:
            a.setflags(write=False)
        _TRAPS[key] = c
    what = "trap data n=%d d=%d k=%d Q=%d%s" % (n, d, k, Q, " aliased" if alias else "")
    kp = default_keys(k) if kp is None else kp
    dec = c.model.decide(c.cands, kp, c.E)
    dec.check(what)
    if three_counts:
        counts = [int(c.model.decide(c.cands, kp, e).certified.sum()) for e in (c.E, c.E / 2, 2 * c.E)]
        assert len(set(counts)) == 3, "%s: certified at E, E/2, 2E = %s" % (what, counts)
    return c, dec
