#!/usr/bin/env python3
"""tools/sorted_bench.py -- the sorted scan (annhip_query_sorted) against fixed mode's tagged query (annhip_query_tagged /
annhip_query_between, pair bits 0) and against the exact scan under the same predicate (annhip_index_exact_query_between),
on ONE index and the same batches, in the style of tools/tag_bench.py.

    python tools/sorted_bench.py [--points N] [--dim d] [--knn k] [--tries T] [--queries Q] [--rounds R] [--warmup W]
                                 [--tenants 10,100,1000,10000] [--exact-queries 1000] [--window-share 100]

Rows are iid N(0,1), generated on the device (tools/tag_bench.py's data).  Settings:
  tenants_S   for every S of --tenants the rows carry a tenant, uniform over S, as their tag word; every query asks for one
              random tenant (mask 0xFFFFFFFF, the pair form): a run of about N / S rows, shared by about Q / S queries
  windows     the tag word is a uniform 16-bit "day"; every query asks for its own window of 1 / --window-share of the
              days (the range form): overlapping runs, no two alike
For every setting, all of them alternated inside every round (the tags are set and sorted again outside the event
bracket), the median over R >= 7 rounds after W warm-up rounds of HIP events around one batch, one process:
  ann_ms      Index.query(y, where=...) at pair bits 0, Q queries
  sorted_ms   Index.query_sorted(y, where), Q queries
  exact_ms    Index.exact_query(y, where=...) on the first --exact-queries queries of the batch (the line says how many)
and, from one more pass: recall@k of the first two against the third on those queries (query_sorted's ids must EQUAL the
exact ones: asserted), the rows the sorted scan fetched per query and per (query, run row) (annhip_stats out[3] with
annhip_profile 1; 1.0 = no sharing), and the run lengths.  One JSON line per setting.

With --split S0,S1,... and / or --sets M0,M1,... the tool measures annhip_query_sorted_set (Index.query_sorted_set) instead,
on the same rows, with the same rounds and timing:
  one_tenant_qQ  Q in --set-queries (default 1,48,1000,10000) queries that all ask for tenant 0 of 10 (a run of about
                 N / 10 rows), and whole_index_q1: one query whose run is every row.  Per split S: set_S<S>_ms; S = 0 is
                 timed twice per round (set_S0_ms and again_S0_ms: the spread of one setting repeated); sorted_ms is
                 Index.query_sorted of the same build, exact_ms Index.exact_query(where=) on at most --exact-queries queries
  skew           10 000 queries over 1 000 tenants plus 48 queries on one tenant of N / 10 rows: the same columns
  sets_M         for every M of --sets, 10 000 queries that each ask for M distinct tenants of 1 000: the same split columns;
                 calls_merge_ms is M Index.query_sorted calls and a torch top-k of their concatenated rows (what a caller
                 does without the set call), exact_hull_ms Index.exact_query on --exact-queries queries under the hull
                 interval [min, max] of the set, recall_ann_hull the recall@k of Index.query(where=hull) against the set's
                 exact rows
The ids of every split must equal those of S = 0, and those of query_sorted where the sets are single intervals:
asserted, as is the equality of the set call's ids with exact_query's per tenant of the set, merged.  entries_S<S> is the
call's entry count; rows_differing_from_calls_merge counts the queries for which the torch merge of the separate calls
names other ids."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", dest="n", type=int, default=4_000_000)
    ap.add_argument("--dim", dest="d", type=int, default=128)
    ap.add_argument("--knn", dest="k", type=int, default=10)
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--queries", dest="q", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--tenants", default="10,100,1000,10000")
    ap.add_argument("--exact-queries", dest="xq", type=int, default=1000)
    ap.add_argument("--window-share", dest="share", type=int, default=100)
    ap.add_argument("--split", default=None, help="query_sorted_set: the split_rows values to time, e.g. 0,4096,16384")
    ap.add_argument("--sets", default=None, help="query_sorted_set: set sizes (tenants per query) to time, e.g. 3,10")
    ap.add_argument("--set-queries", dest="setq", default="1,48,1000,10000")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7 (the median is taken over them)")
    if args.split is not None or args.sets is not None:
        return set_bench(args)

    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T, Q = args.n, args.d, args.k, args.tries, args.q
    XQ = min(args.xq, Q)
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    tenants = [int(tok) for tok in args.tenants.split(",")]
    nbatch = 3
    with park_random():
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        points = torch.randn((n, d), device=dev, generator=gen)
        batches = [torch.randn((Q, d), device=dev, generator=gen) for _ in range(nbatch)]
        full = torch.full((Q,), -1, dtype=torch.int32, device=dev)  # mask 0xFFFFFFFF
        settings = []  # (name, tags, where, selectivity)
        for S in tenants:
            tg = torch.randint(0, S, (n,), device=dev, generator=gen, dtype=torch.int32)
            settings.append(("tenants_%d" % S, tg, (full, torch.randint(0, S, (Q,), device=dev, generator=gen, dtype=torch.int32)), S))
        day = torch.randint(0, 1 << 16, (n,), device=dev, generator=gen, dtype=torch.int32)
        width = max(1, (1 << 16) // args.share)
        lo = torch.randint(0, (1 << 16) - width + 1, (Q,), device=dev, generator=gen, dtype=torch.int32)
        settings.append(("windows", day, (full, lo, lo + (width - 1)), args.share))
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ix.set_fixed(True)
    ix.set_probe(0)

    def apply(tg):  # synchronous, outside the event bracket
        ix.set_tags(tg)
        ix.sort_tags()

    def sub(where):
        return tuple(w[:XQ].contiguous() for w in where)

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        torch.cuda.synchronize()
        ev0.record()
        f()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    times = {s[0]: {"ann": [], "sorted": [], "exact": []} for s in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        yx = y[:XQ].contiguous()
        for name, tg, where, _ in settings:
            apply(tg)
            ms = {"ann": timed(lambda: ix.query(y, where=where)),
                  "sorted": timed(lambda: ix.query_sorted(y, where)),
                  "exact": timed(lambda: ix.exact_query(yx, where=sub(where)))}
            if r >= args.warmup:
                for key, v in ms.items():
                    times[name][key].append(v)
        print("round %d of %d done" % (r + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)

    def med(v):
        v = sorted(v)
        return round(v[len(v) // 2], 4), [round(v[0], 4), round(v[-1], 4)]

    y = batches[0]
    yx = y[:XQ].contiguous()
    for name, tg, where, S in settings:
        apply(tg)
        truth = ix.exact_query(yx, where=sub(where))[0]
        ann = ix.query(y, where=where)[0][:XQ]
        ix.profile(1)
        ix.stats(reset=True)
        got = ix.query_sorted(y, where)[0]
        torch.cuda.synchronize()
        fetched = ix.stats(reset=True)["other_rows"]
        ix.profile(0)
        assert torch.equal(got[:XQ], truth), "%s: query_sorted's ids differ from exact_query's" % name
        length = (ix.tag_runs(where)[1].to(torch.int64) & 0xFFFFFFFF).double()
        out = {"workload": "N=%d d=%d k=%d tries=%d Q=%d float, iid data seed %d, d_short %d" % (n, d, k, T, Q, args.seed, ix.d_short),
               "setting": name, "selectivity_1_in": S, "rounds": args.rounds, "exact_queries": XQ,
               "run_rows_mean": round(length.mean().item(), 1), "run_rows_max": int(length.max().item()),
               "recall_ann": round(A.recall_at_k(ann, truth), 4), "recall_sorted": round(A.recall_at_k(got[:XQ], truth), 4),
               "ids_equal_exact": True,
               "rows_fetched_per_query": round(fetched / Q, 1),
               "rows_fetched_per_query_run_row": round(fetched / max(length.sum().item(), 1.0), 4)}
        for key in ("ann", "sorted", "exact"):
            out[key + "_ms"], out[key + "_ms_min_max"] = med(times[name][key])
        out["exact_ms_scaled_to_Q"] = round(out["exact_ms"] * Q / XQ, 2)  # an extrapolation, not a measurement
        print(json.dumps(out), flush=True)
    ix.close()


def set_bench(args):
    """the --split / --sets mode: see the module's docstring"""
    import numpy as np
    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T = args.n, args.d, args.k, args.tries
    splits = sorted({0} | {int(t) for t in (args.split or "0").split(",")})
    msets = [int(t) for t in args.sets.split(",")] if args.sets else []
    qs = [int(t) for t in args.setq.split(",")]
    QB, BIG = 10_000, 48  # the large batch; the queries on the big tenant of the skewed setting
    Qmax = max(qs + [QB + BIG])
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    FULL = 0xFFFFFFFF
    nbatch = 3
    rng = np.random.default_rng(args.seed)
    with park_random():
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        points = torch.randn((n, d), device=dev, generator=gen)
        batches = [torch.randn((Qmax, d), device=dev, generator=gen) for _ in range(nbatch)]
        tags10 = torch.randint(0, 10, (n,), device=dev, generator=gen, dtype=torch.int32)
        tags1000 = torch.randint(0, 1000, (n,), device=dev, generator=gen, dtype=torch.int32)
        skewed = tags1000.clone()
        skewed[: n // 10] = 1000  # the rows are iid: any n / 10 of them serve as the big tenant
        torch.cuda.synchronize()

    def csr(sets):
        m, off, lo, hi = A.where_in(FULL, sets)
        return (m, off, torch.from_numpy(lo.view(np.int32)).to(dev), torch.from_numpy(hi.view(np.int32)).to(dev))

    def triple(lo, hi):
        Q = len(lo)
        return (torch.full((Q,), -1, dtype=torch.int32, device=dev), torch.from_numpy(np.asarray(lo, dtype=np.uint32).view(np.int32)).to(dev),
                torch.from_numpy(np.asarray(hi, dtype=np.uint32).view(np.int32)).to(dev))

    settings = []  # name, tags, Q, set where, the same as one interval per query (or None), hull, the values per query (or None)
    for Q in qs:
        settings.append(("one_tenant_q%d" % Q, tags10, Q, csr([[0]] * Q), triple([0] * Q, [0] * Q), None))
    settings.append(("whole_index_q1", tags10, 1, csr([[(0, FULL)]]), triple([0], [FULL]), None))
    tq = rng.integers(0, 1000, size=QB).tolist() + [1000] * BIG
    settings.append(("skew", skewed, QB + BIG, csr([[t] for t in tq]), triple(tq, tq), None))
    for M in msets:
        vals = [sorted(rng.choice(1000, size=M, replace=False).tolist()) for _ in range(QB)]
        settings.append(("sets_%d" % M, tags1000, QB, csr(vals), triple([v[0] for v in vals], [v[-1] for v in vals]), vals))

    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ix.set_fixed(True)
    ix.set_probe(0)
    current = [None]

    def apply(tg):  # synchronous, outside the event bracket
        if current[0] is not tg:
            ix.set_tags(tg)
            ix.sort_tags()
            current[0] = tg

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        torch.cuda.synchronize()
        ev0.record()
        f()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    def calls_merge(y, vals):
        M = len(vals[0])
        full = torch.full((len(vals),), -1, dtype=torch.int32, device=dev)
        cols = torch.tensor(vals, dtype=torch.int32, device=dev)
        parts = [ix.query_sorted(y, (full, cols[:, j].contiguous())) for j in range(M)]
        dd, at = torch.cat([p[1] for p in parts], dim=1).topk(k, dim=1, largest=False)
        return torch.cat([p[0] for p in parts], dim=1).gather(1, at), dd

    times = {s[0]: {} for s in settings}
    for r in range(args.warmup + args.rounds):
        for name, tg, Q, where, one, vals in settings:
            apply(tg)
            y = batches[r % nbatch][:Q].contiguous()
            XQ = min(args.xq, Q)
            yx, hull = y[:XQ].contiguous(), tuple(w[:XQ].contiguous() for w in one)
            ms = {}
            for S in splits:
                ms["set_S%d" % S] = timed(lambda: ix.query_sorted_set(y, where, split=S))
            ms["again_S0"] = timed(lambda: ix.query_sorted_set(y, where, split=0))
            if vals is None:
                ms["sorted"] = timed(lambda: ix.query_sorted(y, one))
                ms["exact"] = timed(lambda: ix.exact_query(yx, where=hull))
            else:
                ms["calls_merge"] = timed(lambda: calls_merge(y, vals))
                ms["exact_hull"] = timed(lambda: ix.exact_query(yx, where=hull))
            if r >= args.warmup:
                for key, v in ms.items():
                    times[name].setdefault(key, []).append(v)
        print("round %d of %d done" % (r + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)

    def med(v):
        v = sorted(v)
        return round(v[len(v) // 2], 4), [round(v[0], 4), round(v[-1], 4)]

    for name, tg, Q, where, one, vals in settings:
        apply(tg)
        y = batches[0][:Q].contiguous()
        XQ = min(args.xq, Q)
        base = ix.query_sorted_set(y, where, split=0)
        out = {"workload": "N=%d d=%d k=%d tries=%d Q=%d float, iid data seed %d, d_short %d" % (n, d, k, T, Q, args.seed, ix.d_short),
               "setting": name, "rounds": args.rounds, "exact_queries": XQ, "entries_S0": int(base[2])}
        for S in splits[1:]:
            got = ix.query_sorted_set(y, where, split=S)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), "%s: split %d changes the answer" % (name, S)
            out["entries_S%d" % S] = int(got[2])
        length = (ix.tag_runs_set(where)[1].to(torch.int64) & 0xFFFFFFFF).double()
        out["run_rows_per_query"] = round(length.sum().item() / Q, 1)
        if vals is None:
            assert torch.equal(ix.query_sorted(y, one)[0], base[0]), "%s: query_sorted's ids differ" % name
            out["ids_equal_query_sorted"] = True
        else:
            # the truth for the first XQ queries: exact_query under each tenant of the set, merged as the calls are
            full = torch.full((XQ,), -1, dtype=torch.int32, device=dev)
            cols = torch.tensor(vals[:XQ], dtype=torch.int32, device=dev)
            ex = [ix.exact_query(y[:XQ].contiguous(), where=(full, cols[:, j].contiguous())) for j in range(cols.shape[1])]
            at = torch.cat([p[1] for p in ex], dim=1).topk(k, dim=1, largest=False)[1]
            truth = torch.cat([p[0] for p in ex], dim=1).gather(1, at)
            assert torch.equal(base[0][:XQ], truth), "%s: the set call's ids differ from the merged exact scans'" % name
            out["ids_equal_exact_per_tenant"] = True
            out["rows_differing_from_calls_merge"] = int((calls_merge(y, vals)[0] != base[0]).any(dim=1).sum().item())
            ann = ix.query(y, where=one)[0][:XQ]
            out["recall_ann_hull"] = round(A.recall_at_k(ann, base[0][:XQ]), 4)
        for key, v in times[name].items():
            out[key + "_ms"], out[key + "_ms_min_max"] = med(v)
        print(json.dumps(out), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
