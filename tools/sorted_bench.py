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
annhip_profile 1; 1.0 = no sharing), and the run lengths.  One JSON line per setting."""
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
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7 (the median is taken over them)")

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


if __name__ == "__main__":
    main()
