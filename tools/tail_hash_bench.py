#!/usr/bin/env python3
"""tools/tail_hash_bench.py -- what annhip_index_hash_tail buys a fixed-mode step: appended rows looked up by hash code
against the same rows scanned exactly, on twin indexes and the same batches.

    python tools/tail_hash_bench.py [--data iid|clustered] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                                    [--rounds R] [--warmup W] [--tails 0,10000,100000,400000,1000000]
                                    [--exact-max M] [--recall-queries 1000]

The method of tools/tail_bench.py: one process, the settings alternated inside every round, HIP events around one batch,
median over R >= 7 rounds after W warm-up rounds.  The settings are twin indexes built from the same rows and the same
random() seed: per tail length m one with the exact tail ("exact") and one after hash_tail() ("hashed"), plus a second
tail-free index ("0_again": the spread of the two tail-free readings is the noise floor).  --exact-max: tail lengths
beyond it are not timed with the exact tail (reported as skipped).  Per (m, setting) one JSON line:
  * ms per step, with min and max over the rounds;
  * the tail launches' own time (annhip_profile 1 stage marks, slot "stage2_network", in a separate pass);
  * tail rows scored per query (annhip_stats, the rows-kernel counter: with and without the tail, the difference);
  * the time of hash_tail() itself (host clock around the synchronous call);
  * recall@k against Index.exact_query on --recall-queries queries of the first batch, split by where the TRUE neighbour
    lives: ids below n (the built rows' recall: the reference) and ids in the tail.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", choices=["iid", "clustered"], default="iid")
    ap.add_argument("--points", dest="n", type=int, default=4_000_000)
    ap.add_argument("--dim", dest="d", type=int, default=128)
    ap.add_argument("--knn", dest="k", type=int, default=10)
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--queries", dest="q", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.35)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--tails", default="0,10000,100000,400000,1000000")
    ap.add_argument("--exact-max", type=int, default=1_000_000)
    ap.add_argument("--recall-queries", type=int, default=1000)
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7 (the median is taken over them)")

    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T, Q = args.n, args.d, args.k, args.tries, args.q
    tails = sorted({int(t) for t in args.tails.split(",")} | {0})
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    with park_random():
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        nbatch = 3
        if args.data == "iid":
            def draw(m):
                return torch.randn((m, d), device=dev, generator=gen)
        else:
            cen = torch.randn((args.centres, d), device=dev, generator=gen)

            def draw(m):
                out = torch.randn((m, d), device=dev, generator=gen).mul_(args.sigma)
                step = 1 << 20
                for a in range(0, m, step):  # centre rows added piecewise: no second [m, d] temporary
                    pick = torch.randint(0, args.centres, (min(step, m - a),), device=dev, generator=gen)
                    out[a:a + step] += cen[pick]
                return out
        points = draw(n)
        pool = draw(max(tails))  # the appended rows: from the distribution of the built ones
        batches = [draw(Q) for _ in range(nbatch)]
        torch.cuda.synchronize()

    settings = []  # (m, setting, index, hash_tail seconds): the indexes share the point rows
    plan = [(0, "exact")] + [(m, s) for m in tails if m for s in ("exact", "hashed")] + [(0, "0_again")]
    skipped = []
    for m, setting in plan:
        if setting == "exact" and m > args.exact_max:
            skipped.append(m)
            continue
        libc.srandom(args.seed)
        ix = A.Index.precomp(points, k, T)
        ix.set_fixed(True)
        hash_s = None
        if m:
            ix.reserve_tail(m)
            ix.append(pool[:m])
        if setting == "hashed":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.hash_tail()
            hash_s = time.perf_counter() - t0
            assert ix.tail_hashed == m
        settings.append((m, setting, ix, hash_s))
    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(m, s): [] for m, s, _, _ in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        for m, s, ix, _ in settings:
            ev0.record()
            ix.query(y, out_ids=out_i, out_dists=out_d)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[(m, s)].append(ev0.elapsed_time(ev1))

    def med(v):
        v = sorted(v)
        return v[len(v) // 2] if v else None

    def profiled(ix):
        """(tail launches' ms per step, rows scored by the rows kernels per query) over the batches"""
        ix.profile(1)
        ix.stats(reset=True)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d)
        torch.cuda.synchronize()
        st = ix.stats()
        ms = ix.stage_ms()["stage2_network"] / nbatch
        ix.profile(0)
        return ms, st

    rq = min(args.recall_queries, Q)
    yr = batches[0][:rq].contiguous()
    base_rows = None
    rows = []
    for m, s, ix, hash_s in settings:
        tail_ms, st = profiled(ix)
        scored = st["other_rows"]  # annhip_stats out[3]: the rows kernels of stage 2 and both tail launches
        if m == 0 and base_rows is None:
            base_rows = scored
        per_q = (scored - base_rows) / (nbatch * Q)  # twins: stage 2 scores the same rows on every index
        truth = ix.exact_query(yr)[0]
        got = ix.query(yr)[0]
        found = (got[:, :, None] == truth[:, None, :]).any(dim=1)  # [rq, k]: truth j of query x was returned
        built, tail = truth < n, truth >= n
        t = sorted(times[(m, s)])
        row = {
            "workload": "N=%d d=%d k=%d tries=%d Q=%d float, %s data seed %d" % (n, d, k, T, Q, args.data, args.seed),
            "tail_rows": m, "setting": s,
            "ms_per_step": round(med(t), 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
            "tail_launches_ms": round(tail_ms, 4) if m else 0.0,
            "tail_rows_scored_per_query": round(per_q, 1),
            "hash_tail_s": None if hash_s is None else round(hash_s, 4),
            "recall_queries": rq,
            "truth_in_built": int(built.sum()), "recall_built": round(float(found[built].float().mean()), 4) if built.any() else None,
            "truth_in_tail": int(tail.sum()), "recall_tail": round(float(found[tail].float().mean()), 4) if tail.any() else None}
        rows.append(row)
        print(json.dumps(row), flush=True)
    zero = [r["ms_per_step"] for r in rows if r["tail_rows"] == 0]
    print(json.dumps({"summary": "hashed against exact tail", "index_step_ms": zero[0],
                      "tail_free_spread_ms": round(abs(zero[-1] - zero[0]), 4), "exact_tail_not_timed_at": skipped,
                      "ms_per_step": {str(m): {r["setting"]: r["ms_per_step"] for r in rows if r["tail_rows"] == m}
                                      for m in tails if m}}), flush=True)
    for _, _, ix, _ in settings:
        ix.close()


if __name__ == "__main__":
    main()
