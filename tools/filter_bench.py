#!/usr/bin/env python3
"""tools/filter_bench.py -- the allow-list row filter of fixed mode (annhip_index_set_filter) on ONE index and the same
batches.

    python tools/filter_bench.py [--data iid|clustered] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                                 [--rounds R] [--warmup W] [--recall-queries S] [--bits 0,8] [--shares 0.5,0.1,0.01]

The data sets are tools/probe_bench.py's (iid N(0,1) rows; a mixture of Gaussians), generated on the device.  For every
pair-bit setting b the filter settings are: none (twice per round: "none" and "none_again", whose spread is the noise floor
-- both run the unfiltered kernels), the all-ones filter, and a random allow list for every share.  b = 1 without a filter
is added to the b = 0 group: it runs the probe-shaped kernel on b = 0's candidate sets, which separates the kernel shape
from the filter.  For every setting:
  * ms per step: HIP events around one batch, all settings alternated inside every round, median over R >= 7 rounds after
    W warm-up rounds, one process;
  * the stage-1 kernel alone (annhip_profile 2: one event pair), in a separate pass;
  * rows gathered per query (annhip_stats, annhip_profile 1) and the stage-1 kernel's algorithmic bytes per second
    (gathered rows + the candidate ids read + one bitmap word per candidate id + one segment word per probed bucket + the
    query's row, codes, ranked bits and result keys);
  * recall@k against Index.exact_query under the SAME filter on the first S queries of the first batch.
One JSON line per setting.
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--bits", default="0,8")
    ap.add_argument("--shares", default="0.5,0.1,0.01")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7 (the median is taken over them)")

    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T, Q = args.n, args.d, args.k, args.tries, args.q
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    with park_random():
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        nbatch = 3
        if args.data == "iid":
            points = torch.randn((n, d), device=dev, generator=gen)
            batches = [torch.randn((Q, d), device=dev, generator=gen) for _ in range(nbatch)]
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
            batches = [draw(Q) for _ in range(nbatch)]
        masks = {"ones": torch.ones(n, dtype=torch.bool, device=dev)}
        for tok in args.shares.split(","):
            masks["share_" + tok] = torch.rand(n, device=dev, generator=gen) < float(tok)
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ds = ix.d_short
    settings = []  # (name, pair bits, mask name or None)
    for tok in args.bits.split(","):
        b = min(int(tok), ds)
        settings.append(("b%d_none" % b, b, None))
        if b == 0:
            settings.append(("b1_none", 1, None))  # the probe-shaped kernel on b = 0's candidate sets, no filter
        settings += [("b%d_%s" % (b, m), b, m) for m in masks]
        settings.append(("b%d_none_again" % b, b, None))
    ix.set_fixed(True)

    def apply(b, m):
        ix.set_probe(b)
        ix.set_filter(None if m is None else masks[m])

    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _, _ in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        for name, b, m in settings:
            apply(b, m)  # (synchronous, outside the event bracket)
            ev0.record()
            ix.query(y, out_ids=out_i, out_dists=out_d)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[name].append(ev0.elapsed_time(ev1))

    S = min(args.recall_queries, Q)
    ys = batches[0][:S].contiguous()
    for name, b, m in settings:
        apply(b, m)
        truth, _ = ix.exact_query(ys)  # honours the filter: the exact neighbours among the allowed rows
        ix.profile(2)  # the stage-1 event pair only
        ix.stats(reset=True)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d)
        torch.cuda.synchronize()
        st = ix.stats(reset=True)
        s1_ms = st["s1_ms"] / max(st["s1_launches"], 1.0)
        ix.profile(1)  # row statistics (separate pass)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d)
        torch.cuda.synchronize()
        st1 = ix.stats(reset=True)
        ix.profile(0)
        rows_q = st1["s1_rows"] / max(st1["queries"], 1.0)
        buckets = 1 + ds + b * (b - 1) // 2
        share = 1.0 if m is None else ix.filter_count / n
        ids_q = rows_q / share if share > 0 else 0.0  # candidate ids read = gathered rows / allowed share (random masks)
        bytes_q = rows_q * d * 4 + ids_q * (4 + (4 if m is not None else 0)) + T * buckets * 8 + d * 4 + T * 4 + T * b + (k + 1) * 8
        ids = ix.query(ys)[0]
        torch.cuda.synchronize()
        t = sorted(times[name])
        print(json.dumps({
            "workload": "N=%d d=%d k=%d tries=%d Q=%d float, %s data seed %d, d_short %d" % (n, d, k, T, Q, args.data, args.seed, ds),
            "setting": name, "pair_bits": b, "filter": m, "allowed_rows": ix.filter_count, "buckets_per_try": buckets,
            "ms_per_step": round(t[len(t) // 2], 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
            "stage1_ms": round(s1_ms, 4),
            "rows_gathered_per_query": round(rows_q, 1), "algorithmic_bytes_per_query": int(bytes_q),
            "stage1_TBps": round(bytes_q * Q / (s1_ms * 1e-3) / 1e12, 3) if s1_ms > 0 else None,
            "recall_at_k": round(A.recall_at_k(ids, truth), 4), "recall_queries": S}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
