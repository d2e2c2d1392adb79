#!/usr/bin/env python3
"""tools/probe_bench.py -- the recall knob of fixed mode (annhip_index_set_probe) on ONE index and the same batches.

    python tools/probe_bench.py [--data iid|clustered] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                                [--rounds R] [--warmup W] [--recall-queries S] [--bits 0,4,8,12,all]

Both data sets are generated on the device: iid N(0,1) rows (the benchmark's; a sign hash is nearly blind there) and a
mixture of Gaussians (C centres drawn N(0,1), rows and queries = a random centre + sigma * N(0,1)).  For every setting:
  * ms per step: HIP events around one batch, the settings alternated inside every round, median over R >= 7 rounds after
    W warm-up rounds, one process;
  * the stage-1 kernel alone (annhip_profile 2: one event pair) and the hash kernel alone (annhip_profile 1 stage marks),
    in separate passes;
  * rows gathered per query (annhip_stats, annhip_profile 1) and the stage-1 kernel's algorithmic bytes per second
    (gathered rows + their ids + one segment word per probed bucket + the query's row, codes, ranked bits and result keys);
  * recall@k against Index.exact_query on the first S queries of the first batch.
b = 0 runs the plain fixed-mode kernels; it is listed twice per round ("0" and "0_again") -- the spread between the two
is the noise floor the other settings are read against.  One JSON line per setting.
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
    ap.add_argument("--points", dest="n", type=int, default=10_000_000)
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
    ap.add_argument("--bits", default="0,4,8,12,all")
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
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ds = ix.d_short
    settings = []
    for tok in args.bits.split(","):
        b = ds if tok == "all" else int(tok)
        if b <= ds and b not in [s[1] for s in settings]:
            settings.append((tok, b))
    settings.append(("0_again", 0))
    ix.set_fixed(True)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        for name, b in settings:
            ix.set_probe(b)
            ev0.record()
            ix.query(y, out_ids=out_i, out_dists=out_d)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[name].append(ev0.elapsed_time(ev1))

    S = min(args.recall_queries, Q)
    ys = batches[0][:S].contiguous()
    truth, _ = ix.exact_query(ys)
    torch.cuda.synchronize()
    for name, b in settings:
        ix.set_probe(b)
        ix.profile(2)  # the stage-1 event pair only
        ix.stats(reset=True)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d)
        torch.cuda.synchronize()
        st = ix.stats(reset=True)
        s1_ms = st["s1_ms"] / max(st["s1_launches"], 1.0)
        ix.profile(1)  # row statistics and stage marks (separate pass)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d)
        torch.cuda.synchronize()
        hash_us = ix.stage_ms()["codes"] * 1e3 / nbatch
        st1 = ix.stats(reset=True)
        ix.profile(0)
        rows_q = st1["s1_rows"] / max(st1["queries"], 1.0)
        buckets = 1 + ds + b * (b - 1) // 2
        bytes_q = rows_q * (d * 4 + 4) + T * buckets * 8 + d * 4 + T * 4 + T * b + (k + 1) * 8
        ids = ix.query(ys)[0]
        torch.cuda.synchronize()
        t = sorted(times[name])
        print(json.dumps({
            "workload": "N=%d d=%d k=%d tries=%d Q=%d float, %s data seed %d, d_short %d" % (n, d, k, T, Q, args.data, args.seed, ds),
            "setting": name, "pair_bits": b, "buckets_per_try": buckets,
            "ms_per_step": round(t[len(t) // 2], 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
            "stage1_ms": round(s1_ms, 4), "hash_us": round(hash_us, 1),
            "rows_gathered_per_query": round(rows_q, 1), "algorithmic_bytes_per_query": int(bytes_q),
            "stage1_TBps": round(bytes_q * Q / (s1_ms * 1e-3) / 1e12, 3) if s1_ms > 0 else None,
            "recall_at_k": round(A.recall_at_k(ids, truth), 4), "recall_queries": S}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
