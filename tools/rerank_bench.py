#!/usr/bin/env python3
"""tools/rerank_bench.py -- what re-scoring candidates on the native rows (annhip_index_rerank) costs and buys, on ONE index
and the same batches.

    python tools/rerank_bench.py [--data iid|clustered|offset] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                                 [--rounds R] [--warmup W] [--cands 10,32,100,1024]

The method of tools/topk_bench.py: one process, the settings alternated inside every round, HIP events around one step,
median over R >= 7 rounds after W warm-up rounds.  Float, fixed mode.  Data, generated on the device: iid N(0,1) rows;
tools/tail_bench.py's clustered rows (--centres, --sigma); "offset" rows 1000 + 1e-3 N(0,1), where rounding to binary16
moves every neighbour.  Settings:
  native              query(k) on the native rows: the yardstick, same build, same process
  f16                 query(k) on the binary16 rows (set_rows("f16"))
  f16+rerank          that, then rerank of its k ids on the native rows (in place)
  f16_reranked_x2/x3  query_reranked(k, oversample=2 / 3) on the binary16 rows
  rerank_C=<C>        the rerank kernel alone, k = the index's k, on C uniformly random ids per query: the gather's worst
                      case (a row is read once per (query, candidate) and nothing is near anything).  annhip_index_rerank is
                      called directly on preallocated tensors, --launches times between the two events (the batches in
                      turn), and the interval is divided by that count: one launch at C = 10 is shorter than the host
                      takes to enqueue it
Per setting, one JSON line: ms per step with min .. max; recall@k against Index.exact_query on the first batch; of the
returned ids that are true neighbours, the share whose distance is bit for bit the native-row distance exact_query
reports; for the kernel alone, candidate rows per second, algorithmic bytes per second (row bytes plus the 8-byte ids) and
that rate as a fraction of --ceiling-gbs, the random 512-byte-row gather ceiling of tools/readbw.hip with cached loads
(profiles/r03_readbw_ceilings.log: 6.29 .. 6.30 TB/s), which is what the kernel's loads are.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", choices=["iid", "clustered", "offset"], default="iid")
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
    ap.add_argument("--cands", default="10,32,100,1024")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--ceiling-gbs", dest="ceiling", type=float, default=6300.0)
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7 (the median is taken over them)")

    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T, Q = args.n, args.d, args.k, args.tries, args.q
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    nbatch = 3
    with park_random():
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        if args.data == "clustered":
            cen = torch.randn((args.centres, d), device=dev, generator=gen)

            def draw(m):
                out = torch.randn((m, d), device=dev, generator=gen).mul_(args.sigma)
                step = 1 << 20
                for a in range(0, m, step):  # centre rows added piecewise: no second [m, d] temporary
                    pick = torch.randint(0, args.centres, (min(step, m - a),), device=dev, generator=gen)
                    out[a:a + step] += cen[pick]
                return out
        elif args.data == "offset":
            def draw(m):
                return torch.randn((m, d), device=dev, generator=gen).mul_(1e-3).add_(1000.0)
        else:
            def draw(m):
                return torch.randn((m, d), device=dev, generator=gen)
        points = draw(n)
        batches = [draw(Q) for _ in range(nbatch)]
        cands = {}
        for tok in args.cands.split(","):
            C = int(tok)
            if 1 <= C <= 1024:
                cands[C] = [torch.randint(0, n, (Q, C), device=dev, generator=gen) for _ in range(nbatch)]
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ix.set_fixed(True)
    kmax = ix.max_query_k
    oi = torch.empty((Q, k), dtype=torch.int64, device=dev)
    od = torch.empty((Q, k), dtype=torch.float32, device=dev)

    def native(b):
        return ix.query(batches[b], out_ids=oi, out_dists=od, k=k)[:2]

    def f16(b):
        return ix.query(batches[b], out_ids=oi, out_dists=od, k=k)[:2]

    def f16_rerank(b):
        ix.query(batches[b], out_ids=oi, out_dists=od, k=k)
        return ix.rerank(batches[b], oi, k, out_ids=oi, out_dists=od)

    def reranked(os_):
        return lambda b: ix.query_reranked(batches[b], k, oversample=os_)

    def alone(C):
        def step(b):
            for i in range(args.launches):
                bb = (b + i) % nbatch
                ix.lib.annhip_index_rerank(ix.h, None, Q, batches[bb].data_ptr(), C, cands[C][bb].data_ptr(), k, oi.data_ptr(),
                                           od.data_ptr())
            return oi, od
        return step

    # (name, rows the index is set to, step, candidates per query of the kernel alone)
    settings = [("native", "native", native, 0), ("f16", "f16", f16, 0), ("f16+rerank", "f16", f16_rerank, 0),
                ("f16_reranked_x2", "f16", reranked(2), 0), ("f16_reranked_x3", "f16", reranked(3), 0)]
    settings += [("rerank_C=%d" % C, "native", alone(C), C) for C in sorted(cands)]

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {s[0]: [] for s in settings}
    for r in range(args.warmup + args.rounds):
        b = r % nbatch
        for name, rows, step, _ in settings:
            ix.set_rows(rows)  # outside the timed region; the narrow copy is made once and kept
            torch.cuda.synchronize()
            ev0.record()
            step(b)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[name].append(ev0.elapsed_time(ev1))

    ix.set_rows("native")
    truth_i, truth_d = ix.exact_query(batches[0], k=k)
    for name, rows, step, C in settings:
        ix.set_rows(rows)
        gi, gd = step(0)
        torch.cuda.synchronize()
        t = sorted(times[name])
        per = args.launches if C else 1  # launches between the two events
        t = [v / per for v in t]
        ms = t[len(t) // 2]
        line = {"workload": "N=%d d=%d k=%d tries=%d Q=%d float, %s data seed %d, fixed mode, max_query_k %d"
                            % (n, d, k, T, Q, args.data, args.seed, kmax),
                "setting": name, "rows": rows, "ms_per_step": round(ms, 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)],
                "rounds": len(t)}
        if C:
            line["candidates_per_query"] = C
            line["rows_per_s"] = round(Q * C / (ms * 1e-3), 1)
            line["launches_per_interval"] = per
            line["algorithmic_GB_per_s"] = round(Q * C * (d * 4 + 8) / (ms * 1e-3) / 1e9, 1)
            line["fraction_of_gather_ceiling"] = round(line["algorithmic_GB_per_s"] / args.ceiling, 3)
            line["gather_ceiling_GB_per_s"] = args.ceiling
        else:
            hit = gi.unsqueeze(2) == truth_i.unsqueeze(1)  # [Q, k guess, k truth]
            same = hit & (gd.view(torch.int32).unsqueeze(2) == truth_d.view(torch.int32).unsqueeze(1))
            line["recall_at_k"] = round(A.recall_at_k(gi, truth_i), 5)
            line["hits_with_native_distance_bits"] = round(same.sum().item() / max(hit.sum().item(), 1), 5)
        print(json.dumps(line), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
