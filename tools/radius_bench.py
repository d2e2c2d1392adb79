#!/usr/bin/env python3
"""tools/radius_bench.py -- radius queries of fixed mode (annhip_query_radius) against what a caller could do before:
annhip_query_k with a large k, then annhip_radius_trim.  ONE index, the same batches.

    python tools/radius_bench.py [--data iid|clustered] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                                 [--rounds R] [--warmup W] [--kcap 32,100,256] [--recall-queries 1000]

iid N(0,1) rows, or the mixture of Gaussians of tools/probe_bench.py (C centres drawn N(0,1), rows and queries = a random
centre + sigma * N(0,1)); recall means something only on the mixture.  The radii r1, r10, r50 are the medians, over the
recall queries, of the exact 1st, 10th and 50th neighbour distance (exact_query(k=50)).  Settings: the plain call ("plain"
and "plain_again", timed first and last: the drift yardstick); "k+trim kcap=<c>": query(k=c) followed by the trim, at the
largest radius (its cost does not depend on the radius); "radius kcap=<c> r<j>": query_radius(k=c) at each radius.
For every setting:
  * ms per step: HIP events around one batch, the settings alternated inside every round, median and min..max over R >= 7
    rounds after W warm-up rounds, one process;
  * stage-1 and stage-2 ms per step and the rows gathered per query (annhip_profile 1: stage marks and row counters), in a
    separate pass over the same batches; the trim is not in either figure (the radius call launches it behind stage 2, in
    the segment of the tail merges; the baseline's runs after the call);
  * mean count, the share of queries with count == kcap, and radius_recall against exact_query_radius on the recall
    queries; beside them the plain call's recall@k from the same run.
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
    ap.add_argument("--kcap", default="32,100,256")
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
    ix.set_fixed(True)
    lib, kmax = ix.lib, ix.max_query_k
    RQ = min(args.recall_queries, Q)
    yr = batches[0][:RQ].contiguous()
    ex50 = ix.exact_query(yr, k=50)[1]
    radii = {"r%d" % j: float(ex50[:, j - 1].median().item()) for j in (1, 10, 50)}
    truth_k = ix.exact_query(yr)[0]
    plain_recall = A.recall_at_k(ix.query(yr)[0], truth_k)

    kcaps = [c for c in (int(t) for t in args.kcap.split(",")) if 1 <= c <= kmax]
    settings = [("plain", None, None, None)]  # (name, kind, kcap, radius name)
    for c in kcaps:
        settings.append(("k+trim kcap=%d" % c, "trim", c, "r50"))
        for rn in radii:
            settings.append(("radius kcap=%d %s" % (c, rn), "radius", c, rn))
    settings.append(("plain_again", None, None, None))
    outs = {c: (torch.empty((Q, c), dtype=torch.int64, device=dev), torch.empty((Q, c), dtype=torch.float32, device=dev))
            for c in kcaps + [k]}
    counts = torch.zeros((Q,), dtype=torch.int32, device=dev)
    rads = {rn: torch.full((Q,), r, dtype=torch.float32, device=dev) for rn, r in radii.items()}
    torch.cuda.synchronize()  # (every call below runs on the null stream, as the events do)

    def step(y, kind, c, rn):
        """One step of a setting: raw library calls on the null stream in every setting, so that the host gaps between
        launches, which the events include, are the same on both sides of a comparison."""
        if kind is None:
            lib.annhip_query(ix.h, Q, y.data_ptr(), 0, 0, outs[k][0].data_ptr(), outs[k][1].data_ptr())
            return
        oi, od = outs[c]
        if kind == "trim":
            assert lib.annhip_query_k(ix.h, None, None, Q, y.data_ptr(), 0, c, None, None, oi.data_ptr(), od.data_ptr()) == 0
            assert lib.annhip_radius_trim(Q, c, n, rads[rn].data_ptr(), oi.data_ptr(), od.data_ptr(), counts.data_ptr(), None) == 0
        else:
            assert lib.annhip_query_radius(ix.h, None, None, Q, y.data_ptr(), 0, c, rads[rn].data_ptr(), None, None,
                                           oi.data_ptr(), od.data_ptr(), counts.data_ptr()) == 0

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {s[0]: [] for s in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        for name, kind, c, rn in settings:
            ev0.record()
            step(y, kind, c, rn)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[name].append(ev0.elapsed_time(ev1))

    for name, kind, c, rn in settings:
        ix.profile(1)  # stage marks and row counters (a pass of its own)
        ix.stats(reset=True)
        for y in batches:
            step(y, kind, c, rn)
        torch.cuda.synchronize()
        sm = ix.stage_ms()
        st = ix.stats(reset=True)
        ix.profile(0)
        row = {}
        if kind is not None:
            step(batches[0], kind, c, rn)
            torch.cuda.synchronize()
            cc = counts.clone()
            gi = outs[c][0][:RQ].clone()
            ti, _, tc = ix.exact_query_radius(yr, radii[rn], c)
            rec, counted = A.radius_recall(gi, cc[:RQ], ti, tc)
            row = {"radius": rn, "radius_value": round(radii[rn], 4), "mean_count": round(cc.double().mean().item(), 3),
                   "share_count_eq_kcap": round((cc == c).double().mean().item(), 4),
                   "radius_recall": round(rec, 4), "recall_queries_counted": counted,
                   "truth_mean_count": round(tc.double().mean().item(), 3),
                   "truth_share_count_eq_kcap": round((tc == c).double().mean().item(), 4)}
        t = sorted(times[name])
        print(json.dumps({
            "workload": "N=%d d=%d k=%d tries=%d Q=%d float, %s data seed %d, fixed mode, no pair bits, max_query_k %d"
                        % (n, d, k, T, Q, args.data, args.seed, kmax),
            "setting": name, "kcap": c if c is not None else k,
            "entry": {None: "annhip_query", "trim": "annhip_query_k + annhip_radius_trim", "radius": "annhip_query_radius"}[kind],
            "ms_per_step": round(t[len(t) // 2], 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
            "stage1_ms": round(sm["stage1"] / nbatch, 4), "stage2_ms": round(sm["stage2_rows"] / nbatch, 4),
            "stage1_rows_per_query": round(st["s1_rows"] / max(st["queries"], 1.0), 1),
            "stage2_rows_per_query": round(st["other_rows"] / max(st["queries"], 1.0), 1),
            "plain_recall_at_k": round(plain_recall, 4), **row}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
