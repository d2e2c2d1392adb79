#!/usr/bin/env python3
"""tools/group_bench.py -- grouped queries (annhip_query_grouped) beside the calls they are made of, on rows whose groups
lie together: the case grouping exists for.  ONE index per group size, the same batches.

    python tools/group_bench.py [--group-size 1,10,100] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                                [--rounds R] [--warmup W] [--lists 20,40,100,256] [--recall-queries 200]
                                [--centres C] [--sigma s] [--spread s2]
                                [--out profiles/group_bench_n4m.json.log]

Rows: the mixture of Gaussians of tools/probe_bench.py (C centres drawn N(0,1), sigma) one level deeper: group g = id // size
has a centre = a random mixture centre + sigma * N(0,1), its rows are that centre + spread * N(0,1) with spread < sigma, so
that the members of a group lie nearer to each other than to the neighbouring groups, and neighbouring groups exist.  A
query is a random group's centre + spread * N(0,1).  The tag word is the group number, the group mask all 32 bits.
k = the index's k, per_group = 1.
Settings per group size: the plain call ("plain" and "plain_again", timed first and last: the drift yardstick); for every
K': "query_k K'" = annhip_query_k(kq = K') alone, "grouped K'" = annhip_query_grouped(list = K'), "collapse K'" =
annhip_collapse alone on the [Q][K'] list of the same batch.  For every setting:
  * ms per step: HIP events around one batch, the settings alternated inside every round, median and min..max over R >= 7
    rounds after W warm-up rounds, one process;
  * for the collapse: its bytes, Q * L * (8 + sizeof(ftype) + 4) in plus Q * k * (8 + sizeof(ftype)) out, and the measured
    time over the time those bytes take at 8 TB/s;
  * for a grouped setting: the collapse's share of the query_k step that feeds it, the share of queries with short == 1,
    the mean count, and group-recall@k against annhip_index_exact_query_grouped on the recall queries (candidates = 1024;
    the truth's own short share is printed, and the recall is taken over the queries whose truth is not short).
One JSON line per setting, printed and appended to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group-size", default="1,10,100")
    ap.add_argument("--points", dest="n", type=int, default=4_000_000)
    ap.add_argument("--dim", dest="d", type=int, default=128)
    ap.add_argument("--knn", dest="k", type=int, default=10)
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--queries", dest="q", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.35)
    ap.add_argument("--spread", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--recall-queries", type=int, default=200)
    ap.add_argument("--lists", default="20,40,100,256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_bench_n4m.json.log"))
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
    log = open(args.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    for size in (int(t) for t in args.group_size.split(",")):
        ngroups = (n + size - 1) // size
        with park_random():
            gen = torch.Generator(device=dev)
            gen.manual_seed(args.seed + size)
            top = torch.randn((args.centres, d), device=dev, generator=gen)
            cen = torch.randn((ngroups, d), device=dev, generator=gen).mul_(args.sigma)
            cen += top[torch.randint(0, args.centres, (ngroups,), device=dev, generator=gen)]
            points = torch.randn((n, d), device=dev, generator=gen).mul_(args.spread)
            step = 1 << 20
            for a in range(0, n, step):  # centre rows added piecewise: no second [n, d] temporary
                b = min(n, a + step)
                points[a:b] += cen[torch.arange(a, b, device=dev) // size]
            batches = []
            for _ in range(nbatch):
                pick = torch.randint(0, ngroups, (Q,), device=dev, generator=gen)
                batches.append(torch.randn((Q, d), device=dev, generator=gen).mul_(args.spread).add_(cen[pick]))
            del cen, top
            torch.cuda.synchronize()
        libc.srandom(args.seed)
        ix = A.Index.precomp(points, k, T)
        ix.set_fixed(True)
        tags = (torch.arange(n, device=dev) // size).to(torch.int32)
        ix.set_tags(tags)
        lib, kmax = ix.lib, ix.max_query_k
        gmask = 0xFFFFFFFF
        RQ = min(args.recall_queries, Q)
        yr = batches[0][:RQ].contiguous()
        ti, _, tc, tshort = ix.exact_query_grouped(yr, gmask, k=k, candidates=1024)
        ok = ~tshort
        truth_short = tshort.double().mean().item()
        plain_recall = A.recall_at_k(ix.query(yr)[0], ix.exact_query(yr)[0])

        lists = [c for c in (int(t) for t in args.lists.split(",")) if k <= c <= kmax]
        settings = [("plain", None, None)]
        for c in lists:
            settings += [("query_k %d" % c, "k", c), ("grouped %d" % c, "grouped", c), ("collapse %d" % c, "collapse", c)]
        settings.append(("plain_again", None, None))
        li = {c: torch.empty((Q, c), dtype=torch.int64, device=dev) for c in lists}
        ld = {c: torch.empty((Q, c), dtype=torch.float32, device=dev) for c in lists}
        oi = torch.empty((Q, k), dtype=torch.int64, device=dev)
        od = torch.empty((Q, k), dtype=torch.float32, device=dev)
        counts = torch.zeros((Q,), dtype=torch.int32, device=dev)
        short = torch.zeros((Q,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (every call below runs on the null stream, as the events do)

        def run(y, kind, c):
            """One step of a setting: raw library calls on the null stream in every setting, so that the host gaps between
            launches, which the events include, are the same on both sides of a comparison."""
            if kind is None:
                lib.annhip_query(ix.h, Q, y.data_ptr(), 0, 0, oi.data_ptr(), od.data_ptr())
            elif kind == "k":
                assert lib.annhip_query_k(ix.h, None, None, Q, y.data_ptr(), 0, c, None, None, li[c].data_ptr(), ld[c].data_ptr()) == 0
            elif kind == "grouped":
                assert lib.annhip_query_grouped(ix.h, None, None, Q, y.data_ptr(), 0, c, k, 1, gmask, None, None, None, oi.data_ptr(),
                                                od.data_ptr(), counts.data_ptr(), short.data_ptr()) == 0
            else:  # the list that "query_k" has just written for this batch
                assert lib.annhip_collapse(Q, c, k, 1, gmask, tags.data_ptr(), n, n, li[c].data_ptr(), ld[c].data_ptr(), oi.data_ptr(),
                                           od.data_ptr(), counts.data_ptr(), short.data_ptr(), None) == 0

        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {s[0]: [] for s in settings}
        for r in range(args.warmup + args.rounds):
            y = batches[r % nbatch]
            for name, kind, c in settings:
                ev0.record()
                run(y, kind, c)
                ev1.record()
                ev1.synchronize()
                if r >= args.warmup:
                    times[name].append(ev0.elapsed_time(ev1))

        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        for name, kind, c in settings:
            t = sorted(times[name])
            row = {"workload": "N=%d d=%d k=%d tries=%d Q=%d float, groups of %d rows (spread %.2f) around centres of a mixture (%d centres, "
                               "sigma %.2f) seed %d, fixed mode, no pair bits, per_group 1, max_query_k %d"
                               % (n, d, k, T, Q, size, args.spread, args.centres, args.sigma, args.seed, kmax),
                   "group_size": size, "setting": name, "list": c if c is not None else k,
                   "ms_per_step": round(t[len(t) // 2], 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
                   "plain_recall_at_k": round(plain_recall, 4)}
            if kind == "collapse":
                nbytes = Q * c * (8 + 4 + 4) + Q * k * (8 + 4)
                row.update({"bytes": nbytes, "ms_at_8TBps": round(nbytes / 8e12 * 1e3, 5),
                            "time_over_bound": round(t[len(t) // 2] / (nbytes / 8e12 * 1e3), 1),
                            "share_of_query_k_step": round(t[len(t) // 2] / med["query_k %d" % c], 4)})
            if kind == "grouped":
                run(batches[0], kind, c)
                torch.cuda.synchronize()
                gi = oi[:RQ].clone()
                rec = A.recall_at_k(gi[ok], ti[ok]) if bool(ok.any()) else None
                row.update({"grouped_minus_query_k_ms": round(med[name] - med["query_k %d" % c], 4),
                            "share_short": round(short.double().mean().item(), 4),
                            "mean_count": round(counts.double().mean().item(), 3),
                            "group_recall_at_k": None if rec is None else round(rec, 4),
                            "recall_queries": int(ok.sum().item()), "truth_share_short_at_1024": round(truth_short, 4),
                            "truth_mean_count": round(tc.double().mean().item(), 3)})
            emit(row)
        ix.close()
        del points, batches, tags, ix
        torch.cuda.empty_cache()
    log.close()


if __name__ == "__main__":
    main()
