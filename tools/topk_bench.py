#!/usr/bin/env python3
"""tools/topk_bench.py -- the per-call k of fixed mode (annhip_query_k) on ONE index and the same batches.

    python tools/topk_bench.py [--points N] [--dim d] [--knn k] [--tries T] [--queries Q] [--rounds R] [--warmup W]
                               [--kq 1,32,100]

iid N(0,1) rows and queries generated on the device (the benchmark's data).  Settings: the plain fixed-mode annhip_query
("plain" and "plain_again": read twice per round -- the spread between the two is the noise floor the others are read
against), annhip_query_k with kq = the index's k ("kq=<k>": the yardstick, it should cost what the plain call costs) and
annhip_query_k with every --kq value.  For every setting:
  * ms per step: HIP events around one batch, the settings alternated inside every round, median over R >= 7 rounds after
    W warm-up rounds, one process;
  * stage-2 ms per step and stage-2 rows gathered per query (annhip_profile 1: stage marks and row counters), in a
    separate pass over the same batches.
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
    ap.add_argument("--points", dest="n", type=int, default=4_000_000)
    ap.add_argument("--dim", dest="d", type=int, default=128)
    ap.add_argument("--knn", dest="k", type=int, default=10)
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--queries", dest="q", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--kq", default="1,32,100")
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
        points = torch.randn((n, d), device=dev, generator=gen)
        batches = [torch.randn((Q, d), device=dev, generator=gen) for _ in range(nbatch)]
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ix.set_fixed(True)
    kmax = ix.max_query_k
    # (name, kq): None = the plain call
    settings = [("plain", None), ("kq=%d" % k, k)]
    for tok in args.kq.split(","):
        kq = int(tok)
        if 1 <= kq <= kmax and kq not in [s[1] for s in settings]:
            settings.append(("kq=%d" % kq, kq))
    settings.append(("plain_again", None))
    outs = {kq: (torch.empty((Q, kq or k), dtype=torch.int64, device=dev), torch.empty((Q, kq or k), dtype=torch.float32, device=dev))
            for _, kq in settings}

    def step(y, kq):
        oi, od = outs[kq]
        if kq is None:
            ix.query(y, out_ids=oi, out_dists=od)
        else:
            ix.query(y, out_ids=oi, out_dists=od, k=kq)

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        for name, kq in settings:
            ev0.record()
            step(y, kq)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[name].append(ev0.elapsed_time(ev1))

    same = None
    for name, kq in settings:
        ix.profile(1)  # stage marks and row counters (a pass of its own)
        ix.stats(reset=True)
        for y in batches:
            step(y, kq)
        torch.cuda.synchronize()
        s2_ms = ix.stage_ms()["stage2_rows"] / nbatch
        st = ix.stats(reset=True)
        ix.profile(0)
        if kq == k:  # the yardstick's other half: the same bits as the plain call
            step(batches[0], None), step(batches[0], k)
            torch.cuda.synchronize()
            same = bool(torch.equal(outs[None][0], outs[k][0]) and torch.equal(outs[None][1].view(torch.int32), outs[k][1].view(torch.int32)))
        t = sorted(times[name])
        print(json.dumps({
            "workload": "N=%d d=%d k=%d tries=%d Q=%d float, iid data seed %d, fixed mode, max_query_k %d" % (n, d, k, T, Q, args.seed, kmax),
            "setting": name, "kq": kq if kq is not None else k, "entry": "annhip_query" if kq is None else "annhip_query_k",
            "ms_per_step": round(t[len(t) // 2], 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
            "stage2_ms": round(s2_ms, 4), "stage2_rows_per_query": round(st["other_rows"] / max(st["queries"], 1.0), 1),
            "stage1_rows_per_query": round(st["s1_rows"] / max(st["queries"], 1.0), 1),
            **({"same_bits_as_plain": same} if kq == k else {})}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
