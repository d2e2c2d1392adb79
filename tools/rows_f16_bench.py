#!/usr/bin/env python3
"""tools/rows_f16_bench.py -- native vs narrow point rows (annhip_index_set_rows) on ONE index and the same batches:
binary16 rows in the f32 library (the default), binary32 rows in the f64 library (--dtype f64).

    python tools/rows_f16_bench.py [--dtype f32|f64] [--points N] [--dim d] [--knn k] [--steps K] [--warmup W]
                                   [--rounds R] [--data randn|randnorm]

Workload: bench.py's cfg3 by default (N=10M, d=128, k=10, tries=10, Q=10k per step, float); cfg5 is --dtype f64 --dim 256
--knn 100.  The index is built once (precomp from the native rows); the narrow copy of the rows is made once (the first
set_rows("f16") / set_rows("f32")).  Then:
  * timing: R rounds, each timing the K batches with native rows, then with narrow rows -- the modes alternate in one
    process, so drift of clocks or temperature hits both;
  * stage 1: a separate pass per mode with the stage-1 HIP-event pair only (annhip_profile 2), and one with the row
    statistics (annhip_profile 1) for the algorithmic bytes;
  * quality: recall against the NATIVE rows (annhip_recall_ranks, exact-rank brute force) on a sample of the first batch,
    and the share of result ids that differ between the modes over one whole batch.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (as bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", dest="n", type=int, default=10_000_000)
    ap.add_argument("--dim", dest="d", type=int, default=128)
    ap.add_argument("--knn", dest="k", type=int, default=10)
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--queries", dest="q", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--data", choices=["randn", "randnorm"], default="randn",
                    help="randn = torch.randn on the device (fast); randnorm = the reference drivers' stream (bench.py's default)")
    ap.add_argument("--recall-queries", type=int, default=512)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32",
                    help="f32: float rows vs binary16 rows; f64: double rows (the reference's stock build) vs binary32 rows")
    args = ap.parse_args()

    import numpy as np
    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T, Q = args.n, args.d, args.k, args.tries, args.q
    prec = args.dtype
    narrow, tdt, nsz = ("f16", torch.float32, 4) if prec == "f32" else ("f32", torch.float64, 8)  # nsz: native element bytes
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    with park_random():
        torch.zeros(1, device=dev)
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    nb = args.warmup + args.steps
    if args.data == "randnorm":
        host = A.synth_randnorm(n * d, prec, reset=True).reshape(n, d)
        with park_random():
            points = torch.from_numpy(host).to(dev)
        del host
    else:
        with park_random():
            gen = torch.Generator(device=dev)
            gen.manual_seed(args.seed)
            points = torch.randn((n, d), device=dev, dtype=tdt, generator=gen)
    t0 = time.time()
    ix = A.Index.precomp(points, k, T)
    precomp_s = time.time() - t0
    with park_random():
        if args.data == "randnorm":
            batches = [torch.from_numpy(A.synth_randnorm(Q * d, prec).reshape(Q, d)).to(dev) for _ in range(nb)]
        else:
            batches = [torch.randn((Q, d), device=dev, dtype=tdt, generator=gen) for _ in range(nb)]
        torch.cuda.synchronize()
    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((Q, k), dtype=tdt, device=dev)

    def run(ys):
        for y in ys:
            ix.query(y, out_ids=out_i, out_dists=out_d)

    t0 = time.time()
    ix.set_rows(narrow)  # the one conversion
    torch.cuda.synchronize()
    convert_s = time.time() - t0
    modes = ("native", narrow)
    for m in modes:
        ix.set_rows(m)
        run(batches[:args.warmup])
    torch.cuda.synchronize()

    timed = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            ix.set_rows(m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(batches[args.warmup:])
            torch.cuda.synchronize()
            timed[m].append((time.perf_counter() - t0) * 1e3 / args.steps)

    res = {}
    ids_of = {}
    for m in modes:
        ix.set_rows(m)
        ix.profile(2)                       # the stage-1 event pair only
        ix.stats(reset=True)
        run(batches[args.warmup:])
        torch.cuda.synchronize()
        st = ix.stats(reset=True)
        s1_ms = st["s1_ms"] / max(st["s1_launches"], 1.0)
        ix.profile(1)                       # gathered-row statistics (separate pass)
        run(batches[args.warmup:])
        torch.cuda.synchronize()
        st1 = ix.stats(reset=True)
        ix.profile(0)
        rows_q = st1["s1_rows"] / max(st1["queries"], 1.0)
        esz = nsz // 2 if m == narrow else nsz
        bytes_q = rows_q * d * esz + ix.P1 * 4 + d * nsz + T * 4 + (k + 1) * (nsz + 4)   # bench.py's roofline_of, rows at esz
        ms = sorted(timed[m])[len(timed[m]) // 2]
        res[m] = {"ms_per_step": round(ms, 4), "ms_per_step_rounds": [round(v, 4) for v in timed[m]],
                  "qps": round(Q / (ms * 1e-3), 1), "stage1_ms": round(s1_ms, 4),
                  "rows_gathered_per_query": round(rows_q, 1), "algorithmic_bytes_per_query": int(bytes_q),
                  "stage1_GBps": round(bytes_q * Q / (s1_ms * 1e-3) / 1e9, 1) if s1_ms > 0 else None,
                  "stage1_frac_of_8TBps": round(bytes_q * Q / (s1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if s1_ms > 0 else None,
                  "exact_queries_per_step": st["exact_queries"] / args.steps}
        ids, _, _ = ix.query(batches[0])
        torch.cuda.synchronize()
        ids_of[m] = ids.clone()

    qs = min(args.recall_queries, Q)
    ys = batches[0][:qs].contiguous()
    for m in modes:
        rk = A.recall_ranks(points, ys, ids_of[m][:qs].contiguous())   # exact ranks against the NATIVE rows
        r = rk.to("cpu").double().numpy()
        res[m]["recall_at_k"] = round(float((r < k).mean()), 4)
        res[m]["recall_sample"] = {kk: round(v, 4) for kk, v in A.recall_summary(rk, k).items()}
    diff = float((ids_of["native"] != ids_of[narrow]).double().mean().item())
    line = {
        "workload": "N=%d d=%d k=%d tries=%d Q=%d %s, %s data seed %d" % (n, d, k, T, Q, "float" if prec == "f32" else "double",
                                                                      args.data, args.seed),
        "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
        "precomp_s": round(precomp_s, 2), narrow + "_conversion_s": round(convert_s, 3),
        "native": res["native"], narrow: res[narrow],
        narrow + "_over_native": {"ms_per_step": round(res[narrow]["ms_per_step"] / res["native"]["ms_per_step"], 4),
                                  "stage1_ms": round(res[narrow]["stage1_ms"] / res["native"]["stage1_ms"], 4)
                                  if res["native"]["stage1_ms"] > 0 else None},
        "ids_differing_share": round(diff, 5), "recall_queries": qs,
        "index_bytes_rows": {"native": n * d * nsz, narrow: n * d * nsz // 2},
    }
    ix.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
