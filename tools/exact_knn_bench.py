#!/usr/bin/env python3
"""tools/exact_knn_bench.py -- exact brute-force k-NN (annhip_exact_knn) against the recall scorer (annhip_recall_ranks)
on the same tensors: both compute all n * Q squared distances of d elements with the same arithmetic.

    python tools/exact_knn_bench.py [--points N] [--dim d] [--queries Q] [--knn k] [--dtype f32|f64] [--reps R] [--warmup W]

recall_ranks is fed the exact ids (its cheapest input: almost no point beats a query's farthest guess).  After W warm-up
calls of each, the two calls alternate R times in one process (drift of clocks hits both); each call is synchronous and is
timed with a pair of HIP events.  Prints one JSON line: the median times, their ratio, pairs_per_s = n * Q / t and the
fraction of the vector-ALU bound reached -- without fma a pair element costs a subtract, a multiply and an add, i.e.
peak_flops / 2 / 3 pair elements per second at the packed rate that counts an fma as two operations.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PEAK_FLOPS = {"f32": 157.3e12, "f64": 78.6e12}  # MI355X vector peak, an fma counted as two operations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", dest="d", type=int, default=128)
    ap.add_argument("--queries", dest="q", type=int, default=10_000)
    ap.add_argument("--knn", dest="k", type=int, default=10)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--skip-recall", action="store_true", help="time exact_knn only")
    args = ap.parse_args()
    assert args.reps >= 1

    import torch

    import approximatenn_amd as A
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dt = torch.float32 if args.dtype == "f32" else torch.float64
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    pts = torch.randn((args.n, args.d), dtype=dt, device="cuda", generator=gen)
    y = torch.randn((args.q, args.d), dtype=dt, device="cuda", generator=gen)

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    ids = None
    for _ in range(max(1, args.warmup)):
        ids, _ = A.exact_knn(pts, y, args.k)
        if not args.skip_recall:
            ranks = A.recall_ranks(pts, y, ids)
    t_exact, t_recall = [], []
    for _ in range(args.reps):
        t, (ids2, _) = timed(lambda: A.exact_knn(pts, y, args.k))
        t_exact.append(t)
        if not args.skip_recall:
            t, ranks = timed(lambda: A.recall_ranks(pts, y, ids))
            t_recall.append(t)
    assert torch.equal(ids, ids2)
    if not args.skip_recall:  # the scorer agrees that these are the nearest: nobody is closer than rank j allows
        assert bool((ranks <= torch.arange(args.k, device="cuda")[None, :]).all())
    te = statistics.median(t_exact)
    pair_elems = float(args.n) * args.q * args.d
    bound = VALU_PEAK_FLOPS[args.dtype] / 2 / 3  # pair elements per second
    out = dict(tool="exact_knn_bench", n=args.n, d=args.d, Q=args.q, k=args.k, dtype=args.dtype, reps=args.reps,
               exact_knn_s=te, exact_knn_s_min=min(t_exact), exact_knn_s_max=max(t_exact),
               pairs_per_s=args.n * args.q / te, pair_elems_per_s=pair_elems / te,
               valu_bound_pair_elems_per_s=bound, valu_bound_fraction=pair_elems / te / bound,
               device=torch.cuda.get_device_name(0))
    if not args.skip_recall:
        tr = statistics.median(t_recall)
        out.update(recall_ranks_s=tr, recall_ranks_s_min=min(t_recall), recall_ranks_s_max=max(t_recall),
                   ratio_exact_over_recall=te / tr, recall_pairs_per_s=args.n * args.q / tr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
