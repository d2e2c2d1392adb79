#!/usr/bin/env python3
"""tools/tail_bench.py -- what the appended rows of an index (annhip_index_append) cost a fixed-mode step, on ONE index
and the same batches.

    python tools/tail_bench.py [--data iid|clustered] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                               [--rounds R] [--warmup W] [--tails 0,1000,10000,100000,400000]

The method of tools/probe_bench.py: one process, the settings alternated inside every round, HIP events around one batch,
median over R >= 7 rounds after W warm-up rounds.  The settings are twin indexes built from the same rows and the same
random() seed, one per tail length m (the first m rows of one pool of appended rows), plus a second tail-free index
("0_again": the spread between the two tail-free readings is the noise floor the others are read against).  Per setting:
  * ms per step;
  * the tail kernel's own time (annhip_profile 1 stage marks, slot "stage2_network", in a separate pass) and its rate in
    (query, row) pairs per second;
  * the reference for the kernel: A.exact_knn over the same m tail rows and the same batch, alternated in the same rounds
    -- the repository's existing scan, which does strictly more selection work and starts with no threshold -- and its rate.
One JSON line per setting, then one summary line with the m at which the tail costs as much as the index step itself
(linear interpolation between the measured tail lengths).
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
    ap.add_argument("--tails", default="0,1000,10000,100000,400000")
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

    settings = []  # (name, m, index): the indexes share the point rows
    for name, m in [(str(m), m) for m in tails] + [("0_again", 0)]:
        libc.srandom(args.seed)
        ix = A.Index.precomp(points, k, T)
        ix.set_fixed(True)
        if m:
            ix.reserve_tail(m)
            ix.append(pool[:m])
        settings.append((name, m, ix))
    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _, _ in settings}
    ref = {name: [] for name, _, _ in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        for name, m, ix in settings:
            ev0.record()
            ix.query(y, out_ids=out_i, out_dists=out_d)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[name].append(ev0.elapsed_time(ev1))
            if m >= k:  # the existing scan over the same tail rows and the same batch (synchronous, null stream)
                ev0.record()
                A.exact_knn(pool[:m], y, k, out_ids=out_i, out_dists=out_d)
                ev1.record()
                ev1.synchronize()
                if r >= args.warmup:
                    ref[name].append(ev0.elapsed_time(ev1))

    def med(v):
        v = sorted(v)
        return v[len(v) // 2] if v else None

    rows = []
    for name, m, ix in settings:
        ix.profile(1)  # stage marks (separate pass): slot "stage2_network" is the tail's scan in fixed mode
        ix.stats(reset=True)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d)
        torch.cuda.synchronize()
        ix.stats()  # folds the marks into stage_ms
        tail_ms = ix.stage_ms()["stage2_network"] / nbatch
        ix.profile(0)
        t, rf = sorted(times[name]), sorted(ref[name])
        row = {
            "workload": "N=%d d=%d k=%d tries=%d Q=%d float, %s data seed %d" % (n, d, k, T, Q, args.data, args.seed),
            "setting": name, "tail_rows": m,
            "ms_per_step": round(med(t), 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
            "tail_kernel_ms": round(tail_ms, 4) if m else 0.0,
            "tail_pairs_per_s": round(Q * m / (tail_ms * 1e-3), 0) if m and tail_ms > 0 else None,
            "exact_knn_ms": round(med(rf), 4) if rf else None,
            "exact_knn_ms_min_max": [round(rf[0], 4), round(rf[-1], 4)] if rf else None,
            "exact_knn_pairs_per_s": round(Q * m / (med(rf) * 1e-3), 0) if rf else None}
        rows.append(row)
        print(json.dumps(row), flush=True)
    base = rows[0]["ms_per_step"]
    noise = abs(rows[-1]["ms_per_step"] - base)
    cross = None
    pts = [(r["tail_rows"], r["ms_per_step"] - base) for r in rows[:-1]]
    for (m0, c0), (m1, c1) in zip(pts, pts[1:]):
        if c0 < base <= c1 and c1 > c0:
            cross = m0 + (m1 - m0) * (base - c0) / (c1 - c0)
            break
    print(json.dumps({"summary": "tail cost = index step", "index_step_ms": base, "tail_free_spread_ms": round(noise, 4),
                      "tail_rows_at_equal_cost": None if cross is None else int(cross)}), flush=True)
    for _, _, ix in settings:
        ix.close()


if __name__ == "__main__":
    main()
