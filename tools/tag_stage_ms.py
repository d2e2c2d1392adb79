#!/usr/bin/env python3
"""tools/tag_stage_ms.py -- the per-stage kernel time of the pair-form tagged step, for an A/B of two trees.

    python tools/tag_stage_ms.py [--root TREE] [--build NAME] [--points N] [--dim d] [--knn k] [--tries T] [--queries Q]
                                 [--rounds R] [--bits 0,8] [--tenants 2,10,100]

tools/tag_bench.py times a whole step from the host and the stage-1 kernel alone; stage 2 of a tagged step
(stage2_tag_kernel) is in neither figure by itself.  This tool runs tag_bench's tag_all / tag_S settings (the same data,
seeds and predicates) under annhip_profile 1, where the library brackets every stage of a call with events on the stream,
and prints per setting the median over R rounds of codes, stage 1, finalize and stage 2 in ms, and their sum: kernel time
only, no host time.  --root imports the package of another checkout (its own library), so that the parent commit and this
one are measured by the same script; it uses nothing the pair form's first version did not have.  One JSON line per
setting, stamped with --build.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--build", default="this")
    ap.add_argument("--points", dest="n", type=int, default=4_000_000)
    ap.add_argument("--dim", dest="d", type=int, default=128)
    ap.add_argument("--knn", dest="k", type=int, default=10)
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--queries", dest="q", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--bits", default="0,8")
    ap.add_argument("--tenants", default="2,10,100")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T, Q = args.n, args.d, args.k, args.tries, args.q
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    tenants = [int(tok) for tok in args.tenants.split(",")]
    with park_random():  # tools/tag_bench.py's draws, in its order
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        points = torch.randn((n, d), device=dev, generator=gen)
        batches = [torch.randn((Q, d), device=dev, generator=gen) for _ in range(3)]
        tags, wheres = {}, {}
        for S in tenants:
            tags[S] = torch.randint(0, S, (n,), device=dev, generator=gen, dtype=torch.int32)
            wheres[S] = (torch.full((Q,), -1, dtype=torch.int32, device=dev),
                         torch.randint(0, S, (Q,), device=dev, generator=gen, dtype=torch.int32))
        zeros = torch.zeros((Q,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ix.set_fixed(True)
    settings = []
    for tok in args.bits.split(","):
        b = min(int(tok), ix.d_short)
        settings.append(("b%d_tag_all" % b, b, tenants[0], (zeros, zeros)))
        settings += [("b%d_tag_%d" % (b, S), b, S, wheres[S]) for S in tenants]
    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((Q, k), dtype=torch.float32, device=dev)
    keys = ("codes", "stage1", "finalize_fallback", "stage2_rows")
    seen = {s[0]: [] for s in settings}
    ix.profile(1)
    for r in range(2 + args.rounds):
        for name, b, S, where in settings:
            ix.set_probe(b)
            ix.set_tags(tags[S])
            ix.stats(reset=True)
            ix.query(batches[r % 3], out_ids=out_i, out_dists=out_d, where=where)
            torch.cuda.synchronize()
            ms = ix.stage_ms()
            ix.stats(reset=True)
            if r >= 2:
                seen[name].append([ms[key] for key in keys])
    for name, b, S, where in settings:
        med = [sorted(v[j] for v in seen[name])[len(seen[name]) // 2] for j in range(len(keys))]
        tot = sorted(sum(v) for v in seen[name])
        print(json.dumps({"build": args.build, "setting": name, "rounds": len(tot),
                          "codes_ms": round(med[0], 4), "stage1_ms": round(med[1], 4), "finalize_ms": round(med[2], 4),
                          "stage2_ms": round(med[3], 4), "kernel_ms_per_step": round(tot[len(tot) // 2], 4),
                          "kernel_ms_min_max": [round(tot[0], 4), round(tot[-1], 4)]}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
