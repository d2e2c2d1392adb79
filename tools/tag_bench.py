#!/usr/bin/env python3
"""tools/tag_bench.py -- per-query tag predicates of fixed mode (annhip_query_tagged) against the allow-list bitmap
(annhip_index_set_filter) and against no filter, on ONE index and the same batches.

    python tools/tag_bench.py [--points N] [--dim d] [--knn k] [--tries T] [--queries Q] [--rounds R] [--warmup W]
                              [--bits 0,8] [--tenants 2,10,100] [--ranges]

Rows are iid N(0,1), generated on the device (tools/filter_bench.py's data).  For every tenant count S the rows carry a
tenant field, uniform over S tenants, as their tag word; a tagged batch asks for a random tenant per query (mask
0xFFFFFFFF), so a query keeps a share 1/S of its candidates.  For every pair-bit setting b the settings are:
  none, none_again   no filter, twice per round: their spread is the run's noise floor (both run the unfiltered kernels)
  bitmap_ones        the allow list with every bit set
  tag_all            tagged, (mask, value) = (0, 0) for every query: the same candidates through the tag kernels
  tag_S              tagged, S tenants, a random tenant per query
  bitmap_S           the allow list of ONE tenant of the same S for the whole batch: the same share of the candidates
For every setting:
  * ms per step: HIP events around one batch, all settings alternated inside every round, median over R >= 7 rounds after
    W warm-up rounds, one process;
  * the stage-1 kernel alone (annhip_profile 2: one event pair), in a separate pass;
  * rows gathered per query (annhip_stats, annhip_profile 1) and the stage-1 kernel's algorithmic bytes per second
    (gathered rows + the candidate ids read + per candidate id one tag word and / or one bitmap word + one segment word per
    probed bucket + the query's row, codes, ranked bits, predicate and result keys).
One JSON line per setting.

--ranges adds the range predicate (annhip_query_between), inside the same alternating rounds and with the same fields; the
settings above and their lines are what they are without it.  The rows' tag word for these settings is a uniform 16-bit
value:
  between_all        (mask, lo, hi) = (0xFFFF, 0, 0xFFFF) for every query: the full interval, the same candidates
  between_S          for every S of --tenants: a random window per query that holds 1/S of the value space
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
    ap.add_argument("--bits", default="0,8")
    ap.add_argument("--tenants", default="2,10,100")
    ap.add_argument("--ranges", action="store_true", help="add the between_all / between_S settings (annhip_query_between)")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7 (the median is taken over them)")

    import torch

    import approximatenn_amd as A
    from approximatenn_amd._lib import park_random

    n, d, k, T, Q = args.n, args.d, args.k, args.tries, args.q
    dev = torch.device("cuda", 0)
    libc = __import__("ctypes").CDLL("libc.so.6")
    tenants = [int(tok) for tok in args.tenants.split(",")]
    nbatch = 3
    with park_random():
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        points = torch.randn((n, d), device=dev, generator=gen)
        batches = [torch.randn((Q, d), device=dev, generator=gen) for _ in range(nbatch)]
        tags, wheres, masks = {}, {}, {"ones": torch.ones(n, dtype=torch.bool, device=dev)}
        for S in tenants:
            tags[S] = torch.randint(0, S, (n,), device=dev, generator=gen, dtype=torch.int32)
            wheres[S] = (torch.full((Q,), -1, dtype=torch.int32, device=dev),  # mask 0xFFFFFFFF
                         torch.randint(0, S, (Q,), device=dev, generator=gen, dtype=torch.int32))
            masks[S] = tags[S] == 0
        zeros = torch.zeros((Q,), dtype=torch.int32, device=dev)
        if args.ranges:  # (drawn after everything above: the other settings see the data they see without the flag)
            tags["r16"] = torch.randint(0, 1 << 16, (n,), device=dev, generator=gen, dtype=torch.int32)
            m16 = torch.full((Q,), 0xFFFF, dtype=torch.int32, device=dev)
            between = {"all": (m16, zeros, m16)}
            for S in tenants:
                width = max(1, (1 << 16) // S)
                lo = torch.randint(0, (1 << 16) - width + 1, (Q,), device=dev, generator=gen, dtype=torch.int32)
                between[S] = (m16, lo, lo + (width - 1))
        torch.cuda.synchronize()
    libc.srandom(args.seed)
    ix = A.Index.precomp(points, k, T)
    ds = ix.d_short
    settings = []  # (name, pair bits, bitmap name or None, tag set or None, where or None)
    for tok in args.bits.split(","):
        b = min(int(tok), ds)
        settings.append(("b%d_none" % b, b, None, None, None))
        settings.append(("b%d_bitmap_ones" % b, b, "ones", None, None))
        settings.append(("b%d_tag_all" % b, b, None, tenants[0], (zeros, zeros)))
        if args.ranges:
            settings.append(("b%d_between_all" % b, b, None, "r16", between["all"]))
        for S in tenants:
            settings.append(("b%d_tag_%d" % (b, S), b, None, S, wheres[S]))
            settings.append(("b%d_bitmap_%d" % (b, S), b, S, None, None))
            if args.ranges:
                settings.append(("b%d_between_%d" % (b, S), b, None, "r16", between[S]))
        settings.append(("b%d_none_again" % b, b, None, None, None))
    ix.set_fixed(True)
    state = {"tags": None}

    def apply(b, m, tg):
        ix.set_probe(b)
        ix.set_filter(None if m is None else masks[m])
        if tg is not None and state["tags"] != tg:  # (an untagged query never reads the tags: they may stay)
            ix.set_tags(tags[tg])
            state["tags"] = tg

    out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((Q, k), dtype=torch.float32, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {s[0]: [] for s in settings}
    for r in range(args.warmup + args.rounds):
        y = batches[r % nbatch]
        for name, b, m, tg, where in settings:
            apply(b, m, tg)  # (synchronous, outside the event bracket)
            ev0.record()
            ix.query(y, out_ids=out_i, out_dists=out_d, where=where)
            ev1.record()
            ev1.synchronize()
            if r >= args.warmup:
                times[name].append(ev0.elapsed_time(ev1))

    ids_read = {}  # per b: candidate ids a query reads = the rows an unfiltered query gathers
    for name, b, m, tg, where in settings:
        apply(b, m, tg)
        ix.profile(2)  # the stage-1 event pair only
        ix.stats(reset=True)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d, where=where)
        torch.cuda.synchronize()
        st = ix.stats(reset=True)
        s1_ms = st["s1_ms"] / max(st["s1_launches"], 1.0)
        ix.profile(1)  # row statistics (separate pass)
        for y in batches:
            ix.query(y, out_ids=out_i, out_dists=out_d, where=where)
        torch.cuda.synchronize()
        st1 = ix.stats(reset=True)
        ix.profile(0)
        rows_q = st1["s1_rows"] / max(st1["queries"], 1.0)
        if m is None and where is None:
            ids_read.setdefault(b, rows_q)
        ids_q = ids_read[b]
        buckets = 1 + ds + b * (b - 1) // 2
        per_id = 4 + (4 if m is not None else 0) + (4 if where is not None else 0)
        bytes_q = rows_q * d * 4 + ids_q * per_id + T * buckets * 8 + d * 4 + T * 4 + T * b + (4 * len(where) if where is not None else 0) + (k + 1) * 8
        share = tg  # S of the setting: tag_S keeps one tenant of S, between_S a window of 1/S of the 16-bit values
        if tg == "r16":
            share = None if name.endswith("_all") else int(name.rsplit("_", 1)[1])
        t = sorted(times[name])
        print(json.dumps({
            "workload": "N=%d d=%d k=%d tries=%d Q=%d float, iid data seed %d, d_short %d" % (n, d, k, T, Q, args.seed, ds),
            "setting": name, "pair_bits": b, "bitmap": m, "tenants": share if where is not None else None,
            "allowed_rows": ix.filter_count, "buckets_per_try": buckets,
            "ms_per_step": round(t[len(t) // 2], 4), "ms_per_step_min_max": [round(t[0], 4), round(t[-1], 4)], "rounds": len(t),
            "stage1_ms": round(s1_ms, 4), "candidate_ids_per_query": round(ids_q, 1),
            "rows_gathered_per_query": round(rows_q, 1), "algorithmic_bytes_per_query": int(bytes_q),
            "stage1_TBps": round(bytes_q * Q / (s1_ms * 1e-3) / 1e12, 3) if s1_ms > 0 else None}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
