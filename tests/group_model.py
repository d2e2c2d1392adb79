"""The contract of annhip_collapse (include/ann_hip.h, "grouped queries") in numpy, written from its definition as a loop
per row: no ballots, no chunks, nothing of the kernel's algorithm."""
import numpy as np


def collapse_model(ids, dists, tags, gmask, k, g, rows, pad_id):
    """ids int [Q,L] (any integer dtype; the entries are read as unsigned 64-bit words: -1 is 2^64 - 1), dists [Q,L],
    tags uint32 [>= rows] -> (ids int64 [Q,k], dists [Q,k], counts int32 [Q], short bool [Q])."""
    ids = np.asarray(ids)
    Q, L = ids.shape
    assert dists.shape == (Q, L) and 1 <= k <= L and g >= 1
    out_i = np.full((Q, k), pad_id, dtype=np.int64)
    dists = np.ascontiguousarray(dists)
    out_d = np.full((Q, k), np.inf, dtype=dists.dtype)
    bits = np.uint32 if dists.dtype == np.float32 else np.uint64  # distances are copied as bit patterns
    in_b, out_b = dists.view(bits), out_d.view(bits)
    counts = np.zeros(Q, dtype=np.int32)
    short = np.zeros(Q, dtype=bool)
    for q in range(Q):
        seen = {}  # key -> non-pad entries so far
        pads = 0
        for j in range(L):
            word = int(ids[q, j]) & 0xFFFFFFFFFFFFFFFF
            if word >= rows:
                pads += 1
                continue
            key = int(tags[word]) & gmask
            earlier = seen.get(key, 0)
            seen[key] = earlier + 1
            if earlier < g and counts[q] < k:
                out_i[q, counts[q]] = word
                out_b[q, counts[q]] = in_b[q, j]
                counts[q] += 1
        short[q] = counts[q] < k and pads == 0
    return out_i, out_d, counts, short
