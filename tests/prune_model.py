"""numpy model of the pruned stage 1 (approximatenn_amd/csrc/ann_prune_kernels.h): preselect K' keys on the binary16
copy of the rows, rescore them on the float rows, certify.  Shared by tests/test_prune_model.py (CPU) and
tests/test_gpu_prune.py (which uses it to choose a data set where both outcomes occur)."""
import numpy as np

GAMMA = 2.0 ** -16


def h(p):
    """The rows rounded to binary16 and widened back (what annhip_index_set_rows stores)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(p, dtype=np.float32).astype(np.float16).astype(np.float32))


def row_error(p):
    """E >= max over the rows of ||p - h(p)||_2, in double, rounded up; inf where a row does not survive binary16."""
    df = np.asarray(p, dtype=np.float64) - h(p).astype(np.float64)
    with np.errstate(invalid="ignore"):
        worst = np.max(np.sum(df * df, axis=1))
    if not np.isfinite(worst):
        return np.inf
    return float(np.sqrt(worst) * (1.0 + 2.0 ** -20))


def sqdist32(y, rows):
    """Squared distances in float32 (a float tree of non-negative terms: within (1 + 2^-24)^(few) of the real sum)."""
    df = (rows - y[None, :]).astype(np.float32)
    return np.sum(df * df, axis=1, dtype=np.float32)


def keys_sorted(dist, ids):
    """Indices that order (distance bits, id) ascending: the selection path's total order."""
    return np.lexsort((ids, dist.view(np.uint32)))


def certify(B, tau, E):
    """The certificate of one query whose preselection is full: LB > tau, written so that everything odd fails."""
    B, tau = np.float64(B), np.float64(tau)
    g1 = 1.0 - GAMMA
    with np.errstate(invalid="ignore"):
        r = np.sqrt(B * g1) - E
    if not (B >= 2.0 ** -100 and r > 0.0):
        return False
    LB = (r * r) * g1 * (1.0 - 2.0 ** -40)
    return bool(LB > tau)


def prune_query(y, rows, rows_h, ids, k, kp, E):
    """One query against the candidate rows `rows` (ids `ids`, distinct).  Returns (certified, rescored, truth):
    rescored = the k+1 smallest exact keys among the preselection, truth = among ALL candidates, as (dist, id) arrays."""
    K1 = k + 1
    dh = sqdist32(y, rows_h)
    pre = keys_sorted(dh, ids)[:kp]
    m = pre.size
    dx = sqdist32(y, rows[pre])
    o = keys_sorted(dx, ids[pre])[:K1]
    rescored = (dx[o], ids[pre][o])
    dall = sqdist32(y, rows)
    oa = keys_sorted(dall, ids)[:K1]
    truth = (dall[oa], ids[oa])
    if m < kp:
        cert = True
    elif o.size < K1:
        cert = False
    else:
        cert = certify(dh[pre[-1]], rescored[0][K1 - 1], E)
    return cert, rescored, truth


def default_keys(k):
    return min(64, max(16, 3 * (k + 1) // 2))
