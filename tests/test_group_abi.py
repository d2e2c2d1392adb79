"""CPU-only: the grouped entry points (annhip_collapse, annhip_query_grouped, annhip_index_exact_query_grouped) exist in both
libraries, in the binding list and in the header with matching argument counts; the Python names and defaults exist; the
numpy model of the collapse (tests/group_model.py) against a brute-force restatement, and its prefix stability.  No device
call."""
import inspect
import os
import re

import numpy as np
import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib
from tests.group_model import collapse_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"annhip_collapse": ("c_int", 15), "annhip_query_grouped": ("c_long", 17),
           "annhip_index_exact_query_grouped": ("c_int", 15)}


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_both_libraries_export_the_three_symbols(prec):
    _lib.build()
    lib = _lib.load(prec)
    for sym, (restype, nargs) in SYMBOLS.items():
        assert hasattr(lib, sym), sym
        fn = getattr(lib, sym)
        assert fn.restype.__name__ == restype and len(fn.argtypes) == nargs, sym


def test_the_binding_list_and_the_header_carry_them():
    src = open(os.path.join(ROOT, "include", "ann_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym, (_, nargs) in SYMBOLS.items():
        assert sym in _lib.EXPORTED, sym
        m = re.search(r"\b%s\s*\(([^;{]*)\)\s*;" % sym, code)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
    text = " ".join(re.sub(r"^\s*\*", " ", src, flags=re.M).split())
    assert "collapse(first L entries of an ordering)[:k] == collapse(the whole ordering)[:k]" in text
    assert "a non-pad entry j is KEPT iff fewer than g earlier non-pad entries i < j have the same key" in text
    assert os.path.exists(os.path.join(ROOT, "approximatenn_amd", "csrc", "ann_group_kernels.h"))


def test_python_names_and_defaults():
    p = inspect.signature(A.collapse).parameters
    assert list(p) == ["ids", "dists", "tags", "group", "k", "per_group", "rows", "pad_id", "stream"]
    assert p["per_group"].default == 1 and p["rows"].default is None and p["pad_id"].default is None
    assert p["stream"].default is None
    p = inspect.signature(A.Index.query_grouped).parameters
    assert list(p) == ["self", "y", "group", "k", "per_group", "candidates", "oversample", "where", "alias", "ws", "stream"]
    assert p["k"].default is None and p["per_group"].default == 1 and p["candidates"].default is None
    assert p["oversample"].default == 4 and p["where"].default is None and p["alias"].default is False
    p = inspect.signature(A.Index.exact_query_grouped).parameters
    assert list(p) == ["self", "y", "group", "k", "per_group", "candidates", "oversample", "where", "alias"]
    # the existing signatures stay as they are
    assert list(inspect.signature(A.Index.query).parameters) == ["self", "y", "alias", "mode", "out_ids", "out_dists", "ws",
                                                                 "stream", "where", "k"]
    assert list(inspect.signature(A.Index.exact_query).parameters) == ["self", "y", "alias", "where", "k"]


def brute(ids, dists, tags, gmask, k, g, rows, pad_id):
    """The definition once more, entry by entry with no running state: entry j is kept iff it is no pad and fewer than g
    of the entries i < j are non-pads with its key."""
    Q, L = ids.shape
    oi = np.full((Q, k), pad_id, dtype=np.int64)
    od = np.full((Q, k), np.inf, dtype=dists.dtype)
    cnt, short = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=bool)
    word = ids.astype(np.uint64)
    for q in range(Q):
        real = word[q] < np.uint64(rows)
        key = np.where(real, tags[np.where(real, word[q], 0).astype(np.int64)] & np.uint32(gmask), 0)
        kept = [j for j in range(L)
                if real[j] and sum(1 for i in range(j) if real[i] and key[i] == key[j]) < g][:k]
        oi[q, :len(kept)] = word[q, kept].astype(np.int64)
        od[q, :len(kept)] = dists[q, kept]
        cnt[q] = len(kept)
        short[q] = len(kept) < k and bool(real.all())
    return oi, od, cnt, short


def _lists(rng, Q, L, rows, groups, dt, pad_share):
    """Random lists: ids below rows in random order (a repeated id now and then), a share of pads of several kinds
    anywhere in the row, ascending distances.  tags: `groups` values in bits 8.. beside a random low byte."""
    tags = ((rng.integers(0, groups, size=rows).astype(np.uint32) << 8) | rng.integers(0, 256, size=rows).astype(np.uint32))
    ids = rng.integers(0, rows, size=(Q, L)).astype(np.int64)
    pad = rng.random((Q, L)) < pad_share
    ids[pad] = rng.choice(np.array([rows, rows + 7, -1, 2 ** 32 + 5], dtype=np.int64), size=int(pad.sum()))
    dists = np.sort(rng.random((Q, L)).astype(dt), axis=1)
    return ids, dists, tags


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))
            and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))


@pytest.mark.parametrize("groups", [1, 3, 4000])
def test_model_against_the_brute_force_restatement(groups):
    rng = np.random.default_rng(9100 + groups)
    rows = 500
    for L, k, g, share in ((1, 1, 1, 0.0), (17, 5, 1, 0.2), (64, 64, 2, 0.1), (90, 10, 3, 0.0), (130, 40, 90, 0.3)):
        ids, dists, tags = _lists(rng, 12, L, rows, groups, np.float32 if L % 2 else np.float64, share)
        got = collapse_model(ids, dists, tags, 0xFFFFFF00, k, g, rows, rows)
        assert _same(got, brute(ids, dists, tags, 0xFFFFFF00, k, g, rows, rows)), (groups, L, k, g)
        assert np.all(got[2] <= k) and np.all(got[0][np.arange(k)[None, :] >= got[2][:, None]] == rows)


@pytest.mark.parametrize("groups", [1, 3, 4000])
def test_prefix_stability_of_the_model(groups):
    """collapse(first L entries)[:k] == collapse(whole list)[:k] wherever the left side is not short; where it is short
    (fewer than k although the prefix was full) its entries are still a prefix of the whole list's."""
    rng = np.random.default_rng(9200 + groups)
    rows, N = 600, 300
    seen_short = seen_exact = 0
    for k, g, share in ((10, 1, 0.0), (7, 2, 0.05), (1, 1, 0.0), (25, 3, 0.02)):
        ids, dists, tags = _lists(rng, 10, N, rows, groups, np.float64, share)
        whole = collapse_model(ids, dists, tags, 0xFFFFFF00, k, g, rows, rows)
        if share == 0.0:  # pads last, as a query returns them: a list that is not full has seen the whole ordering
            longer = collapse_model(np.concatenate([ids, np.full((10, 5), rows, dtype=np.int64)], axis=1),
                                    np.concatenate([dists, np.full((10, 5), np.inf)], axis=1), tags, 0xFFFFFF00, k, g, rows, rows)
            assert _same(longer[:3] + (whole[3],), whole) and not longer[3].any()
        for L in (k, 2 * k, 64, 65, 200, N):
            part = collapse_model(ids[:, :L], dists[:, :L], tags, 0xFFFFFF00, k, g, rows, rows)
            for q in range(10):
                c = int(part[2][q])
                assert np.array_equal(part[0][q, :c], whole[0][q, :c]) and np.array_equal(part[1][q, :c], whole[1][q, :c])
                if part[3][q]:
                    seen_short += 1
                    assert c < k
                else:  # k entries, or the prefix held a pad: the row is that of the whole list unless the list goes on
                    seen_exact += 1
                    if c == k:
                        assert np.array_equal(part[0][q], whole[0][q]) and part[2][q] == whole[2][q]
    assert seen_exact and (seen_short or groups > 3)
