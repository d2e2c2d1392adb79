"""CPU-only: the set form of the sorted scan (include/ann_hip.h) exists in both libraries and in the Python package, the
header states its contract, and the host-side models of its staging -- A.normalize_intervals and A.set_pieces -- agree with
brute force (no compute calls on a device)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib

SYMS = {"annhip_tag_runs_set": (C.c_int, "int", 8), "annhip_query_sorted_set": (C.c_long, "long", 15)}
FULL = 0xFFFFFFFF


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_set_symbols_are_exported(prec):
    lib = _lib.load(prec)
    for sym, (restype, _, nargs) in SYMS.items():
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).restype is restype, sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    assert lib.annhip_query_sorted_set.argtypes[11] is C.c_size_t  # split_rows


def test_header_declares_the_symbols_and_states_the_contract():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym, (_, ctype, nargs) in SYMS.items():
        m = re.search(r"\b(long|int|size_t)\s+%s\s*\(([^;{]*)\)\s*;" % sym, code)
        assert m, sym
        assert m.group(1) == ctype, sym
        assert len(m.group(2).split(",")) == nargs, sym
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for sentence in ("a UNION of intervals",
                     "lo[j] <= (tags[i] & field_mask) <= hi[j] for some such j",
                     "A query with no interval matches nothing and gets all pads",
                     "off_host is a HOST array [ycnt + 1]",
                     "ordered by (lo, hi)",
                     "clipped to start above the largest hi before it",
                     "nothing follows hi = 0xFFFFFFFF",
                     "no row is offered twice to one query",
                     "(0, 0) for the slots that the normalisation emptied",
                     "cut at the GLOBAL positions S, 2S, 3S, ... of the order",
                     "the set call splits long runs",
                     "SYNCHRONISES hip_stream once",
                     "With S = 0 the call does not synchronise",
                     "Returns the entry count E >= 0",
                     "for 0 < S < 64",
                     "for a set of more than 256 intervals",
                     "E * kq > 2^27 partial slots",
                     "they compete exactly once",
                     "the outputs untouched",
                     "long runs are not split"):  # still true of annhip_query_sorted
        assert sentence in flat, sentence


def test_the_kernel_header_says_which_call_splits():
    src = open(os.path.join(_lib.CSRC, "ann_sorted_kernels.h")).read()
    assert "Long runs are not split" in src and "long runs ARE split" in src
    for name in ("sorted_set_merge_kernel", "SortedSetArgs", "set_store", "set_runs_kernel", "set_pieces_kernel"):
        assert name in src, name


def test_python_signatures():
    qs = inspect.signature(A.Index.query_sorted_set).parameters
    assert list(qs)[1:] == ["y", "where", "k", "radius", "split", "alias", "ws", "stream"]
    assert all(qs[p].default is None for p in ("k", "radius", "ws", "stream")) and qs["alias"].default is False
    assert qs["split"].default == 0
    assert list(inspect.signature(A.Index.tag_runs_set).parameters)[1:] == ["where"]
    assert list(inspect.signature(A.where_in).parameters) == ["mask", "sets"]
    assert list(inspect.signature(A.normalize_intervals).parameters) == ["off", "lo", "hi"]
    # query_sorted keeps its signature
    assert list(inspect.signature(A.Index.query_sorted).parameters)[1:] == ["y", "where", "k", "radius", "alias", "ws", "stream"]


def test_where_in_builds_the_csr_form():
    mask, off, lo, hi = A.where_in(0xFF, [[3, (1, 2)], [], [(7, 5)]])
    assert mask == 0xFF and off.tolist() == [0, 2, 2, 3] and np.issubdtype(off.dtype, np.integer)
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32 and lo.tolist() == [3, 1, 7] and hi.tolist() == [3, 2, 5]
    for bad in ([[(1, 2, 3)]], [[-1]], [[1 << 32]], [[1.5]], [[True]], [list(range(257))]):
        with pytest.raises(ValueError):
            A.where_in(FULL, bad)
    for off_bad in (np.array([1, 2]), np.array([0, 2, 1]), np.array([0.0, 1.0]), [0, 1], np.array([0, 257])):
        with pytest.raises(ValueError):
            A.normalize_intervals(off_bad, np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32))


def _random_sets(rng, Qn, edge):
    """small value space so that intervals touch, nest, repeat and overlap; with `edge` the space ends at 0xFFFFFFFF"""
    top = 40
    shift = FULL - top if edge else 0
    sets = []
    for q in range(Qn):
        m = int(rng.integers(0, 9))
        a = rng.integers(0, top + 1, size=m)
        b = a + rng.integers(-3, 12, size=m)  # some empty (b < a)
        items = [(int(x) + shift, min(max(int(z), 0), top) + shift) for x, z in zip(a, b)]
        if edge and q % 3 == 0:
            items.insert(int(rng.integers(0, len(items) + 1)), (FULL, FULL))
        if q % 7 == 0:
            items.insert(0, (0, FULL))
        sets.append(items)
    return sets, np.arange(0, top + 1, dtype=np.int64) + shift


@pytest.mark.parametrize("edge", [False, True], ids=["low", "0xFFFFFFFF"])
def test_normalize_intervals_against_set_membership(edge):
    rng = np.random.default_rng(31 + edge)
    sets, space = _random_sets(rng, 200, edge)
    mask, off, lo, hi = A.where_in(FULL, sets)
    nlo, nhi = A.normalize_intervals(off, lo, hi)
    assert nlo.dtype == np.uint32 and nlo.shape == lo.shape
    probe = np.unique(np.concatenate([space, [0, 1, FULL - 1, FULL]]))
    for q, items in enumerate(sets):
        a, b = int(off[q]), int(off[q + 1])
        raw = np.zeros(probe.size, dtype=np.int64)
        for l, h in items:
            raw += (probe >= l) & (probe <= h)
        cover = np.zeros(probe.size, dtype=np.int64)
        live = []
        for l, h in zip(nlo[a:b].tolist(), nhi[a:b].tolist()):
            if l <= h:
                cover += (probe >= l) & (probe <= h)
                live.append((l, h))
            else:
                assert (l, h) == (1, 0)  # the one spelling of an emptied slot
        assert np.array_equal(cover, (raw > 0).astype(np.int64)), (q, items)  # the same union, every value once
        assert live == sorted(live) and all(x[1] < y[0] for x, y in zip(live, live[1:])), (q, live)  # ascending, disjoint
        for l, h in live:  # every survivor ends where an input interval ends
            assert any(h == hh and l >= ll for ll, hh in items)


def test_the_piece_model():
    start = np.array([0, 10, 64, 100, 5, 0, 127], dtype=np.int64)
    length = np.array([0, 5, 64, 200, 59, 300, 2], dtype=np.int64)
    slot, ps, pe = A.set_pieces(start, length, 0)
    assert slot.tolist() == list(range(7)) and ps.tolist() == start.tolist() and pe.tolist() == (start + length).tolist()
    slot, ps, pe = A.set_pieces(start, length, 64)
    want = [(1, 10, 15), (2, 64, 128), (3, 100, 128), (3, 128, 192), (3, 192, 256), (3, 256, 300), (4, 5, 64),
            (5, 0, 64), (5, 64, 128), (5, 128, 192), (5, 192, 256), (5, 256, 300), (6, 127, 128), (6, 128, 129)]
    assert list(zip(slot.tolist(), ps.tolist(), pe.tolist())) == want
    rng = np.random.default_rng(5)
    for S in (64, 100, 4096):
        s = rng.integers(0, 5000, size=300)
        n = rng.integers(0, 700, size=300)
        slot, ps, pe = A.set_pieces(s, n, S)
        assert (pe > ps).all() and ((pe - 1) // S == ps // S).all()  # non-empty, inside one global block
        assert np.array_equal(np.bincount(slot, weights=pe - ps, minlength=300).astype(np.int64), n)  # a partition of the run
        first = np.r_[True, slot[1:] != slot[:-1]]
        assert (ps[~first] % S == 0).all() and (ps[~first] == pe[:-1][~first[1:]]).all()  # later pieces start on a multiple of S, where the previous one ends
        huge = A.set_pieces(s, n, 1 << 31)
        assert huge[0].size == int((n > 0).sum())
