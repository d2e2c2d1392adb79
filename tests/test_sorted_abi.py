"""CPU-only: the tag order and the sorted scan (include/ann_hip.h) exist in both libraries and in the Python package, and
the header states their contract (no compute calls on a device)."""
import ctypes as C
import inspect
import os
import re

import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib

SYMS = {"annhip_index_sort_tags": (C.c_int, "int", 2), "annhip_index_tag_order": (C.c_size_t, "size_t", 2),
        "annhip_tag_runs": (C.c_int, "int", 7), "annhip_query_sorted": (C.c_long, "long", 13)}


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sorted_symbols_are_exported(prec):
    lib = _lib.load(prec)
    for sym, (restype, _, nargs) in SYMS.items():
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).restype is restype, sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    assert lib.annhip_index_sort_tags.argtypes[1] is C.c_uint32


def test_header_declares_every_symbol_and_states_the_contract():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym, (_, ctype, nargs) in SYMS.items():
        m = re.search(r"\b(long|int|size_t)\s+%s\s*\(([^;{]*)\)\s*;" % sym, code)
        assert m, sym
        assert m.group(1) == ctype, sym
        assert len(m.group(2).split(",")) == nargs, sym  # the binding's argument count is the declaration's
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for sentence in ("ordered by (tags[id] & field_mask, id)",
                     "Equal masked words are ordered by id".lower(),
                     "field_mask == 0 drops the order",
                     "start = lower_bound(keys, qlo)",
                     "len = upper_bound(keys, qhi) - start",
                     "(0, 0) where qlo > qhi",
                     "padded with (n_total, +inf)",
                     "qlo[q] <= (tags[i] & field_mask) <= qhi[q]",
                     "row q is left out for query q when aliased",
                     "on the NATIVE rows",
                     "annhip_radius_trim's rule and counts apply",
                     "nothing launched and the outputs untouched",
                     "one order and one mask per index",
                     "native rows only",
                     "the order is not saved in index files",
                     "parity mode, sharded indexes and annhip_stream_* do not use it",
                     "long runs are not split"):
        assert sentence in flat or sentence in flat.lower(), sentence
    for keeps in ("annhip_index_set_filter", "annhip_index_append"):
        assert re.search(r"Keeps the order:[^.]*%s" % keeps, flat), keeps
    for drops in ("annhip_index_set_tags", "annhip_index_drop_tail", "annhip_index_reshard"):
        assert re.search(r"Drops the order:[^;]*%s" % drops, flat), drops


def test_the_kernel_header_states_the_known_limit():
    src = open(os.path.join(_lib.CSRC, "ann_sorted_kernels.h")).read()
    assert "Long runs are not split" in src and "sorted_scan_generic_kernel" in src


def test_index_methods_and_properties_exist():
    for name in ("sort_tags", "tag_runs", "query_sorted", "query_routed"):
        assert callable(getattr(A.Index, name)), name
    assert isinstance(A.Index.tag_order, property)
    assert inspect.signature(A.Index.sort_tags).parameters["mask"].default == 0xFFFFFFFF
    q = inspect.signature(A.Index.query_routed).parameters
    assert list(q)[1:4] == ["y", "where", "scan_below"] and q["scan_below"].default is None
    qs = inspect.signature(A.Index.query_sorted).parameters
    assert list(qs)[1:] == ["y", "where", "k", "radius", "alias", "ws", "stream"]
    assert all(qs[p].default is None for p in ("k", "radius", "ws", "stream")) and qs["alias"].default is False
