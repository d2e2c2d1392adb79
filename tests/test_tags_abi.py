"""CPU-only: the per-query tag predicates (include/ann_hip.h) exist in both libraries and in the Python package (no
compute calls on a device)."""
import inspect
import os

import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib, api

SYMS = ("annhip_index_set_tags", "annhip_index_has_tags", "annhip_query_tagged", "annhip_exact_knn_tagged",
        "annhip_index_exact_query_tagged")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_tag_symbols_are_exported(prec):
    lib = _lib.load(prec)
    for sym in SYMS:
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).restype is not None  # return codes, declared
        assert getattr(lib, sym).argtypes is not None


def test_python_interface_exists():
    assert callable(A.Index.set_tags)
    assert isinstance(A.Index.has_tags, property)
    for fn in (A.Index.query, A.Index.exact_query, api.exact_knn):
        assert inspect.signature(fn).parameters["where"].default is None, fn
    assert inspect.signature(api.exact_knn).parameters["tags"].default is None
    assert inspect.signature(api.exact_knn).parameters["allow"].default is None  # still there: ANDed with the tag test


def test_header_declares_every_symbol_and_states_the_predicate():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    for sym in SYMS:
        assert sym + "(" in src
    assert "(tags[i] & qmask[q]) == qvalue[q]" in src
