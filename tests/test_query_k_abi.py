"""CPU-only: the per-call k of fixed-mode queries and of the exact scan (annhip_query_k, annhip_index_max_query_k,
annhip_index_exact_query_k; include/ann_hip.h) exists in both libraries and in the Python package (no compute calls on a
device)."""
import ctypes as C
import inspect
import os

import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib

SYMS = ("annhip_query_k", "annhip_index_max_query_k", "annhip_index_exact_query_k")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_query_k_symbols_are_exported_with_declared_types(prec):
    lib = _lib.load(prec)
    for sym in SYMS:
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes is not None
    assert lib.annhip_query_k.restype is C.c_long and len(lib.annhip_query_k.argtypes) == 11
    assert lib.annhip_index_max_query_k.restype is C.c_size_t and len(lib.annhip_index_max_query_k.argtypes) == 1
    assert lib.annhip_index_exact_query_k.restype is C.c_int and len(lib.annhip_index_exact_query_k.argtypes) == 9


def test_python_interface_exists():
    for fn in (A.Index.query, A.Index.exact_query):
        assert inspect.signature(fn).parameters["k"].default is None, fn
    assert isinstance(A.Index.max_query_k, property)


def test_header_declares_every_symbol_and_states_the_contract():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    for sym in SYMS:
        assert sym + "(" in src
    assert "kq == kg returns the bits of today's call" in src
