"""CPU-only: the hashed tail's two exports (annhip_index_hash_tail, annhip_index_tail_hashed) are in both backend
libraries, in the header and in the bindings, and the Python Index carries hash_tail / tail_hashed.  No compute calls."""
import ctypes as C
import os
import re

import pytest

from approximatenn_amd import _lib
from approximatenn_amd.api import Index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("annhip_index_hash_tail", "annhip_index_tail_hashed")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_both_libraries_export_the_symbols(prec):
    raw = C.CDLL(os.path.join(ROOT, "approximatenn_amd", "csrc", "libapproxnn_hip_%s.so" % prec))
    for name in NEW:
        assert hasattr(raw, name), name


def test_the_header_declares_them():
    src = open(os.path.join(ROOT, "include", "ann_hip.h")).read()
    assert re.search(r"\bint\s+annhip_index_hash_tail\s*\(\s*annhip_index\s*\*\s*ix\s*\)\s*;", src)
    assert re.search(r"\bsize_t\s+annhip_index_tail_hashed\s*\(\s*const\s+annhip_index\s*\*\s*ix\s*\)\s*;", src)
    for name in NEW:
        assert name in _lib.EXPORTED


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_bindings_carry_types(prec):
    lib = _lib.load(prec)
    assert lib.annhip_index_hash_tail.restype is C.c_int
    assert list(lib.annhip_index_hash_tail.argtypes) == [C.c_void_p]
    assert lib.annhip_index_tail_hashed.restype is C.c_size_t
    assert list(lib.annhip_index_tail_hashed.argtypes) == [C.c_void_p]


def test_the_index_has_the_method_and_the_property():
    assert callable(Index.hash_tail)
    assert isinstance(Index.tail_hashed, property)
