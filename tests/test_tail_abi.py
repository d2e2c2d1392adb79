"""CPU-only: rows appended to a built index (annhip_index_append, annhip_index_reserve_tail, annhip_index_tail,
annhip_index_copy_rows, annhip_index_drop_tail; include/ann_hip.h) exist in both libraries and in the Python package (no
compute calls on a device)."""
import ctypes as C
import inspect
import os

import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib

SYMS = ("annhip_index_append", "annhip_index_reserve_tail", "annhip_index_tail", "annhip_index_copy_rows",
        "annhip_index_drop_tail")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_tail_symbols_are_exported_with_declared_types(prec):
    lib = _lib.load(prec)
    for sym in SYMS + ("annhip_index_fixed", "annhip_index_copy_words"):
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes is not None
    assert lib.annhip_index_append.restype is C.c_int and len(lib.annhip_index_append.argtypes) == 6
    assert lib.annhip_index_reserve_tail.restype is C.c_int and len(lib.annhip_index_reserve_tail.argtypes) == 2
    assert lib.annhip_index_tail.restype is C.c_size_t and len(lib.annhip_index_tail.argtypes) == 1
    assert lib.annhip_index_copy_rows.restype is C.c_int and len(lib.annhip_index_copy_rows.argtypes) == 4
    assert lib.annhip_index_drop_tail.restype is C.c_int and len(lib.annhip_index_drop_tail.argtypes) == 1


def test_python_interface_exists():
    for name in ("append", "reserve_tail", "drop_tail", "rows_tensor", "compact"):
        assert callable(getattr(A.Index, name)), name
    assert isinstance(A.Index.tail, property) and isinstance(A.Index.n_total, property)
    assert inspect.signature(A.Index.append).parameters["tags"].default is None
    assert "tries" in inspect.signature(A.Index.compact).parameters


def test_header_declares_every_symbol_and_states_the_contract():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    for sym in SYMS:
        assert sym + "(" in src
    for phrase in ("tail row j has id n + j", "padded with (n_total, +inf)", "With m == 0 every entry point launches exactly",
                   "annhip_index_reshard drops the tail", "these never see the tail", "narrow rows and a tail do not compose"):
        assert phrase in src, phrase
