"""CPU-only: the opt-in binary32 point rows of the f64 library (annhip_index_set_rows with ANNHIP_ROWS_F32): the header's
constant, the Python per-precision table of names, and the two symbols in both libraries (no compute calls)."""
import os
import re

import pytest

from approximatenn_amd import _lib
from approximatenn_amd.api import Index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constants():
    src = open(os.path.join(ROOT, "include", "ann_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+ANNHIP_ROWS_(\w+)\s+(\d+)\s*$", src, re.M)}


def test_header_defines_f32_rows_as_2():
    assert _header_constants() == {"NATIVE": 0, "F16": 1, "F32": 2}


def test_python_table_matches_the_header():
    c = _header_constants()
    assert Index.ROWS_BY_PREC == {"f32": {"native": c["NATIVE"], "f16": c["F16"]},
                                  "f64": {"native": c["NATIVE"], "f32": c["F32"]}}
    assert Index.ROWS == {"native": 0, "f16": 1}  # the f32 index's names, as before
    assert Index.ROWS_BY_PREC["f32"] == Index.ROWS


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rows_symbols_still_exported(prec):
    _lib.build()
    lib = _lib.load(prec)
    for sym in ("annhip_index_set_rows", "annhip_index_rows"):
        assert hasattr(lib, sym), sym
        assert sym in _lib.EXPORTED, sym
