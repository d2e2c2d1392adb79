"""CPU-only: the probe setting of fixed mode (include/ann_hip.h) exists in both libraries and in the Python package (no
compute calls on a device)."""
import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib

SYMS = ("annhip_index_set_probe", "annhip_index_probe", "annhip_probe_bits")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_probe_symbols_are_exported(prec):
    lib = _lib.load(prec)
    for sym in SYMS:
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).restype is not None  # int return codes, declared


def test_python_interface_exists():
    assert callable(A.Index.set_probe) and callable(A.Index.probe_bits)
    assert isinstance(A.Index.probe, property)


def test_header_states_the_contract():
    import os
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    assert "ANNHIP_PROBE_ALL = -1" in src
    for sym in SYMS:
        assert sym + "(" in src
