"""CPU-only: the allow-list row filter (include/ann_hip.h) exists in both libraries and in the Python package, and the
numpy packing helper writes the bitmap format the library reads (no compute calls on a device)."""
import inspect
import os

import numpy as np
import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib, api

SYMS = ("annhip_index_set_filter", "annhip_index_filter_count", "annhip_filter_pack", "annhip_exact_knn_filtered")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_filter_symbols_are_exported(prec):
    lib = _lib.load(prec)
    for sym in SYMS:
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).restype is not None  # return codes / the count, declared
        assert getattr(lib, sym).argtypes is not None


def test_python_interface_exists():
    assert callable(A.Index.set_filter)
    assert isinstance(A.Index.filter_count, property)
    assert "allow" in inspect.signature(api.exact_knn).parameters
    assert inspect.signature(api.exact_knn).parameters["allow"].default is None


def test_header_declares_every_symbol():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    for sym in SYMS:
        assert sym + "(" in src
    assert "bits[i >> 5] >> (i & 31) & 1" in src


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_numpy_packing_puts_row_i_at_bit_i_of_its_word(n):
    rng = np.random.default_rng(n)
    for mask in (rng.random(n) < 0.5, np.ones(n, dtype=bool), np.zeros(n, dtype=bool)):
        words = api.pack_allow(mask)
        assert words.dtype == np.uint32 and words.shape == ((n + 31) // 32,)
        want = [0] * ((n + 31) // 32)
        for i in range(n):
            if mask[i]:
                want[i >> 5] |= 1 << (i & 31)
        assert [int(w) for w in words] == want  # (the tail bits of the last word are zero)
        for i in range(n):
            assert (int(words[i >> 5]) >> (i & 31)) & 1 == int(mask[i])
