"""CPU-only: the range predicates on the tag word (include/ann_hip.h) exist in both libraries and in the Python package,
and order_key keeps the order of the columns it maps (no compute calls on a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib

SYMS = {"annhip_query_between": (C.c_long, 14), "annhip_index_exact_query_between": (C.c_int, 12),
        "annhip_exact_knn_between": (C.c_int, 14)}


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_between_symbols_are_exported(prec):
    lib = _lib.load(prec)
    for sym, (restype, nargs) in SYMS.items():
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).restype is restype, sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym


def test_header_declares_every_symbol_and_states_the_predicate():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ann_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym, (restype, nargs) in SYMS.items():
        m = re.search(r"\b(long|int)\s+%s\s*\(([^;{]*)\)\s*;" % sym, code)
        assert m, sym
        assert m.group(1) == ("long" if restype is C.c_long else "int"), sym
        assert len(m.group(2).split(",")) == nargs, sym  # the binding's argument count is the declaration's
    assert "qlo[q] <= (tags[i] & qmask[q]) <= qhi[q]" in src
    assert re.search(r"qlo\[q\] == qhi\[q\]\s+the row of the pair-form call", src)
    assert "(tags[i] & qmask[q]) == qvalue[q]" in src  # the pair form's sentence stays


def _increasing(keys, values):
    """keys ascend with values, and rise exactly where the values do."""
    k = keys.astype(np.int64)
    return np.all(np.diff(k) >= 0) and np.array_equal(np.diff(k) > 0, np.diff(values) > 0)


def test_order_key_keeps_the_order():
    rng = np.random.default_rng(5)
    i32 = np.sort(np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 4000), [-2 ** 31, -1, 0, 1, 2 ** 31 - 1]]).astype(np.int32))
    k = A.order_key(i32)
    assert k.dtype == np.uint32 and k.shape == i32.shape and _increasing(k, i32)
    assert np.array_equal(k, i32.view(np.uint32) ^ np.uint32(0x80000000))
    tiny = np.float32(1e-45)  # the smallest subnormal
    f32 = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(1e3),
                          rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                          np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, np.inf, -np.inf, 3.4e38, -3.4e38], dtype=np.float32)])
    f32 = np.sort(f32[~np.isnan(f32)])
    k = A.order_key(f32)
    assert k.dtype == np.uint32 and k.shape == f32.shape and _increasing(k, f32)
    assert A.order_key(np.float32(-0.0)) == A.order_key(np.float32(0.0))  # the two zeros are one value
    assert A.order_key(np.array([-tiny], dtype=np.float32))[0] < A.order_key(np.float32(0.0)) < A.order_key(np.array([tiny], dtype=np.float32))[0]
    assert A.order_key(np.float32(-np.inf)) == 0x007FFFFF and A.order_key(np.float32(np.inf)) == 0xFF800000


def test_order_key_refuses_nan_and_other_dtypes():
    for bad in (np.array([1.0, np.nan], dtype=np.float32), np.arange(3, dtype=np.float64), np.arange(3, dtype=np.int64),
                np.arange(3, dtype=np.uint32), [1.0, 2.0], 3):
        with pytest.raises(ValueError):
            A.order_key(bad)
