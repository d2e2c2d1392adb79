"""CPU-only: the rerank entry points (annhip_rerank, annhip_index_rerank) exist in both libraries, in the binding list and
in the header; the Python names and defaults exist; the signatures of Index.query and Index.exact_query are unchanged.
No device call."""
import inspect
import os
import re

import pytest

import approximatenn_amd as A
from approximatenn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"annhip_rerank": ("c_int", 11), "annhip_index_rerank": ("c_int", 9)}


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_both_libraries_export_the_two_symbols(prec):
    _lib.build()
    lib = _lib.load(prec)
    for sym, (restype, nargs) in SYMBOLS.items():
        assert hasattr(lib, sym), sym
        fn = getattr(lib, sym)
        assert fn.restype.__name__ == restype and len(fn.argtypes) == nargs, sym


def test_the_binding_list_and_the_header_carry_them():
    src = open(os.path.join(ROOT, "include", "ann_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym, (_, nargs) in SYMBOLS.items():
        assert sym in _lib.EXPORTED, sym
        m = re.search(r"\b%s\s*\(([^;{]*)\)\s*;" % sym, code)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
    text = " ".join(re.sub(r"^\s*\*", " ", src, flags=re.M).split())
    assert "An entry >= rows is skipped and never dereferenced" in text
    assert "ids_dev may be cand_dev itself where ccnt == k" in text


def test_python_names_and_defaults():
    assert "rerank" in A.__all__
    p = inspect.signature(A.rerank).parameters
    assert list(p) == ["points", "y", "cand", "k", "out_ids", "out_dists"]
    assert p["k"].default is inspect.Parameter.empty and p["out_ids"].default is None and p["out_dists"].default is None
    p = inspect.signature(A.Index.rerank).parameters
    assert list(p) == ["self", "y", "cand", "k", "stream", "out_ids", "out_dists"]
    assert all(p[name].default is None for name in ("k", "stream", "out_ids", "out_dists"))
    assert p["cand"].default is inspect.Parameter.empty
    p = inspect.signature(A.Index.query_reranked).parameters
    assert list(p) == ["self", "y", "k", "oversample", "alias", "where", "ws", "stream"]
    assert p["k"].default is None and p["oversample"].default == 2 and p["alias"].default is False
    assert p["where"].default is None and p["ws"].default is None and p["stream"].default is None
    # the existing signatures stay as they are
    assert list(inspect.signature(A.Index.query).parameters) == ["self", "y", "alias", "mode", "out_ids", "out_dists", "ws",
                                                                 "stream", "where", "k"]
    assert list(inspect.signature(A.Index.exact_query).parameters) == ["self", "y", "alias", "where", "k"]
