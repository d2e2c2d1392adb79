"""CPU-only: the radius entry points (annhip_query_radius, annhip_index_exact_query_radius, annhip_radius_trim) exist in both
libraries, in the binding list and in the header; the Python names and defaults exist; radius_recall on hand-made tensors.
No device call."""
import inspect
import os
import re

import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"annhip_query_radius": ("c_long", 13), "annhip_index_exact_query_radius": ("c_int", 11),
           "annhip_radius_trim": ("c_int", 8)}


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_both_libraries_export_the_three_symbols(prec):
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
    assert "with radius[q] = +inf the row is, bit for bit, the row of annhip_query_k(kq = kcap)" in text
    assert "with kcap == kg as well, it is the row of the plain fixed-mode call" in text


def test_python_names_and_defaults():
    p = inspect.signature(A.Index.query_radius).parameters
    assert list(p) == ["self", "y", "radius", "k", "alias", "where", "ws", "stream"]
    assert p["k"].default is None and p["alias"].default is False
    assert p["where"].default is None and p["ws"].default is None and p["stream"].default is None
    assert p["radius"].default is inspect.Parameter.empty
    p = inspect.signature(A.Index.exact_query_radius).parameters
    assert list(p) == ["self", "y", "radius", "k", "alias", "where"]
    assert p["k"].default is inspect.Parameter.empty and p["alias"].default is False and p["where"].default is None
    assert list(inspect.signature(A.radius_trim).parameters) == ["ids", "dists", "radius", "pad_id"]
    assert list(inspect.signature(A.radius_recall).parameters) == ["guess_ids", "guess_counts", "truth_ids", "truth_counts"]
    # the existing signatures stay as they are
    assert list(inspect.signature(A.Index.query).parameters) == ["self", "y", "alias", "mode", "out_ids", "out_dists", "ws",
                                                                 "stream", "where", "k"]
    assert list(inspect.signature(A.Index.exact_query).parameters) == ["self", "y", "alias", "where", "k"]


def test_radius_recall_on_hand_made_tensors():
    pad = 99
    truth = torch.tensor([[1, 2, 3, 4], [5, 6, pad, pad], [pad, pad, pad, pad], [7, pad, pad, pad]])
    tcnt = torch.tensor([4, 2, 0, 1], dtype=torch.int32)
    guess = torch.tensor([[2, 4, 9, pad, pad], [5, 6, pad, pad, pad], [8, pad, pad, pad, pad], [pad, pad, pad, pad, pad]])
    gcnt = torch.tensor([3, 2, 1, 0], dtype=torch.int32)
    rec, counted = A.radius_recall(guess, gcnt, truth, tcnt)
    assert counted == 3  # the query without a true hit is not counted, whatever was guessed for it
    assert rec == pytest.approx((2 / 4 + 2 / 2 + 0 / 1) / 3, abs=1e-15)
    # entries behind the counts never match, not even equal ids (pads, or stale entries)
    guess2 = torch.tensor([[1, 2, 3, 4, 0]] * 4)
    rec, counted = A.radius_recall(guess2, torch.tensor([2, 0, 0, 0]), truth, tcnt)
    assert counted == 3 and rec == pytest.approx((2 / 4) / 3, abs=1e-15)
    truth3 = torch.tensor([[1, 2, 3, 4]])
    rec, counted = A.radius_recall(torch.tensor([[4, 3, 2, 1]]), torch.tensor([4]), truth3, torch.tensor([2]))
    assert counted == 1 and rec == 1.0  # only truth[:2] = {1, 2} is asked for
    assert A.radius_recall(guess, gcnt, truth, torch.zeros(4, dtype=torch.int32)) == (0.0, 0)
