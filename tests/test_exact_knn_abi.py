"""CPU-only: the exact k-nearest-neighbour interface exists in both libraries and in the Python package, and recall_at_k
computes the standard recall@k (no compute calls on a device)."""
import pytest
import torch

import approximatenn_amd as A
from approximatenn_amd import _lib

SYMS = ("annhip_exact_knn", "annhip_exact_knn_host", "annhip_index_exact_query")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_exact_knn_symbols_are_exported(prec):
    lib = _lib.load(prec)
    for sym in SYMS:
        assert sym in _lib.EXPORTED
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).restype is not None  # int return codes, declared


def test_python_interface_exists():
    assert callable(A.exact_knn) and callable(A.recall_at_k) and callable(A.Index.exact_query)
    assert "exact_knn" in A.__all__ and "recall_at_k" in A.__all__


def test_recall_at_k_by_hand():
    n = 100
    truth = torch.tensor([[1, 2, 3, 4], [10, 11, 12, 13], [20, 21, 22, 23]], dtype=torch.int64)
    guess = torch.tensor([[4, 3, 2, 1],          # a permuted row: 4 of 4
                          [10, n + 5, 99, 13],   # an id >= n (query()'s "no neighbour") and a wrong one: 2 of 4
                          [7, 8, 9, 20]],        # 1 of 4
                         dtype=torch.int64)
    assert A.recall_at_k(guess, truth) == pytest.approx((4 / 4 + 2 / 4 + 1 / 4) / 3, abs=1e-15)
    assert A.recall_at_k(truth, truth) == 1.0
    assert A.recall_at_k(truth + 1000, truth) == 0.0
    # a guess list longer than the truth (k' > k) and one with a repeated id: set overlap, still over k
    wide = torch.tensor([[9, 1, 9, 2, 3, 3]], dtype=torch.int64)
    assert A.recall_at_k(wide, truth[:1]) == pytest.approx(3 / 4, abs=1e-15)


def test_refusals_need_no_device():
    """The preconditions are checked on the host before anything touches a device: null pointers are never read."""
    for prec in ("f32", "f64"):
        lib = _lib.load(prec)
        assert lib.annhip_exact_knn(10, 4, 0, None, 3, None, 0, None, None) != 0      # k = 0
        assert lib.annhip_exact_knn(2000, 4, 1025, None, 3, None, 0, None, None) != 0  # k > 1024
        assert lib.annhip_exact_knn(10, 4, 11, None, 3, None, 0, None, None) != 0     # k > n
        assert lib.annhip_exact_knn(10, 4, 10, None, 3, None, 1, None, None) != 0     # k = n with self
        assert lib.annhip_exact_knn(0xFFFFFFF0, 4, 1, None, 3, None, 0, None, None) != 0
        assert lib.annhip_exact_knn(10, 4, 10, None, 0, None, 0, None, None) == 0     # ycnt = 0: nothing to do
