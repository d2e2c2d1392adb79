"""CPU-only: the row-layout code the query launchers dispatch for a row length d (annhip_layout_code: layout_code()
looked up through the layout table of approximatenn_amd/csrc/ann_host.hip), pinned in both libraries (no compute calls)."""
import pytest

from approximatenn_amd import _lib
from tests.test_gpu_exact_knn import SWEEP
from tests.test_gpu_probe import RANKING_D, RANKING_MORE
from tests.test_gpu_rows_f16 import LAYOUTS

UNALIGNED, FOLD2, FOLD3, FOLD4, FOLD4G, FOLD5G = -241, -243, -244, -245, -246, -247  # ANN_D_* (ann_device.h)
INT_MIN = -(2 ** 31)

# f32: the layouts tests/test_gpu_rows_f16.py runs, d -> code
F32 = {128: 128, 80: -84, 96: -100, 160: -164, 192: -104, 320: -168, 384: -200, 24: -50, 48: -52, 28: -1, 280: -2,
       112: -4, 224: -8, 100: FOLD3, 70: FOLD3, 50: FOLD2, 36: FOLD2, 150: FOLD4, 30: UNALIGNED, 260: FOLD4G,
       300: FOLD5G, 2084: 0}
# f64: a row length per code (ANN_VEC = 2: the same chunk counts at half the d; no 1024, no ANN_D_FOLD4)
F64 = {128: 128, 512: 512, 1024: -8, 40: -84, 80: -164, 48: -100, 96: -104, 160: -168, 192: -200, 12: -50, 24: -52,
       20: -82, 14: -1, 28: -2, 56: -4, 112: -8, 100: FOLD3, 36: FOLD2, 33: UNALIGNED, 150: FOLD4G, 300: FOLD5G, 2084: 0}


def _codes(prec, ds):
    lib = _lib.load(prec)
    return {d: lib.annhip_layout_code(d) for d in ds}


def test_f32_codes_of_the_f16_row_layouts():
    assert sorted(F32) == sorted(d for d, _ in LAYOUTS)
    assert _codes("f32", F32) == F32


def test_f64_codes():
    assert _codes("f64", F64) == F64


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_sweep_list_has_a_row_length_for_every_code(prec):
    """tests/test_gpu_exact_knn.py::SWEEP is the case list of the per-layout GPU sweeps: every code that any row length
    dispatches to must have a row length in it."""
    every = set(_codes(prec, range(1, 4097)).values())
    swept = set(_codes(prec, SWEEP[prec]).values())
    assert every == swept, "codes without a row length in SWEEP[%s]: %s" % (prec, sorted(every - swept))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_probe_ranking_list_has_one_row_length_for_every_code(prec):
    """tests/test_gpu_probe.py::test_ranking_is_the_smallest_projection_magnitudes runs RANKING_D + RANKING_MORE[prec]."""
    ds = RANKING_D + RANKING_MORE[prec]
    codes = _codes(prec, ds)
    assert set(codes.values()) == set(_codes(prec, range(1, 4097)).values())
    assert len(set(codes.values())) == len(ds), "two row lengths of one code: %s" % sorted(codes.items())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_every_row_length_has_kernels(prec):
    missing = [d for d, c in _codes(prec, range(1, 4097)).items() if c == INT_MIN]
    assert not missing, "row lengths without a layout-table entry: %s" % missing[:20]
