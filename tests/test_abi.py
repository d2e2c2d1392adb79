"""CPU-only: the C-ABI libraries load and export every symbol include/*.h declares (no compute calls)."""
import ctypes as C
import os
import re

import pytest

from approximatenn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_backend_exports(prec):
    _lib.build()
    lib = _lib.load(prec)
    assert lib.annhip_precision().decode() == prec
    for sym in _lib.EXPORTED:
        assert hasattr(lib, sym), sym
    disp = C.CDLL(os.path.join(_lib.CSRC, "libann_dispatch_%s.so" % prec))
    for sym in _lib.DISPATCH_EXPORTED:
        assert hasattr(disp, sym), sym


def test_headers_and_bindings_agree():
    """Every function declared in include/{algg,gpu_comp,ann_hip}.h is in the binding list and vice versa."""
    declared = set()
    for h in ("algg.h", "gpu_comp.h", "ann_hip.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        declared |= set(re.findall(r"\b(\w+)\s*\([^;{]*\)\s*;", src))
    declared -= {"defined"}
    assert declared == set(_lib.EXPORTED), declared ^ set(_lib.EXPORTED)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_prune_accessors_are_exported_and_declared(prec):
    """annhip_index_set_prune / annhip_index_prune and the read-only annhip_index_prune_bound (E and K' of the
    certificate): in both libraries, in the binding list, in the header with the documented signature, and on Index."""
    from approximatenn_amd.api import Index
    lib = _lib.load(prec)
    for sym in ("annhip_index_set_prune", "annhip_index_prune", "annhip_index_prune_bound"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED, sym
    assert lib.annhip_index_prune_bound.restype is C.c_int
    assert lib.annhip_index_prune_bound.argtypes[1:] == [C.POINTER(C.c_double), C.POINTER(C.c_int)]
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ann_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+annhip_index_prune_bound\s*\(\s*const\s+annhip_index\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,"
                     r"\s*int\s*\*\s*\w+\s*\)\s*;", code)
    assert isinstance(Index.prune_bound, property) and Index.prune_bound.fset is None


def test_save_t_layout_matches_reference_abi():
    # ann.h:8-12: int, 4 size_t, 3 pointers, 2 pointers -> 80 bytes on LP64
    assert C.sizeof(_lib.SaveT) == 80
    assert _lib.SaveT.n.offset == 8 and _lib.SaveT.which_par.offset == 40 and _lib.SaveT.bases.offset == 72


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_synth_randnorm_is_the_reference_drivers_stream(prec):
    """annhip_synth_randnorm (host-only, threads for the libm part) against the oracle's serial generator -- which is
    pinned to the reference's rand_norm/genRand by the golden point sets (tests/test_oracle_golden.py): same values bit for bit, same number of
    random() draws, the pending second value of an odd-length call carried into the next call."""
    import numpy as np

    import approximatenn_amd as A
    from oracle import oracle_py as O
    orc = O.CpuBackend(prec, "oracle")
    for counts in ([7, 1, 2, 5], [100001, 3, 20000], [4096 * 2 * 3 + 1, 10]):
        O.srandom(77)
        orc.rand_norm_reset()
        want = [orc.gen_rand(c) for c in counts]
        after_want = O.libc_random()
        O.srandom(77)
        got = [A.synth_randnorm(c, prec, reset=(i == 0)) for i, c in enumerate(counts)]
        after_got = O.libc_random()
        for a, b in zip(want, got):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert after_want == after_got
