"""approximatenn_amd -- MI355X-native (gfx950, HIP) backend for approximateNN's precomp()/query() hot path.

The product is the C-ABI shared library under csrc/ (include/*.h); this package is the thin host-side
mirror of the reference's interface used by the tests, the bench and multi-GPU hosts.
"""
from . import _lib
from .api import (HostStream, Index, Save, checksum, collapse, exact_knn, gpu_cleanup, gpu_init, normalize_intervals, order_key, precomp, query,
                  radius_recall, radius_trim, recall_at_k, recall_ranks, recall_summary, rerank, set_pieces, synth_randnorm, where_in)

__all__ = ["HostStream", "Index", "Save", "precomp", "query", "recall_ranks", "recall_summary", "exact_knn", "recall_at_k", "radius_trim", "radius_recall", "rerank", "collapse", "gpu_init", "gpu_cleanup", "synth_randnorm", "checksum", "order_key",
           "where_in", "normalize_intervals", "set_pieces",
           "_lib"]
