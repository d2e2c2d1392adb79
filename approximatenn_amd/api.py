"""Host-side mirror of the reference's operator interface for the precomp/query path.

Names and argument meaning follow /root/reference/ann.h:46-49,61-62 (precomp, query, save_t, free_save); the
numpy arrays stand where the reference takes malloc'd C arrays.  Everything runs through the C-ABI of
csrc/libapproxnn_hip_{f32,f64}.so -- there is no Python or CPU implementation of the path in this package.

    save = Save.from_arrays(...)            # or: ids, dists, save = precomp(points, k, ...)
    ids, dists = query(save, points, y)     # drop-in symbols precomp_gpu / query_gpu (host pointers)
    ix = Index.from_save(save, points)      # resident index (HBM) for repeated queries
    ids, dists = ix.query(y_torch)          # device tensors in, device tensors out
"""
import ctypes as C

import numpy as np

from . import _lib

_libc = C.CDLL("libc.so.6")
_libc.free.argtypes = [C.c_void_p]


def _ft(prec):
    return np.float32 if prec == "f32" else np.float64


def _prec_of(arr):
    if arr.dtype == np.float32:
        return "f32"
    if arr.dtype == np.float64:
        return "f64"
    raise TypeError("points must be float32 (USE_FLOAT build) or float64 (stock build), got %s" % arr.dtype)


class Save:
    """A save_t (include/ann.h).  Either owns numpy-backed memory or wraps a malloc'd struct the library filled."""

    def __init__(self, prec):
        self.prec = prec
        self.c = _lib.SaveT()
        self._keep = None
        self._malloced = False

    @classmethod
    def from_arrays(cls, prec, tries, n, k, d_short, d_long, which_par, par_maxes, graph, row_means, bases):
        s = cls(prec)
        ft = _ft(prec)
        wp = [np.ascontiguousarray(w, dtype=np.uint64) for w in which_par]
        pm = np.ascontiguousarray(par_maxes, dtype=np.uint64)
        gr = np.ascontiguousarray(graph, dtype=np.uint64)
        rm = np.ascontiguousarray(row_means, dtype=ft)
        bs = np.ascontiguousarray(bases, dtype=ft)
        ptrs = (C.POINTER(C.c_size_t) * int(tries))(*[w.ctypes.data_as(C.POINTER(C.c_size_t)) for w in wp])
        s._keep = (wp, pm, gr, rm, bs, ptrs)
        s.c.tries = int(tries)
        s.c.n, s.c.k, s.c.d_short, s.c.d_long = int(n), int(k), int(d_short), int(d_long)
        s.c.which_par = C.cast(ptrs, C.POINTER(C.POINTER(C.c_size_t)))
        s.c.par_maxes = pm.ctypes.data_as(C.POINTER(C.c_size_t))
        s.c.graph = gr.ctypes.data_as(C.POINTER(C.c_size_t))
        s.c.row_means = rm.ctypes.data
        s.c.bases = bs.ctypes.data
        return s

    @classmethod
    def from_dict(cls, prec, a):
        return cls.from_arrays(prec, a["tries"], a["n"], a["k"], a["d_short"], a["d_long"], a["which_par"],
                               a["par_maxes"], a["graph"], a["row_means"], a["bases"])

    def to_dict(self):
        """Deep copy of every field into numpy arrays."""
        c, ft = self.c, _ft(self.prec)
        T, n, k, ds, d = c.tries, c.n, c.k, c.d_short, c.d_long
        pm = np.ctypeslib.as_array(c.par_maxes, shape=(T,)).copy()
        cft = np.ctypeslib.as_ctypes_type(ft)
        return dict(tries=T, n=n, k=k, d_short=ds, d_long=d, par_maxes=pm.astype(np.uint64),
                    graph=np.ctypeslib.as_array(c.graph, shape=(n, k)).copy().astype(np.uint64),
                    which_par=[np.ctypeslib.as_array(c.which_par[t], shape=(1 << ds, int(pm[t]))).copy().astype(np.uint64)
                               for t in range(T)],
                    row_means=np.ctypeslib.as_array(C.cast(c.row_means, C.POINTER(cft)), shape=(d,)).copy(),
                    bases=np.ctypeslib.as_array(C.cast(c.bases, C.POINTER(cft)), shape=(T, ds, d)).copy())

    def write(self, path):
        """annhip_save_write: one checksummed index file (include/ann_hip.h)."""
        if _lib.load(self.prec).annhip_save_write(C.byref(self.c), str(path).encode()) != 0:
            raise OSError("could not write index file %s" % path)

    @classmethod
    def read(cls, prec, path):
        """annhip_save_read: load an index file written by the same-precision library."""
        s = cls(prec)
        if _lib.load(prec).annhip_save_read(str(path).encode(), C.byref(s.c)) != 0:
            raise OSError("could not read index file %s" % path)
        s._malloced = True
        return s

    def free(self):
        """free_save (/root/reference/ann.c:25-34) for library-filled structs."""
        if self._malloced:
            for t in range(self.c.tries):
                _libc.free(C.cast(self.c.which_par[t], C.c_void_p))
            for p in (self.c.which_par, self.c.par_maxes, self.c.graph):
                _libc.free(C.cast(p, C.c_void_p))
            _libc.free(self.c.row_means)
            _libc.free(self.c.bases)
            self._malloced = False


def _take(ptr, count, ctype, dtype):
    out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(count,)).copy().astype(dtype)
    _libc.free(C.cast(ptr, C.c_void_p))
    return out


def gpu_init(prec="f32"):
    _lib.load(prec).gpu_init()


def gpu_cleanup(prec="f32"):
    _lib.load(prec).gpu_cleanup()


def precomp(points, k, tries=10, rots_before=6, rot_len_before=1, rots_after=1, rot_len_after=1, want_save=True):
    """precomp_gpu (include/algg.h; /root/reference/algg.h:7-11).  Returns (ids[n,k], sq_dists[n,k], Save|None).
    Draws its random rotations from libc random(): call srandom() first for a reproducible index."""
    points = np.ascontiguousarray(points)
    prec = _prec_of(points)
    lib = _lib.load(prec)
    n, d = points.shape
    save = Save(prec) if want_save else None
    dptr = C.c_void_p()
    ids = lib.precomp_gpu(n, k, d, points.ctypes.data, tries, rots_before, rot_len_before, rots_after, rot_len_after,
                          C.byref(save.c) if want_save else None, C.byref(dptr))
    if want_save:
        save._malloced = True
        save._points_ref = points  # the residency cache is keyed on this host pointer
    cft = C.c_float if prec == "f32" else C.c_double
    return (_take(ids, n * k, C.c_size_t, np.uint64).reshape(n, k),
            _take(dptr, n * k, cft, _ft(prec)).reshape(n, k), save)


def query(save, points, y, want_dists=True):
    """query_gpu (include/algg.h; /root/reference/algg.h:5-6).  `y is points` (same buffer) excludes self."""
    points = np.ascontiguousarray(points)
    prec = _prec_of(points)
    assert prec == save.prec
    lib = _lib.load(prec)
    if y is points or (isinstance(y, np.ndarray) and y.ctypes.data == points.ctypes.data):
        yy = points[: len(y)]
    else:
        yy = np.ascontiguousarray(y, dtype=points.dtype)
    ycnt, k = yy.shape[0], int(save.c.k)
    dptr = C.c_void_p()
    ids = lib.query_gpu(C.byref(save.c), points.ctypes.data, ycnt, yy.ctypes.data, C.byref(dptr) if want_dists else None)
    cft = C.c_float if prec == "f32" else C.c_double
    ids = _take(ids, ycnt * k, C.c_size_t, np.uint64).reshape(ycnt, k)
    if not want_dists:
        return ids, None
    return ids, _take(dptr, ycnt * k, cft, _ft(prec)).reshape(ycnt, k)


def synth_randnorm(count, prec="f32", reset=False):
    """annhip_synth_randnorm: `count` N(0,1) values from the caller's libc random() stream, exactly the values the
    reference's drivers generate (time_results.c:10-13, randNorm.c:9-21).  Seed with libc srandom() first."""
    lib = _lib.load(prec)
    if reset:
        lib.annhip_synth_reset()
    out = np.empty(int(count), dtype=_ft(prec))
    lib.annhip_synth_randnorm(int(count), out.ctypes.data)
    return out


class HostStream:
    """annhip_stream_*: numpy batches in, numpy results out, up to `lanes` batches in flight.

        hs = ix.host_stream(max_ycnt=10000, lanes=3)
        for ids, dists in hs.map(batches):      # results in submission order
            ...
    """

    def __init__(self, ix, max_ycnt, lanes=3):
        self.ix, self.lib, self.lanes = ix, ix.lib, lanes
        self.h = self.lib.annhip_stream_open(ix.h, max_ycnt, lanes)
        self.ft = _ft(ix.prec)
        self._pending = {}

    def submit(self, y, alias=False):
        y = np.ascontiguousarray(y, dtype=self.ft)
        t = self.lib.annhip_stream_submit(self.h, y.shape[0], y.ctypes.data, int(alias))
        if t >= 0:
            self._pending[t] = y.shape[0]
        return t

    def collect(self, ticket):
        n = self._pending.pop(ticket)
        ids = np.empty((n, self.ix.k), dtype=np.uint64)
        dists = np.empty((n, self.ix.k), dtype=self.ft)
        if self.lib.annhip_stream_collect(self.h, ticket, ids.ctypes.data, dists.ctypes.data) != 0:
            raise RuntimeError("unknown ticket %d" % ticket)
        return ids, dists

    def map(self, batches, alias=False):
        inflight = []
        for y in batches:
            if len(inflight) == self.lanes:
                yield self.collect(inflight.pop(0))
            t = self.submit(y, alias)
            assert t >= 0
            inflight.append(t)
        while inflight:
            yield self.collect(inflight.pop(0))

    def close(self):
        if self.h:
            self.lib.annhip_stream_close(self.h)
            self.h = None


def recall_ranks(points, y, guess, self_exclude=False):
    """annhip_recall_ranks: torch device tensors points [n,d], y [Q,d], guess int64 [Q,k] -> int64 ranks [Q,k]
    (number of points strictly closer than each guessed neighbour)."""
    import torch
    prec = "f32" if points.dtype == torch.float32 else "f64"
    lib = _lib.load(prec)
    assert points.is_cuda and y.is_cuda and guess.is_cuda and guess.dtype == torch.int64
    points, y, guess = points.contiguous(), y.contiguous(), guess.contiguous()
    ranks = torch.empty(guess.shape, dtype=torch.int64, device=guess.device)
    lib.annhip_recall_ranks(points.shape[0], points.shape[1], guess.shape[1], points.data_ptr(), y.shape[0], y.data_ptr(),
                            guess.data_ptr(), int(self_exclude), ranks.data_ptr())
    return ranks


def pack_allow(allow):
    """A numpy bool (or 0/1) array [n] -> the allow-list words uint32[ceil(n/32)] of annhip_index_set_filter: row i is bit
    i & 31 of word i >> 5; the tail bits of the last word are zero."""
    flags = np.ascontiguousarray(np.asarray(allow).reshape(-1) != 0)
    by = np.packbits(flags, bitorder="little")
    by = np.concatenate([by, np.zeros(-len(by) % 4, dtype=np.uint8)])
    return by.view("<u4").astype(np.uint32)


def _pack_allow_dev(lib, allow, n):
    """A torch bool / uint8 device tensor [n] -> int32 device tensor holding the allow-list words (annhip_filter_pack)."""
    import torch
    if not isinstance(allow, torch.Tensor) or not allow.is_cuda or allow.dtype not in (torch.bool, torch.uint8) or allow.dim() != 1 or allow.shape[0] != n:
        raise ValueError("allow must be a bool or uint8 device tensor of length n = %d" % n)
    flags = allow.contiguous()
    bits = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=allow.device)
    lib.annhip_filter_pack(n, flags.data_ptr(), bits.data_ptr(), torch.cuda.current_stream(allow.device).cuda_stream)
    torch.cuda.current_stream(allow.device).synchronize()  # the consumers run on the null stream / copy synchronously
    return bits


def _words_dev(words, length, device, what):
    """32-bit words for the tag calls -> an int32 device tensor [length] (keep it alive for the call): a numpy uint32
    array (copied to the device) or a torch int32 device tensor (its bits taken as they are).  ValueError for anything
    else, a wrong dtype or a wrong length."""
    import torch
    if isinstance(words, np.ndarray):
        if words.dtype != np.uint32 or words.shape != (length,):
            raise ValueError("%s must be uint32 of length %d" % (what, length))
        return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(device)
    if (not isinstance(words, torch.Tensor) or not words.is_cuda or words.dtype != torch.int32
            or tuple(words.shape) != (length,)):
        raise ValueError("%s must be a numpy uint32 array or an int32 device tensor of length %d" % (what, length))
    return words.contiguous()


def _where_dev(where, Q, device):
    """where = (qmask, qvalue), each as _words_dev takes it -> two int32 device tensors [Q]: query q's predicate is
    (tags[i] & qmask[q]) == qvalue[q].  where = (qmask, qlo, qhi) -> three: qlo[q] <= (tags[i] & qmask[q]) <= qhi[q],
    unsigned (the *_between calls)."""
    if not isinstance(where, (tuple, list)) or len(where) not in (2, 3):
        raise ValueError("where must be a pair (qmask, qvalue) or a triple (qmask, qlo, qhi)")
    if len(where) == 2:  # (the pair's path as it always was: it sits inside the timed step of every tagged call)
        return _words_dev(where[0], Q, device, "where[0] (qmask)"), _words_dev(where[1], Q, device, "where[1] (qvalue)")
    return (_words_dev(where[0], Q, device, "where[0] (qmask)"), _words_dev(where[1], Q, device, "where[1] (qlo)"),
            _words_dev(where[2], Q, device, "where[2] (qhi)"))


def where_in(mask, sets):
    """The CSR form of per-query sets of values or intervals for Index.query_sorted_set / tag_runs_set -> (mask, off, lo, hi):
    sets[q] is a list whose items are values v -- the interval [v, v] -- or pairs (lo, hi), all 32-bit words; off is numpy
    int64 [Q + 1], lo and hi numpy uint32 [off[-1]].  ValueError for a mask or an item that is no 32-bit word, for an item
    of another shape and for a set of more than 256 items."""
    def word(x, what):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) <= 0xFFFFFFFF:
            raise ValueError("where_in: %s must be a 32-bit word, got %r" % (what, x))
        return int(x)
    mask = word(mask, "mask")
    off, lo, hi = [0], [], []
    for q, items in enumerate(sets):
        items = list(items)
        if len(items) > 256:
            raise ValueError("where_in: query %d has %d intervals, at most 256 are allowed" % (q, len(items)))
        for it in items:
            if isinstance(it, (tuple, list)):
                if len(it) != 2:
                    raise ValueError("where_in: an item is a value or a pair (lo, hi), got %r" % (it,))
                lo.append(word(it[0], "lo")), hi.append(word(it[1], "hi"))
            else:
                v = word(it, "a value")
                lo.append(v), hi.append(v)
        off.append(len(lo))
    return mask, np.asarray(off, dtype=np.int64), np.asarray(lo, dtype=np.uint32), np.asarray(hi, dtype=np.uint32)


def _check_off(off):
    """the offsets of a CSR set form -> numpy uint32 [Q + 1]; ValueError unless they are an integer array that starts at 0,
    does not decrease and gives no query more than 256 intervals"""
    if not isinstance(off, np.ndarray) or off.ndim != 1 or off.shape[0] < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("off must be a one-dimensional numpy integer array [Q + 1]")
    o = off.astype(np.int64)
    if o[0] != 0 or (np.diff(o) < 0).any() or o[-1] > 0xFFFFFFFF:
        raise ValueError("off must start at 0 and must not decrease")
    if o.shape[0] > 1 and int(np.diff(o).max()) > 256:
        raise ValueError("a query has more than 256 intervals")
    return np.ascontiguousarray(o.astype(np.uint32))


def normalize_intervals(off, lo, hi):
    """The normalisation that annhip_query_sorted_set applies to its sets, in numpy -> (lo, hi) uint32 of the same length:
    within each query's slice the intervals are ordered by (lo, hi); empty ones (lo > hi) and those that an earlier one
    covers become (1, 0); each other one is clipped to start above the largest hi before it.  The non-empty results of a
    query are pairwise disjoint and their union is the union of the input."""
    o = _check_off(off).astype(np.int64)
    lo, hi = np.asarray(lo, dtype=np.uint32), np.asarray(hi, dtype=np.uint32)
    if lo.shape != (int(o[-1]),) or hi.shape != lo.shape:
        raise ValueError("lo and hi must have length off[-1]")
    nlo, nhi = np.empty_like(lo), np.empty_like(hi)
    for q in range(o.shape[0] - 1):
        a, b = int(o[q]), int(o[q + 1])
        order = np.lexsort((hi[a:b], lo[a:b]))
        top = -1  # the largest hi so far
        for j, i in enumerate(order):
            l, h = int(lo[a + i]), int(hi[a + i])
            if l > h or h <= top:
                l, h = 1, 0
            else:
                l, top = max(l, top + 1), h
            nlo[a + j], nhi[a + j] = l, h
    return nlo, nhi


def set_pieces(start, length, split):
    """The list entries that annhip_query_sorted_set makes of runs (start, length) -> (slot, piece start, piece end) int64
    arrays: split=0 one entry per run, empty ones included; split=S > 0 every non-empty run cut at the global multiples of
    S.  The host-side model of the staging."""
    start, length = np.asarray(start).astype(np.int64) & 0xFFFFFFFF, np.asarray(length).astype(np.int64) & 0xFFFFFFFF
    slot, ps, pe = [], [], []
    for j, (s, n) in enumerate(zip(start.tolist(), length.tolist())):
        if not split:
            slot.append(j), ps.append(s), pe.append(s + n)
        elif n:
            for t in range(s // split, (s + n - 1) // split + 1):
                slot.append(j), ps.append(max(s, t * split)), pe.append(min(s + n, (t + 1) * split))
    return np.asarray(slot, dtype=np.int64), np.asarray(ps, dtype=np.int64), np.asarray(pe, dtype=np.int64)


def order_key(values):
    """The order-preserving map of a numeric column into tag words -> numpy uint32 of the same shape: a <= b iff
    order_key(a) <= order_key(b) as unsigned words, so the result serves as, or inside, a tag word and as the bounds of
    where=(qmask, qlo, qhi).  int32: x ^ 0x80000000.  float32: the bits with the sign bit flipped for non-negative values
    and all bits flipped for negative ones; -0.0 counts as +0.0.  ValueError for NaN and for any other dtype.  A float
    window [a, b] is where=(0xFFFFFFFF, order_key(a), order_key(b))."""
    v = np.asarray(values)
    if v.dtype == np.int32:
        return v.view(np.uint32) ^ np.uint32(0x80000000)
    if v.dtype == np.float32:
        if np.isnan(v).any():
            raise ValueError("order_key: NaN has no place in the order")
        b = (v + np.float32(0)).view(np.uint32)  # -0.0 + 0.0 = +0.0
        return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    raise ValueError("order_key: values must be int32 or float32, got %s" % v.dtype)


def exact_knn(points, y, k, self_exclude=False, out_ids=None, out_dists=None, allow=None, tags=None, where=None):
    """annhip_exact_knn: torch device tensors points [n,d], y [Q,d] -> (ids int64 [Q,k], sq dists [Q,k]): the exact k
    nearest rows of every query, ordered by (distance, id), distances bit-identical to the query path's (include/ann_hip.h).
    self_exclude: query q leaves out point q.  Precision from the dtype.  ValueError where the library refuses (k outside
    1..1024 or larger than the rows on offer) and for tensors of mixed or unsupported dtype; the outputs are then untouched.
    allow: a bool device tensor [n] -- annhip_exact_knn_filtered: only rows with allow[i] set compete; a query with fewer
    than k of them gets (n, +inf) in the tail.
    tags + where: annhip_exact_knn_tagged -- tags: the rows' 32-bit tag words (numpy uint32 [n] or int32 device tensor [n]),
    where = (qmask, qvalue) (numpy uint32 [Q] or int32 device tensors [Q]): row i competes for query q iff
    (tags[i] & qmask[q]) == qvalue[q]; allow may be given too and is ANDed with that test.  One of the two without the
    other is a ValueError.  where = (qmask, qlo, qhi): annhip_exact_knn_between -- qlo[q] <= (tags[i] & qmask[q]) <= qhi[q],
    unsigned compares."""
    import torch
    if (tags is None) != (where is None):
        raise ValueError("exact_knn: tags and where=(qmask, qvalue) go together")
    if points.dtype != y.dtype or points.dtype not in (torch.float32, torch.float64):
        raise ValueError("exact_knn: points and y must both be float32 or both float64")
    if points.dim() != 2 or y.dim() != 2 or points.shape[1] != y.shape[1]:
        raise ValueError("exact_knn: points [n,d] and y [Q,d] must have the same d")
    assert points.is_cuda and y.is_cuda
    lib = _lib.load("f32" if points.dtype == torch.float32 else "f64")
    points, y, k = points.contiguous(), y.contiguous(), int(k)
    Q = y.shape[0]
    if k < 0:
        raise ValueError("exact_knn: k must be in 1..1024")
    ids = out_ids if out_ids is not None else torch.empty((Q, k), dtype=torch.int64, device=y.device)
    dists = out_dists if out_dists is not None else torch.empty((Q, k), dtype=y.dtype, device=y.device)
    assert ids.is_contiguous() and dists.is_contiguous() and ids.dtype == torch.int64 and dists.dtype == y.dtype
    if tags is not None:
        tg = _words_dev(tags, points.shape[0], y.device, "tags")
        pred = _where_dev(where, Q, y.device)
        bits = _pack_allow_dev(lib, allow, points.shape[0]) if allow is not None else None
        torch.cuda.current_stream(y.device).synchronize()  # the scan runs on the null stream
        if len(pred) == 3:
            rc = lib.annhip_exact_knn_between(points.shape[0], points.shape[1], k, points.data_ptr(), Q, y.data_ptr(),
                                              int(bool(self_exclude)), tg.data_ptr(), bits.data_ptr() if bits is not None else None,
                                              pred[0].data_ptr(), pred[1].data_ptr(), pred[2].data_ptr(), ids.data_ptr(),
                                              dists.data_ptr())
            if rc != 0:
                raise ValueError("annhip_exact_knn_between refused n=%d k=%d self_exclude=%r" % (points.shape[0], k, bool(self_exclude)))
            return ids, dists
        qm, qv = pred
        rc = lib.annhip_exact_knn_tagged(points.shape[0], points.shape[1], k, points.data_ptr(), Q, y.data_ptr(),
                                         int(bool(self_exclude)), tg.data_ptr(), bits.data_ptr() if bits is not None else None,
                                         qm.data_ptr(), qv.data_ptr(), ids.data_ptr(), dists.data_ptr())
        if rc != 0:
            raise ValueError("annhip_exact_knn_tagged refused n=%d k=%d self_exclude=%r" % (points.shape[0], k, bool(self_exclude)))
        return ids, dists
    if allow is not None:
        bits = _pack_allow_dev(lib, allow, points.shape[0])
        rc = lib.annhip_exact_knn_filtered(points.shape[0], points.shape[1], k, points.data_ptr(), Q, y.data_ptr(),
                                           int(bool(self_exclude)), bits.data_ptr(), ids.data_ptr(), dists.data_ptr())
        if rc != 0:
            raise ValueError("annhip_exact_knn_filtered refused n=%d k=%d self_exclude=%r" % (points.shape[0], k, bool(self_exclude)))
        return ids, dists
    if lib.annhip_exact_knn(points.shape[0], points.shape[1], k, points.data_ptr(), Q, y.data_ptr(), int(bool(self_exclude)),
                            ids.data_ptr(), dists.data_ptr()) != 0:
        raise ValueError("annhip_exact_knn refused n=%d k=%d self_exclude=%r" % (points.shape[0], k, bool(self_exclude)))
    return ids, dists


def _radius_dev(radius, Q, dtype, device, what="radius"):
    """The radii of a batch -> a device tensor [Q] of `dtype` (keep it alive for the call): a Python float, broadcast; a
    numpy array [Q] of that dtype, copied; or a device tensor [Q] of that dtype, taken as it is.  ValueError for anything
    else, a wrong dtype or a wrong shape."""
    import torch
    if isinstance(radius, bool):
        raise ValueError("%s must be a float, a numpy array or a device tensor of length %d" % (what, Q))
    if isinstance(radius, (int, float, np.floating, np.integer)):
        return torch.full((Q,), float(radius), dtype=dtype, device=device)
    if isinstance(radius, np.ndarray):
        if radius.dtype != (np.float32 if dtype == torch.float32 else np.float64):
            raise ValueError("%s must have the index's dtype" % what)
        if radius.shape != (Q,):
            raise ValueError("%s must have length %d" % (what, Q))
        return torch.from_numpy(np.ascontiguousarray(radius)).to(device)
    if not isinstance(radius, torch.Tensor) or not radius.is_cuda or radius.dtype != dtype or tuple(radius.shape) != (Q,):
        raise ValueError("%s must be a float, a numpy array or a device tensor of the index's dtype and length %d" % (what, Q))
    return radius.contiguous()


def _ptr(t, hold):
    """data_ptr() of a device tensor for a call that refuses NULL arrays; an empty tensor has none, `hold` (never read
    or written: the batch is empty) stands in for it."""
    return t.data_ptr() if t.numel() else hold.data_ptr()


def _check_cand(what, cand, Q, device):
    """cand of a rerank call: a contiguous int64 [Q, C] device tensor -> C; ValueError for anything else"""
    import torch
    if (not isinstance(cand, torch.Tensor) or not cand.is_cuda or cand.dtype != torch.int64 or cand.dim() != 2
            or cand.shape[0] != Q or not cand.is_contiguous() or cand.device != device):
        raise ValueError("%s: cand must be a contiguous int64 [Q, C] device tensor with one row per query" % what)
    return int(cand.shape[1])


def _rerank_out(what, out_ids, out_dists, Q, k, dtype, device):
    import torch
    ids = out_ids if out_ids is not None else torch.empty((Q, k), dtype=torch.int64, device=device)
    dists = out_dists if out_dists is not None else torch.empty((Q, k), dtype=dtype, device=device)
    if (tuple(ids.shape) != (Q, k) or tuple(dists.shape) != (Q, k) or ids.dtype != torch.int64 or dists.dtype != dtype
            or not ids.is_cuda or not dists.is_cuda or not ids.is_contiguous() or not dists.is_contiguous()):
        raise ValueError("%s: out_ids int64 [Q,k] and out_dists [Q,k] must be contiguous device tensors" % what)
    return ids, dists


def rerank(points, y, cand, k, out_ids=None, out_dists=None):
    """annhip_rerank: the exact top-k of caller-supplied candidates.  Torch device tensors points [n,d], y [Q,d] and cand,
    a contiguous int64 [Q,C] tensor of row ids -> (ids int64 [Q,k], sq dists [Q,k]): per query the k smallest
    (distance, id) among its distinct candidates below n, ascending, padded with (n, +inf).  An entry >= n (a pad, -1,
    anything) is skipped; a repeated id counts once; k may exceed C.  The distances are bit for bit exact_knn's and the
    query path's.  Precision from the dtype; runs on the current stream and returns at once.  out_ids may be cand where
    C == k.  ValueError for a mixed or unsupported dtype, for a cand that is not a contiguous int64 [Q,C] device tensor,
    and where the library refuses (k or C outside 1..1024, d == 0, a row too long for the LDS of one CU); the outputs are
    then untouched."""
    import torch
    if (not isinstance(points, torch.Tensor) or not isinstance(y, torch.Tensor) or points.dtype != y.dtype
            or points.dtype not in (torch.float32, torch.float64)):
        raise ValueError("rerank: points and y must both be float32 or both float64")
    if points.dim() != 2 or y.dim() != 2 or points.shape[1] != y.shape[1] or not points.is_cuda or not y.is_cuda:
        raise ValueError("rerank: points [n,d] and y [Q,d] must be device tensors with the same d")
    Q = y.shape[0]
    C_ = _check_cand("rerank", cand, Q, y.device)
    k = Index._check_k(k)
    if k < 0:
        raise ValueError("rerank: k must be in 1..1024")
    lib = _lib.load("f32" if points.dtype == torch.float32 else "f64")
    points, y = points.contiguous(), y.contiguous()
    ids, dists = _rerank_out("rerank", out_ids, out_dists, Q, k, y.dtype, y.device)
    hold = torch.empty((1,), dtype=torch.int64, device=y.device)
    rc = lib.annhip_rerank(points.shape[0], points.shape[1], _ptr(points, hold), Q, _ptr(y, hold), C_, _ptr(cand, hold), k,
                           _ptr(ids, hold), _ptr(dists, hold), torch.cuda.current_stream(y.device).cuda_stream)
    if rc != 0:
        raise ValueError("annhip_rerank refused n=%d d=%d C=%d k=%d (k or C outside 1..1024, d == 0, ids beyond 32 bits, or a "
                         "row too long for the LDS of one CU)"
                         % (points.shape[0], points.shape[1], C_, k))
    return ids, dists


def radius_trim(ids, dists, radius, pad_id):
    """annhip_radius_trim: cut a result in (distance, id) order at a radius, in place.  ids int64 [Q,k] and dists [Q,k]
    contiguous device tensors (query(k=), exact_query(k=) or exact_knn's), radius as Index.query_radius takes it, pad_id the
    id of a pad (n, or n_total of an index with a tail).  An entry stays iff its id is not pad_id and its distance is <=
    the query's radius; the rest of the row becomes (pad_id, +inf).  Runs on the current stream.  -> counts int32 [Q]."""
    import torch
    if (not isinstance(ids, torch.Tensor) or not isinstance(dists, torch.Tensor) or not ids.is_cuda or not dists.is_cuda
            or ids.dtype != torch.int64 or dists.dtype not in (torch.float32, torch.float64) or ids.dim() != 2
            or ids.shape != dists.shape or not ids.is_contiguous() or not dists.is_contiguous()):
        raise ValueError("radius_trim: ids int64 [Q,k] and dists [Q,k] must be contiguous device tensors of one shape")
    Q, k = ids.shape
    rad = _radius_dev(radius, Q, dists.dtype, dists.device)
    counts = torch.zeros((Q,), dtype=torch.int32, device=ids.device)
    lib = _lib.load("f32" if dists.dtype == torch.float32 else "f64")
    if not Q or not k:
        return counts
    if lib.annhip_radius_trim(Q, k, int(pad_id), rad.data_ptr(), ids.data_ptr(), dists.data_ptr(), counts.data_ptr(),
                              torch.cuda.current_stream(ids.device).cuda_stream) != 0:
        raise ValueError("annhip_radius_trim refused its arguments")
    return counts


def _check_group(what, group, k, per_group):
    """the arguments every grouped call shares -> (gmask, k, per_group) as ints; ValueError for a bool or non-integer, a
    group mask that is no non-zero 32-bit word, k < 1 or per_group < 1"""
    for name, v in (("group", group), ("k", k), ("per_group", per_group)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: %s must be an integer, got %r" % (what, name, v))
    if not 0 < int(group) <= 0xFFFFFFFF:
        raise ValueError("%s: group must be a non-zero 32-bit mask, got %r" % (what, group))
    if int(k) < 1 or int(per_group) < 1:
        raise ValueError("%s: k and per_group must be at least 1" % what)
    return int(group), int(k), int(per_group)


def collapse(ids, dists, tags, group, k, per_group=1, rows=None, pad_id=None, stream=None):
    """annhip_collapse: at most per_group entries per group of any list.  ids int64 [Q,L] and dists [Q,L] contiguous device
    tensors, read in the order given (query(k=), exact_query(k=) and exact_knn give ascending (distance, id), pads last);
    tags the 32-bit tag words of the rows, a numpy uint32 array or an int32 device tensor; group the mask whose bits of
    the tag word are the group key -> (ids int64 [Q,k], dists [Q,k], counts int32 [Q], short bool [Q]).  An entry whose
    id is not in [0, rows) is a pad and skipped (rows=None: len(tags)); a non-pad entry is kept iff fewer than per_group
    earlier non-pad entries of its row have its key; the first k kept entries are the row, padded with (pad_id, +inf)
    (pad_id=None: rows); counts = entries kept; short[q] = fewer than k kept although the list held no pad: a longer
    list might have found more groups.  Distances are copied bit for bit.  Runs on `stream` (the current stream when
    none is given) and returns at once; the inputs stay as they are (annhip_collapse itself may run in place where
    k == L).  ValueError for tensors of another kind, a bool or non-integer argument, and where the library refuses (L outside 1..1024, k outside 1..L,
    per_group < 1, group == 0, rows beyond len(tags) or 32 bits); the outputs are then untouched."""
    import torch
    if (not isinstance(ids, torch.Tensor) or not isinstance(dists, torch.Tensor) or not ids.is_cuda or not dists.is_cuda
            or ids.dtype != torch.int64 or dists.dtype not in (torch.float32, torch.float64) or ids.dim() != 2
            or ids.shape != dists.shape or not ids.is_contiguous() or not dists.is_contiguous()):
        raise ValueError("collapse: ids int64 [Q,L] and dists [Q,L] must be contiguous device tensors of one shape")
    gmask, k, per_group = _check_group("collapse", group, k, per_group)
    if isinstance(tags, np.ndarray) and tags.ndim != 1 or isinstance(tags, torch.Tensor) and tags.dim() != 1:
        raise ValueError("collapse: tags must be one-dimensional")
    tg = _words_dev(tags, len(tags) if hasattr(tags, "__len__") else 0, ids.device, "tags")
    for name, v in (("rows", rows), ("pad_id", pad_id)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0):
            raise ValueError("collapse: %s must be a non-negative integer, got %r" % (name, v))
    rows = tg.shape[0] if rows is None else int(rows)
    if rows > tg.shape[0]:
        raise ValueError("collapse: rows = %d exceeds the %d tag words given" % (rows, tg.shape[0]))
    pad_id = rows if pad_id is None else int(pad_id)
    Q, L = ids.shape
    if not 1 <= L <= 1024 or k > L:
        raise ValueError("collapse: L = %d must be in 1..1024 and k = %d in 1..L" % (L, k))
    o_ids = torch.empty((Q, k), dtype=torch.int64, device=ids.device)
    o_dists = torch.empty((Q, k), dtype=dists.dtype, device=ids.device)
    counts = torch.zeros((Q,), dtype=torch.int32, device=ids.device)
    short = torch.zeros((Q,), dtype=torch.uint8, device=ids.device)
    lib = _lib.load("f32" if dists.dtype == torch.float32 else "f64")
    cur = torch.cuda.current_stream(ids.device)
    run = stream if stream is not None else cur
    if run != cur:
        run.wait_stream(cur)  # the arrays were made on that one
    hold = torch.empty((1,), dtype=torch.int64, device=ids.device)
    rc = lib.annhip_collapse(Q, L, k, per_group, gmask, _ptr(tg, hold), rows, pad_id, _ptr(ids, hold), _ptr(dists, hold),
                             _ptr(o_ids, hold), _ptr(o_dists, hold), counts.data_ptr(), short.data_ptr(), run.cuda_stream)
    if rc != 0:
        raise ValueError("annhip_collapse refused L=%d k=%d per_group=%d group=%#x rows=%d" % (L, k, per_group, gmask, rows))
    if run != cur:  # keep the arrays until the pass has read them
        for t in (ids, dists, tg, o_ids, o_dists, counts, short, hold):
            t.record_stream(run)
        cur.wait_stream(run)  # short.bool() below runs on the current stream
    return o_ids, o_dists, counts, short.bool()


def radius_recall(guess_ids, guess_counts, truth_ids, truth_counts):
    """Recall of a radius query against its ground truth: the mean, over the queries with truth_counts > 0, of
    |guess[q][:guess_counts[q]] ∩ truth[q][:truth_counts[q]]| / truth_counts[q] -> (recall, queries counted); (0.0, 0) where
    no query has a true hit.  Integer tensors guess_ids [Q,kg], truth_ids [Q,kt], counts [Q]; pure torch, any device."""
    import torch
    dev = guess_ids.device
    gi, ti = guess_ids.long(), truth_ids.long().to(dev)
    gc, tc = guess_counts.long().to(dev), truth_counts.long().to(dev)
    glive = torch.arange(gi.shape[1], device=dev)[None, :] < gc[:, None]  # [Q,kg]
    tlive = torch.arange(ti.shape[1], device=dev)[None, :] < tc[:, None]  # [Q,kt]
    hit = ((ti.unsqueeze(2) == gi.unsqueeze(1)) & glive.unsqueeze(1)).any(dim=2) & tlive  # [Q,kt]: truth id found
    use = tc > 0
    counted = int(use.sum().item())
    if not counted:
        return 0.0, 0
    return (hit.double().sum(dim=1)[use] / tc[use].double()).mean().item(), counted


def recall_at_k(guess, truth):
    """Standard recall@k: the mean over queries of |guess[q] ∩ truth[q]| / k, for integer tensors guess [Q,kg] (as query()
    returns them; ids >= n are its "no neighbour" marks and never match) and truth [Q,k] (exact_knn's ids)."""
    k = truth.shape[1]
    hit = (guess.unsqueeze(2) == truth.to(guess.device).unsqueeze(1)).any(dim=1)  # [Q,k]: truth id found among the guesses
    return hit.double().sum(dim=1).div(k).mean().item()


def checksum(t, prec="f32"):
    """annhip_checksum_dev: 64-bit content checksum of a contiguous torch device tensor."""
    assert t.is_cuda and t.is_contiguous()
    return int(_lib.load(prec).annhip_checksum_dev(t.data_ptr(), t.numel() * t.element_size(), None))


def recall_summary(ranks, k):
    """The three numbers /root/reference/test_correctness.c:131-139 prints, from a rank tensor [Q,k]:
    average index score (mean rank excess per neighbour), probability correct (rank < k), max index score / k."""
    r = ranks.to("cpu").double()
    per_query = r.sum(dim=1).mean().item()
    return dict(avg_index_score=(per_query - k * (k - 1) / 2) / k,
                prob_correct=1.0 - (r >= k).double().mean().item(),
                max_index_score=r.max().item() / k)


class Index:
    """A device-resident index (include/ann_hip.h).  Tensors are torch CUDA(HIP) tensors; torch is only the
    allocator and stream provider here."""

    def __init__(self, prec, handle, keep=()):
        self.prec, self.h, self._keep = prec, handle, keep
        self.lib = _lib.load(prec)
        info = (C.c_size_t * 12)()
        self.lib.annhip_index_info(self.h, C.byref(info))
        (self.n, self.k, self.d, self.d_short, self.tries, self.L1, self.P1, self.Lc1, self.L2, self.P2, self.Lc2,
         self.sum_pm) = [int(v) for v in info]

    @staticmethod
    def _torch_ft(prec):
        import torch
        return torch.float32 if prec == "f32" else torch.float64

    @classmethod
    def from_save(cls, save, points, row_lo=0, row_hi=None):
        """points: numpy array (copied to HBM) or torch device tensor (borrowed) holding rows [row_lo,row_hi)."""
        lib = _lib.load(save.prec)
        row_hi = int(save.c.n) if row_hi is None else row_hi
        if isinstance(points, np.ndarray):
            pts = np.ascontiguousarray(points, dtype=_ft(save.prec))
            assert pts.shape == (row_hi - row_lo, save.c.d_long)
            h = lib.annhip_index_create(C.byref(save.c), pts.ctypes.data, 0, row_lo, row_hi)
            return cls(save.prec, h)
        assert points.is_cuda and points.is_contiguous() and points.dtype == cls._torch_ft(save.prec)
        assert tuple(points.shape) == (row_hi - row_lo, save.c.d_long)
        h = lib.annhip_index_create(C.byref(save.c), points.data_ptr(), 1, row_lo, row_hi)
        return cls(save.prec, h, keep=(points,))

    @classmethod
    def precomp(cls, points, k, tries=10, rots_before=6, rot_len_before=1, rots_after=1, rot_len_after=1,
                want_dists=False):
        """annhip_precomp_index: build the index on the device from a torch device tensor [n,d] (borrowed)."""
        import torch
        prec = "f32" if points.dtype == torch.float32 else "f64"
        assert points.is_cuda and points.is_contiguous()
        lib = _lib.load(prec)
        n, d = points.shape
        gd = torch.empty((n, k), dtype=points.dtype, device=points.device) if want_dists else None
        h = lib.annhip_precomp_index(n, k, d, points.data_ptr(), 1, tries, rots_before, rot_len_before, rots_after,
                                     rot_len_after, gd.data_ptr() if want_dists else None)
        ix = cls(prec, h, keep=(points,))
        ix.graph_dists = gd
        return ix

    def export(self):
        s = Save(self.prec)
        self.lib.annhip_index_export(self.h, C.byref(s.c))
        s._malloced = True
        return s

    def reshard(self, shard_points, row_lo, row_hi):
        """annhip_index_reshard: own rows [row_lo,row_hi) only, read from the torch device tensor shard_points."""
        assert shard_points.is_cuda and shard_points.is_contiguous() and tuple(shard_points.shape) == (row_hi - row_lo, self.d)
        self.lib.annhip_index_reshard(self.h, shard_points.data_ptr(), row_lo, row_hi)
        self._keep = (shard_points,)
        self.row_lo, self.row_hi = row_lo, row_hi

    def set_stream(self, stream_ptr):
        self.lib.annhip_index_set_stream(self.h, stream_ptr)

    def set_fixed(self, on=True):
        """annhip_index_set_fixed: opt-in non-parity query mode (own hash codes, every candidate slot; include/ann_hip.h)."""
        self.lib.annhip_index_set_fixed(self.h, int(bool(on)))

    def set_probe(self, pair_bits):
        """annhip_index_set_probe: the recall knob of fixed mode -- per try, also probe the buckets reached by flipping two of
        the query's `pair_bits` least certain hash bits (0 = plain fixed mode, the default; "all" = d_short, the whole
        Hamming-2 ball; include/ann_hip.h).  No effect while fixed mode is off.  ValueError where the library refuses
        (outside 0..d_short); the setting is then unchanged."""
        code = -1 if pair_bits == "all" else pair_bits
        if isinstance(code, bool) or not isinstance(code, int) or self.lib.annhip_index_set_probe(self.h, code) != 0:
            raise ValueError("annhip_index_set_probe refused pair_bits=%r (d_short = %d)" % (pair_bits, self.d_short))

    @property
    def probe(self):
        """annhip_index_probe: the current pair bits (an int; "all" reads back as d_short)."""
        return int(self.lib.annhip_index_probe(self.h))

    def probe_bits(self, y):
        """annhip_probe_bits: what a fixed-mode query of y [Q,d] would probe with -> (codes int64 [Q,T] (code[q*T+t]),
        bits uint8 [Q,T,b]: per (query, try) the b projection indices of smallest magnitude, ascending).  ValueError
        while the probe setting is 0."""
        import torch
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q, b = y.shape[0], self.probe
        codes = torch.empty((Q, self.tries), dtype=torch.int32, device=y.device)
        bits = torch.empty((Q, self.tries, b), dtype=torch.uint8, device=y.device)
        stream = torch.cuda.current_stream(y.device).cuda_stream
        if self.lib.annhip_probe_bits(self.h, stream, Q, y.data_ptr(), codes.data_ptr(), bits.data_ptr()) != 0:
            raise ValueError("annhip_probe_bits: the probe setting is 0 (Index.set_probe)")
        return codes.to(torch.int64) & 0xFFFFFFFF, bits

    def set_filter(self, allow):
        """annhip_index_set_filter: restrict fixed-mode queries (and exact_query) to the rows with allow[i] set.  allow:
        None (clear), a torch bool or uint8 device tensor [n], or a numpy bool array [n]; the index keeps its own packed
        copy.  ValueError for a wrong length and where the library refuses (fixed mode off, resharded index); the setting
        is then unchanged.  set_fixed(False) and reshard drop the filter.  Do not change it while batches are in flight."""
        if allow is None:
            self.lib.annhip_index_set_filter(self.h, None, 0)
            return
        rows = self.n_total  # the built rows and the appended ones: one array serves both
        if isinstance(allow, np.ndarray):
            if allow.shape != (rows,):
                raise ValueError("allow must have length n_total = %d" % rows)
            bits = pack_allow(allow)
            rc = self.lib.annhip_index_set_filter(self.h, bits.ctypes.data, 0)
        else:
            bits = _pack_allow_dev(self.lib, allow, rows)
            rc = self.lib.annhip_index_set_filter(self.h, bits.data_ptr(), 1)
        if rc != 0:
            raise ValueError("annhip_index_set_filter refused (fixed mode off, or a resharded index)")

    @property
    def filter_count(self):
        """annhip_index_filter_count: the number of allowed rows, or None while no filter is set."""
        c = int(self.lib.annhip_index_filter_count(self.h))
        return None if c < 0 else c

    def set_tags(self, tags):
        """annhip_index_set_tags: give every row a 32-bit tag word for query(where=...) and exact_query(where=...).  tags:
        None (clear), a numpy uint32 array [n], or a torch int32 device tensor [n] whose bits are taken as they are; the
        index keeps its own copy.  ValueError for a wrong length or dtype and where the library refuses (a resharded
        index); the setting is then unchanged.  Tags are row attributes: fixed mode need not be on, set_fixed(False)
        keeps them, reshard drops them, and no query without where= reads them.  Do not change them while batches are
        in flight."""
        import torch
        if tags is None:
            self.lib.annhip_index_set_tags(self.h, None, 0)
            return
        rows = self.n_total  # the built rows and the appended ones: one array serves both
        if isinstance(tags, np.ndarray):
            if tags.dtype != np.uint32 or tags.shape != (rows,):
                raise ValueError("tags must be uint32 of length n_total = %d" % rows)
            host = np.ascontiguousarray(tags)
            rc = self.lib.annhip_index_set_tags(self.h, host.ctypes.data, 0)
        else:
            if (not isinstance(tags, torch.Tensor) or not tags.is_cuda or tags.dtype != torch.int32
                    or tuple(tags.shape) != (rows,)):
                raise ValueError("tags must be a numpy uint32 array or an int32 device tensor of length n_total = %d" % rows)
            dev = tags.contiguous()
            torch.cuda.current_stream(dev.device).synchronize()  # the copy runs on the null stream
            rc = self.lib.annhip_index_set_tags(self.h, dev.data_ptr(), 1)
        if rc != 0:
            raise ValueError("annhip_index_set_tags refused (a resharded index)")

    @property
    def has_tags(self):
        """annhip_index_has_tags: True while the index holds tag words."""
        return bool(self.lib.annhip_index_has_tags(self.h))

    # ---- appended rows (include/ann_hip.h, "Appended rows of fixed mode: the tail")
    @property
    def tail(self):
        """annhip_index_tail: m, the number of rows appended since the build."""
        return int(self.lib.annhip_index_tail(self.h))

    @property
    def n_total(self):
        """n + tail: the rows a fixed-mode query answers from; ids run over [0, n_total), pads carry n_total."""
        return self.n + self.tail

    def append(self, rows, tags=None):
        """annhip_index_append: add rows [count, d] -- a numpy array or a torch device tensor of the index's precision -- to
        the index's tail; every fixed-mode query scans the tail exactly and merges it into its answer.  tags: the new rows'
        tag words (numpy uint32 [count] or int32 device tensor [count]), required exactly when the index has tags.  Returns
        the id of the first new row (n_total before the call).  With an allow list set the new rows are allowed.
        ValueError for a wrong shape or dtype and where the library refuses (fixed mode off, a resharded index, narrow
        rows, tags missing or unexpected); nothing changes then.  Do not append while batches are in flight."""
        import torch
        first = self.n_total
        if isinstance(rows, np.ndarray):
            if rows.ndim != 2 or rows.shape[1] != self.d or rows.dtype != _ft(self.prec):
                raise ValueError("append: rows must be %s [count, %d]" % (np.dtype(_ft(self.prec)).name, self.d))
            src, on_dev = np.ascontiguousarray(rows), 0
            ptr = src.ctypes.data
        else:
            if (not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dim() != 2 or rows.shape[1] != self.d
                    or rows.dtype != self._torch_ft(self.prec)):
                raise ValueError("append: rows must be a numpy array or a device tensor [count, %d] of the index's precision" % self.d)
            src, on_dev = rows.contiguous(), 1
            torch.cuda.current_stream(src.device).synchronize()  # the copy runs on the null stream
            ptr = src.data_ptr()
        count = int(src.shape[0])
        tg = tptr = None
        tags_on_dev = 0
        if tags is not None:
            if isinstance(tags, np.ndarray):
                if tags.dtype != np.uint32 or tags.shape != (count,):
                    raise ValueError("append: tags must be uint32 of length count = %d" % count)
                tg = np.ascontiguousarray(tags)
                tptr = tg.ctypes.data
            else:
                tg = _words_dev(tags, count, tags.device if isinstance(tags, torch.Tensor) else None, "append: tags")
                torch.cuda.current_stream(tg.device).synchronize()
                tptr, tags_on_dev = tg.data_ptr(), 1
        if self.lib.annhip_index_append(self.h, ptr if count else None, on_dev, count, tptr, tags_on_dev) != 0:
            raise ValueError("annhip_index_append refused (fixed mode off, a resharded index, narrow rows, too many rows, or "
                             "tags given without / missing with the index's tags)")
        return first

    def reserve_tail(self, rows):
        """annhip_index_reserve_tail: capacity for at least `rows` appended rows, so that later appends do not reallocate.
        ValueError where the library refuses (as append)."""
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or rows < 0 or \
                self.lib.annhip_index_reserve_tail(self.h, int(rows)) != 0:
            raise ValueError("annhip_index_reserve_tail refused rows=%r" % (rows,))

    def drop_tail(self):
        """annhip_index_drop_tail: forget the appended rows (the capacity is kept); filter and tags are read up to n again."""
        self.lib.annhip_index_drop_tail(self.h)

    def hash_tail(self):
        """annhip_index_hash_tail: file all current tail rows under their hash codes, so that a fixed-mode query fetches only
        the tail rows of the buckets it probes instead of scanning them all.  Those rows are then found approximately, like
        built rows; rows appended later are scanned exactly until the next call.  ValueError where the library refuses
        (fixed mode off, a resharded index); nothing changes then.  Do not call it while batches are in flight."""
        if self.lib.annhip_index_hash_tail(self.h) != 0:
            raise ValueError("annhip_index_hash_tail refused (fixed mode off, or a resharded index)")

    @property
    def tail_hashed(self):
        """annhip_index_tail_hashed: mh, the tail rows [0, mh) that queries look up by hash code."""
        return int(self.lib.annhip_index_tail_hashed(self.h))

    def rows_tensor(self, lo, hi):
        """annhip_index_copy_rows: a new device tensor [hi - lo, d] holding native rows [lo, hi) of the combined row set
        (built rows, then the tail).  ValueError for a range outside 0..n_total or a resharded index."""
        import torch
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.n_total:
            raise ValueError("rows_tensor: [%d, %d) outside 0..n_total = %d" % (lo, hi, self.n_total))
        out = torch.empty((hi - lo, self.d), dtype=self._torch_ft(self.prec), device="cuda")
        torch.cuda.current_stream(out.device).synchronize()
        if self.lib.annhip_index_copy_rows(self.h, lo, hi, out.data_ptr()) != 0:
            raise ValueError("annhip_index_copy_rows refused [%d, %d) (a resharded index)" % (lo, hi))
        return out

    def compact(self, tries=10, rots_before=6, rot_len_before=1, rots_after=1, rot_len_after=1):
        """Fold the tail into a rebuilt index: Index.precomp over rows_tensor(0, n_total) with this index's k.  Returns a
        NEW index with n = n_total and no tail; fixed mode, the probe setting, the allow list and the tags (n_total words
        each) are carried over, ids are unchanged.  The rotations are drawn from libc random(): the caller seeds it.  This
        index stays as it is; close it when the new one has taken over."""
        import torch
        rows = self.rows_tensor(0, self.n_total)
        new = Index.precomp(rows, self.k, tries, rots_before, rot_len_before, rots_after, rot_len_after)
        new.set_fixed(bool(self.lib.annhip_index_fixed(self.h)))
        new.set_probe(min(self.probe, new.d_short))
        nt = self.n_total
        if self.filter_count is not None:
            bits = torch.empty(((nt + 31) // 32,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            self.lib.annhip_index_copy_words(self.h, 0, bits.data_ptr())
            if new.lib.annhip_index_set_filter(new.h, bits.data_ptr(), 1) != 0:
                raise ValueError("compact: the allow list could not be carried over")
        if self.has_tags:
            tg = torch.empty((nt,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            self.lib.annhip_index_copy_words(self.h, 1, tg.data_ptr())
            new.set_tags(tg)
        if self.tag_order is not None:  # the order is carried over by sorting again with the same mask
            new.sort_tags(self.tag_order[0])
        return new

    ROWS = {"native": 0, "f16": 1}  # ANNHIP_ROWS_NATIVE, ANNHIP_ROWS_F16 (include/ann_hip.h)
    # the names an index of each precision knows: every library serves its own narrow row type (ANNHIP_ROWS_F32 = 2)
    ROWS_BY_PREC = {"f32": ROWS, "f64": {"native": 0, "f32": 2}}

    def set_rows(self, rows):
        """annhip_index_set_rows: opt-in narrow point rows -- "f16" (binary16) on an f32 index, "f32" (binary32) on an
        f64 index: results = the reference's on the rows rounded to that type; all rows on this device.  "native" = the
        rows as given (the default).  ValueError for a name this index's precision does not know and where the library
        refuses (the other library's type, resharded index, unknown value); the setting is then unchanged."""
        code = self.ROWS_BY_PREC[self.prec].get(rows) if isinstance(rows, str) else rows
        if not isinstance(code, int) or self.lib.annhip_index_set_rows(self.h, code) != 0:
            raise ValueError("annhip_index_set_rows refused rows=%r for this index (%s)" % (rows, self.prec))

    @property
    def rows(self):
        """annhip_index_rows: "native", or the narrow type of this index's precision ("f16" / "f32")."""
        code = int(self.lib.annhip_index_rows(self.h))
        return {v: k for k, v in self.ROWS_BY_PREC[self.prec].items()}.get(code, code)

    PRUNE = {"off": 0, "on": 1, "auto": -1}

    def set_prune(self, mode):
        """annhip_index_set_prune: the parity path's stage 1 on half the bytes with the same answers (f32 indexes) --
        "auto" (the default: on for large eligible indexes), "on" (wherever eligible), "off"; or True / False / -1, 0, 1.
        ValueError where the library refuses (an f64 index, a resharded one, appended rows, k > 31, a row that overflows
        binary16); the setting is then unchanged."""
        code = self.PRUNE.get(mode) if isinstance(mode, str) else int(mode)
        if code is None or self.lib.annhip_index_set_prune(self.h, code) != 0:
            raise ValueError("annhip_index_set_prune refused mode=%r for this index (%s)" % (mode, self.prec))

    @property
    def prune(self):
        """annhip_index_prune: True while this index's parity-mode queries take the pruned stage 1."""
        return bool(self.lib.annhip_index_prune(self.h))

    @property
    def prune_bound(self):
        """annhip_index_prune_bound: (E, keys) -- the certificate's E >= max ||p - binary16(p)||_2 and the K' keys the
        preselection keeps, as the last set_prune (or the auto rule) fixed them -- or None while the index holds no
        narrow copy and bound.  Read-only."""
        E, keys = C.c_double(), C.c_int()
        if not self.lib.annhip_index_prune_bound(self.h, C.byref(E), C.byref(keys)):
            return None
        return float(E.value), int(keys.value)

    def workspace(self):
        """annhip_workspace_create: scratch for one in-flight batch (pass to query(ws=..., stream=...))."""
        ws = self.lib.annhip_workspace_create(self.h)
        self._workspaces = getattr(self, "_workspaces", []) + [ws]
        return ws

    @staticmethod
    def _check_k(k):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError("k must be an integer, got %r" % (k,))
        return int(k)

    @property
    def max_query_k(self):
        """annhip_index_max_query_k: the largest k that query(k=...) accepts on this index (at most 1024)."""
        return int(self.lib.annhip_index_max_query_k(self.h))

    # ---- the tag order (include/ann_hip.h, "the tag order")
    def sort_tags(self, mask=0xFFFFFFFF):
        """annhip_index_sort_tags: sort the row ids by (tags & mask, id), so that query_sorted answers a predicate on that
        mask exactly by scanning only the rows it admits.  mask=0 or None drops the order.  One order and mask per index;
        8 bytes per row.  set_tags, drop_tail and reshard drop it; set_filter and append keep it (rows appended later are
        scanned as the tail is).  ValueError for a mask that is no 32-bit word and where the library refuses (no tags, a
        resharded index); nothing changes then.  Do not call it while batches are in flight."""
        mask = 0 if mask is None else mask
        if isinstance(mask, bool) or not isinstance(mask, (int, np.integer)) or not 0 <= int(mask) <= 0xFFFFFFFF:
            raise ValueError("sort_tags: mask must be a 32-bit word, got %r" % (mask,))
        if self.lib.annhip_index_sort_tags(self.h, int(mask)) != 0:
            raise ValueError("annhip_index_sort_tags refused (no tags, or a resharded index)")

    @property
    def tag_order(self):
        """annhip_index_tag_order: (mask, rows) of the current tag order -- rows = n_total at the sort_tags call -- or None."""
        mask = C.c_uint32()
        rows = int(self.lib.annhip_index_tag_order(self.h, C.byref(mask)))
        return (int(mask.value), rows) if rows else None

    def _sorted_pred(self, what, where, Q, device):
        """where of a sorted call -> (qmask, qlo, qhi) int32 device tensors [Q]; a pair is the interval [value, value].  ValueError
        without an order and for a mask word other than the order's (free for numpy input, one reduction for device input)."""
        order = self.tag_order
        if order is None:
            raise ValueError("%s: the index has no tag order (Index.sort_tags)" % what)
        pred = _where_dev(where, Q, device)
        qm = where[0]
        if isinstance(qm, np.ndarray):
            same = bool(np.all(qm == np.uint32(order[0])))
        else:
            want = order[0] - (1 << 32) if order[0] >= (1 << 31) else order[0]
            same = not bool((pred[0] != want).any().item())
        if not same:
            raise ValueError("%s: every mask word must equal the order's mask 0x%08X" % (what, order[0]))
        return (pred[0], pred[1], pred[1]) if len(pred) == 2 else pred

    def tag_runs(self, where):
        """annhip_tag_runs: per query the run of the tag order its predicate selects -> (start, length), int32 device
        tensors [Q] (their bits are unsigned): the rows that compete are positions [start, start + length) of the order.
        where = (qmask, qvalue) or (qmask, qlo, qhi) as in query(); every mask word must equal the order's.  Runs on the
        current stream.  ValueError without an order, for a wrong mask, shape or dtype."""
        import torch
        if not isinstance(where, (tuple, list)) or len(where) not in (2, 3):
            raise ValueError("where must be a pair (qmask, qvalue) or a triple (qmask, qlo, qhi)")
        Q = int(where[0].shape[0]) if hasattr(where[0], "shape") and len(where[0].shape) == 1 else -1
        if Q < 0:
            raise ValueError("tag_runs: where[0] (qmask) must be a one-dimensional array")
        dev = where[0].device if isinstance(where[0], torch.Tensor) else torch.device("cuda")
        return self._runs(*self._sorted_pred("tag_runs", where, Q, dev)[1:])

    def _runs(self, qlo, qhi):
        """annhip_tag_runs on the current stream for bounds already on the device"""
        import torch
        Q, dev = int(qlo.shape[0]), qlo.device
        start = torch.zeros((Q,), dtype=torch.int32, device=dev)
        length = torch.zeros((Q,), dtype=torch.int32, device=dev)
        hold = torch.empty((1,), dtype=torch.int64, device=dev)
        if self.lib.annhip_tag_runs(self.h, torch.cuda.current_stream(dev).cuda_stream, Q, _ptr(qlo, hold), _ptr(qhi, hold),
                                    _ptr(start, hold), _ptr(length, hold)) != 0:
            raise ValueError("annhip_tag_runs refused (no tag order)")
        return start, length

    def query_sorted(self, y, where, k=None, radius=None, alias=False, ws=None, stream=None):
        """annhip_query_sorted: the exact answer of a tag predicate by a scan of the rows it admits -> (ids int64 [Q,k],
        sq dists [Q,k]), or (ids, dists, counts int32 [Q]) with a radius: bit for bit exact_query(y, k=k, where=where) /
        exact_query_radius, at a cost proportional to the matching rows.  where = (qmask, qvalue) -- the interval
        [value, value] -- or (qmask, qlo, qhi), every mask word equal to the order's mask (sort_tags).  k=None: the index's
        k.  The allow list applies, built rows, the tail and rows appended after sort_tags all compete, and the distances
        are the native rows' whatever set_rows says.  ws and stream as in query(where=).  ValueError without an order, for
        a wrong mask, a bool or non-integer k, a radius of wrong shape or dtype, and where the library refuses (k outside
        1..1024 or larger than the rows on offer, a resharded index); nothing is launched then."""
        import torch
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q = y.shape[0]
        kq = self.k if k is None else self._check_k(k)
        if kq < 1:
            raise ValueError("query_sorted: k must be in 1..1024")
        _, qlo, qhi = self._sorted_pred("query_sorted", where, Q, y.device)
        rad = _radius_dev(radius, Q, y.dtype, y.device) if radius is not None else None
        ids = torch.empty((Q, kq), dtype=torch.int64, device=y.device)
        dists = torch.empty((Q, kq), dtype=y.dtype, device=y.device)
        counts = torch.zeros((Q,), dtype=torch.int32, device=y.device) if rad is not None else None
        self._sorted(y, alias, kq, rad, qlo, qhi, ids, dists, counts, ws, stream)
        return (ids, dists) if rad is None else (ids, dists, counts)

    def _sorted(self, y, alias, kq, rad, qlo, qhi, ids, dists, counts, ws, stream):
        """annhip_query_sorted on `stream` / `ws`: _between's stream and lifetime handling."""
        import torch
        if stream is not None and torch.cuda.current_stream(y.device) != stream:
            stream.wait_stream(torch.cuda.current_stream(y.device))  # the predicate (and radius) arrays were made on that one
        hold = torch.empty((1,), dtype=torch.int64, device=y.device)
        rc = self.lib.annhip_query_sorted(self.h, ws, stream.cuda_stream if stream is not None else None, y.shape[0], _ptr(y, hold),
                                          int(bool(alias)), kq, _ptr(rad, hold) if rad is not None else None, _ptr(qlo, hold),
                                          _ptr(qhi, hold), _ptr(ids, hold), _ptr(dists, hold),
                                          counts.data_ptr() if counts is not None else None)
        if rc == -2:
            raise ValueError("annhip_query_sorted refused k=%d (no tag order, k outside 1..1024 or larger than the rows on "
                             "offer, or a resharded index)" % kq)
        if stream is not None:  # keep the arrays until the batch has read them
            for t in (qlo, qhi, rad, ids, dists, counts, hold):
                if t is not None:
                    t.record_stream(stream)
        return rc

    def _set_pred(self, what, where, device):
        """where = (mask, off, lo, hi) of a set call -> (off uint32 numpy [Q + 1], lo, hi int32 device tensors [off[-1]]);
        ValueError without an order, for a mask other than the order's and for malformed arrays"""
        order = self.tag_order
        if order is None:
            raise ValueError("%s: the index has no tag order (Index.sort_tags)" % what)
        if not isinstance(where, (tuple, list)) or len(where) != 4:
            raise ValueError("%s: where must be (mask, off, lo, hi)" % what)
        mask, off, lo, hi = where
        if isinstance(mask, bool) or not isinstance(mask, (int, np.integer)) or int(mask) != order[0]:
            raise ValueError("%s: the mask must equal the order's mask 0x%08X" % (what, order[0]))
        off = _check_off(off)
        T = int(off[-1])
        return off, _words_dev(lo, T, device, "where[2] (lo)"), _words_dev(hi, T, device, "where[3] (hi)")

    def tag_runs_set(self, where):
        """annhip_tag_runs_set: the runs of the normalised intervals of every query's set -> (start, length), int32 device
        tensors [off[-1]] (their bits are unsigned), in the order of normalize_intervals; (0, 0) for the slots it
        emptied.  where = (mask, off, lo, hi) as where_in builds it.  Runs on the current stream and stages its offsets
        in the index's own workspace.  ValueError without an order, for a wrong mask and for malformed arrays."""
        import torch
        dev = where[2].device if isinstance(where, (tuple, list)) and len(where) == 4 and isinstance(where[2], torch.Tensor) \
            else torch.device("cuda")
        off, lo, hi = self._set_pred("tag_runs_set", where, dev)
        T = int(off[-1])
        start = torch.zeros((T,), dtype=torch.int32, device=dev)
        length = torch.zeros((T,), dtype=torch.int32, device=dev)
        hold = torch.empty((1,), dtype=torch.int64, device=dev)
        if self.lib.annhip_tag_runs_set(self.h, torch.cuda.current_stream(dev).cuda_stream, off.shape[0] - 1, off.ctypes.data,
                                        _ptr(lo, hold), _ptr(hi, hold), _ptr(start, hold), _ptr(length, hold)) != 0:
            raise ValueError("annhip_tag_runs_set refused")
        return start, length

    def query_sorted_set(self, y, where, k=None, radius=None, split=0, alias=False, ws=None, stream=None):
        """annhip_query_sorted_set: query_sorted for a union of intervals per query -> (ids int64 [Q,k], sq dists [Q,k],
        entries), or (ids, dists, counts int32 [Q], entries) with a radius.  where = (mask, off, lo, hi): mask the
        order's, off a numpy integer array [Q + 1], lo / hi numpy uint32 arrays or int32 device tensors [off[-1]]
        (where_in builds them); row i competes for query q iff lo[j] <= (tags[i] & mask) <= hi[j] for some j in
        [off[q], off[q + 1]).  split=S > 0 cuts every run at the global multiples of S rows of the order, so that a long
        run is scanned by many workgroups; the call then waits once for its stream to learn the piece count.  split=0
        cuts nothing and waits for nothing.  entries = the non-empty runs (split=0: a device scalar, reading it
        synchronises) or the pieces (split > 0: an int).  Everything else is query_sorted's.  ValueError where that raises
        it, for malformed sets, more than 256 intervals in one, 0 < split < 64 and more than 2^27 entries x k; nothing of
        the scan is launched then."""
        import torch
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q = y.shape[0]
        kq = self.k if k is None else self._check_k(k)
        if kq < 1:
            raise ValueError("query_sorted_set: k must be in 1..1024")
        if isinstance(split, bool) or not isinstance(split, (int, np.integer)) or not (split == 0 or 64 <= split <= 0xFFFFFFFF):
            raise ValueError("query_sorted_set: split must be 0 or an integer in 64..2^32-1, got %r" % (split,))
        off, lo, hi = self._set_pred("query_sorted_set", where, y.device)
        if off.shape[0] != Q + 1:
            raise ValueError("query_sorted_set: off must have length Q + 1 = %d" % (Q + 1))
        rad = _radius_dev(radius, Q, y.dtype, y.device) if radius is not None else None
        ids = torch.empty((Q, kq), dtype=torch.int64, device=y.device)
        dists = torch.empty((Q, kq), dtype=y.dtype, device=y.device)
        counts = torch.zeros((Q,), dtype=torch.int32, device=y.device) if rad is not None else None
        if stream is not None and torch.cuda.current_stream(y.device) != stream:
            stream.wait_stream(torch.cuda.current_stream(y.device))
        hold = torch.empty((1,), dtype=torch.int64, device=y.device)
        rc = self.lib.annhip_query_sorted_set(self.h, ws, stream.cuda_stream if stream is not None else None, Q, _ptr(y, hold),
                                              int(bool(alias)), kq, _ptr(rad, hold) if rad is not None else None, off.ctypes.data,
                                              _ptr(lo, hold), _ptr(hi, hold), int(split), _ptr(ids, hold), _ptr(dists, hold),
                                              counts.data_ptr() if counts is not None else None)
        if rc < 0:
            raise ValueError("annhip_query_sorted_set refused k=%d split=%d (see its line on stderr)" % (kq, split))
        if stream is not None:  # keep the arrays until the batch has read them
            for t in (lo, hi, rad, ids, dists, counts, hold):
                if t is not None:
                    t.record_stream(stream)
        entries = int(rc)
        if not split:  # the library counted every interval slot; the non-empty runs, without waiting for them
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(y.device)):
                entries = (self.tag_runs_set((where[0], off, lo, hi))[1] != 0).sum()
        return (ids, dists, entries) if rad is None else (ids, dists, counts, entries)

    def query_routed(self, y, where, scan_below=None, k=None, alias=False, ws=None, stream=None, out_ids=None, out_dists=None):
        """query(y, where=where, k=k) with a router in front -> (ids int64 [Q,k], sq dists [Q,k], rc).  scan_below=None is
        that call, nothing else.  With an integer R the queries whose run of the tag order (sort_tags, tag_runs) has at
        most R rows are answered exactly by query_sorted, the others by the ANN path, and both results are scattered into
        one output (the host learns the split: one synchronisation).  ValueError without an order, with alias=True (the
        alias rule names a query by its position in the batch, which a split changes), with a mask other than the order's,
        and as query(where=) and query_sorted raise it."""
        import torch
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        if scan_below is None:
            return self.query(y, alias=alias, out_ids=out_ids, out_dists=out_dists, ws=ws, stream=stream, where=where, k=k)
        if isinstance(scan_below, bool) or not isinstance(scan_below, (int, np.integer)) or scan_below < 0:
            raise ValueError("query_routed: a non-negative integer, got %r" % (scan_below,))
        if where is None:
            raise ValueError("query_routed: where must be given")
        if alias:
            raise ValueError("query_routed: alias names a query by its position in the batch, which a split changes")
        Q = y.shape[0]
        kq = self.k if k is None else self._check_k(k)
        if kq < 1:
            raise ValueError("query(k=...): k must be at least 1")
        qm, qlo, qhi = self._sorted_pred("query_routed", where, Q, y.device)  # an order, and its mask
        pred = (qm, qlo) + ((qhi,) if len(where) == 3 else ())
        cur = torch.cuda.current_stream(y.device)
        run = stream if stream is not None else torch.cuda.default_stream(y.device)  # where the library's launches go
        if cur != run:
            run.wait_stream(cur)
        with torch.cuda.stream(run):
            _, length = self._runs(qlo, qhi)
            short = (length.to(torch.int64) & 0xFFFFFFFF) <= int(scan_below)
            si, li = torch.nonzero(short).reshape(-1), torch.nonzero(~short).reshape(-1)  # (the host learns the split here)
            ids = out_ids if out_ids is not None else torch.empty((Q, kq), dtype=torch.int64, device=y.device)
            dists = out_dists if out_dists is not None else torch.empty((Q, kq), dtype=y.dtype, device=y.device)
            assert tuple(ids.shape) == (Q, kq) and tuple(dists.shape) == (Q, kq)
            rc = 0
            if si.numel():
                i1, d1 = self.query_sorted(y[si].contiguous(), tuple(p[si].contiguous() for p in pred), k=kq, ws=ws, stream=stream)
                ids[si], dists[si] = i1, d1
            if li.numel():
                i2, d2, rc = self.query(y[li].contiguous(), where=tuple(p[li].contiguous() for p in pred), k=k, ws=ws, stream=stream)
                ids[li], dists[li] = i2, d2
            if cur != run:
                for t in (y,) + tuple(pred):
                    t.record_stream(run)
        return ids, dists, rc

    def query(self, y, alias=False, mode=0, out_ids=None, out_dists=None, ws=None, stream=None, where=None, k=None):
        """annhip_query / annhip_query_on: y torch tensor [Q,d] on the device -> (ids int64 [Q,k], sq dists [Q,k], n_exact).
        ws + stream (a torch.cuda.Stream): run this batch on its own workspace and stream so that it can overlap others.
        where = (qmask, qvalue), numpy uint32 [Q] or torch int32 device tensors [Q]: annhip_query_tagged -- fixed mode
        with row i competing for query q iff (tags[i] & qmask[q]) == qvalue[q] (set_tags; the index's filter applies as
        well).  It runs on `stream` (the null stream when none is given) and `ws` (the index's own when none is given).
        ValueError for a wrong shape or dtype and where the library refuses (fixed mode off, no tags); nothing is
        launched then and the outputs are untouched.  where=None is the untagged call.
        k: None = the index's k, the calls above, unchanged.  An integer: annhip_query_k -- fixed mode with the k of this
        call, 1 <= k <= max_query_k, -> (ids int64 [Q,k], sq dists [Q,k], 0); with or without where=, on `stream` / `ws`
        as where= is.  ValueError for a bool or a non-integer and where the library refuses (fixed mode off, k out of
        range, where= without tags, a resharded index); nothing is launched then and the outputs are untouched.
        where = (qmask, qlo, qhi), each as above: annhip_query_between -- row i competes for query q iff
        qlo[q] <= (tags[i] & qmask[q]) <= qhi[q], unsigned; with or without k=, -> (ids, dists, rc); refusals as above.
        query_routed(y, where, scan_below=R) is this call with the selective queries answered exactly by query_sorted."""
        import torch
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q = y.shape[0]
        if where is not None or k is not None:  # the entries of fixed mode
            kq = self.k if k is None else self._check_k(k)
            if kq < 1:
                raise ValueError("query(k=...): k must be at least 1")
            pred = _where_dev(where, Q, y.device) if where is not None else None
            if k is None and len(pred) == 2 and not self.has_tags:  # (the other forms leave this to the library)
                raise ValueError("query(where=...): the index has no tags (Index.set_tags)")
            ids, dists, _, rc = self._fixed_call(self._fixed_entry(pred, k is not None, False), y, alias, kq, None, pred,
                                                 out_ids, out_dists, ws, stream)
            return ids, dists, rc
        ids = out_ids if out_ids is not None else torch.empty((Q, self.k), dtype=torch.int64, device=y.device)
        dists = out_dists if out_dists is not None else torch.empty((Q, self.k), dtype=y.dtype, device=y.device)
        if ws is None and stream is None:
            nex = self.lib.annhip_query(self.h, Q, y.data_ptr(), int(alias), mode, ids.data_ptr(), dists.data_ptr())
        else:
            nex = self.lib.annhip_query_on(self.h, ws, stream.cuda_stream if stream is not None else None, Q, y.data_ptr(),
                                           int(alias), mode, ids.data_ptr(), dists.data_ptr())
        return ids, dists, nex

    # Which C entry a call takes -- the same one for every argument combination as ever -- as (name, the tail of its
    # ValueError, its arguments after `alias`: made from kq, the radius, the predicate's pointers, (ids, dists), counts).
    # pred: None, a pair or a triple of arrays; k_given / radius: the call names a k of its own / is a radius call.
    @staticmethod
    def _fixed_entry(pred, k_given, radius):
        refused = "k=%(k)d (fixed mode off, k outside 1..%(kmax)d, no tags, or a resharded index)"
        if pred is not None and len(pred) == 3:
            return "annhip_query_between", refused, lambda kq, r, q, o, c: (kq, r) + q + o + (c,)
        if radius:
            return "annhip_query_radius", refused, lambda kq, r, q, o, c: (kq, r) + q + o + (c,)
        if k_given:
            return "annhip_query_k", refused, lambda kq, r, q, o, c: (kq,) + q + o
        return "annhip_query_tagged", "(fixed mode off, or no tags)", lambda kq, r, q, o, c: q + o

    @staticmethod
    def _exact_entry(pred, k_given, radius):
        refused = "k=%(k)d (k outside 1..1024 or larger than the rows on offer, no tags, or a resharded index)"
        if pred is not None and len(pred) == 3:
            return "annhip_index_exact_query_between", refused, lambda kq, r, q, o, c: (kq, r) + q + o + (c,)
        if radius:
            return "annhip_index_exact_query_radius", refused, lambda kq, r, q, o, c: (kq, r) + q + o + (c,)
        if k_given:
            return "annhip_index_exact_query_k", refused, lambda kq, r, q, o, c: (kq,) + q + o
        if pred is not None:
            return ("annhip_index_exact_query_tagged", "this index (no tags, resharded, or k larger than the rows on offer)",
                    lambda kq, r, q, o, c: q + o)
        return ("annhip_index_exact_query", "this index (resharded, or k larger than the rows on offer)",
                lambda kq, r, q, o, c: o)

    def _fixed_call(self, entry, y, alias, kq, rad, pred, out_ids, out_dists, ws, stream):
        """One call of a fixed-mode entry (_fixed_entry) on `stream` / `ws` -> (ids, dists, counts, rc); counts is None
        without a radius.  The outputs, the order of the two streams, the ValueError of a refusal, and every device tensor
        of the call kept until `stream` has passed it."""
        import torch
        name, refused, layout = entry
        Q = y.shape[0]
        ids = out_ids if out_ids is not None else torch.empty((Q, kq), dtype=torch.int64, device=y.device)
        dists = out_dists if out_dists is not None else torch.empty((Q, kq), dtype=y.dtype, device=y.device)
        assert tuple(ids.shape) == (Q, kq) and tuple(dists.shape) == (Q, kq) and ids.is_contiguous() and dists.is_contiguous()
        counts = torch.zeros((Q,), dtype=torch.int32, device=y.device) if rad is not None else None
        given = tuple(t for t in (pred or ()) + (rad,) if t is not None)
        if given and stream is not None and torch.cuda.current_stream(y.device) != stream:
            stream.wait_stream(torch.cuda.current_stream(y.device))  # the predicate, radius and output arrays were made on that one
        # (a radius call may have no rows: the library wants non-NULL radius and ids pointers then)
        hold = torch.empty((1,), dtype=torch.int64, device=y.device) if rad is not None else None
        rc = getattr(self.lib, name)(
            self.h, ws, stream.cuda_stream if stream is not None else None, Q, y.data_ptr(), int(alias),
            *layout(kq, _ptr(rad, hold) if rad is not None else None,
                    tuple(t.data_ptr() for t in pred) if pred is not None else (None, None),
                    (_ptr(ids, hold) if rad is not None else ids.data_ptr(), dists.data_ptr()),
                    counts.data_ptr() if counts is not None else None))
        if rc == -2:
            raise ValueError("%s refused %s" % (name, refused % {"k": kq, "kmax": self.max_query_k}))
        if stream is not None:  # the arrays may be freed once this call returns: keep them until the batch has read them
            for t in (y, ids, dists) + given + tuple(t for t in (counts, hold) if t is not None):
                t.record_stream(stream)
        return ids, dists, counts, rc

    def _exact_call(self, entry, y, alias, kq, rad, pred):
        """One call of an exact entry (_exact_entry), synchronous on the null stream -> (ids, dists, counts); counts is
        None without a radius.  ValueError where the library refuses."""
        import torch
        name, refused, layout = entry
        Q = y.shape[0]
        ids = torch.empty((Q, kq), dtype=torch.int64, device=y.device)
        dists = torch.empty((Q, kq), dtype=y.dtype, device=y.device)
        counts = torch.zeros((Q,), dtype=torch.int32, device=y.device) if rad is not None else None
        torch.cuda.current_stream(y.device).synchronize()  # the scan runs on the null stream
        hold = torch.empty((1,), dtype=torch.int64, device=y.device)  # (an empty batch: the radius entries refuse NULL arrays)
        if getattr(self.lib, name)(
                self.h, Q, y.data_ptr(), int(bool(alias)),
                *layout(kq, _ptr(rad, hold) if rad is not None else None,
                        tuple(t.data_ptr() for t in pred) if pred is not None else (None, None),
                        (_ptr(ids, hold), _ptr(dists, hold)), counts.data_ptr() if counts is not None else None)) != 0:
            raise ValueError("%s refused %s" % (name, refused % {"k": kq}))
        return ids, dists, counts

    def exact_query(self, y, alias=False, where=None, k=None):
        """annhip_index_exact_query: the exact k nearest of the index's (native) rows for y [Q,d], k = the index's k ->
        (ids int64 [Q,k], sq dists [Q,k]), ordered by (distance, id).  alias: query q leaves out point q.  ValueError where
        the library refuses (a resharded index).  where = (qmask, qvalue) as in query(): annhip_index_exact_query_tagged,
        the exact neighbours among the rows that pass query q's tag test (and the index's filter); ValueError for a wrong
        shape or dtype and for an index without tags.
        k: None = the index's k, the calls above.  An integer: annhip_index_exact_query_k, the exact k nearest ->
        [Q,k] tensors; ValueError for a bool or a non-integer and where the library refuses (k outside 1..1024,
        k > n - alias, a resharded index, where= without tags).  where = (qmask, qlo, qhi) as in query():
        annhip_index_exact_query_between, with or without k=."""
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q = y.shape[0]
        kq = self.k if k is None else self._check_k(k)
        if kq < 1:
            raise ValueError("exact_query(k=...): k must be in 1..1024")
        pred = _where_dev(where, Q, y.device) if where is not None else None
        if pred is not None and (k is None or len(pred) == 3) and not self.has_tags:  # (k= with a pair leaves it to the library)
            raise ValueError("exact_query(where=...): the index has no tags (Index.set_tags)")
        return self._exact_call(self._exact_entry(pred, k is not None, False), y, alias, kq, None, pred)[:2]

    def rerank(self, y, cand, k=None, stream=None, out_ids=None, out_dists=None):
        """annhip_index_rerank: the exact top-k of caller-supplied candidates on the index's NATIVE rows (whatever set_rows
        says, fixed mode on or off).  y [Q,d], cand a contiguous int64 [Q,C] device tensor of row ids over [0, n_total):
        the built rows, then the tail -> (ids int64 [Q,k], sq dists [Q,k]), the k smallest (distance, id) among each
        query's distinct in-range candidates, padded with (n_total, +inf).  Entries >= n_total are skipped, a repeated id
        counts once, k may exceed C; k=None: the index's k.  No allow list, tags, probe or alias rule applies: the caller
        chose the candidates.  Distances are bit for bit query()'s and exact_query()'s on native rows.  Runs on `stream`
        (the null stream when none is given) and returns at once; out_ids may be cand where C == k.  ValueError for a
        cand that is not a contiguous int64 [Q,C] device tensor, a bool or non-integer k, and where the library refuses
        (k or C outside 1..1024, a row too long for the LDS of one CU, a resharded index); nothing is launched then and
        the outputs are untouched."""
        import torch
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q = y.shape[0]
        C_ = _check_cand("Index.rerank", cand, Q, y.device)
        k = self.k if k is None else self._check_k(k)
        if k < 0:
            raise ValueError("Index.rerank: k must be in 1..1024")
        ids, dists = _rerank_out("Index.rerank", out_ids, out_dists, Q, k, y.dtype, y.device)
        cur = torch.cuda.current_stream(y.device)
        if stream is not None and cur != stream:
            stream.wait_stream(cur)  # the candidate and output arrays were made on that one
        hold = torch.empty((1,), dtype=torch.int64, device=y.device)
        rc = self.lib.annhip_index_rerank(self.h, stream.cuda_stream if stream is not None else None, Q, _ptr(y, hold), C_,
                                          _ptr(cand, hold), k, _ptr(ids, hold), _ptr(dists, hold))
        if rc != 0:
            raise ValueError("annhip_index_rerank refused C=%d k=%d (k or C outside 1..1024, a row too long for the LDS of one "
                             "CU, or a resharded index)" % (C_, k))
        if stream is not None:  # keep the arrays until the batch has read them
            for t in (y, cand, ids, dists, hold):
                t.record_stream(stream)
        return ids, dists

    def query_reranked(self, y, k=None, oversample=2, alias=False, where=None, ws=None, stream=None):
        """query(k=min(max_query_k, k * oversample)) on the rows the index is set to, then rerank(..., k) of those
        candidates on the native rows, both on `stream` -> (ids int64 [Q,k], sq dists [Q,k]).  With narrow rows
        (set_rows) this is the usual two-step scheme: search the cheap rows for a few more candidates than needed, re-score
        them at full precision; the distances that come back are the native rows'.  k=None: the index's k.  Fixed mode
        only, as query(k=); alias, where, ws and stream as there (they shape the candidates; rerank itself tests nothing).
        ValueError for oversample < 1 or a non-integer oversample, and as query(k=) and rerank raise it."""
        if isinstance(oversample, bool) or not isinstance(oversample, (int, np.integer)) or oversample < 1:
            raise ValueError("query_reranked: oversample must be an integer >= 1, got %r" % (oversample,))
        k = self.k if k is None else self._check_k(k)
        if k < 1:
            raise ValueError("query_reranked: k must be at least 1")
        kq = min(self.max_query_k, k * int(oversample))
        cand, _, _ = self.query(y, alias=alias, ws=ws, stream=stream, where=where, k=kq)
        return self.rerank(y, cand, k=k, stream=stream)

    def query_radius(self, y, radius, k=None, alias=False, where=None, ws=None, stream=None):
        """annhip_query_radius: fixed mode's candidates within a squared-L2 radius, capped at k per query (k=None: the
        index's k) -> (ids int64 [Q,k], sq dists [Q,k], counts int32 [Q]): rows ascending by (distance, id), padded with
        (n_total, +inf); counts[q] == k means there may be more.  radius: a Python float, broadcast; a device tensor [Q] of
        the index's dtype; or a numpy array [Q] of that dtype, copied.  A row is in range iff dist <= radius; a negative or
        NaN radius matches nothing, +inf gives the row of query(k=k) bit for bit.  where, ws and stream as in query(k=).
        ValueError for a bool or non-integer k, for a radius of wrong shape or dtype, and where the library refuses (fixed
        mode off, k outside 1..max_query_k, where= without tags, a resharded index); nothing is launched then."""
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q = y.shape[0]
        k = self.k if k is None else self._check_k(k)
        if k < 1:
            raise ValueError("query_radius: k must be at least 1")
        rad = _radius_dev(radius, Q, y.dtype, y.device)
        pred = _where_dev(where, Q, y.device) if where is not None else None
        return self._fixed_call(self._fixed_entry(pred, True, True), y, alias, k, rad, pred, None, None, ws, stream)[:3]

    def exact_query_radius(self, y, radius, k, alias=False, where=None):
        """annhip_index_exact_query_radius: the ground truth of query_radius -- exact_query(k=k) cut at the radius ->
        (ids int64 [Q,k], sq dists [Q,k], counts int32 [Q]), padded with (n_total, +inf).  radius and where as in
        query_radius.  ValueError as exact_query(k=) raises it, and for a radius of wrong shape or dtype."""
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        Q = y.shape[0]
        k = self._check_k(k)
        if k < 1:
            raise ValueError("exact_query_radius: k must be in 1..1024")
        rad = _radius_dev(radius, Q, y.dtype, y.device)
        pred = _where_dev(where, Q, y.device) if where is not None else None
        return self._exact_call(self._exact_entry(pred, True, True), y, alias, k, rad, pred)

    def _group_args(self, what, y, group, k, per_group, candidates, oversample, where, kmax):
        """What query_grouped and exact_query_grouped share -> (gmask, k, per_group, K', the three predicate tensors or
        None); ValueError for a bool or non-integer argument, k or per_group < 1, K' outside k..kmax, a group mask that is
        no non-zero 32-bit word, a where of wrong shape or dtype and an index without tags."""
        assert y.is_cuda and y.is_contiguous() and y.dtype == self._torch_ft(self.prec) and y.shape[1] == self.d
        gmask, k, per_group = _check_group(what, group, self.k if k is None else k, per_group)
        if candidates is None:
            if isinstance(oversample, bool) or not isinstance(oversample, (int, np.integer)) or oversample < 1:
                raise ValueError("%s: oversample must be an integer >= 1, got %r" % (what, oversample))
            candidates = min(kmax, k * int(oversample))
        elif isinstance(candidates, bool) or not isinstance(candidates, (int, np.integer)):
            raise ValueError("%s: candidates must be an integer, got %r" % (what, candidates))
        kc = int(candidates)
        if not k <= kc <= kmax:
            raise ValueError("%s: candidates = %d must be in k = %d .. %d" % (what, kc, k, kmax))
        if not self.has_tags:
            raise ValueError("%s: the index has no tags (Index.set_tags)" % what)
        pred = _where_dev(where, y.shape[0], y.device) if where is not None else None
        if pred is not None and len(pred) == 2:  # the pair is the range whose two bounds are the value
            pred = (pred[0], pred[1], pred[1])
        return gmask, k, per_group, kc, pred

    def query_grouped(self, y, group, k=None, per_group=1, candidates=None, oversample=4, where=None, alias=False, ws=None,
                      stream=None):
        """annhip_query_grouped: fixed mode's k nearest with at most per_group rows of each group ("the k nearest
        documents, not the k nearest chunks") -> (ids int64 [Q,k], sq dists [Q,k], counts int32 [Q], short bool [Q]).
        group: the mask whose bits of the tag word (set_tags, append(tags=)) are the group key.  The row is collapse()
        of the row of query(k=candidates, where=where): ascending (distance, id), padded with (n_total, +inf);
        counts = entries that are no pads.  short[q]: fewer than k groups among a full list of candidates -- ask again
        with more; where short[q] is False the row is exact for the ordering the candidates are a prefix of.  k=None: the
        index's k; candidates=None: min(max_query_k, k * oversample).  where (pair or triple), alias, ws and stream as in
        query(k=).  ValueError for a bool or non-integer argument, for k or per_group < 1, candidates outside
        k..max_query_k, a group that is no non-zero 32-bit mask, an index without tags, and where the library refuses
        (fixed mode off, a resharded index); nothing is launched then."""
        import torch
        gmask, k, per_group, kc, pred = self._group_args("query_grouped", y, group, k, per_group, candidates, oversample, where,
                                                         self.max_query_k)
        Q = y.shape[0]
        ids = torch.empty((Q, k), dtype=torch.int64, device=y.device)
        dists = torch.empty((Q, k), dtype=y.dtype, device=y.device)
        counts = torch.zeros((Q,), dtype=torch.int32, device=y.device)
        short = torch.zeros((Q,), dtype=torch.uint8, device=y.device)
        cur = torch.cuda.current_stream(y.device)
        if stream is not None and cur != stream:
            stream.wait_stream(cur)  # the predicate and output arrays were made on that one
        hold = torch.empty((1,), dtype=torch.int64, device=y.device)  # (an empty batch: the library refuses a NULL ids array)
        rc = self.lib.annhip_query_grouped(self.h, ws, stream.cuda_stream if stream is not None else None, Q, y.data_ptr(),
                                           int(bool(alias)), kc, k, per_group, gmask,
                                           *(tuple(t.data_ptr() for t in pred) if pred is not None else (None, None, None)),
                                           _ptr(ids, hold), dists.data_ptr(), counts.data_ptr(), short.data_ptr())
        if rc != 0:
            raise ValueError("annhip_query_grouped refused candidates=%d k=%d per_group=%d (fixed mode off, candidates outside "
                             "1..%d, or a resharded index)" % (kc, k, per_group, self.max_query_k))
        if stream is not None:  # keep the arrays until the batch has read them
            for t in (y, ids, dists, counts, short, hold) + (pred or ()):
                t.record_stream(stream)
            if cur != stream:
                cur.wait_stream(stream)  # short.bool() below runs on the current stream
        return ids, dists, counts, short.bool()

    def exact_query_grouped(self, y, group, k=None, per_group=1, candidates=None, oversample=4, where=None, alias=False):
        """annhip_index_exact_query_grouped: the ground truth of query_grouped -- collapse() of the row of
        exact_query(k=candidates, where=where) on the native rows -> (ids, dists, counts, short) as there.  Where
        short[q] is False the row is the collapse of ALL valid rows in (distance, id) order.  candidates=None:
        min(1024, k * oversample).  Synchronous.  ValueError as query_grouped raises it, with 1024 in the place of
        max_query_k, and where the library refuses (candidates beyond the rows on offer, a resharded index)."""
        import torch
        gmask, k, per_group, kc, pred = self._group_args("exact_query_grouped", y, group, k, per_group, candidates, oversample,
                                                         where, 1024)
        Q = y.shape[0]
        ids = torch.empty((Q, k), dtype=torch.int64, device=y.device)
        dists = torch.empty((Q, k), dtype=y.dtype, device=y.device)
        counts = torch.zeros((Q,), dtype=torch.int32, device=y.device)
        short = torch.zeros((Q,), dtype=torch.uint8, device=y.device)
        torch.cuda.current_stream(y.device).synchronize()  # the scan runs on the null stream
        hold = torch.empty((1,), dtype=torch.int64, device=y.device)
        rc = self.lib.annhip_index_exact_query_grouped(
            self.h, Q, y.data_ptr(), int(bool(alias)), kc, k, per_group, gmask,
            *(tuple(t.data_ptr() for t in pred) if pred is not None else (None, None, None)),
            _ptr(ids, hold), _ptr(dists, hold), counts.data_ptr(), short.data_ptr())
        if rc != 0:
            raise ValueError("annhip_index_exact_query_grouped refused candidates=%d k=%d per_group=%d (candidates beyond the "
                             "rows on offer, or a resharded index)" % (kc, k, per_group))
        return ids, dists, counts, short.bool()

    def host_stream(self, max_ycnt, lanes=3):
        """annhip_stream_open: pipeline for host-resident (numpy) batches; see HostStream."""
        return HostStream(self, max_ycnt, lanes)

    def checksum(self):
        """annhip_index_checksum: 64-bit checksum of everything a query reads except the point rows."""
        return int(self.lib.annhip_index_checksum(self.h))

    def profile(self, on=True):
        self.lib.annhip_profile(self.h, int(on))

    def stats(self, reset=False):
        out = (C.c_double * 8)()
        self.lib.annhip_stats(self.h, C.byref(out), int(reset))
        return dict(s1_launches=out[0], s1_ms=out[1], s1_rows=out[2], other_rows=out[3], exact_queries=out[4],
                    queries=out[5], tie_queries=out[6],  # tie_queries: flagged queries answered without the network (ann_tie.h)
                    uncertified_queries=out[7])         # set_prune: flagged because the certificate failed

    def stage_ms(self):
        out = (C.c_double * 6)()
        self.lib.annhip_stage_ms(self.h, C.byref(out))
        return dict(zip(("codes", "stage1", "finalize_fallback", "stage2_rows", "stage2_network", "widen"), [float(v) for v in out]))

    def close(self):
        if self.h:
            for ws in getattr(self, "_workspaces", []):
                self.lib.annhip_workspace_destroy(ws)
            self._workspaces = []
            self.lib.annhip_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
