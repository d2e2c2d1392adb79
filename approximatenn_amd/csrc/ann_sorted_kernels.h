// ann_sorted_kernels.h -- the tag order of an index and the exact scan of its runs (annhip_index_sort_tags,
// annhip_tag_runs, annhip_query_sorted, annhip_tag_runs_set, annhip_query_sorted_set; gfx950).
//
// The order: perm[ms] = the row ids sorted by (tags[id] & field_mask, id), keys[ms] = the masked words in that order.  A
// predicate qlo <= (tag & field_mask) <= qhi then selects ONE contiguous run [start, end) of positions of the order, found
// with two binary searches (tag_runs_kernel), and the rows that compete for the query are perm[start .. end): the scan
// costs what the predicate admits, not n_total.
//
// The sort (not on the hot path): a least-significant-digit radix sort of (key, id) pairs, 8 bits per pass, stable, in
// the style of thash_count / scan / place -- tsort_count_kernel, tsort_scan_kernel, tsort_place_kernel.  One wave owns
// ANN_SORT_ITEMS consecutive pairs per pass and ranks them in order, so equal masked words stay ordered by id.
//
// The scan: sorted_scan_kernel<D, V> is tail_merge_kernel (ann_tail_kernels.h) over the runs of the order instead of the
// tail.  The batch's queries are ordered by (start, end, q) first (sorted_order_kernel), and one workgroup takes
// G = W x ANN_EX_QB consecutive entries of that list: queries of one tenant sit in one workgroup and share every tile.
// The workgroup cuts its entries into spans -- maximal groups of consecutive entries whose runs overlap or touch -- and
// streams each span once, tile by tile: perm[pos ..] into LDS, the rows of those ids gathered into the LDS tile (from the
// built rows for id < n, from the tail for id >= n), the allow-list bit of every tile row into an LDS flag word (the ids
// are scattered: a slice of bitmap words does not serve).  Every wave scores the tile against its four queries with
// ex_reduce<D> -- the query path's bits -- and position pos competes for query i iff start_i <= pos < end_i (one unsigned
// compare in place of the tag test), its flag is set and it is not the aliased self.  The gaps between spans are never
// fetched; a wave none of whose queries meets a tile skips it.  Selection is ExSel, the store tail_store's at the query's
// ORIGINAL position.  Every position is streamed at most once per query (a run lies inside one span), so the keys of a
// query stay distinct, as ex_compact needs.
//
// Known limit: one workgroup streams a whole span, so a single query whose run is millions of rows runs on one CU.
// Long runs are not split over workgroups; such queries belong on the ANN path (Index.query_routed(scan_below=)).
// That remains true of annhip_query_sorted.  annhip_query_sorted_set (the end of this file) lets a query own several entries
// of the list -- one per interval of its set, or one per piece of a run cut at global multiples of split_rows -- so its
// long runs ARE split over workgroups: the entries' results go to partial lists and sorted_set_merge_kernel merges them.
// LDS carve-up: exact_shape(..., sorted = true) on the host: tile, per-wave buffers, then the tile's ids, its flags and the
// workgroup's (q, start, end) triples.  No register prefetch of the next tile.
#pragma once
#include "ann_tail_kernels.h"

// ------------------------------------------------------------------------------------------ the sort
#define ANN_SORT_ITEMS 2048  // pairs one wave ranks per pass

__global__ void tsort_init_kernel(u32 count, const u32 *__restrict__ tags, u32 mask, u32 *__restrict__ keys, u32 *__restrict__ perm) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    keys[i] = tags[i] & mask, perm[i] = (u32)i;
}

// hist[digit * nblk + blk] := the pairs of block blk whose key has that digit (one wave per block)
__global__ __launch_bounds__(64) void tsort_count_kernel(const u32 *__restrict__ keys, u32 count, int shift, u32 nblk,
                                                          u32 *__restrict__ hist) {
  __shared__ u32 h[256];
  const u32 lane = threadIdx.x, blk = blockIdx.x;
  for (u32 i = lane; i < 256; i += 64) h[i] = 0;
  __syncthreads();
  const size_t base = (size_t)blk * ANN_SORT_ITEMS, end = min((size_t)count, base + ANN_SORT_ITEMS);
  for (size_t i = base + lane; i < end; i += 64) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  __syncthreads();
  for (u32 i = lane; i < 256; i += 64) hist[(size_t)i * nblk + blk] = h[i];
}

// exclusive prefix sum of hist[0 .. total) in place: digit-major, so a pair's offset counts every smaller digit and the
// same digit of every earlier block (one workgroup)
__global__ __launch_bounds__(1024) void tsort_scan_kernel(u32 *__restrict__ hist, size_t total) {
  __shared__ u32 part[1024];
  const u32 tid = threadIdx.x;
  u32 carry = 0;
  for (size_t b0 = 0; b0 < total; b0 += 1024) {
    const size_t idx = b0 + tid;
    const u32 v = idx < total ? hist[idx] : 0;
    part[tid] = v;
    __syncthreads();
    for (u32 off = 1; off < 1024; off <<= 1) {
      const u32 t = tid >= off ? part[tid - off] : 0;
      __syncthreads();
      part[tid] += t;
      __syncthreads();
    }
    if (idx < total) hist[idx] = carry + part[tid] - v;
    carry += part[1023];
    __syncthreads();
  }
}

// the pairs of block blk, in order, to their places: offset of (digit, block) + rank among the block's earlier pairs of
// that digit.  One wave per block, 64 pairs at a time: the lanes of one digit find each other with eight ballots.
__global__ __launch_bounds__(64) void tsort_place_kernel(const u32 *__restrict__ keys, const u32 *__restrict__ vals, u32 count,
                                                          int shift, u32 nblk, const u32 *__restrict__ hist,
                                                          u32 *__restrict__ okeys, u32 *__restrict__ ovals) {
  __shared__ u32 h[256];
  const u32 lane = threadIdx.x, blk = blockIdx.x;
  for (u32 i = lane; i < 256; i += 64) h[i] = hist[(size_t)i * nblk + blk];
  __syncthreads();
  const size_t base = (size_t)blk * ANN_SORT_ITEMS, end = min((size_t)count, base + ANN_SORT_ITEMS);
  for (size_t i0 = base; i0 < end; i0 += 64) {
    const size_t i = i0 + lane;
    const bool act = i < end;
    const u32 key = act ? keys[i] : 0, val = act ? vals[i] : 0;
    const u32 dg = (key >> shift) & 255u;
    u64 peers = __ballot(act);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (dg >> b) & 1u;
      const u64 m = __ballot(act && bit);
      peers &= bit ? m : ~m;
    }
    const u32 rank = (u32)__builtin_popcountll(peers & (((u64)1 << lane) - 1));
    const u32 pos = h[act ? dg : 0] + rank;
    __syncthreads();  // every lane has read its offset
    if (act && rank == 0) h[dg] += (u32)__builtin_popcountll(peers);
    __syncthreads();
    if (act) okeys[pos] = key, ovals[pos] = val;
  }
}

// ------------------------------------------------------------------------------------------ the runs
// start = lower_bound(keys, qlo), len = upper_bound(keys, qhi) - start; (0, 0) where qlo > qhi.  One thread per query.
__global__ void tag_runs_kernel(const u32 *__restrict__ keys, u32 ms, u32 Q, const u32 *__restrict__ qlo,
                                const u32 *__restrict__ qhi, u32 *__restrict__ start, u32 *__restrict__ len) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const u32 lo = qlo[q], hi = qhi[q];
  if (lo > hi) {
    start[q] = 0, len[q] = 0;
    return;
  }
  u32 a = 0, b = ms;
  while (a < b) {
    const u32 mid = a + ((b - a) >> 1);
    if (keys[mid] < lo) a = mid + 1;
    else b = mid;
  }
  const u32 s = a;
  b = ms;
  while (a < b) {
    const u32 mid = a + ((b - a) >> 1);
    if (keys[mid] <= hi) a = mid + 1;
    else b = mid;
  }
  start[q] = s, len[q] = a - s;
}

// list[rank(q)] := (q, start, end), rank = the queries that come before q by (start, end, q): Q is thousands, every
// thread counts them all (tiles of 256 through LDS).  Deterministic: the triples are distinct.
__global__ __launch_bounds__(256) void sorted_order_kernel(u32 Q, const u32 *__restrict__ start, const u32 *__restrict__ len,
                                                            u32 *__restrict__ list) {
  __shared__ u32 ss[256], se[256];
  const u32 tid = threadIdx.x, q = blockIdx.x * 256 + tid;
  const bool live = q < Q;
  const u32 ms = live ? start[q] : 0, me = live ? ms + len[q] : 0;
  u32 rank = 0;
  for (u32 t0 = 0; t0 < Q; t0 += 256) {
    __syncthreads();
    const u32 j = t0 + tid;
    ss[tid] = j < Q ? start[j] : 0;
    se[tid] = j < Q ? start[j] + len[j] : 0;
    __syncthreads();
    const u32 cnt = min(256u, Q - t0);
    for (u32 t = 0; t < cnt; t++) {
      const u32 s = ss[t], e = se[t];
      rank += (s < ms || (s == ms && (e < me || (e == me && t0 + t < q)))) ? 1u : 0u;
    }
  }
  if (live) list[3 * (size_t)rank] = q, list[3 * (size_t)rank + 1] = ms, list[3 * (size_t)rank + 2] = me;
}

__global__ void sorted_fill_kernel(u32 count, u32 value, u32 *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) out[i] = value;
}

// ------------------------------------------------------------------------------------------ the scan
// t: tail_merge_kernel's arguments as far as they apply -- tail, y, out_ids, out_d, bits, n (built rows), m (n + m = the
// pad id n_total), Q, d, k, self, tile_rows, cap; scored = the rows fetched into tiles (profiling), 64 padded shards.
struct SortedArgs {
  TailArgs t;
  const FT *points;  // built rows [n][d]
  const u32 *perm;   // the order
  const u32 *list;   // [Q][3]: (q, start, end), ascending by (start, end, q)
};

// the workgroup's entries of the ordered list -> trip[0..G) = q, [G..2G) = start, [2G..3G) = end; an entry beyond the list
// repeats the last query with an empty run (its loads stay inside y; nothing is admitted for it)
// LS: words per list entry -- 3, or 4 in the set form, whose fourth word (the entry's slot) stays in global memory
template <int LS>
__device__ __forceinline__ void sorted_load_list(const SortedArgs &SA, u32 *trip, u32 G, u32 e0, u32 ne) {
  for (u32 i = threadIdx.x; i < G; i += blockDim.x) {
    const bool live = i < ne;
    const u32 *src = SA.list + LS * (size_t)(e0 + (live ? i : ne - 1));
    trip[i] = src[0];
    trip[G + i] = live ? src[1] : 0;
    trip[2 * G + i] = live ? src[2] : 0;
  }
}

// positions [pos0, pos0 + rows) of the order -> their ids and allow-list flags in LDS
template <int V>
__device__ __forceinline__ void sorted_fill_ids(const SortedArgs &SA, u32 *tids, u32 *tflag, u32 pos0, u32 rows) {
  for (u32 i = threadIdx.x; i < rows; i += blockDim.x) {
    const u32 id = SA.perm[pos0 + i];
    tids[i] = id;
    if constexpr (V == EX_BITS) tflag[i] = (SA.t.bits[id >> 5] >> (id & 31u)) & 1u;
  }
}

// the rows of tids[0 .. rows) -> tile (row stride d): ex_fill_tile's cases, one row address per id
__device__ __forceinline__ void sorted_gather_tile(const SortedArgs &SA, FT *tile, const u32 *tids, u32 rows, int d) {
  const u32 n = SA.t.n;
  if (d % ANN_VEC == 0) {
    const u32 ppr = (u32)(d / ANN_VEC);
    VT *t = reinterpret_cast<VT *>(tile);
    for (u32 i = threadIdx.x; i < rows * ppr; i += blockDim.x) {
      const u32 r = i / ppr, c = i - r * ppr, id = tids[r];
      const FT *src = id < n ? SA.points + (size_t)id * d : SA.t.tail + (size_t)(id - n) * d;
      t[i] = reinterpret_cast<const VT *>(src)[c];
    }
  } else {
    for (u32 i = threadIdx.x; i < rows * (u32)d; i += blockDim.x) {
      const u32 r = i / (u32)d, c = i - r * (u32)d, id = tids[r];
      const FT *src = id < n ? SA.points + (size_t)id * d : SA.t.tail + (size_t)(id - n) * d;
      tile[i] = src[c];
    }
  }
}

// the k best of query I of an entry of the set form, ascending, key_max() where the piece had fewer rows -> the entry's
// slot of the partial lists [E][k] (ExSel::store's format)
template <int I>
__device__ __forceinline__ void set_store(ExSel &S, const TailArgs &A, Key *part, u32 slot, bool live) {
  if (!live) return;
  const int lane = lane_id();
  Key *b = S.buf + (size_t)I * S.cap;
  const int c = ex_compact(b, S.cnt[I], A.k, S.out);
  Key *dst = part + (size_t)slot * A.k;
  for (int j = lane; j < A.k; j += ANN_WAVE) dst[j] = j < c ? b[j] : key_max();
}

// SET (annhip_query_sorted_set): the list has four words per entry and entry e's result goes to part[slot(e)], not to the
// output row of its query; everything else is the same code.
struct SortedSetArgs {
  SortedArgs s;  // s.list: [E][4] = (q, start, end, slot), ascending by start; s.t.Q = E; s.t.out_ids / out_d unused
  Key *part;     // [E][k]
};
template <bool SET>
using SortedKernelArgs = std::conditional_t<SET, SortedSetArgs, SortedArgs>;
__device__ __forceinline__ const SortedArgs &sorted_args(const SortedArgs &a) { return a; }
__device__ __forceinline__ const SortedArgs &sorted_args(const SortedSetArgs &a) { return a.s; }
__device__ __forceinline__ Key *sorted_part(const SortedArgs &) { return NULL; }
__device__ __forceinline__ Key *sorted_part(const SortedSetArgs &a) { return a.part; }

template <int D, int V, bool SET = false>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void sorted_scan_kernel(SortedKernelArgs<SET> SX) {
  const SortedArgs &SA = sorted_args(SX);
  Key *part = sorted_part(SX);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
  constexpr int LS = SET ? 4 : 3;
  const TailArgs &A = SA.t;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.d;
  FT *tile = reinterpret_cast<FT *>(smem);
  const size_t tile_bytes = ((size_t)A.tile_rows * d * sizeof(FT) + 15) & ~(size_t)15;
  Key *kbase = reinterpret_cast<Key *>(smem + tile_bytes) + (size_t)w * ((size_t)ANN_EX_QB * A.cap + A.k);
  u32 *tids = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * sizeof(Key) * ((size_t)ANN_EX_QB * A.cap + A.k));
  u32 *tflag = tids + A.tile_rows;
  u32 *trip = tflag + A.tile_rows;
  const u32 G = (u32)W * ANN_EX_QB, e0 = blockIdx.x * G, ne = min(G, A.Q - e0);
  sorted_load_list<LS>(SA, trip, G, e0, ne);
  __syncthreads();
  // first entry of this wave; wave-uniform, which the compiler cannot see: scalar registers, and so are the wave's four
  // (q, start, end)
  const u32 ebase = __builtin_amdgcn_readfirstlane((u32)w * ANN_EX_QB);
  ExSel S;
  S.init(kbase, kbase + (size_t)ANN_EX_QB * A.cap, A.cap, A.k, e0 + ebase, A.Q);
  const ExLanes<D> ln(d, lane);
  VT a[ANN_EX_QB][C];
  u32 qi[ANN_EX_QB], qs[ANN_EX_QB], qn[ANN_EX_QB];  // query, start of its run, rows of its run
#pragma unroll
  for (int i = 0; i < ANN_EX_QB; i++) {
    qi[i] = __builtin_amdgcn_readfirstlane(trip[ebase + i]);
    qs[i] = __builtin_amdgcn_readfirstlane(trip[G + ebase + i]);
    qn[i] = __builtin_amdgcn_readfirstlane(trip[2 * G + ebase + i]) - qs[i];
    const FT *yq = A.y + (size_t)qi[i] * d;
#pragma unroll
    for (int c = 0; c < C; c++) {
      if constexpr (D > 0) a[i][c] = reinterpret_cast<const VT *>(yq)[ln.p + c * ln.oc];
      else a[i][c] = oc_load_chunk<D, false>(yq, ln.p + c * ln.oc, d);
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // the queries have arrived before the loops start (see exact_scan_kernel)
  u32 nf = 0;  // rows this workgroup fetched into tiles (profiling only)
  u32 e = 0;
  while (e < ne) {  // one span per turn; everything here is uniform over the workgroup
    const u32 lo = __builtin_amdgcn_readfirstlane(trip[G + e]);
    u32 hi = __builtin_amdgcn_readfirstlane(trip[2 * G + e]);
    e++;
    while (e < ne && (u32)__builtin_amdgcn_readfirstlane(trip[G + e]) <= hi) {
      hi = max(hi, (u32)__builtin_amdgcn_readfirstlane(trip[2 * G + e]));
      e++;
    }
    for (u32 pos0 = lo; pos0 < hi; pos0 += (u32)A.tile_rows) {
      const u32 rows = min((u32)A.tile_rows, hi - pos0);
      __syncthreads();  // every wave has read the previous tile
      sorted_fill_ids<V>(SA, tids, tflag, pos0, rows);
      __syncthreads();
      sorted_gather_tile(SA, tile, tids, rows, d);
      __syncthreads();  // the tile, its ids and its flags are in LDS
      nf += rows;
      // wave-uniform: does any of the four runs meet [pos0, pos0 + rows)?
      bool meets = false;
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++) meets = meets || (qs[i] < pos0 + rows && qs[i] + qn[i] > pos0);
      if (!meets) continue;
      for (u32 r0 = 0; r0 < rows; r0 += ln.rpw) {
        const u32 r = r0 + ln.g;
        const bool act = ln.valid && r < rows;
        const u32 pos = pos0 + r;
        bool allowed = act && (pos - qs[0] < qn[0] || pos - qs[1] < qn[1] || pos - qs[2] < qn[2] || pos - qs[3] < qn[3]);
        if constexpr (V == EX_BITS) allowed = allowed && tflag[act ? r : r0] != 0;
        if (!__ballot(allowed)) continue;  // wave-uniform: no row of this pass can survive for any of the four queries
        const FT *rp = tile + (size_t)(act ? r : r0) * d;
        VT b[C];
#pragma unroll
        for (int c = 0; c < C; c++) {
          if constexpr (D > 0) b[c] = reinterpret_cast<const VT *>(rp)[ln.p + c * ln.oc];
          else b[c] = oc_load_chunk<D, false>(rp, ln.p + c * ln.oc, d);
        }
        const u32 id = tids[act ? r : r0];
        const bool head = allowed && ln.p == 0;
        // all four trees first (independent chains the scheduler interleaves), then ONE branch for the rare survivors
        Key key[ANN_EX_QB];
        bool pass[ANN_EX_QB];
#pragma unroll
        for (int i = 0; i < ANN_EX_QB; i++) key[i] = key_make(ex_reduce<D>(a[i], b, ln.oc, ln.p, d), id);
#pragma unroll
        for (int i = 0; i < ANN_EX_QB; i++)
          pass[i] = head && pos - qs[i] < qn[i] && !(A.self && id == qi[i]) && key_less(key[i], S.tau[i]);
        if (__ballot(pass[0] || pass[1] || pass[2] || pass[3])) {
          S.offer<0>(pass[0], key[0]);
          S.offer<1>(pass[1], key[1]);
          S.offer<2>(pass[2], key[2]);
          S.offer<3>(pass[3], key[3]);
        }
      }
    }
  }
  if constexpr (SET) {
#define ANN_SET_STORE(I) \
  if (ebase + (I) < ne) set_store<I>(S, A, part, __builtin_amdgcn_readfirstlane(SA.list[LS * (size_t)(e0 + ebase + (I)) + 3]), true);
    ANN_SET_STORE(0) ANN_SET_STORE(1) ANN_SET_STORE(2) ANN_SET_STORE(3)
#undef ANN_SET_STORE
  } else {
    tail_store<0>(S, A, qi[0], ebase + 0 < ne);
    tail_store<1>(S, A, qi[1], ebase + 1 < ne);
    tail_store<2>(S, A, qi[2], ebase + 2 < ne);
    tail_store<3>(S, A, qi[3], ebase + 3 < ne);
  }
  if (A.scored && threadIdx.x == 0 && nf) atomicAdd(&A.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nf);
}
static_assert(ANN_EX_QB == 4, "sorted_scan_kernel names its four queries");

// Any d without a register layout: tail_merge_generic_kernel's literal in-place tree over the spans of the order.  V is a
// kernel argument here (bits NULL or not): this form is bound by its LDS tree.
template <bool SET = false>
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void sorted_scan_generic_kernel(SortedKernelArgs<SET> SX) {
  const SortedArgs &SA = sorted_args(SX);
  Key *part = sorted_part(SX);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int LS = SET ? 4 : 3;
  const TailArgs &A = SA.t;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.d;
  int NP = ANN_EX_GEN_ELEMS / d;
  NP = NP < 1 ? 1 : (NP > ANN_WAVE ? ANN_WAVE : NP);
  FT *tile = reinterpret_cast<FT *>(smem);
  const size_t tile_bytes = ((size_t)A.tile_rows * d * sizeof(FT) + 15) & ~(size_t)15;
  const size_t wave_ft = ((size_t)(1 + NP) * d * sizeof(FT) + 15) & ~(size_t)15;  // yq[d], m[NP][d]
  const size_t wave_bytes = wave_ft + sizeof(Key) * ((size_t)ANN_EX_QB * A.cap + A.k);
  unsigned char *wb = smem + tile_bytes + (size_t)w * wave_bytes;
  FT *yq = reinterpret_cast<FT *>(wb), *m = yq + d;
  Key *kbase = reinterpret_cast<Key *>(wb + wave_ft);
  u32 *tids = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * wave_bytes);
  u32 *tflag = tids + A.tile_rows;
  u32 *trip = tflag + A.tile_rows;
  const bool bits = A.bits != NULL;
  const u32 G = (u32)W * ANN_EX_QB, e0 = blockIdx.x * G, ne = min(G, A.Q - e0);
  sorted_load_list<LS>(SA, trip, G, e0, ne);
  __syncthreads();
  const u32 ebase = __builtin_amdgcn_readfirstlane((u32)w * ANN_EX_QB);
  ExSel S;
  S.init(kbase, kbase + (size_t)ANN_EX_QB * A.cap, A.cap, A.k, e0 + ebase, A.Q);
  int sh0 = 0;  // d <= 1 << sh0
  while ((1 << sh0) < d) sh0++;
  const FT zero = 0;
  u32 nf = 0;
  u32 e = 0;
  while (e < ne) {
    const u32 lo = __builtin_amdgcn_readfirstlane(trip[G + e]);
    u32 hi = __builtin_amdgcn_readfirstlane(trip[2 * G + e]);
    e++;
    while (e < ne && (u32)__builtin_amdgcn_readfirstlane(trip[G + e]) <= hi) {
      hi = max(hi, (u32)__builtin_amdgcn_readfirstlane(trip[2 * G + e]));
      e++;
    }
    for (u32 pos0 = lo; pos0 < hi; pos0 += (u32)A.tile_rows) {
      const u32 rows = min((u32)A.tile_rows, hi - pos0);
      __syncthreads();
      if (bits) sorted_fill_ids<EX_BITS>(SA, tids, tflag, pos0, rows);
      else sorted_fill_ids<EX_ALL>(SA, tids, tflag, pos0, rows);
      __syncthreads();
      sorted_gather_tile(SA, tile, tids, rows, d);
      __syncthreads();
      nf += rows;
#define ANN_SORTED_GEN_QUERY(I)                                                                              \
  if (ebase + (I) < ne) {                                                                                    \
    const u32 qq = __builtin_amdgcn_readfirstlane(trip[ebase + (I)]);                                        \
    const u32 s0 = __builtin_amdgcn_readfirstlane(trip[G + ebase + (I)]);                                    \
    const u32 cn = __builtin_amdgcn_readfirstlane(trip[2 * G + ebase + (I)]) - s0;                           \
    if (s0 < pos0 + rows && s0 + cn > pos0) {                                                                \
      ANN_EX_GEN_QUERY(qq, {                                                                                 \
        const bool in = lane < np;                                                                           \
        const u32 id = tids[in ? r0 + lane : r0];                                                            \
        const bool act = in && pos0 + r0 + lane - s0 < cn && (!bits || tflag[r0 + lane] != 0) &&             \
                         !(A.self && id == qq);                                                              \
        const Key key = key_make(act ? m[lane * d] : zero, id);                                              \
        wave_lds_sync(); /* m is rewritten by the next batch */                                              \
        S.offer<I>(act && key_less(key, S.tau[I]), key);                                                     \
      })                                                                                                     \
    }                                                                                                        \
  }
      ANN_SORTED_GEN_QUERY(0) ANN_SORTED_GEN_QUERY(1) ANN_SORTED_GEN_QUERY(2) ANN_SORTED_GEN_QUERY(3)
#undef ANN_SORTED_GEN_QUERY
    }
  }
#define ANN_SORTED_GEN_STORE(I)                                                                                          \
  if constexpr (SET) {                                                                                                   \
    if (ebase + (I) < ne)                                                                                                \
      set_store<I>(S, A, part, __builtin_amdgcn_readfirstlane(SA.list[LS * (size_t)(e0 + ebase + (I)) + 3]), true);      \
  } else {                                                                                                               \
    tail_store<I>(S, A, __builtin_amdgcn_readfirstlane(trip[ebase + (I)]), ebase + (I) < ne);                            \
  }
  ANN_SORTED_GEN_STORE(0) ANN_SORTED_GEN_STORE(1) ANN_SORTED_GEN_STORE(2) ANN_SORTED_GEN_STORE(3)
#undef ANN_SORTED_GEN_STORE
  if (A.scored && threadIdx.x == 0 && nf) atomicAdd(&A.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nf);
}

// ------------------------------------------------------------------------------------------ sets of intervals
// annhip_tag_runs_set / annhip_query_sorted_set (include/ann_hip.h).  Query q owns the intervals [off[q], off[q + 1]) of
// (lo, hi); they are normalised to pairwise disjoint ones, every non-empty run becomes one list entry or -- cut at the
// global positions S, 2S, ... of the order -- several, the entries are ordered by start (tsort_count / scan / place with
// the start as key and the slot as value: ties stay in creation order), scanned by the set form of the scan above into
// part[E][k], and merged per query.  The slots of one query are consecutive: [eoff[off[q]], eoff[off[q + 1]]).
#define ANN_SET_MAX 256  // intervals per query

// One thread per query.  Its intervals, copied to start / len, are ordered there by (lo, hi); empty ones and those covered
// by an earlier one become (1, 0), the others are clipped to begin above the largest hi before them (nothing follows
// hi = 0xFFFFFFFF: hi + 1 is never formed then).  nlo / nhi (may be NULL) := the normalised intervals; start / len := their
// runs as tag_runs_kernel finds them, (0, 0) for the emptied slots; qof (may be NULL) := q; cnt (may be NULL) := the list
// entries of the slot: 1 with S = 0, else the pieces of a non-empty run.
__global__ void set_runs_kernel(const u32 *__restrict__ keys, u32 ms, u32 Q, const u32 *__restrict__ off, const u32 *__restrict__ lo,
                                const u32 *__restrict__ hi, u32 S, u32 *__restrict__ nlo, u32 *__restrict__ nhi, u32 *start, u32 *len,
                                u32 *__restrict__ qof, u32 *__restrict__ cnt) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const u32 a = off[q], b = off[q + 1];
  for (u32 j = a; j < b; j++) {  // insertion sort by (lo, hi): at most ANN_SET_MAX items
    const u32 l = lo[j], h = hi[j];
    u32 i = j;
    while (i > a && (start[i - 1] > l || (start[i - 1] == l && len[i - 1] > h))) {
      start[i] = start[i - 1], len[i] = len[i - 1];
      i--;
    }
    start[i] = l, len[i] = h;
  }
  bool any = false, full = false;
  u32 top = 0;  // the largest hi so far
  for (u32 j = a; j < b; j++) {
    u32 l = start[j], h = len[j];
    bool live = l <= h && !full;
    if (live && any) {
      if (h <= top) live = false;
      else l = max(l, top + 1);  // top < 0xFFFFFFFF: not full
    }
    if (live) any = true, top = h, full = h == 0xFFFFFFFFu;
    else l = 1, h = 0;
    if (nlo) nlo[j] = l, nhi[j] = h;
    u32 s = 0, n = 0;
    if (live) {
      u32 x = 0, y = ms;
      while (x < y) {
        const u32 mid = x + ((y - x) >> 1);
        if (keys[mid] < l) x = mid + 1;
        else y = mid;
      }
      s = x, y = ms;
      while (x < y) {
        const u32 mid = x + ((y - x) >> 1);
        if (keys[mid] <= h) x = mid + 1;
        else y = mid;
      }
      n = x - s;
    }
    start[j] = s, len[j] = n;
    if (qof) qof[j] = q;
    if (cnt) cnt[j] = !S ? 1u : !n ? 0u : (s + n - 1) / S - s / S + 1;
  }
}

// One wave per interval slot j: its entries (q, start, end) to slots eoff[j] ...  S = 0: one entry, the run itself (an empty
// run is an entry that admits nothing).  S > 0: the pieces [max(s, tS), min(e, (t + 1)S)) of a non-empty run.
__global__ __launch_bounds__(256) void set_pieces_kernel(u32 T, const u32 *__restrict__ start, const u32 *__restrict__ len,
                                                          const u32 *__restrict__ qof, const u32 *__restrict__ eoff, u32 S,
                                                          u32 *__restrict__ eq, u32 *__restrict__ es, u32 *__restrict__ ee) {
  const u32 lane = lane_id(), j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= T) return;
  const u32 s = start[j], n = len[j], q = qof[j];
  if (!S) {
    if (lane == 0) eq[j] = q, es[j] = s, ee[j] = s + n;
    return;
  }
  if (!n) return;
  const u32 e = s + n, base = eoff[j], first = s / S, np = (e - 1) / S - first + 1;
  for (u32 p = lane; p < np; p += ANN_WAVE) {
    const u64 ps = (u64)(first + p) * S, pe = ps + S;
    eq[base + p] = q, es[base + p] = max(s, (u32)ps), ee[base + p] = pe < (u64)e ? (u32)pe : e;
  }
}

// list[r] := (q, start, end, slot) of the slot that the sort put at rank r
__global__ void set_list_kernel(u32 E, const u32 *__restrict__ slots, const u32 *__restrict__ eq, const u32 *__restrict__ es,
                                const u32 *__restrict__ ee, u32 *__restrict__ list) {
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < E; r += (size_t)gridDim.x * blockDim.x) {
    const u32 v = slots[r];
    list[4 * r] = eq[v], list[4 * r + 1] = es[v], list[4 * r + 2] = ee[v], list[4 * r + 3] = v;
  }
}

// the intervals of rank r of every query for the scan of the rows appended after the sort: (1, 0) where the set is shorter
__global__ void set_rank_kernel(u32 Q, u32 r, const u32 *__restrict__ off, const u32 *__restrict__ nlo, const u32 *__restrict__ nhi,
                                u32 *__restrict__ rlo, u32 *__restrict__ rhi) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const u32 a = off[q], b = off[q + 1];
  const bool has = r < b - a;
  rlo[q] = has ? nlo[a + r] : 1u, rhi[q] = has ? nhi[a + r] : 0u;
}

// One wave per query: the k smallest keys of its partial lists part[e0 .. e1)[k], ascending, unpacked to the output row,
// pad (pad_id, +inf).  Every list is ascending with key_max() last, and the keys are distinct across lists (the pieces
// are disjoint positions of the order).  Lane l owns the lists e0 + l, e0 + l + 64, ...; head[e] (zeroed by the host) is
// how many keys of list e are out; a lane holds the smallest head key of its lists, and each of the k rounds takes the
// wave's smallest and advances that one list.  eoff == NULL: slot j is entry j (S = 0).
__global__ __launch_bounds__(256) void sorted_set_merge_kernel(const Key *__restrict__ part, u32 *__restrict__ head, u32 Q,
                                                                const u32 *__restrict__ off, const u32 *__restrict__ eoff, int k,
                                                                size_t pad_id, size_t *__restrict__ ids, FT *__restrict__ dists) {
  const u32 lane = lane_id();
  const u32 q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= Q) return;
  const u32 e0 = eoff ? eoff[off[q]] : off[q], e1 = eoff ? eoff[off[q + 1]] : off[q + 1];
  size_t *io = ids + (size_t)q * k;
  FT *dout = dists + (size_t)q * k;
  Key cur = key_max();
  u32 mine = 0;  // the list cur came from
  for (u32 e = e0 + lane; e < e1; e += ANN_WAVE) {
    const Key c = part[(size_t)e * k];
    if (key_less(c, cur)) cur = c, mine = e;
  }
  for (int j = 0; j < k; j++) {
    const Key best = wave_min_key(cur);
    const bool none = key_eq(best, key_max());  // wave-uniform
    if (lane == 0) io[j] = none ? pad_id : (size_t)key_id(best), dout[j] = none ? ft_inf() : key_dist(best);
    if (none) continue;
    if (key_eq(cur, best)) {  // one lane: the keys are distinct
      head[mine]++;
      cur = key_max();
      for (u32 e = e0 + lane; e < e1; e += ANN_WAVE) {
        const u32 h = head[e];
        const Key c = h < (u32)k ? part[(size_t)e * k + h] : key_max();
        if (key_less(c, cur)) cur = c, mine = e;
      }
    }
  }
}

// One wave per query: C := the k smallest of A and B, two ascending rows of k (ids, distances) padded with (pad_id, +inf)
// whose keys are distinct, in the same format.  An entry's place is its index plus the entries of the other row below it.
// C is neither A nor B.  (The rows appended after the sort: tail_merge_kernel cannot take the running row as its seed
// twice -- it drops seed entries whose id lies in the range it scans -- so every interval rank is scanned from nothing
// and merged here.)
__global__ __launch_bounds__(256) void set_merge2_kernel(u32 Q, int k, size_t pad_id, const size_t *__restrict__ a_ids,
                                                          const FT *__restrict__ a_d, const size_t *__restrict__ b_ids,
                                                          const FT *__restrict__ b_d, size_t *__restrict__ c_ids, FT *__restrict__ c_d) {
  const int lane = lane_id();
  const u32 q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= Q) return;
  const size_t *ai = a_ids + (size_t)q * k, *bi = b_ids + (size_t)q * k;
  const FT *ad = a_d + (size_t)q * k, *bd = b_d + (size_t)q * k;
  size_t *ci = c_ids + (size_t)q * k;
  FT *cd = c_d + (size_t)q * k;
  auto live = [&](const size_t *ids) {  // the entries before the pads
    int lo = 0, hi = k;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ids[mid] != pad_id) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const int ca = live(ai), cb = live(bi);
  auto place = [&](const size_t *xi, const FT *xd, int cx, const size_t *oi, const FT *od, int co) {
    for (int i = lane; i < cx; i += ANN_WAVE) {
      const Key x = key_make(xd[i], (u32)xi[i]);
      int lo = 0, hi = co;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key_less(key_make(od[mid], (u32)oi[mid]), x)) lo = mid + 1;
        else hi = mid;
      }
      if (i + lo < k) ci[i + lo] = xi[i], cd[i + lo] = xd[i];
    }
  };
  place(ai, ad, ca, bi, bd, cb);
  place(bi, bd, cb, ai, ad, ca);
  for (int j = ca + cb + lane; j < k; j += ANN_WAVE) ci[j] = pad_id, cd[j] = ft_inf();
}
