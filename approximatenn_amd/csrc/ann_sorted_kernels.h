// ann_sorted_kernels.h -- the tag order of an index and the exact scan of its runs (annhip_index_sort_tags,
// annhip_tag_runs, annhip_query_sorted; gfx950).
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
__device__ __forceinline__ void sorted_load_list(const SortedArgs &SA, u32 *trip, u32 G, u32 e0, u32 ne) {
  for (u32 i = threadIdx.x; i < G; i += blockDim.x) {
    const bool live = i < ne;
    const u32 *src = SA.list + 3 * (size_t)(e0 + (live ? i : ne - 1));
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

template <int D, int V>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void sorted_scan_kernel(SortedArgs SA) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
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
  sorted_load_list(SA, trip, G, e0, ne);
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
  tail_store<0>(S, A, qi[0], ebase + 0 < ne);
  tail_store<1>(S, A, qi[1], ebase + 1 < ne);
  tail_store<2>(S, A, qi[2], ebase + 2 < ne);
  tail_store<3>(S, A, qi[3], ebase + 3 < ne);
  if (A.scored && threadIdx.x == 0 && nf) atomicAdd(&A.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nf);
}
static_assert(ANN_EX_QB == 4, "sorted_scan_kernel names its four queries");

// Any d without a register layout: tail_merge_generic_kernel's literal in-place tree over the spans of the order.  V is a
// kernel argument here (bits NULL or not): this form is bound by its LDS tree.
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void sorted_scan_generic_kernel(SortedArgs SA) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
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
  sorted_load_list(SA, trip, G, e0, ne);
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
#define ANN_SORTED_GEN_STORE(I) \
  tail_store<I>(S, A, __builtin_amdgcn_readfirstlane(trip[ebase + (I)]), ebase + (I) < ne);
  ANN_SORTED_GEN_STORE(0) ANN_SORTED_GEN_STORE(1) ANN_SORTED_GEN_STORE(2) ANN_SORTED_GEN_STORE(3)
#undef ANN_SORTED_GEN_STORE
  if (A.scored && threadIdx.x == 0 && nf) atomicAdd(&A.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nf);
}
