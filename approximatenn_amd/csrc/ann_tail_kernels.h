// ann_tail_kernels.h -- the appended rows of a built index (annhip_index_append; gfx950).
//
// Rows appended after the build live in a flat tail that every fixed-mode query scans exactly.  tail_merge_kernel is
// exact_scan_kernel (ann_exact_kernels.h) over the tail alone, with two differences:
//   - it STARTS from the answer the index has just produced.  The non-pad keys of the query's result row R(q) seed the
//     wave's ExSel buffer, and when R(q) is full its k-th key is the threshold tau from the first tail row on: nearly
//     every tail row dies in one compare, where a scan from nothing admits every row until k are known;
//   - there are no row ranges and no merge pass: one workgroup streams the WHOLE tail for its W x ANN_EX_QB queries and
//     writes the merged row -- size_t ids, distances, pad (n_total, +inf) -- straight into the call's output arrays.
// The distances come out of the same trees as in exact_scan_kernel (ex_reduce: row_reduce / ex_reduce_pk / row_reduce_oc,
// and the literal in-place tree of the any-d form), so they are the query path's bits.  Tail row j has id n + j.
//
// Validity (ExValid) is what exact_scan_kernel's EX_BITS and EX_TAGS forms test, on ids n + j: the allow-list words and the tag
// words of a tile are staged in LDS behind the waves' buffers and tested before a row is scored.  The bitmap and the tag
// array cover [0, n_total): the index extends its copies on append (ann_host.hip).
//
// The input row may be the output row (the query path merges in place): a wave reads the rows of its own queries before
// it writes them, and no other wave touches them.  in_ids / in_d hold kin <= k entries per query (kin < k only where the
// built rows cannot fill a row: the exact entries on an index with n - alias < k).
// LDS carve-up: exact_shape() on the host, the one that sizes every form of exact_scan_kernel.
#pragma once
#include "ann_tag_kernels.h"

struct TailArgs {
  const FT *tail, *y;      // tail rows [m][d]; queries [Q][d]
  const size_t *in_ids;    // R(q): [Q][kin], ascending by (distance, id), entries with id >= n are pads
  const FT *in_d;
  size_t *out_ids;         // [Q][k]
  FT *out_d;
  const u32 *bits, *tags;  // over ids [0, n_total); NULL where the form does not test them
  const u32 *qmask, *qlo, *qhi;  // the pair form: qlo = qhi = its value array
  unsigned long long *scored;  // profiling: (query, valid tail row) pairs, 64 padded shards; or NULL
  u32 n, m, Q;             // built rows, tail rows, queries
  int d, k, kin, self, tile_rows, cap, prefetch;
};

// R(q) of the wave's query I -> its selection buffer; tau = the k-th key where the row is full
template <int I>
__device__ __forceinline__ void tail_seed(ExSel &S, const TailArgs &A, u32 q, bool live) {
  if (!live) return;
  const int lane = lane_id();
  Key *b = S.buf + (size_t)I * S.cap;
  int c = 0;
  for (int j0 = 0; j0 < A.kin; j0 += ANN_WAVE) {  // kin <= k = cap - ANN_EX_SLACK
    const int j = j0 + lane;
    const size_t id = j < A.kin ? A.in_ids[(size_t)q * A.kin + j] : (size_t)A.n;
    const bool real = id < (size_t)A.n;
    const Key key = key_make(real ? A.in_d[(size_t)q * A.kin + j] : ft_inf(), (u32)id);
    const u64 mm = __ballot(real);
    if (real) b[c + mask_rank(mm)] = key;
    c += __builtin_popcountll(mm);
  }
  wave_lds_sync();
  S.cnt[I] = c;
  if (c >= A.k) S.tau[I] = b[A.k - 1];
}

// the k best of query I, ascending -> the output row; pad (n_total, +inf)
template <int I>
__device__ __forceinline__ void tail_store(ExSel &S, const TailArgs &A, u32 q, bool live) {
  if (!live) return;
  const int lane = lane_id();
  Key *b = S.buf + (size_t)I * S.cap;
  const int c = ex_compact(b, S.cnt[I], A.k, S.out);
  const size_t pad = (size_t)A.n + A.m;
  for (int j = lane; j < A.k; j += ANN_WAVE) {
    A.out_ids[(size_t)q * A.k + j] = j < c ? (size_t)key_id(b[j]) : pad;
    A.out_d[(size_t)q * A.k + j] = j < c ? key_dist(b[j]) : ft_inf();
  }
}

// the validity words of tile [t0, t0 + rows) of the tail (ids n + t0 ...) -> LDS
template <int V>
__device__ __forceinline__ void tail_fill_words(const TailArgs &A, u32 *ttags, u32 *tbits, u32 t0, u32 rows) {
  const u32 id0 = A.n + t0;
  if constexpr (V == EX_TAGS)
    for (u32 i = threadIdx.x; i < rows; i += blockDim.x) ttags[i] = A.tags[id0 + i];
  if constexpr (V != EX_ALL)
    if (A.bits)
      for (u32 i = threadIdx.x; i < ex_tile_words(id0, rows); i += blockDim.x) tbits[i] = A.bits[(id0 >> 5) + i];
}

template <int D, int V>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void tail_merge_kernel(TailArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.d;
  FT *tile = reinterpret_cast<FT *>(smem);
  const size_t tile_bytes = ((size_t)A.tile_rows * d * sizeof(FT) + 15) & ~(size_t)15;
  Key *kbase = reinterpret_cast<Key *>(smem + tile_bytes) + (size_t)w * ((size_t)ANN_EX_QB * A.cap + A.k);
  u32 *ttags = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * sizeof(Key) * ((size_t)ANN_EX_QB * A.cap + A.k));
  u32 *tbits = V == EX_TAGS ? ttags + A.tile_rows : ttags;
  const u32 *__restrict__ bits = V == EX_ALL ? (const u32 *)NULL : A.bits;
  // first query of this wave; the wave index is uniform, which the compiler cannot see: a scalar register, and so are the
  // four ids of the aliased test and the four "query inside the batch" flags
  const u32 qbase = __builtin_amdgcn_readfirstlane((blockIdx.x * W + w) * ANN_EX_QB), qend = A.Q;
  ExSel S;
  S.init(kbase, kbase + (size_t)ANN_EX_QB * A.cap, A.cap, A.k, qbase, qend);
  const ExLanes<D> ln(d, lane);
  VT a[ANN_EX_QB][C];
  u32 qm[ANN_EX_QB], ql[ANN_EX_QB], qs[ANN_EX_QB];  // TagPred (mask, lo, span) of each query; wave-uniform: scalar registers
#pragma unroll
  for (int i = 0; i < ANN_EX_QB; i++) {
    const u32 q = qbase + i < qend ? qbase + i : qend - 1;  // loads stay inside y; the result is never admitted
    const FT *yq = A.y + (size_t)q * d;
    if constexpr (V == EX_TAGS) {
      const u32 qu = __builtin_amdgcn_readfirstlane(q);
      const TagPred tp = tag_pred(A.qmask, A.qlo, A.qhi, qu);
      qm[i] = tp.qm, ql[i] = tp.lo, qs[i] = tp.span;
    } else {
      qm[i] = 0, ql[i] = 0, qs[i] = 0;
    }
#pragma unroll
    for (int c = 0; c < C; c++) {
      if constexpr (D > 0) a[i][c] = reinterpret_cast<const VT *>(yq)[ln.p + c * ln.oc];
      else a[i][c] = oc_load_chunk<D, false>(yq, ln.p + c * ln.oc, d);
    }
  }
  tail_seed<0>(S, A, qbase + 0, qbase + 0 < qend);
  tail_seed<1>(S, A, qbase + 1, qbase + 1 < qend);
  tail_seed<2>(S, A, qbase + 2, qbase + 2 < qend);
  tail_seed<3>(S, A, qbase + 3, qbase + 3 < qend);
  const bool prefetch = ExCfg<D>::PREFETCH && A.prefetch;
  const u32 r_end = A.m;
  u32 t0 = 0, rows = min((u32)A.tile_rows, r_end);
  u32 nsc = 0;  // wave-uniform: valid (query, row) pairs of this wave (profiling only)
  if (rows) {
    ex_fill_tile(tile, A.tail, t0, rows, d);
    tail_fill_words<V>(A, ttags, tbits, t0, rows);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // the queries have arrived before the loop starts (see exact_scan_kernel)
  while (rows) {
    __syncthreads();  // the tile and its validity words are in LDS
    const u32 t1 = t0 + rows;
    const u32 rows1 = t1 < r_end ? min((u32)A.tile_rows, r_end - t1) : 0;
    const u32 id0 = A.n + t0;
    // the next tile's loads are in flight while this one is scored
    typedef FT pf_t __attribute__((ext_vector_type(ANN_VEC)));
    pf_t pf0 = 0, pf1 = 0;
    u32 pfw = 0;  // EX_BITS: the next tile's bitmap word of this thread; EX_TAGS: its tag word (exact_scan_kernel)
    if constexpr (ExCfg<D>::PREFETCH) {
      if (prefetch && rows1) {  // unconditional loads from clamped addresses: plain registers, nothing waits here
        const pf_t *src = reinterpret_cast<const pf_t *>(A.tail + (size_t)t1 * d);
        const u32 last = rows1 * (u32)(d / ANN_VEC) - 1;
        pf0 = src[min(threadIdx.x, last)];
        pf1 = src[min(threadIdx.x + blockDim.x, last)];
        if constexpr (V == EX_BITS) pfw = bits[((A.n + t1) >> 5) + min(threadIdx.x, ex_tile_words(A.n + t1, rows1) - 1)];
        if constexpr (V == EX_TAGS) pfw = A.tags[A.n + t1 + min(threadIdx.x, rows1 - 1)];
      }
    }
    for (u32 r0 = 0; r0 < rows; r0 += ln.rpw) {
      const u32 r = r0 + ln.g;
      const bool act = ln.valid && r < rows;
      bool allowed = act;
      if constexpr (V != EX_ALL) {
        allowed = act && (!bits || ex_tile_allows(tbits, id0, id0 + r));
        if constexpr (V == EX_TAGS) {
          const u32 tg = ttags[act ? r : r0];
          allowed = allowed && (tag_match(tg, qm[0], ql[0], qs[0]) || tag_match(tg, qm[1], ql[1], qs[1]) ||
                                tag_match(tg, qm[2], ql[2], qs[2]) || tag_match(tg, qm[3], ql[3], qs[3]));
        }
        if (!__ballot(allowed)) continue;  // wave-uniform: no row of this pass can survive for any of the four queries
      }
      const FT *rp = tile + (size_t)(act ? r : r0) * d;
      VT b[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        if constexpr (D > 0) b[c] = reinterpret_cast<const VT *>(rp)[ln.p + c * ln.oc];
        else b[c] = oc_load_chunk<D, false>(rp, ln.p + c * ln.oc, d);
      }
      const u32 id = id0 + r;
      const bool head = allowed && ln.p == 0;
      // all four trees first (independent chains the scheduler interleaves), then ONE branch for the rare survivors
      Key key[ANN_EX_QB];
      bool ok[ANN_EX_QB], pass[ANN_EX_QB];
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++) key[i] = key_make(ex_reduce<D>(a[i], b, ln.oc, ln.p, d), id);
      u32 tg = 0;
      if constexpr (V == EX_TAGS) {
        asm volatile("" ::: "memory");  // a second LDS read, not a register kept through the reduction
        tg = ttags[act ? r : r0];
      }
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++) {
        ok[i] = head && (V != EX_TAGS || tag_match(tg, qm[i], ql[i], qs[i])) && !(A.self && id == qbase + i);
        pass[i] = ok[i] && key_less(key[i], S.tau[i]);
      }
      if (A.scored) {  // wave-uniform; a query beyond the batch counts nothing
#pragma unroll
        for (int i = 0; i < ANN_EX_QB; i++)
          if (qbase + i < qend) nsc += (u32)__builtin_popcountll(__ballot(ok[i]));
      }
      if (__ballot(pass[0] || pass[1] || pass[2] || pass[3])) {
        S.offer<0>(pass[0], key[0]);
        S.offer<1>(pass[1], key[1]);
        S.offer<2>(pass[2], key[2]);
        S.offer<3>(pass[3], key[3]);
      }
    }
    if (!rows1) break;
    __syncthreads();  // every wave has read the tile
    bool stored = false;
    if constexpr (ExCfg<D>::PREFETCH) {
      if (prefetch) {
        pf_t *t = reinterpret_cast<pf_t *>(tile);
        const u32 pieces = rows1 * (u32)(d / ANN_VEC);
        if (threadIdx.x < pieces) t[threadIdx.x] = pf0;
        if (threadIdx.x + blockDim.x < pieces) t[threadIdx.x + blockDim.x] = pf1;
        if constexpr (V == EX_BITS) {
          if (threadIdx.x < ex_tile_words(A.n + t1, rows1)) tbits[threadIdx.x] = pfw;
        }
        if constexpr (V == EX_TAGS) {
          if (threadIdx.x < rows1) ttags[threadIdx.x] = pfw;  // (rows1 <= blockDim.x: exact_shape)
          if (bits && threadIdx.x < ex_tile_words(A.n + t1, rows1)) tbits[threadIdx.x] = bits[((A.n + t1) >> 5) + threadIdx.x];
        }
        stored = true;
      }
    }
    if (!stored) {
      ex_fill_tile(tile, A.tail, t1, rows1, d);
      tail_fill_words<V>(A, ttags, tbits, t1, rows1);
    }
    t0 = t1, rows = rows1;
  }
  tail_store<0>(S, A, qbase + 0, qbase + 0 < qend);
  tail_store<1>(S, A, qbase + 1, qbase + 1 < qend);
  tail_store<2>(S, A, qbase + 2, qbase + 2 < qend);
  tail_store<3>(S, A, qbase + 3, qbase + 3 < qend);
  if (A.scored && lane == 0 && nsc) atomicAdd(&A.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nsc);
}
static_assert(ANN_EX_QB == 4 && ANN_EX_PF == 2, "tail_merge_kernel names its four queries and its two prefetch registers");

// Any d without a register layout: exact_scan_generic_kernel's literal in-place tree over the tail, seeded and stored
// like tail_merge_kernel.  V is a kernel argument here (bits / tags NULL or not): this form is bound by its LDS tree.
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void tail_merge_generic_kernel(TailArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
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
  u32 *ttags = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * wave_bytes);
  u32 *tbits = A.tags ? ttags + A.tile_rows : ttags;
  const u32 *__restrict__ tags = A.tags, *__restrict__ bits = A.bits;
  const u32 qbase = (blockIdx.x * W + w) * ANN_EX_QB, qend = A.Q;
  ExSel S;
  S.init(kbase, kbase + (size_t)ANN_EX_QB * A.cap, A.cap, A.k, qbase, qend);
  tail_seed<0>(S, A, qbase + 0, qbase + 0 < qend);
  tail_seed<1>(S, A, qbase + 1, qbase + 1 < qend);
  tail_seed<2>(S, A, qbase + 2, qbase + 2 < qend);
  tail_seed<3>(S, A, qbase + 3, qbase + 3 < qend);
  int sh0 = 0;  // d <= 1 << sh0
  while ((1 << sh0) < d) sh0++;
  const FT zero = 0;
  u32 nsc = 0;
  for (u32 t0 = 0; t0 < A.m; t0 += A.tile_rows) {
    const u32 rows = min((u32)A.tile_rows, A.m - t0);
    const u32 id0 = A.n + t0;
    __syncthreads();
    ex_fill_tile(tile, A.tail, t0, rows, d);
    if (tags)
      for (u32 i = threadIdx.x; i < rows; i += blockDim.x) ttags[i] = tags[id0 + i];
    if (bits)
      for (u32 i = threadIdx.x; i < ex_tile_words(id0, rows); i += blockDim.x) tbits[i] = bits[(id0 >> 5) + i];
    __syncthreads();
#define ANN_TAIL_GEN_QUERY(I)                                                                                \
  if (qbase + (I) < qend) {                                                                                  \
    TagPred tp{0, 0, 0};                                                                                     \
    if (tags) tp = tag_pred(A.qmask, A.qlo, A.qhi, __builtin_amdgcn_readfirstlane(qbase + (I)));             \
    ANN_EX_GEN_QUERY(qbase + (I), {                                                                          \
      const u32 id = id0 + r0 + lane;                                                                        \
      const bool act = lane < np && (!tags || tag_match(ttags[r0 + lane], tp)) &&                            \
                       (!bits || ex_tile_allows(tbits, id0, id)) && !(A.self && id == qbase + (I));          \
      const Key key = key_make(act ? m[lane * d] : zero, id);                                                \
      wave_lds_sync(); /* m is rewritten by the next batch */                                                \
      if (A.scored) nsc += (u32)__builtin_popcountll(__ballot(act));                                         \
      S.offer<I>(act && key_less(key, S.tau[I]), key);                                                       \
    })                                                                                                       \
  }
    ANN_TAIL_GEN_QUERY(0) ANN_TAIL_GEN_QUERY(1) ANN_TAIL_GEN_QUERY(2) ANN_TAIL_GEN_QUERY(3)
#undef ANN_TAIL_GEN_QUERY
  }
  tail_store<0>(S, A, qbase + 0, qbase + 0 < qend);
  tail_store<1>(S, A, qbase + 1, qbase + 1 < qend);
  tail_store<2>(S, A, qbase + 2, qbase + 2 < qend);
  tail_store<3>(S, A, qbase + 3, qbase + 3 < qend);
  if (A.scored && lane == 0 && nsc) atomicAdd(&A.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nsc);
}

// ------------------------------------------------------------------------------------------ the index's own copies
// the allow list grows with the tail: bits [lo, hi) of the bitmap := 1 (one thread per word; other bits kept)
__global__ void tail_set_bits_kernel(u32 *__restrict__ bits, size_t lo, size_t hi) {
  const size_t w0 = lo >> 5, w1 = (hi + 31) >> 5;
  for (size_t wd = w0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; wd < w1; wd += (size_t)gridDim.x * blockDim.x) {
    const size_t b0 = wd << 5;
    u32 mask = 0xFFFFFFFFu;
    if (lo > b0) mask &= 0xFFFFFFFFu << (u32)(lo - b0);
    if (hi < b0 + 32) mask &= (1u << (u32)(hi - b0)) - 1u;
    bits[wd] |= mask;
  }
}
