// ann_exact_kernels.h -- exact brute-force k nearest neighbours (annhip_exact_knn).
//
// Every (query, row) squared distance comes out of the same tree as in the query path (row_reduce / row_reduce_oc / the
// literal in-place tree), so the distances are bit-identical to what query() returns for the same pair.  The k best of a
// query are the k smallest packed keys (distance bits, then id): ties go to the smaller id.
//
// exact_scan_kernel: grid (query group, row range).  A wave keeps ANN_EX_QB queries in registers in the lane map of the
// row layout; the workgroup streams its row range through an LDS tile that every wave reads once for all its queries:
// a query is loaded once per row range, a row tile once per query group.  While a tile is scored the next one is
// already on its way through registers (ANN_EX_PF 16-byte pieces per thread).  A candidate that does not beat the query's
// current k-th best key is dropped with one compare; survivors go to a per-query LDS buffer owned by the wave (no
// workgroup synchronisation in the selection) that is compacted to the k best when it fills.  Every (query, range)
// leaves its k best keys, ascending, in the workspace; exact_merge_kernel merges the ranges of a query.
//
// One family for every form of the scan: exact_scan_kernel<D, V> for the register layouts and exact_scan_generic_kernel<V>
// for any d, V (ExValid) saying where a row's validity comes from -- nothing (annhip_exact_knn), a bit of the allow list
// (annhip_exact_knn_filtered), or a tag word plus an optional bit (annhip_exact_knn_tagged).  The lines that differ are
// chosen with `if constexpr`: an instance holds no line of another form, and compiles to the code of a kernel written for
// that form alone (profiles/exact_scan_fold_devcode.md).
#pragma once
#include "ann_query_kernels.h"

#define ANN_EX_QB 4            // queries a wave holds in registers
#define ANN_EX_PF 2            // 16-byte pieces of the NEXT tile a thread keeps in flight while the current one is scored
#define ANN_EX_GEN_WAVES 4     // any-d kernel: waves per workgroup at most
#define ANN_EX_GEN_TILE_BYTES 16384  // any-d kernel: row tile in LDS (one row at least)
#define ANN_EX_SLACK 64        // free buffer entries a wave pass may need: one key per lane at most
#define ANN_EX_GEN_ELEMS 1024  // any-d path: elements of tree scratch per wave (pairs per batch = this / d, 1..64)

struct ExArgs {
  const FT *points, *y;
  Key *ws;          // [qn][ranges][k]
  u32 n, q0, qn;    // rows; first query and number of queries of this launch
  u32 range_rows;   // rows per row range (blockIdx.y)
  int d, k, self, tile_rows, cap, ranges;
  int prefetch;     // the next tile travels through registers (tile_rows * d / VEC <= ANN_EX_PF * threads)
};

// Waves per workgroup at most (fewer where k needs the LDS).  One workgroup is meant to fill a CU: the more queries share
// a tile, the fewer times a row is fetched (12 waves x 4 queries = 48 queries per tile).  The kernels with up to 4 chunks
// per lane fit the 168 registers that 12 waves leave each lane; those with 8 chunks per lane get 8 waves (256 registers).
template <int D>
struct ExCfg {
  static constexpr int WAVES = RowChunks<D>::C <= 4 ? 12 : 8;
  // rows of 16-byte chunks; not with 8 chunks per lane: those kernels have no registers to spare (d = 160 double spilled two)
  static constexpr bool PREFETCH = !OcCode<D>::UA && RowChunks<D>::C <= 4;
};

// The k smallest keys of buf[0..cnt) to buf[0..min(cnt, k)), ascending, by counting for every key how many are smaller
// (keys of one query are distinct: every row is seen once).  out: k keys of scratch.  One wave; returns the new count.
__device__ inline int ex_compact(Key *buf, int cnt, int k, Key *out) {
  const int lane = lane_id();
  wave_lds_sync();
  for (int j = lane; j < cnt; j += ANN_WAVE) {
    const Key me = buf[j];
    int rank = 0;
    for (int t = 0; t < cnt; t++) rank += key_less(buf[t], me) ? 1 : 0;
    if (rank < k) out[rank] = me;
  }
  wave_lds_sync();
  const int m = cnt < k ? cnt : k;
  for (int j = lane; j < m; j += ANN_WAVE) buf[j] = out[j];
  wave_lds_sync();
  return m;
}

// Per-wave selection state of ANN_EX_QB queries: buffers in LDS, counts and thresholds in registers.
struct ExSel {
  Key *buf, *out;  // buf[ANN_EX_QB][cap], out[k]
  Key tau[ANN_EX_QB];
  int cnt[ANN_EX_QB];
  int cap, k;
  __device__ __forceinline__ void init(Key *b, Key *o, int cap_, int k_, u32 qbase, u32 qend) {
    buf = b, out = o, cap = cap_, k = k_;
#pragma unroll
    for (int i = 0; i < ANN_EX_QB; i++) {
      cnt[i] = 0;
      tau[i] = qbase + i < qend ? key_max() : key_make((FT)0, 0);  // a query beyond the batch admits nothing
    }
  }
  // offer the keys of the lanes with `pass` set to query i (I compile-time)
  template <int I>
  __device__ __forceinline__ void offer(bool pass, Key key) {
    const u64 m = __ballot(pass);
    if (m) {  // rare after the first tiles
      Key *b = buf + (size_t)I * cap;
      if (pass) b[cnt[I] + mask_rank(m)] = key;
      cnt[I] += __builtin_popcountll(m);
      if (cnt[I] + ANN_EX_SLACK > cap) {  // cnt > k here (cap = k + slack)
        cnt[I] = ex_compact(b, cnt[I], k, out);
        tau[I] = b[k - 1];
      }
    }
  }
  // the k best of every query, ascending, key_max() where the range had fewer rows
  __device__ __forceinline__ void store(Key *ws, u32 qrel, u32 qn, int ranges, int range) {
    const int lane = lane_id();
#pragma unroll
    for (int i = 0; i < ANN_EX_QB; i++) {
      if (qrel + i >= qn) continue;
      Key *b = buf + (size_t)i * cap;
      const int m = ex_compact(b, cnt[i], k, out);
      Key *dst = ws + ((size_t)(qrel + i) * ranges + range) * k;
      for (int j = lane; j < k; j += ANN_WAVE) dst[j] = j < m ? b[j] : key_max();
    }
  }
};

// lane -> (row of the wave pass, position in the row's lane group) for every register layout
template <int D>
struct ExLanes {
  int oc, rpw, g, p;
  bool valid;
  __device__ __forceinline__ ExLanes(int d, int lane) {
    if constexpr (D > 0) {
      typedef RowLay<D> L;
      oc = L::LPR, rpw = L::RPW, g = lane / L::LPR, p = lane % L::LPR, valid = true;
    } else {
      const OcLanes<D> ol(d, lane);
      oc = ol.oc, rpw = ol.rpw, g = ol.g, p = ol.p, valid = ol.valid;
    }
  }
};

#ifdef USE_FLOAT
// row_reduce<D, ROW_SQDIFF> with the in-lane part written on pairs of floats, so that it compiles to the packed
// instructions (v_pk_add_f32 / v_pk_mul_f32: two IEEE operations each, nothing fused): the same subtractions,
// multiplications and additions between the same operands -- element j of chunk c with element j of chunk c + h, lane p with
// p + M, then j with j + 2 and j + 1 -- hence the same bits.  The scan is bound by vector-ALU issue; this removes a third
// of its instructions.
typedef float ex_f2 __attribute__((ext_vector_type(2)));
template <int D>
__device__ __forceinline__ FT ex_reduce_pk(const VT (&a)[RowLay<D>::C], const VT (&b)[RowLay<D>::C]) {
  typedef RowLay<D> L;
  ex_f2 e[L::C][2];
#pragma unroll
  for (int c = 0; c < L::C; c++) {
    const ex_f2 d0 = ex_f2{a[c].x, a[c].y} - ex_f2{b[c].x, b[c].y};
    const ex_f2 d1 = ex_f2{a[c].z, a[c].w} - ex_f2{b[c].z, b[c].w};
    e[c][0] = d0 * d0;
    e[c][1] = d1 * d1;
  }
#pragma unroll
  for (int h = L::C / 2; h >= 1; h >>= 1)
#pragma unroll
    for (int c = 0; c < h; c++) {
      e[c][0] = e[c][0] + e[c + h][0];
      e[c][1] = e[c][1] + e[c + h][1];
    }
  FT s[ANN_VEC] = {e[0][0].x, e[0][0].y, e[0][1].x, e[0][1].y};
#define ANN_EX_LEVEL(M)                                                        \
  if constexpr (L::LPR / 2 >= (M)) {                                           \
    _Pragma("unroll") for (int j = 0; j < ANN_VEC; j++) s[j] = s[j] + tree_partner<(M)>(s[j]); \
  }
  ANN_EX_LEVEL(32) ANN_EX_LEVEL(16) ANN_EX_LEVEL(8) ANN_EX_LEVEL(4) ANN_EX_LEVEL(2) ANN_EX_LEVEL(1)
#undef ANN_EX_LEVEL
  const ex_f2 t = ex_f2{s[0], s[1]} + ex_f2{s[2], s[3]};
  return t.x + t.y;
}
#endif

template <int D>
__device__ __forceinline__ FT ex_reduce(const VT (&a)[RowChunks<D>::C], const VT (&b)[RowChunks<D>::C], int oc, int p, int d) {
#ifdef USE_FLOAT
  if constexpr (D > 0) return ex_reduce_pk<D>(a, b);
#endif
  if constexpr (D > 0)
    return row_reduce<D, ROW_SQDIFF>(a, b);
  else
    return row_reduce_oc<OcCode<D>::C, ROW_SQDIFF, OcCode<D>::OC>(a, b, oc, p, oc_tree_len<D>(d));
}

// rows [t0, t0 + rows) of points -> tile (the same bytes, row stride d); 16-byte pieces where rows are aligned
__device__ __forceinline__ void ex_fill_tile(FT *tile, const FT *points, u32 t0, u32 rows, int d) {
  const FT *src = points + (size_t)t0 * d;
  const u32 count = rows * (u32)d;
  if (d % ANN_VEC == 0) {
    const VT *s = reinterpret_cast<const VT *>(src);
    VT *t = reinterpret_cast<VT *>(tile);
    for (u32 i = threadIdx.x; i < count / ANN_VEC; i += blockDim.x) t[i] = s[i];
  } else {
    for (u32 i = threadIdx.x; i < count; i += blockDim.x) tile[i] = src[i];
  }
}

// ------------------------------------------------------------------------------------------ validity
// Which rows compete.  The values are what exact_shape()'s argument means on the host; the tail's kernels
// (ann_tail_kernels.h, ann_tail_hash_kernels.h) take the same enum.
enum ExValid { EX_ALL = 0, EX_BITS = 1, EX_TAGS = 2 };  // EX_TAGS: the tag test, and the allow list where bits != NULL

// EX_BITS: one bit of the allow list (ann_filter_kernels.h) for every row of a tile: the bitmap words that cover rows
// [t0, t0 + rows) sit in LDS from word t0 >> 5 on -- fetched once per tile, read by every wave for all its queries.
#define ANN_EX_TBITS(tile_rows) ((size_t)(tile_rows) / 32 + 2)  // words of LDS behind the waves' buffers
__device__ __forceinline__ u32 ex_tile_words(u32 t0, u32 rows) { return ((t0 + rows - 1) >> 5) - (t0 >> 5) + 1; }
__device__ __forceinline__ bool ex_tile_allows(const u32 *tbits, u32 t0, u32 id) {
  return (tbits[(id >> 5) - (t0 >> 5)] >> (id & 31u)) & 1u;
}

// EX_TAGS: one tag word (ann_tag_kernels.h) for every row of a tile: ttags[r] = tags[t0 + r], A.tile_rows words of LDS
// behind the waves' buffers, then the ANN_EX_TBITS words of the allow list (used only where bits != NULL).  Host mirror:
// exact_shape's smem_of.
struct ExValidArgs {
  const u32 *tags, *bits;  // EX_BITS: bits (read through the kernels' `allow`); EX_TAGS: tags, and bits or NULL
  const u32 *qmask, *qlo, *qhi;  // EX_TAGS: qlo <= (tag & qmask) <= qhi; the pair form passes its value array twice
};

// the validity words of tile [t0, t0 + rows) -> LDS.  A macro: the kernels' loops as they stand, not an inlined function
// (which moved registers in the unaligned layouts' EX_BITS kernels).  Names of the enclosing kernel: V, tags, bits, ttags, tbits.
#define ANN_EX_FILL_WORDS(t0, rows)                                                                            \
  {                                                                                                            \
    if constexpr (V == EX_TAGS)                                                                                \
      for (u32 i = threadIdx.x; i < (rows); i += blockDim.x) ttags[i] = tags[(t0) + i];                        \
    if constexpr (V != EX_ALL)                                                                                 \
      if (V == EX_BITS || bits)                                                                                \
        for (u32 i = threadIdx.x; i < ex_tile_words(t0, rows); i += blockDim.x) tbits[i] = bits[((t0) >> 5) + i]; \
  }

// ------------------------------------------------------------------------------------------ the scan
// EX_BITS: a row whose bit is clear is never a survivor, and a wave pass without an allowed row is not scored at all.
// Where the next tile travels through registers, so does its bitmap: one word per thread (such a tile has at most 128
// rows per wave, hence fewer words than the workgroup has threads).
// EX_TAGS: each of the wave's ANN_EX_QB queries applies its own (mask, lo, hi) in pass[i]; a wave pass in which no row
// matches any of the four is not scored at all.  Where the next tile travels through registers, so do its tags: one word
// per thread (the host prefetches only where a tile has no more rows than the workgroup has threads, i.e. rows of 32
// bytes at least).  That word takes the place of the prefetched bitmap word -- these kernels have no register to spare
// (168 per lane with 12 waves) -- so where an allow list is given TOO, its words for the next tile are fetched after the
// current one is scored, latency exposed.  The tag word is read from LDS twice per wave pass (before the row loads for
// the skip, after the reduction for pass[i]) rather than kept live across the reduction.
// The allow list reaches the kernel twice: EX_BITS reads it through `allow`, a __restrict__ kernel argument of its own,
// EX_TAGS through G.bits like its tags.  The compiler treats the two differently (only the former is `noalias`), and
// each form's code is what it is with its own: with `allow` the tagged kernels grow by five instructions, with G.bits
// the allow-list kernels of the layouts that do not prefetch change.  The host passes the same pointer in both.
// tail_merge_kernel (ann_tail_kernels.h) is this loop once more, seeded from a result row and without row ranges: it
// stays a kernel of its own, since a body shared through a function does not compile to the same code
// (profiles/fixed_body_devcode.md).
template <int D, int V>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void exact_scan_kernel(ExArgs A, ExValidArgs G, const u32 *__restrict__ allow) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.d;
  FT *tile = reinterpret_cast<FT *>(smem);
  const size_t tile_bytes = ((size_t)A.tile_rows * d * sizeof(FT) + 15) & ~(size_t)15;
  Key *kbase = reinterpret_cast<Key *>(smem + tile_bytes) + (size_t)w * ((size_t)ANN_EX_QB * A.cap + A.k);
  u32 *ttags = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * sizeof(Key) * ((size_t)ANN_EX_QB * A.cap + A.k));
  u32 *tbits = V == EX_TAGS ? ttags + A.tile_rows : ttags;
  const u32 *__restrict__ tags = G.tags, *__restrict__ bits = V == EX_BITS ? allow : G.bits;
  const u32 qrel = (blockIdx.x * W + w) * ANN_EX_QB;  // first query of this wave, relative to q0
  const u32 qbase = A.q0 + qrel, qend = A.q0 + A.qn;
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
      const u32 qu = __builtin_amdgcn_readfirstlane(q);  // (the wave index is uniform, which the compiler cannot see)
      const TagPred tp = tag_pred(G.qmask, G.qlo, G.qhi, qu);  // scalar loads into scalar registers
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
  const bool prefetch = ExCfg<D>::PREFETCH && A.prefetch;
  const u32 r_begin = blockIdx.y * A.range_rows;
  const u32 r_end = min(A.n, r_begin + A.range_rows);
  u32 t0 = r_begin, rows = r_begin < r_end ? min((u32)A.tile_rows, r_end - r_begin) : 0;
  if (rows) {
    ex_fill_tile(tile, A.points, t0, rows, d);
    ANN_EX_FILL_WORDS(t0, rows)
  }
  // The queries have arrived before the loop starts (s_waitcnt vmcnt(0)).  Otherwise the waits for them sit in the first
  // row pass of EVERY tile, where vmcnt counts the prefetched pieces of the next tile as well and waits those out too.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  while (rows) {
    __syncthreads();  // the tile and its validity words are in LDS
    const u32 t1 = t0 + rows;
    const u32 rows1 = t1 < r_end ? min((u32)A.tile_rows, r_end - t1) : 0;
    // the next tile's loads are in flight while this one is scored
    typedef FT pf_t __attribute__((ext_vector_type(ANN_VEC)));
    pf_t pf0 = 0, pf1 = 0;
    u32 pfw = 0;  // EX_BITS: the next tile's bitmap word of this thread; EX_TAGS: its tag word
    if constexpr (ExCfg<D>::PREFETCH) {
      if (prefetch && rows1) {  // unconditional loads from clamped addresses: plain registers, nothing waits here
        const pf_t *src = reinterpret_cast<const pf_t *>(A.points + (size_t)t1 * d);
        const u32 last = rows1 * (u32)(d / ANN_VEC) - 1;
        pf0 = src[min(threadIdx.x, last)];
        pf1 = src[min(threadIdx.x + blockDim.x, last)];
        if constexpr (V == EX_BITS) pfw = bits[(t1 >> 5) + min(threadIdx.x, ex_tile_words(t1, rows1) - 1)];
        if constexpr (V == EX_TAGS) pfw = tags[t1 + min(threadIdx.x, rows1 - 1)];
      }
    }
    for (u32 r0 = 0; r0 < rows; r0 += ln.rpw) {
      const u32 r = r0 + ln.g;
      const bool act = ln.valid && r < rows;
      bool allowed = act;
      if constexpr (V != EX_ALL) {
        allowed = act && ((V == EX_TAGS && !bits) || ex_tile_allows(tbits, t0, t0 + r));
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
      const u32 id = t0 + r;
      const bool head = allowed && ln.p == 0;
      // all four trees first (independent chains the scheduler interleaves), then ONE branch for the rare survivors
      Key key[ANN_EX_QB];
      bool pass[ANN_EX_QB];
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++) key[i] = key_make(ex_reduce<D>(a[i], b, ln.oc, ln.p, d), id);
      u32 tg = 0;
      if constexpr (V == EX_TAGS) {
        asm volatile("" ::: "memory");  // a second LDS read, not a register kept through the reduction
        tg = ttags[act ? r : r0];
      }
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++)
        pass[i] = head && (V != EX_TAGS || tag_match(tg, qm[i], ql[i], qs[i])) && key_less(key[i], S.tau[i]) && !(A.self && id == qbase + i);
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
          if (threadIdx.x < ex_tile_words(t1, rows1)) tbits[threadIdx.x] = pfw;
        }
        if constexpr (V == EX_TAGS) {
          if (threadIdx.x < rows1) ttags[threadIdx.x] = pfw;  // (rows1 <= blockDim.x: exact_shape)
          if (bits && threadIdx.x < ex_tile_words(t1, rows1)) tbits[threadIdx.x] = bits[(t1 >> 5) + threadIdx.x];
        }
        stored = true;
      }
    }
    if (!stored) {
      ex_fill_tile(tile, A.points, t1, rows1, d);
      ANN_EX_FILL_WORDS(t1, rows1)
    }
    t0 = t1, rows = rows1;
  }
  S.store(A.ws, qrel, A.qn, A.ranges, (int)blockIdx.y);
}
static_assert(ANN_EX_QB == 4 && ANN_EX_PF == 2, "exact_scan_kernel names its four queries and its two prefetch registers");

// Any d without a register layout: the literal in-place tree through LDS, several (query, row) pairs of a wave at once.
// Lanes are spread over pair x z (z padded to a power of two: no division), so one fence per tree level serves
// npairs pairs.  A wave takes its ANN_EX_QB queries one after another over each tile (the query sits in LDS).
//
// ANN_EX_GEN_QUERY(q, select): query q of A.y over the rows of the tile, NP at a time.  The distance part -- the query
// into yq, the squared differences into m, the tree in place -- is the one text of the literal tree for this kernel and
// for tail_merge_generic_kernel; `select` are the statements that follow it for every batch, where m[lane * d] holds the
// distance of row r0 + lane (lane < np): they make the key, fence (m is rewritten by the next batch) and offer it.
// Names of the enclosing kernel: A, lane, d, rows, NP, sh0, zero, tile, yq, m.
#define ANN_EX_GEN_QUERY(q, ...)                                                                             \
  {                                                                                                          \
    wave_lds_sync();                                                                                         \
    for (int z = lane; z < d; z += ANN_WAVE) yq[z] = A.y[(size_t)(q) * d + z];                               \
    wave_lds_sync();                                                                                         \
    for (u32 r0 = 0; r0 < rows; r0 += NP) {                                                                  \
      const int np = (int)min((u32)NP, rows - r0);                                                           \
      for (int it = lane; it < (np << sh0); it += ANN_WAVE) {                                                \
        const int pr = it >> sh0, z = it & ((1 << sh0) - 1);                                                 \
        if (z < d) {                                                                                         \
          const FT df = yq[z] - tile[(size_t)(r0 + pr) * d + z];                                             \
          m[pr * d + z] = df * df;                                                                           \
        }                                                                                                    \
      }                                                                                                      \
      wave_lds_sync();                                                                                       \
      int sh = sh0;                                                                                          \
      for (int s = d; s >> 1; s >>= 1) {                                                                     \
        const int h = s >> 1;                                                                                \
        while (sh > 0 && (1 << (sh - 1)) >= h) sh--; /* h <= 1 << sh */                                      \
        for (int it = lane; it < (np << sh); it += ANN_WAVE) {                                               \
          const int pr = it >> sh, z = it & ((1 << sh) - 1);                                                 \
          if (z < h) {                                                                                       \
            FT *mp = m + pr * d;                                                                             \
            const FT g = ((s & 1) && z == 0) ? mp[s - 1] : zero;                                             \
            mp[z] = mp[z] + (mp[z + h] + g);                                                                 \
          }                                                                                                  \
        }                                                                                                    \
        wave_lds_sync();                                                                                     \
      }                                                                                                      \
      __VA_ARGS__                                                                                            \
    }                                                                                                        \
  }

template <int V>
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void exact_scan_generic_kernel(ExArgs A, ExValidArgs G, const u32 *__restrict__ allow) {
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
  u32 *tbits = V == EX_TAGS ? ttags + A.tile_rows : ttags;
  const u32 *__restrict__ tags = G.tags, *__restrict__ bits = V == EX_BITS ? allow : G.bits;
  const u32 qrel = (blockIdx.x * W + w) * ANN_EX_QB;
  const u32 qbase = A.q0 + qrel, qend = A.q0 + A.qn;
  ExSel S;
  S.init(kbase, kbase + (size_t)ANN_EX_QB * A.cap, A.cap, A.k, qbase, qend);
  int sh0 = 0;  // d <= 1 << sh0
  while ((1 << sh0) < d) sh0++;
  const FT zero = 0;
  const u32 r_begin = blockIdx.y * A.range_rows;
  const u32 r_end = min(A.n, r_begin + A.range_rows);
  for (u32 t0 = r_begin; t0 < r_end; t0 += A.tile_rows) {
    const u32 rows = min((u32)A.tile_rows, r_end - t0);
    __syncthreads();
    ex_fill_tile(tile, A.points, t0, rows, d);
    ANN_EX_FILL_WORDS(t0, rows)
    __syncthreads();
#define ANN_EX_GEN_SCAN(I)                                                                                   \
  if (qbase + (I) < qend) {                                                                                  \
    const u32 qu = __builtin_amdgcn_readfirstlane(qbase + (I));                                              \
    TagPred tp{0, 0, 0};                                                                                     \
    if constexpr (V == EX_TAGS) tp = tag_pred(G.qmask, G.qlo, G.qhi, qu);                                    \
    ANN_EX_GEN_QUERY(qbase + (I), {                                                                          \
      const u32 id = t0 + r0 + lane;                                                                         \
      bool act;                                                                                              \
      if constexpr (V == EX_TAGS) {                                                                          \
        act = lane < np && tag_match(ttags[r0 + lane], tp) && (!bits || ex_tile_allows(tbits, t0, id));      \
      } else {                                                                                               \
        act = lane < np;                                                                                     \
        if constexpr (V == EX_BITS) act = act && ex_tile_allows(tbits, t0, id);                              \
      }                                                                                                      \
      const Key key = key_make(act ? m[lane * d] : zero, id);                                                \
      wave_lds_sync(); /* m is rewritten by the next batch */                                                \
      S.offer<I>(act && key_less(key, S.tau[I]) && !(A.self && id == qbase + (I)), key);                     \
    })                                                                                                       \
  }
    ANN_EX_GEN_SCAN(0) ANN_EX_GEN_SCAN(1) ANN_EX_GEN_SCAN(2) ANN_EX_GEN_SCAN(3)
#undef ANN_EX_GEN_SCAN
  }
  S.store(A.ws, qrel, A.qn, A.ranges, (int)blockIdx.y);
}

// One wave per query: the k smallest of the query's ranges * k workspace keys (distinct, key_max() padding last), in
// ascending order, unpacked to ids (size_t) and distances.
__global__ __launch_bounds__(256) void exact_merge_kernel(const Key *__restrict__ ws, u32 qn, int ranges, int k,
                                                          size_t *__restrict__ ids, FT *__restrict__ dists) {
  const int lane = lane_id();
  const u32 q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= qn) return;
  const Key *src = ws + (size_t)q * ranges * k;
  size_t *io = ids + (size_t)q * k;
  FT *dout = dists + (size_t)q * k;
  if (ranges == 1) {
    for (int j = lane; j < k; j += ANN_WAVE) io[j] = key_id(src[j]), dout[j] = key_dist(src[j]);
    return;
  }
  const int total = ranges * k;
  Key prev = key_max();
  for (int j = 0; j < k; j++) {
    Key best = key_max();
    for (int i = lane; i < total; i += ANN_WAVE) {
      const Key c = src[i];
      if ((j == 0 || key_less(prev, c)) && key_less(c, best)) best = c;
    }
    best = wave_min_key(best);
    if (lane == 0) io[j] = key_id(best), dout[j] = key_dist(best);
    prev = best;
  }
}

// exact_merge_kernel unpacks key_max() where a query has fewer than k valid rows (EX_BITS / EX_TAGS): those entries ->
// (n, +inf)
__global__ void exact_tail_kernel(size_t count, size_t n, size_t *__restrict__ ids, FT *__restrict__ dists) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x)
    if (ids[e] == (size_t)ANN_ID_NONE) ids[e] = n, dists[e] = ft_inf();
}
