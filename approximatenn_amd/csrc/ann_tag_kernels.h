// ann_tag_kernels.h -- per-query tag predicates of the fixed query mode and of the exact scan (annhip_index_set_tags,
// annhip_query_tagged, annhip_exact_knn_tagged; gfx950).
//
// Rows carry a 32-bit tag word, every query a (mask, value) pair: row i competes for query q iff
// (tags[i] & qmask[q]) == qvalue[q].  Like the allow list (ann_filter_kernels.h, the model of every kernel here) the
// predicate only narrows what fixed mode calls a valid id, and it is tested where an id ENTERS the wave's LDS list: a row
// that does not match costs its 4-byte id and its 4-byte tag, never a row.
//
//   AdmitTags        the predicate of one query as an admission policy
//   stage1_tag / stage2_tag   stage1_fixed_body (ann_probe_kernels.h) / stage2_fixed_body (ann_filter_kernels.h) with it
//   exact_scan_tag / exact_scan_generic_tag   the filtered exact scan's two kernels with the tile's tag words in LDS; the
//                    wave's ANN_EX_QB queries each apply their own (mask, value)
//
// `bits`, the index's allow list, may be NULL: both tests apply when it is set.  NULL or not is a kernel argument, hence one
// wave-uniform branch and no second template axis.  tags, bits, qmask and qvalue are separate kernel arguments, and no
// untagged call launches anything from this file.
#pragma once
#include "ann_filter_kernels.h"

// id < n (the caller's test).  The two loads are independent of each other where both tests apply.
__device__ __forceinline__ bool tag_allows(const u32 *__restrict__ tags, const u32 *__restrict__ bits, u32 qm, u32 qv, u32 id) {
  if (bits) {
    const u32 t = tags[id], wd = bits[id >> 5];
    return (t & qm) == qv && ((wd >> (id & 31u)) & 1u);
  }
  return (tags[id] & qm) == qv;
}

// the admission policy of query x's predicate (see stage1_fixed_body): qmask[x] / qvalue[x] are read once per workgroup and
// are wave-uniform
struct AdmitTags {
  static constexpr bool ALWAYS = false;
  const u32 *__restrict__ tags, *__restrict__ bits;
  u32 qm, qv;
  __device__ __forceinline__ AdmitTags(const u32 *tags, const u32 *bits, const u32 *qmask, const u32 *qvalue, u32 x)
      : tags(tags), bits(bits), qm(qmask[x]), qv(qvalue[x]) {}
  __device__ __forceinline__ bool operator()(u32 id) const { return tag_allows(tags, bits, qm, qv, id); }
};

// ------------------------------------------------------------------------------------------ stage 1
// stage1_fixed_body with the predicate of query x: nv_own = matching valid ids (self included when it matches).
template <int D, bool SEG, typename RT>
__global__ __launch_bounds__(256) void stage1_tag_kernel(QParams P, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ codes,
                                                            const unsigned char *__restrict__ pbits, int pb, u32 rpt,
                                                            const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                         const u32 *__restrict__ qmask, const u32 *__restrict__ qvalue, int K1, int cap,
                                                            FT *__restrict__ cand_dist, u32 *__restrict__ cand_id,
                                                            u32 *__restrict__ nv_tot, u32 *__restrict__ nv_own) {
  stage1_fixed_body<D, SEG, RT>(P, y, alias, codes, pbits, pb, rpt, AdmitTags(tags, bits, qmask, qvalue, blockIdx.x), key_max(),
                                K1, cap, cand_dist, cand_id, nv_tot, nv_own);
}

// ------------------------------------------------------------------------------------------ stage 2
// stage2_fixed_body over the stage-1 results and those of their graph neighbours that pass query x's test.
template <int D, typename IdOut, typename RT>
__global__ __launch_bounds__(256) void stage2_tag_kernel(QParams P, int Q, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ top_id, const FT *__restrict__ top_dist,
                                                            const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                         const u32 *__restrict__ qmask, const u32 *__restrict__ qvalue, u32 P2, int K1, int cap,
                                                            IdOut *__restrict__ out_ids, FT *__restrict__ out_dist,
                                                            u32 *__restrict__ flist, u32 *__restrict__ fcount,
                                                            unsigned long long *__restrict__ exact_total,
                                                            unsigned long long *__restrict__ rows_done, u32 xbase) {
  stage2_fixed_body<D, IdOut, RT>(P, y, alias, top_id, top_dist, AdmitTags(tags, bits, qmask, qvalue, xbase + blockIdx.x), P2, K1,
                                  cap, out_ids, out_dist, flist, fcount, exact_total, rows_done, xbase);
}

// ------------------------------------------------------------------------------------------ exact scan
// One tag word for every row of a tile: ttags[r] = tags[t0 + r], A.tile_rows words of LDS behind the waves' buffers, then
// the ANN_EX_TBITS words of the allow list (used only where bits != NULL).  Host mirror: exact_run's smem_of.
struct ExTagArgs {
  const u32 *tags, *bits;  // bits may be NULL
  const u32 *qmask, *qvalue;
};

// exact_scan_filtered_kernel with the tag test: each of the wave's ANN_EX_QB queries applies its own (mask, value) in
// pass[i]; a wave pass in which no row matches any of the four is not scored at all.  Where the next tile travels through
// registers, so do its tags: one word per thread (the host prefetches only where a tile has no more rows than the workgroup
// has threads, i.e. rows of 32 bytes at least).  That word takes the place of the filtered kernel's prefetched bitmap word --
// these kernels have no register to spare (168 per lane with 12 waves) -- so where an allow list is given TOO, its words for
// the next tile are fetched after the current one is scored, latency exposed.  The tag word is read from LDS twice per wave
// pass (before the row loads for the skip, after the reduction for pass[i]) rather than kept live across the reduction.
template <int D>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void exact_scan_tag_kernel(ExArgs A, ExTagArgs G) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.d;
  FT *tile = reinterpret_cast<FT *>(smem);
  const size_t tile_bytes = ((size_t)A.tile_rows * d * sizeof(FT) + 15) & ~(size_t)15;
  Key *kbase = reinterpret_cast<Key *>(smem + tile_bytes) + (size_t)w * ((size_t)ANN_EX_QB * A.cap + A.k);
  u32 *ttags = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * sizeof(Key) * ((size_t)ANN_EX_QB * A.cap + A.k));
  u32 *tbits = ttags + A.tile_rows;
  const u32 *__restrict__ tags = G.tags, *__restrict__ bits = G.bits;
  const u32 qrel = (blockIdx.x * W + w) * ANN_EX_QB;  // first query of this wave, relative to q0
  const u32 qbase = A.q0 + qrel, qend = A.q0 + A.qn;
  ExSel S;
  S.init(kbase, kbase + (size_t)ANN_EX_QB * A.cap, A.cap, A.k, qbase, qend);
  const ExLanes<D> ln(d, lane);
  VT a[ANN_EX_QB][C];
  u32 qm[ANN_EX_QB], qv[ANN_EX_QB];  // wave-uniform: scalar registers
#pragma unroll
  for (int i = 0; i < ANN_EX_QB; i++) {
    const u32 q = qbase + i < qend ? qbase + i : qend - 1;  // loads stay inside y; the result is never admitted
    const FT *yq = A.y + (size_t)q * d;
    const u32 qu = __builtin_amdgcn_readfirstlane(q);  // (the wave index is uniform, which the compiler cannot see)
    qm[i] = G.qmask[qu], qv[i] = G.qvalue[qu];         // scalar loads into scalar registers
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
    for (u32 i = threadIdx.x; i < rows; i += blockDim.x) ttags[i] = tags[t0 + i];
    if (bits)
      for (u32 i = threadIdx.x; i < ex_tile_words(t0, rows); i += blockDim.x) tbits[i] = bits[(t0 >> 5) + i];
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // the queries have arrived before the loop starts (see exact_scan_kernel)
  while (rows) {
    __syncthreads();  // the tile, its tags and its bits are in LDS
    const u32 t1 = t0 + rows;
    const u32 rows1 = t1 < r_end ? min((u32)A.tile_rows, r_end - t1) : 0;
    // the next tile's loads are in flight while this one is scored
    typedef FT pf_t __attribute__((ext_vector_type(ANN_VEC)));
    pf_t pf0 = 0, pf1 = 0;
    u32 ptg = 0;
    if constexpr (ExCfg<D>::PREFETCH) {
      if (prefetch && rows1) {  // unconditional loads from clamped addresses: plain registers, nothing waits here
        const pf_t *src = reinterpret_cast<const pf_t *>(A.points + (size_t)t1 * d);
        const u32 last = rows1 * (u32)(d / ANN_VEC) - 1;
        pf0 = src[min(threadIdx.x, last)];
        pf1 = src[min(threadIdx.x + blockDim.x, last)];
        ptg = tags[t1 + min(threadIdx.x, rows1 - 1)];
      }
    }
    for (u32 r0 = 0; r0 < rows; r0 += ln.rpw) {
      const u32 r = r0 + ln.g;
      const bool act = ln.valid && r < rows;
      bool allowed = act && (!bits || ex_tile_allows(tbits, t0, t0 + r));
      {
        const u32 tg = ttags[act ? r : r0];
        allowed = allowed && ((tg & qm[0]) == qv[0] || (tg & qm[1]) == qv[1] || (tg & qm[2]) == qv[2] || (tg & qm[3]) == qv[3]);
      }
      if (!__ballot(allowed)) continue;  // wave-uniform: no row of this pass can survive for any of the four queries
      const FT *rp = tile + (size_t)(act ? r : r0) * d;
      VT b[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        if constexpr (D > 0) b[c] = reinterpret_cast<const VT *>(rp)[ln.p + c * ln.oc];
        else b[c] = oc_load_chunk<D, false>(rp, ln.p + c * ln.oc, d);
      }
      const u32 id = t0 + r;
      const bool head = allowed && ln.p == 0;
      Key key[ANN_EX_QB];
      bool pass[ANN_EX_QB];
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++) key[i] = key_make(ex_reduce<D>(a[i], b, ln.oc, ln.p, d), id);
      asm volatile("" ::: "memory");  // a second LDS read, not a register kept through the reduction
      const u32 tg = ttags[act ? r : r0];
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++)
        pass[i] = head && (tg & qm[i]) == qv[i] && key_less(key[i], S.tau[i]) && !(A.self && id == qbase + i);
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
        if (threadIdx.x < rows1) ttags[threadIdx.x] = ptg;  // (rows1 <= blockDim.x: exact_run)
        if (bits && threadIdx.x < ex_tile_words(t1, rows1)) tbits[threadIdx.x] = bits[(t1 >> 5) + threadIdx.x];
        stored = true;
      }
    }
    if (!stored) {
      ex_fill_tile(tile, A.points, t1, rows1, d);
      for (u32 i = threadIdx.x; i < rows1; i += blockDim.x) ttags[i] = tags[t1 + i];
      if (bits)
        for (u32 i = threadIdx.x; i < ex_tile_words(t1, rows1); i += blockDim.x) tbits[i] = bits[(t1 >> 5) + i];
    }
    t0 = t1, rows = rows1;
  }
  S.store(A.ws, qrel, A.qn, A.ranges, (int)blockIdx.y);
}

// exact_scan_generic_filtered_kernel with the tag test
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void exact_scan_generic_tag_kernel(ExArgs A, ExTagArgs G) {
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
  u32 *tbits = ttags + A.tile_rows;
  const u32 *__restrict__ tags = G.tags, *__restrict__ bits = G.bits;
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
    for (u32 i = threadIdx.x; i < rows; i += blockDim.x) ttags[i] = tags[t0 + i];
    if (bits)
      for (u32 i = threadIdx.x; i < ex_tile_words(t0, rows); i += blockDim.x) tbits[i] = bits[(t0 >> 5) + i];
    __syncthreads();
#define ANN_EX_GEN_QUERY(I)                                                                                  \
  if (qbase + (I) < qend) {                                                                                  \
    const u32 qu = __builtin_amdgcn_readfirstlane(qbase + (I));                                              \
    const u32 qm = G.qmask[qu], qv = G.qvalue[qu];                                                           \
    wave_lds_sync();                                                                                         \
    for (int z = lane; z < d; z += ANN_WAVE) yq[z] = A.y[(size_t)(qbase + (I)) * d + z];                     \
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
      const u32 id = t0 + r0 + lane;                                                                         \
      const bool act = lane < np && (ttags[r0 + lane] & qm) == qv && (!bits || ex_tile_allows(tbits, t0, id)); \
      const Key key = key_make(act ? m[lane * d] : zero, id);                                                \
      wave_lds_sync(); /* m is rewritten by the next batch */                                                \
      S.offer<I>(act && key_less(key, S.tau[I]) && !(A.self && id == qbase + (I)), key);                     \
    }                                                                                                        \
  }
    ANN_EX_GEN_QUERY(0) ANN_EX_GEN_QUERY(1) ANN_EX_GEN_QUERY(2) ANN_EX_GEN_QUERY(3)
#undef ANN_EX_GEN_QUERY
  }
  S.store(A.ws, qrel, A.qn, A.ranges, (int)blockIdx.y);
}
