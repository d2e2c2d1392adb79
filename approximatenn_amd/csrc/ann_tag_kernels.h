// ann_tag_kernels.h -- per-query tag predicates of the fixed query mode and of the exact scan (annhip_index_set_tags,
// annhip_query_tagged, annhip_exact_knn_tagged; gfx950).
//
// Rows carry a 32-bit tag word, every query a (mask, value) pair: row i competes for query q iff
// (tags[i] & qmask[q]) == qvalue[q].  Like the allow list (ann_filter_kernels.h, the model of every kernel here) the
// predicate only narrows what fixed mode calls a valid id, and it is tested where an id ENTERS the wave's LDS list: a row
// that does not match costs its 4-byte id and its 4-byte tag, never a row.
//
//   stage1_tag       stage1_filter_kernel's structure, both forms (segment walk, slot scan); qmask[x] / qvalue[x] are read
//                    once per workgroup and are wave-uniform
//   stage2_tag       stage2_filter_kernel with the predicate in `ok`
//   exact_scan_tag / exact_scan_generic_tag   the filtered exact scan's two kernels with the tile's tag words in LDS; the
//                    wave's ANN_EX_QB queries each apply their own (mask, value)
//
// `bits`, the index's allow list, may be NULL: both tests apply when it is set.  NULL or not is a kernel argument, hence one
// wave-uniform branch and no second template axis.  tags, bits, qmask and qvalue are separate kernel arguments: QParams and
// the existing kernels are not touched, and no untagged call launches anything from this file.
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

// ------------------------------------------------------------------------------------------ stage 1
// stage1_filter_kernel with the predicate of query x in the place of the bit test (same LDS carve-up: stage1_probe_lds_bytes
// on the host; probe_gather, the selection state, the merge and the outputs unchanged).  pb = 0 with rpt = 1 + ds gives the
// plain buckets of fixed mode.  nv_own = ids in the list = rows gathered = matching valid ids (self included when it matches).
template <int D, bool SEG, typename RT>
__global__ __launch_bounds__(256) void stage1_tag_kernel(QParams P, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ codes,
                                                            const unsigned char *__restrict__ pbits, int pb, u32 rpt,
                                                            const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                         const u32 *__restrict__ qmask, const u32 *__restrict__ qvalue, int K1, int cap,
                                                            FT *__restrict__ cand_dist, u32 *__restrict__ cand_id,
                                                            u32 *__restrict__ nv_tot, u32 *__restrict__ nv_own) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  // ---- LDS carve-up: stage1_probe_kernel's (stage1_probe_lds_bytes on the host)
  unsigned char *sp = smem;
  Key *kbuf_all = reinterpret_cast<Key *>(sp);           sp += sizeof(Key) * (size_t)W * cap;
  Key *kout_all = reinterpret_cast<Key *>(sp);           sp += sizeof(Key) * (size_t)W * K1;
  Key *mbuf = reinterpret_cast<Key *>(sp);               sp += sizeof(Key) * (size_t)W * K1;
  TryInfo *tries = reinterpret_cast<TryInfo *>(sp);      sp += sizeof(TryInfo) * (size_t)P.T;
  const u32 **rptr_all = reinterpret_cast<const u32 **>(sp);  sp += sizeof(u32 *) * (size_t)W * ANN_WAVE;
  u32 *list_all = reinterpret_cast<u32 *>(sp);           sp += sizeof(u32) * (size_t)W * ANN_S1_CHUNK;
  u32 *pref_all = reinterpret_cast<u32 *>(sp);           sp += sizeof(u32) * (size_t)W * ANN_WAVE;
  u32 *qcode = reinterpret_cast<u32 *>(sp);              sp += sizeof(u32) * (size_t)P.T;
  int *mcnt = reinterpret_cast<int *>(sp);               sp += sizeof(int) * (size_t)W;
  u32 *cnts = reinterpret_cast<u32 *>(sp);               sp += sizeof(u32) * 4;  // [0] valid [1] gathered
  unsigned char *qbits = sp;                             sp += (size_t)P.T * pb;  // [T][pb] ranked projection indices
  sp = smem + (((sp - smem) + 15) & ~(size_t)15);
  FT *yq = reinterpret_cast<FT *>(sp);  // generic d only: [d] + W*[d]
  u32 *list = list_all + (size_t)w * ANN_S1_CHUNK;
  u32 *pref = pref_all + (size_t)w * ANN_WAVE;
  const u32 **rptr = rptr_all + (size_t)w * ANN_WAVE;

  const u32 x = blockIdx.x;
  const u32 qm = qmask[x], qv = qvalue[x];  // wave-uniform: this query's predicate, read once
  for (int i = threadIdx.x; i < P.T; i += blockDim.x) {
    tries[i] = P.tries[i];
    qcode[i] = codes[(size_t)x * P.T + i];  // the query's OWN codes (fixed mode)
  }
  for (int i = threadIdx.x; i < P.T * pb; i += blockDim.x) qbits[i] = pbits[(size_t)x * P.T * pb + i];
  if (threadIdx.x < 4) cnts[threadIdx.x] = 0;
  if constexpr (D == 0 || OcCode<D>::GEN)
    for (int z = threadIdx.x; z < P.d; z += blockDim.x) yq[z] = y[(size_t)x * P.d + z];
  __syncthreads();

  SelState S;
  S.kbuf = kbuf_all + (size_t)w * cap, S.kout = kout_all + (size_t)w * K1;
  S.kcnt = 0, S.K1 = K1, S.cap = cap, S.tau = key_max();
  FT *scratch = yq + (size_t)(1 + w) * P.d;
  u32 vtot = 0, vown = 0;

  // the query row, as this lane's slice
  VT a[RowChunks<D>::C];
  if constexpr (D > 0) {
    typedef RowLay<D> L;
    const VT *yp = reinterpret_cast<const VT *>(y + (size_t)x * D) + (lane % L::LPR);
#pragma unroll
    for (int c = 0; c < L::C; c++) a[c] = yp[c * L::LPR];
  } else if constexpr (D < 0 && !OcCode<D>::GEN) {
    const OcLanes<D> ol(P.d, lane);
#pragma unroll
    for (int c = 0; c < OcCode<D>::C; c++) a[c] = oc_load_chunk<D, false>(y + (size_t)x * P.d, ol.p + c * ol.oc, P.d);
  }

  int cnt = 0;
  const u32 runs = (u32)P.T * rpt;
  const u32 per = (runs + W - 1) / W;  // runs of this wave: [r0, r1)
  const u32 r0 = min(runs, (u32)w * per), r1 = min(runs, r0 + per);
  if constexpr (SEG) {
    for (u32 rb = r0; rb < r1; rb += ANN_WAVE) {
      const u32 r = rb + lane;
      u32 c = 0, va = 0;
      const u32 *src = NULL;
      if (r < r1) {
        const u32 i = r / rpt, j = r - i * rpt;
        const TryInfo tr = tries[i];
        const u32 b = qcode[i] ^ probe_mask(j, (u32)P.ds, qbits + (size_t)i * pb);
        const uint2 sg = tr.seg[b];
        const u32 zs = sg.x & 0xFFFFu, co = sg.x >> 16;
        va = sg.y;
        c = min(co, tr.pm - min(zs, tr.pm));  // (a segment never leaves its row)
        src = tr.tab + (size_t)b * tr.pm + zs;
      }
      vtot += va;
      const u32 incl = wave_incl_scan(c);
      const u32 total = __shfl(incl, ANN_WAVE - 1);
      pref[lane] = incl - c;
      rptr[lane] = src;
      wave_lds_sync();
      for (u32 e0 = 0; e0 < total; e0 += ANN_WAVE) {  // the `total` ids of these runs, 64 at a time, through the bit test
        const u32 e = e0 + lane;
        u32 id = ANN_ID_NONE;
        if (e < total) {
          int lo_ = 0, hi_ = ANN_WAVE - 1;  // last run j with pref[j] <= e (it has c_j > 0)
          while (lo_ < hi_) {
            const int mid = (lo_ + hi_ + 1) >> 1;
            if (pref[mid] <= e) lo_ = mid; else hi_ = mid - 1;
          }
          id = rptr[lo_][e - pref[lo_]];
        }
        const bool own = id < P.n && tag_allows(tags, bits, qm, qv, id);
        const u64 mm = __ballot(own);
        if (own) list[cnt + mask_rank(mm)] = id;
        cnt += __popcll(mm);
        if (cnt + ANN_WAVE > ANN_S1_CHUNK) {
          wave_lds_sync();
          vown += cnt;
          probe_gather<D, RT>(P, list, cnt, alias, x, a, yq, scratch, S, y + (size_t)x * P.d);
          cnt = 0;
        }
      }
      wave_lds_sync();  // pref / rptr are rewritten by the next 64 runs
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) vtot += __shfl_xor(vtot, m);
  } else {
    for (u32 r = r0; r < r1; r++) {  // wave-uniform: one run at a time, the lanes walk its bucket row
      const u32 i = r / rpt, j = r - i * rpt;
      const TryInfo tr = tries[i];
      const u32 b = qcode[i] ^ probe_mask(j, (u32)P.ds, qbits + (size_t)i * pb);
      const u32 *row = tr.tab + (size_t)b * tr.pm;
      for (u32 z0 = 0; z0 < tr.pm; z0 += ANN_WAVE) {
        const u32 z = z0 + lane;
        const u32 id = z < tr.pm ? row[z] : ANN_ID_NONE;
        const bool ok = id < P.n && !(alias && id == x);
        // (the aliased query itself is counted when it is allowed, as in the segment path; probe_gather drops it)
        const bool own = id < P.n && id >= P.lo && id < P.hi && tag_allows(tags, bits, qm, qv, id);
        vtot += __popcll(__ballot(ok));
        const u64 mm = __ballot(own);
        if (own) list[cnt + mask_rank(mm)] = id;
        cnt += __popcll(mm);
        if (cnt + ANN_WAVE > ANN_S1_CHUNK) {
          wave_lds_sync();
          vown += cnt;
          probe_gather<D, RT>(P, list, cnt, alias, x, a, yq, scratch, S, y + (size_t)x * P.d);
          cnt = 0;
        }
      }
    }
  }
  wave_lds_sync();
  vown += cnt;
  probe_gather<D, RT>(P, list, cnt, alias, x, a, yq, scratch, S, y + (size_t)x * P.d);

  // ---- this wave's survivors -> merge buffer
  {
    const int m = wave_select_smallest(S.kbuf, S.kcnt, K1, S.kout);
    for (int i = lane; i < m; i += ANN_WAVE) mbuf[(size_t)w * K1 + i] = S.kout[i];
    if (lane == 0) {
      mcnt[w] = m;
      atomicAdd(&cnts[0], vtot);
      atomicAdd(&cnts[1], vown);
    }
  }
  __syncthreads();
  if (w == 0) {
    int total = 0;
    for (int ww = 0; ww < W; ww++) {  // cap >= W*K1 (host guarantees)
      const int m = mcnt[ww];
      for (int i = lane; i < m; i += ANN_WAVE) S.kbuf[total + i] = mbuf[(size_t)ww * K1 + i];
      total += m;
    }
    wave_lds_sync();
    const int m = wave_select_smallest(S.kbuf, total, K1, S.kout);
    for (int i = lane; i < K1; i += ANN_WAVE) {
      cand_dist[(size_t)x * K1 + i] = i < m ? key_dist(S.kout[i]) : ft_inf();
      cand_id[(size_t)x * K1 + i] = i < m ? key_id(S.kout[i]) : ANN_ID_NONE;
    }
    if (lane == 0) {
      nv_tot[x] = cnts[0];
      nv_own[x] = cnts[1];
    }
  }
}

// ------------------------------------------------------------------------------------------ stage 2
// stage2_filter_kernel over the stage-1 results and those of their graph neighbours that pass query x's test.  The gather
// goes through probe_gather for the reason given there: no FoldPlan private segment in the folded layouts.
template <int D, typename IdOut, typename RT>
__global__ __launch_bounds__(256) void stage2_tag_kernel(QParams P, int Q, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ top_id, const FT *__restrict__ top_dist,
                                                            const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                         const u32 *__restrict__ qmask, const u32 *__restrict__ qvalue, u32 P2, int K1, int cap,
                                                            IdOut *__restrict__ out_ids, FT *__restrict__ out_dist,
                                                            u32 *__restrict__ flist, u32 *__restrict__ fcount,
                                                            unsigned long long *__restrict__ exact_total,
                                                            unsigned long long *__restrict__ rows_done, u32 xbase) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const u32 x = xbase + blockIdx.x;
  const u32 qm = qmask[x], qv = qvalue[x];
  const int k = P.k;
  unsigned char *sp = smem;
  Key *kbuf_all = reinterpret_cast<Key *>(sp);   sp += sizeof(Key) * (size_t)W * cap;
  Key *kout_all = reinterpret_cast<Key *>(sp);   sp += sizeof(Key) * (size_t)W * K1;
  Key *mbuf = reinterpret_cast<Key *>(sp);       sp += sizeof(Key) * (size_t)W * K1;
  Key *top = reinterpret_cast<Key *>(sp);        sp += sizeof(Key) * (size_t)k;
  u32 *list_all = reinterpret_cast<u32 *>(sp);   sp += sizeof(u32) * (size_t)W * ANN_S1_CHUNK;
  int *mcnt = reinterpret_cast<int *>(sp);       sp += sizeof(int) * (size_t)W;
  u32 *cnts = reinterpret_cast<u32 *>(sp);       sp += sizeof(u32) * 4;  // [0] finite entries of the prefix [1] rows gathered
  sp = smem + (((sp - smem) + 15) & ~(size_t)15);
  FT *yq = reinterpret_cast<FT *>(sp);  // generic d only: [d] + W*[d]
  u32 *list = list_all + (size_t)w * ANN_S1_CHUNK;

  for (int t = threadIdx.x; t < k; t += blockDim.x) top[t] = key_make(top_dist[(size_t)x * k + t], top_id[(size_t)x * k + t]);
  if (threadIdx.x < 4) cnts[threadIdx.x] = 0;
  if constexpr (D == 0 || OcCode<D>::GEN)
    for (int z = threadIdx.x; z < P.d; z += blockDim.x) yq[z] = y[(size_t)x * P.d + z];
  VT a[RowChunks<D>::C];
  if constexpr (D > 0) {
    typedef RowLay<D> L;
    const VT *yp = reinterpret_cast<const VT *>(y + (size_t)x * D) + (lane % L::LPR);
#pragma unroll
    for (int c = 0; c < L::C; c++) a[c] = yp[c * L::LPR];
  } else if constexpr (D < 0 && !OcCode<D>::GEN) {
    const OcLanes<D> ol(P.d, lane);
#pragma unroll
    for (int c = 0; c < OcCode<D>::C; c++) a[c] = oc_load_chunk<D, false>(y + (size_t)x * P.d, ol.p + c * ol.oc, P.d);
  }
  __syncthreads();

  SelState S;
  S.kbuf = kbuf_all + (size_t)w * cap, S.kout = kout_all + (size_t)w * K1;
  S.kcnt = 0, S.K1 = K1, S.cap = cap, S.tau = key_max();
  FT *scratch = yq + (size_t)(1 + w) * P.d;
  u32 nfin = 0, vown = 0;
  int cnt = 0;
  const u32 per = (((P2 + W - 1) / W) + 63u) & ~63u;  // this wave's slice of the row [0, P2)
  const u32 s0 = min(P2, (u32)w * per), s1 = min(P2, s0 + per);
  for (u32 base = s0; base < s1; base += ANN_WAVE) {
    const u32 j = base + lane;
    bool direct = false, ok = false;
    Key dk = key_max();
    u32 id = ANN_ID_NONE;
    if (j < s1) {
      if (j < (u32)k) {  // the stage-1 result itself, with the distance it already has
        dk = top[j];
        direct = key_dist(dk) < ft_inf();
      } else {
        const u32 parent = key_id(top[j / k - 1]), z = j % k;
        id = parent < P.n ? P.graph[(size_t)parent * k + z] : (P.graph[z] | P.n);  // supercharge, Q7
        ok = id < P.n && !(alias && id == x) && id >= P.lo && id < P.hi && tag_allows(tags, bits, qm, qv, id);
      }
    }
    nfin += __popcll(__ballot(direct || ok));
    if (base < (u32)k) {  // wave-uniform: only the first passes of wave 0 hold direct keys
      if (S.kcnt + ANN_WAVE > S.cap) sel_shrink(S);
      const bool push = direct && key_less(dk, S.tau);
      const u64 dm = __ballot(push);
      if (push) S.kbuf[S.kcnt + mask_rank(dm)] = dk;
      S.kcnt += __popcll(dm);
    }
    const u64 mm = __ballot(ok);
    if (ok) list[cnt + mask_rank(mm)] = id;
    cnt += __popcll(mm);
    if (cnt + ANN_WAVE > ANN_S1_CHUNK) {
      wave_lds_sync();
      vown += cnt;
      probe_gather<D, RT>(P, list, cnt, alias, x, a, yq, scratch, S, y + (size_t)x * P.d);
      cnt = 0;
    }
  }
  wave_lds_sync();
  vown += cnt;
  probe_gather<D, RT>(P, list, cnt, alias, x, a, yq, scratch, S, y + (size_t)x * P.d);

  {  // this wave's survivors -> merge buffer
    const int m = wave_select_smallest(S.kbuf, S.kcnt, K1, S.kout);
    for (int i = lane; i < m; i += ANN_WAVE) mbuf[(size_t)w * K1 + i] = S.kout[i];
    if (lane == 0) {
      mcnt[w] = m;
      atomicAdd(&cnts[0], nfin);
      atomicAdd(&cnts[1], vown);
    }
  }
  __syncthreads();
  if (w == 0) {
    int total = 0;
    for (int ww = 0; ww < W; ww++) {  // cap >= W*K1 (host guarantees)
      const int m = mcnt[ww];
      for (int i = lane; i < m; i += ANN_WAVE) S.kbuf[total + i] = mbuf[(size_t)ww * K1 + i];
      total += m;
    }
    wave_lds_sync();
    const int m = wave_select_smallest(S.kbuf, total, K1, S.kout);
    bool bad = m < k;
    for (int t = lane; t + 1 < m; t += ANN_WAVE)
      if (ft_bits(key_dist(S.kout[t])) == ft_bits(key_dist(S.kout[t + 1]))) bad = true;
    if (m >= k && !(key_dist(S.kout[k - 1]) < ft_inf())) bad = true;
    if (P.L2 > P2 && cnts[0] >= P2 && m < K1) bad = true;
    const bool reject = !P.fixed && __ballot(bad) != 0;
    if (reject) {
      if (lane == 0) {
        flist[atomicAdd(fcount, 1u)] = x;
        if (exact_total) atomicAdd(exact_total, 1ull);
      }
    } else {  // (fixed mode: the k smallest distinct keys in (distance, id) order, (+inf, n) where fewer exist)
      for (int t = lane; t < k; t += ANN_WAVE) {
        out_ids[(size_t)x * k + t] = t < m ? (IdOut)key_id(S.kout[t]) : (IdOut)P.n;
        out_dist[(size_t)x * k + t] = t < m ? key_dist(S.kout[t]) : ft_inf();
      }
    }
    if (rows_done && lane == 0) atomicAdd(&rows_done[(x & 63u) * 8u], (unsigned long long)cnts[1]);
  }
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
