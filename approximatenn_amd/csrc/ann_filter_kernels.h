// ann_filter_kernels.h -- allow-list row filter of the fixed query mode and of the exact scan (annhip_index_set_filter,
// annhip_exact_knn_filtered; gfx950).
//
// The allow list is a bitmap, u32 bits[ceil(n / 32)]: row i is allowed iff bits[i >> 5] >> (i & 31) & 1.  A filter only
// narrows what fixed mode calls a valid id, so the kernels here are the fixed-mode kernels with one more test:
//
//   AdmitBits        the bit test as an admission policy: it sits where an id ENTERS the wave's LDS list, so a
//                    disallowed row is never fetched
//   stage1_filter    stage1_fixed_body's tested form (ann_probe_kernels.h) with the bit test, as a copy of its own
//   stage2_fixed_body   stage2_select_kernel with the policy in its `ok` predicate: stage 2 of the filter and tag
//                    families; stage2_filter is its entry point for the allow list
//   filter_pack      u8 flags -> bitmap;   filter_count   popcount of bits [0, n)
//   exact_scan_filtered / exact_scan_generic_filtered   the exact scan's two kernels with the tile's bitmap words in LDS
//   exact_tail       the exact scan's "no row" padding -> (n, +inf)
//
// The bitmap is a separate kernel argument everywhere, and an unfiltered query launches nothing from this file.
#pragma once
#include "ann_exact_kernels.h"
#include "ann_probe_kernels.h"

// id < n (the caller's test): the word is inside the bitmap
__device__ __forceinline__ bool filter_allows(const u32 *__restrict__ bits, u32 id) { return (bits[id >> 5] >> (id & 31u)) & 1u; }

// the admission policy of the allow list (see stage1_fixed_body)
struct AdmitBits {
  static constexpr bool ALWAYS = false;
  const u32 *__restrict__ bits;
  __device__ __forceinline__ bool operator()(u32 id) const { return filter_allows(bits, id); }
};

// ------------------------------------------------------------------------------------------ stage 1
// stage1_fixed_body's tested form (ann_probe_kernels.h) with the bit test, kept as its own copy: shared through the body,
// three instances of this kernel need more registers than they have here and lose a wave per SIMD
// (profiles/fixed_body_devcode.md).  A fix to the body's segment walk, list or merge has to be made here as well.
// nv_tot = valid ids seen, as before; nv_own = ids in the list = rows gathered = allowed valid ids (self included when
// allowed: the gather drops it).
template <int D, bool SEG, typename RT>
__global__ __launch_bounds__(256) void stage1_filter_kernel(QParams P, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ codes,
                                                            const unsigned char *__restrict__ pbits, int pb, u32 rpt,
                                                            const u32 *__restrict__ bits, int K1, int cap,
                                                            FT *__restrict__ cand_dist, u32 *__restrict__ cand_id,
                                                            u32 *__restrict__ nv_tot, u32 *__restrict__ nv_own) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  // ---- LDS carve-up: stage1_fixed_body's (stage1_probe_lds_bytes on the host)
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
        const bool own = id < P.n && filter_allows(bits, id);
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
        const bool own = id < P.n && id >= P.lo && id < P.hi && filter_allows(bits, id);
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
// stage2_select_kernel (same arguments, same LDS carve-up, same rejection rule outside fixed mode) over the stage-1
// results and the ADMITTED graph neighbours of those results: `ok` gains adm().  The stage-1 results enter with the
// distances they have; stage 1 of the same family returns admitted rows only.  The gather goes through probe_gather: the
// same arithmetic as gather_select, without the 72-byte private segment the folded layouts' FoldPlan constructor costs.
template <int D, typename IdOut, typename RT, typename Admit>
__device__ __forceinline__ void stage2_fixed_body(const QParams &P, const FT *y, int alias, const u32 *top_id,
                                                  const FT *top_dist, const Admit &adm, u32 P2, int K1, int cap,
                                                  IdOut *out_ids, FT *out_dist, u32 *flist, u32 *fcount,
                                                  unsigned long long *exact_total, unsigned long long *rows_done, u32 xbase) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const u32 x = xbase + blockIdx.x;
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
  load_query_slice<D>(P, y, x, lane, a);
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
        ok = id < P.n && !(alias && id == x) && id >= P.lo && id < P.hi && adm(id);
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
    list_push<D, RT>(ok, id, P, list, cnt, vown, alias, x, a, yq, scratch, S, y);
  }
  list_flush<D, RT>(P, list, cnt, vown, alias, x, a, yq, scratch, S, y);

  const int m = merge_waves(S, mbuf, mcnt, w, W, K1, [&] {
    atomicAdd(&cnts[0], nfin);
    atomicAdd(&cnts[1], vown);
  });
  if (w == 0) {
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

template <int D, typename IdOut, typename RT>
__global__ __launch_bounds__(256) void stage2_filter_kernel(QParams P, int Q, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ top_id, const FT *__restrict__ top_dist,
                                                            const u32 *__restrict__ bits, u32 P2, int K1, int cap,
                                                            IdOut *__restrict__ out_ids, FT *__restrict__ out_dist,
                                                            u32 *__restrict__ flist, u32 *__restrict__ fcount,
                                                            unsigned long long *__restrict__ exact_total,
                                                            unsigned long long *__restrict__ rows_done, u32 xbase) {
  stage2_fixed_body<D, IdOut, RT>(P, y, alias, top_id, top_dist, AdmitBits{bits}, P2, K1, cap, out_ids, out_dist, flist, fcount,
                                  exact_total, rows_done, xbase);
}

// ------------------------------------------------------------------------------------------ bitmap helpers
// flags[i] != 0 -> bit i: a wave packs 64 flags with one ballot (two words; the tail bits of the last word are zero)
__global__ __launch_bounds__(256) void filter_pack_kernel(size_t n, const unsigned char *__restrict__ flags,
                                                          u32 *__restrict__ bits) {
  const size_t nw = (n + 31) / 32, waves = (size_t)gridDim.x * (blockDim.x >> 6);
  const int lane = lane_id();
  for (size_t g = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g * ANN_WAVE < n; g += waves) {
    const size_t i = g * ANN_WAVE + lane;
    const u64 m = __ballot(i < n && flags[i] != 0);
    if (lane == 0) {
      bits[2 * g] = (u32)m;
      if (2 * g + 1 < nw) bits[2 * g + 1] = (u32)(m >> 32);
    }
  }
}

// *out += set bits among [0, n)
__global__ __launch_bounds__(256) void filter_count_kernel(size_t n, const u32 *__restrict__ bits,
                                                           unsigned long long *__restrict__ out) {
  const size_t nw = (n + 31) / 32;
  unsigned long long acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (size_t)gridDim.x * blockDim.x) {
    u32 v = bits[i];
    if (i == nw - 1 && (n & 31)) v &= (1u << (n & 31)) - 1u;
    acc += __popc(v);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
  if (lane_id() == 0 && acc) atomicAdd(out, acc);
}

// ------------------------------------------------------------------------------------------ exact scan
// One bit of the allow list for every row of a tile: the bitmap words that cover rows [t0, t0 + rows) sit in LDS from
// word t0 >> 5 on -- fetched once per tile, read by every wave for all its queries.
#define ANN_EX_TBITS(tile_rows) ((size_t)(tile_rows) / 32 + 2)  // words of LDS behind the waves' buffers
__device__ __forceinline__ u32 ex_tile_words(u32 t0, u32 rows) { return ((t0 + rows - 1) >> 5) - (t0 >> 5) + 1; }
__device__ __forceinline__ bool ex_tile_allows(const u32 *tbits, u32 t0, u32 id) {
  return (tbits[(id >> 5) - (t0 >> 5)] >> (id & 31u)) & 1u;
}

// exact_scan_kernel with the allow list: a row whose bit is clear is never a survivor, and a wave pass without an allowed
// row is not scored at all.  Where the next tile travels through registers, so does its bitmap: one word per thread (such
// a tile has at most 128 rows per wave, hence fewer words than the workgroup has threads).
template <int D>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void exact_scan_filtered_kernel(ExArgs A, const u32 *__restrict__ bits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.d;
  FT *tile = reinterpret_cast<FT *>(smem);
  const size_t tile_bytes = ((size_t)A.tile_rows * d * sizeof(FT) + 15) & ~(size_t)15;
  Key *kbase = reinterpret_cast<Key *>(smem + tile_bytes) + (size_t)w * ((size_t)ANN_EX_QB * A.cap + A.k);
  u32 *tbits = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * sizeof(Key) * ((size_t)ANN_EX_QB * A.cap + A.k));
  const u32 qrel = (blockIdx.x * W + w) * ANN_EX_QB;  // first query of this wave, relative to q0
  const u32 qbase = A.q0 + qrel, qend = A.q0 + A.qn;
  ExSel S;
  S.init(kbase, kbase + (size_t)ANN_EX_QB * A.cap, A.cap, A.k, qbase, qend);
  const ExLanes<D> ln(d, lane);
  VT a[ANN_EX_QB][C];
#pragma unroll
  for (int i = 0; i < ANN_EX_QB; i++) {
    const u32 q = qbase + i < qend ? qbase + i : qend - 1;  // loads stay inside y; the result is never admitted
    const FT *yq = A.y + (size_t)q * d;
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
    for (u32 i = threadIdx.x; i < ex_tile_words(t0, rows); i += blockDim.x) tbits[i] = bits[(t0 >> 5) + i];
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // the queries have arrived before the loop starts (see exact_scan_kernel)
  while (rows) {
    __syncthreads();  // the tile and its bits are in LDS
    const u32 t1 = t0 + rows;
    const u32 rows1 = t1 < r_end ? min((u32)A.tile_rows, r_end - t1) : 0;
    // the next tile's loads are in flight while this one is scored
    typedef FT pf_t __attribute__((ext_vector_type(ANN_VEC)));
    pf_t pf0 = 0, pf1 = 0;
    u32 pfw = 0;
    if constexpr (ExCfg<D>::PREFETCH) {
      if (prefetch && rows1) {  // unconditional loads from clamped addresses: plain registers, nothing waits here
        const pf_t *src = reinterpret_cast<const pf_t *>(A.points + (size_t)t1 * d);
        const u32 last = rows1 * (u32)(d / ANN_VEC) - 1;
        pf0 = src[min(threadIdx.x, last)];
        pf1 = src[min(threadIdx.x + blockDim.x, last)];
        pfw = bits[(t1 >> 5) + min(threadIdx.x, ex_tile_words(t1, rows1) - 1)];
      }
    }
    for (u32 r0 = 0; r0 < rows; r0 += ln.rpw) {
      const u32 r = r0 + ln.g;
      const bool act = ln.valid && r < rows;
      const bool allowed = act && ex_tile_allows(tbits, t0, t0 + r);
      if (!__ballot(allowed)) continue;  // wave-uniform: no row of this pass can survive
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
#pragma unroll
      for (int i = 0; i < ANN_EX_QB; i++) pass[i] = head && key_less(key[i], S.tau[i]) && !(A.self && id == qbase + i);
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
        if (threadIdx.x < ex_tile_words(t1, rows1)) tbits[threadIdx.x] = pfw;
        stored = true;
      }
    }
    if (!stored) {
      ex_fill_tile(tile, A.points, t1, rows1, d);
      for (u32 i = threadIdx.x; i < ex_tile_words(t1, rows1); i += blockDim.x) tbits[i] = bits[(t1 >> 5) + i];
    }
    t0 = t1, rows = rows1;
  }
  S.store(A.ws, qrel, A.qn, A.ranges, (int)blockIdx.y);
}

// exact_scan_generic_kernel with the allow list
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void exact_scan_generic_filtered_kernel(ExArgs A,
                                                                                           const u32 *__restrict__ bits) {
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
  u32 *tbits = reinterpret_cast<u32 *>(smem + tile_bytes + (size_t)W * wave_bytes);
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
    for (u32 i = threadIdx.x; i < ex_tile_words(t0, rows); i += blockDim.x) tbits[i] = bits[(t0 >> 5) + i];
    __syncthreads();
#define ANN_EX_GEN_QUERY(I)                                                                                  \
  if (qbase + (I) < qend) {                                                                                  \
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
      const bool act = lane < np && ex_tile_allows(tbits, t0, id);                                           \
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

// exact_merge_kernel (reused) unpacks key_max() where a query has fewer than k allowed rows: those entries -> (n, +inf)
__global__ void exact_tail_kernel(size_t count, size_t n, size_t *__restrict__ ids, FT *__restrict__ dists) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x)
    if (ids[e] == (size_t)ANN_ID_NONE) ids[e] = n, dists[e] = ft_inf();
}
