// ann_filter_kernels.h -- allow-list row filter of the fixed query mode (annhip_index_set_filter; gfx950).  The exact scan
// tests the same bitmap in its EX_BITS form (ann_exact_kernels.h).
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
