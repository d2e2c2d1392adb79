// ann_radius_kernels.h -- radius queries of the fixed query mode (annhip_query_radius, annhip_index_exact_query_radius,
// annhip_radius_trim; gfx950).
//
// Row i is IN RANGE for query q iff dist(q, i) <= radius[q], compared as floating-point values: -0.0 counts as 0, a
// negative or NaN radius puts nothing in range, +inf puts every row in range (a row whose distance overflowed to +inf
// included).  A radius query returns the kcap smallest (distance, id) keys among the in-range candidates of fixed mode.
//
//   stage1_radius    stage1_fixed_body's tested form (ann_probe_kernels.h), both forms (segment walk, slot scan), as a
//                    copy of its own, with:
//                    - validity behind nullable pointers as in stage2_kq_kernel: `bits` (the allow list) and `tags`
//                      may each be NULL.  NULL or not is a kernel argument, hence one wave-uniform branch each and no
//                      template axis: one family serves plain, probe, allow list and tags.
//                    - the admission threshold S.tau starts at the query's radius, not at key_max(): only in-range keys
//                      ever reach a selection buffer, so wave_select_smallest's K1 passes run over the in-range keys and
//                      nothing else.  sel_shrink only ever lowers tau: nothing else in the selection changes.
//   radius_trim      the end of both radius calls: cuts a [Q][kcap] result in (distance, id) order at the radius, pads the
//                    rest and counts.
//
// Stage 2 and the tail merges stay the k-per-call kernels (ann_kq_kernels.h, ann_tail*_kernels.h): their input holds
// in-range results and pads only, every key they add that is beyond the radius sorts behind every key within it, and the
// trim cuts the row there -- the kcap smallest of a superset, trimmed, are the kcap smallest of the in-range subset.
// No call but the radius entry points launches anything from this file.
#pragma once
#include "ann_kq_kernels.h"

// id < n (the caller's test).  The two loads are independent of each other where both tests apply.
__device__ __forceinline__ bool radius_allows(const u32 *__restrict__ tags, const u32 *__restrict__ bits, const TagPred &tp, u32 id) {
  if (tags) return tag_allows(tags, bits, tp, id);
  if (bits) return filter_allows(bits, id);
  return true;
}

// The initial admission threshold of a query with radius r: key_less(key, tau) <=> the key's distance is <= r.
//   r >= +0 (or -0.0, which counts as 0): (r, 0xFFFFFFFF).  Row ids stay below 0xFFFFFFF0 and the order of keys is the
//     unsigned order of the bits of non-negative values in both key widths, so every (dist <= r, id) is smaller and every
//     (dist > r, id) is larger; with r = +inf the keys with distance +inf are admitted, NaNs are not.
//   r < 0 or NaN: the smallest key there is, (+0, 0) -- nothing is smaller, nothing is admitted.
__device__ __forceinline__ Key radius_tau(FT r) {
  const FT zero = 0;
  if (!(r >= zero)) return key_make(zero, 0u);
  return key_make(r == zero ? zero : r, 0xFFFFFFFFu);
}

// ------------------------------------------------------------------------------------------ stage 1
// stage1_fixed_body's tested form (ann_probe_kernels.h) kept as a copy of its own, like stage1_filter_kernel and for the
// same reason: two f64 instances lose a wave per SIMD through the shared body (profiles/fixed_body_devcode.md).  Same LDS
// carve-up (stage1_probe_lds_bytes on the host); probe_gather, the selection state, the merge and the outputs unchanged.  pb = 0 with rpt = 1 + ds gives the plain buckets of fixed mode.  nv_own = ids in the
// list = rows gathered = the valid ids of the probed buckets (the radius is known only after a row is fetched).
template <int D, bool SEG, typename RT>
__global__ __launch_bounds__(256) void stage1_radius_kernel(QParams P, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ codes,
                                                            const unsigned char *__restrict__ pbits, int pb, u32 rpt,
                                                            const FT *__restrict__ radius,
                                                            const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                            const u32 *__restrict__ qmask, const u32 *__restrict__ qlo, const u32 *__restrict__ qhi,
                                                            int K1, int cap, FT *__restrict__ cand_dist,
                                                            u32 *__restrict__ cand_id, u32 *__restrict__ nv_tot,
                                                            u32 *__restrict__ nv_own) {
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
  TagPred tp{0, 0, 0};  // wave-uniform: this query's predicate and radius, read once
  if (tags) tp = tag_pred(qmask, qlo, qhi, x);
  const Key tau0 = radius_tau(radius[x]);
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
  S.kcnt = 0, S.K1 = K1, S.cap = cap, S.tau = tau0;
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
      for (u32 e0 = 0; e0 < total; e0 += ANN_WAVE) {  // the `total` ids of these runs, 64 at a time, through the validity test
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
        const bool own = id < P.n && radius_allows(tags, bits, tp, id);
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
        // (the aliased query itself is counted when it is valid, as in the segment path; probe_gather drops it)
        const bool own = id < P.n && id >= P.lo && id < P.hi && radius_allows(tags, bits, tp, id);
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

// ------------------------------------------------------------------------------------------ trim
// One wave per row of a [Q][kcap] result in (distance, id) order, the lanes 64 entries at a time (coalesced).  An entry stays
// iff its id is not pad_id and its distance is <= radius[q]; a pad is told by its ID, never by its distance (a pad's +inf is
// <= +inf).  Every other entry becomes (pad_id, +inf); counts[q] = entries kept.  In a row that is ascending with its pads
// at the end the kept entries are a prefix: the row is cut behind the last of them.  In place; only rejected entries are
// written.
__global__ __launch_bounds__(256) void radius_trim_kernel(size_t Q, size_t kcap, size_t pad_id, const FT *__restrict__ radius,
                                                          size_t *__restrict__ ids, FT *__restrict__ dists,
                                                          u32 *__restrict__ counts) {
  const int lane = lane_id();
  const size_t q = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= Q) return;  // wave-uniform
  const FT r = radius[q];
  size_t *ri = ids + q * kcap;
  FT *rd = dists + q * kcap;
  u32 kept = 0;
  for (size_t t0 = 0; t0 < kcap; t0 += ANN_WAVE) {
    const size_t t = t0 + lane;
    bool keep = false;
    if (t < kcap) {
      keep = ri[t] != pad_id && rd[t] <= r;  // (false for a NaN radius; -0.0 compares equal to 0)
      if (!keep) ri[t] = pad_id, rd[t] = ft_inf();
    }
    kept += (u32)__popcll(__ballot(keep));
  }
  if (counts && lane == 0) counts[q] = kept;
}
