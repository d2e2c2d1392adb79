// ann_probe_kernels.h -- query-directed multi-probe for the fixed query mode (annhip_index_set_probe; gfx950).
//
// Fixed mode looks, per try, into the query's own bucket and the ds buckets at Hamming distance 1.  With "pair bits"
// b > 0 it also looks into the C(b,2) buckets reached by flipping TWO of the query's b least certain hash bits: the
// hash is the sign of ds projections, and a projection close to zero is a bit that is likely to differ for a true
// neighbour.
//
//   codes_probe_lpq / codes_probe   the hash kernels' dot products, literally (same tree, same "+ 0": the codes are
//                                   bit-identical to codes_lpq_kernel / codes_kernel), plus the ranking: per (query, try)
//                                   the b projection indices of smallest magnitude, ascending by (|p| bits, s)
//   stage1_fixed_body               stage 1 of the fixed-mode families that decode their runs as (try, mask) -- masks 0,
//                                   1<<z, and bit(o[u]) | bit(o[v]) for u < v < b -- with admission to the wave's list as
//                                   a policy type; stage1_probe is its entry point that admits every valid id, stage1_tag
//                                   (ann_tag_kernels.h) the one with a test.  stage1_filter and stage1_radius keep a copy
//                                   of its tested form in their own headers (the reason is given there).
//   load_query_slice, list_push / list_flush, merge_waves   the pieces that body shares with the stage-2 bodies
//
// b = 0 without a filter, tags or a radius launches stage1_select_kernel as before.
#pragma once
#include "ann_query_kernels.h"

// |x| as raw bits: orders like the magnitude for everything that is not a NaN; +-0 -> 0.
__device__ __forceinline__ UB ft_mag_bits(FT x) { return ft_bits(x) & (~(UB)0 >> 1); }

// Position of (mine, s) among the ds keys (strip[s2 * stride], s2) of one (query, try): the number of keys below it.
// Keys are distinct (s differs), so the positions are a permutation of 0 .. ds-1.  `strip` is LDS; nothing here is a
// register array, so nothing can end up in scratch memory.
__device__ __forceinline__ int probe_rank(const UB *strip, int stride, int ds, UB mine, int s) {
  int rank = 0;
  for (int s2 = 0; s2 < ds; s2++) {
    const UB o = strip[(size_t)s2 * stride];
    rank += (o < mine || (o == mine && s2 < s)) ? 1 : 0;
  }
  return rank;
}

// ------------------------------------------------------------------------------------------ codes + ranking
// codes_lpq_kernel with the ranking: a lane owns a query, the workgroup's waves split the try's ds projections.  Every
// projection's magnitude goes to an LDS strip mag[s][lane]; after the barrier each wave ranks the projections it
// computed against all ds of its lane's query (ds^2 / waves LDS reads per lane: ~200 at ds = 20 against ~7 700 lane
// instructions of dot products) and stores s at pbits[q][t][rank] where rank < pb.
template <int D>
__global__ __launch_bounds__(64 * ANN_LPQ_WAVES) void codes_probe_lpq_kernel(QParams P, int Q, const FT *__restrict__ y,
                                                                             u32 *__restrict__ codes, u32 *__restrict__ zero_me,
                                                                             int pb, unsigned char *__restrict__ pbits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (zero_me && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *zero_me = 0;
  constexpr int NC = D / ANN_VEC;  // 16-byte chunks per row
  const int lane = lane_id(), t = blockIdx.y, w = threadIdx.x >> 6;
  VT *rows = reinterpret_cast<VT *>(smem);  // [ds][NC], then the means [NC], the waves' partial codes, the magnitudes
  VT *mean = rows + (size_t)P.ds * NC;
  u32 *pcode = reinterpret_cast<u32 *>(mean + NC);                      // [ANN_LPQ_WAVES][64]
  UB *mag = reinterpret_cast<UB *>(pcode + ANN_LPQ_WAVES * ANN_WAVE);  // [ds][64]
  const VT *src = reinterpret_cast<const VT *>(P.bases + (size_t)t * P.ds * D);
  for (int i = threadIdx.x; i < P.ds * NC; i += blockDim.x) rows[i] = src[i];
  for (int i = threadIdx.x; i < NC; i += blockDim.x) mean[i] = reinterpret_cast<const VT *>(P.means)[i];
  __syncthreads();
  const int q = blockIdx.x * ANN_WAVE + lane;
  const bool live = q < Q;
  const VT *yp = reinterpret_cast<const VT *>(y + (size_t)(live ? q : Q - 1) * D);
  FT a[D];
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const VT yv = yp[c], mv = mean[c];
    const FT *py = reinterpret_cast<const FT *>(&yv), *pm = reinterpret_cast<const FT *>(&mv);
#pragma unroll
    for (int j = 0; j < ANN_VEC; j++) a[c * ANN_VEC + j] = py[j] - pm[j];  // subtract_off, compute.cl:44-49
  }
  const FT zero = 0;
  u32 code = 0;
  const int sper = (P.ds + ANN_LPQ_WAVES - 1) / ANN_LPQ_WAVES, s_lo = w * sper, s_hi = min(P.ds, s_lo + sper);
#pragma unroll 1
  for (int s = s_lo; s < s_hi; s++) {
    const VT *b = rows + (size_t)s * NC;
    FT m[D / 2];
#pragma unroll
    for (int c = 0; c < NC / 2; c++) {  // products + the tree's first level: z with z + D/2 (see codes_lpq_kernel)
      if (c % 4 == 0 && c) __builtin_amdgcn_sched_barrier(0);
      const VT b0 = b[c], b1 = b[c + NC / 2];
      const FT *p0 = reinterpret_cast<const FT *>(&b0), *p1 = reinterpret_cast<const FT *>(&b1);
#pragma unroll
      for (int j = 0; j < ANN_VEC; j++) {
        const int z = c * ANN_VEC + j;
        m[z] = a[z] * p0[j] + (a[z + D / 2] * p1[j] + zero);
      }
    }
#pragma unroll
    for (int h = D / 4; h >= 1; h >>= 1)
#pragma unroll
      for (int z = 0; z < h; z++) m[z] = m[z] + (m[z + h] + zero);
    const u32 sign = (u32)(ft_bits(m[0]) >> (sizeof(FT) * 8 - 1));
    code |= sign << (P.ds - 1 - s);  // coord 0 = MSB, compute.cl:223-231
    mag[s * ANN_WAVE + lane] = ft_mag_bits(m[0]);
  }
  pcode[w * ANN_WAVE + lane] = code;
  __syncthreads();
  if (w == 0 && live) {
#pragma unroll
    for (int ww = 1; ww < ANN_LPQ_WAVES; ww++) code |= pcode[ww * ANN_WAVE + lane];
    codes[(size_t)q * P.T + t] = code;
  }
  if (live) {
    unsigned char *out = pbits + ((size_t)q * P.T + t) * pb;
#pragma unroll 1
    for (int s = s_lo; s < s_hi; s++) {
      const int rank = probe_rank(mag + lane, ANN_WAVE, P.ds, mag[s * ANN_WAVE + lane], s);
      if (rank < pb) out[rank] = (unsigned char)s;
    }
  }
}

// codes_kernel with the ranking, for every other row length: a wave computes the ds projections of one (query, try);
// the lane that holds a projection's value stores its magnitude into the wave's LDS strip, then lane s ranks
// projection s against the strip.
#define ANN_PROBE_WPB 4  // waves per workgroup of codes_probe_kernel (the host launches exactly this many)
template <int D>
__global__ __launch_bounds__(64 * ANN_PROBE_WPB) void codes_probe_kernel(QParams P, int Q, const FT *__restrict__ y,
                                                                         u32 *__restrict__ codes, u32 *__restrict__ zero_me,
                                                                         int pb, unsigned char *__restrict__ pbits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ UB wmag[ANN_PROBE_WPB][32];  // ds <= 31
  if (zero_me && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *zero_me = 0;
  const int lane = lane_id(), w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  UB *strip = wmag[w];
  if constexpr (D > 0) {
    typedef RowLay<D> L;
    const int t = blockIdx.y;
    const int q0 = blockIdx.x * ANN_CODES_QPB, q1 = min(Q, q0 + ANN_CODES_QPB);
    VT *rows = reinterpret_cast<VT *>(smem);  // [ds][D/VEC]
    const VT *src = reinterpret_cast<const VT *>(P.bases + (size_t)t * P.ds * D);
    for (int i = threadIdx.x; i < P.ds * (D / ANN_VEC); i += blockDim.x) rows[i] = src[i];
    __syncthreads();
    const int p = lane % L::LPR, g = lane / L::LPR;
    VT mean[L::C];
    const VT *mp = reinterpret_cast<const VT *>(P.means) + p;
#pragma unroll
    for (int c = 0; c < L::C; c++) mean[c] = mp[c * L::LPR];
    for (int q = q0 + w; q < q1; q += wpb) {
      VT a[L::C];
      const VT *yp = reinterpret_cast<const VT *>(y + (size_t)q * D) + p;
#pragma unroll
      for (int c = 0; c < L::C; c++) {
        VT yv = yp[c * L::LPR];
        FT *o = reinterpret_cast<FT *>(&a[c]);
        const FT *py = reinterpret_cast<const FT *>(&yv), *pm = reinterpret_cast<const FT *>(&mean[c]);
#pragma unroll
        for (int j = 0; j < ANN_VEC; j++) o[j] = py[j] - pm[j];  // subtract_off, compute.cl:44-49
      }
      u32 code = 0;
      for (int s0 = 0; s0 < P.ds; s0 += L::RPW) {
        const int s = s0 + g;
        const bool act = s < P.ds;
        const VT *bp = rows + (size_t)(act ? s : 0) * (D / ANN_VEC) + p;
        VT b[L::C];
#pragma unroll
        for (int c = 0; c < L::C; c++) b[c] = bp[c * L::LPR];
        FT v = row_reduce<D, ROW_PRODUCT>(a, b);
        u32 sign = (u32)(ft_bits(v) >> (sizeof(FT) * 8 - 1));
        if (act && p == 0 && sign) code |= 1u << (P.ds - 1 - s);  // coord 0 = MSB, compute.cl:223-231
        if (act && p == 0) strip[s] = ft_mag_bits(v);
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) code |= __shfl_xor(code, m);
      if (lane == 0) codes[(size_t)q * P.T + t] = code;
      wave_lds_sync();
      if (lane < P.ds) {
        const int rank = probe_rank(strip, 1, P.ds, strip[lane], lane);
        if (rank < pb) pbits[((size_t)q * P.T + t) * pb + rank] = (unsigned char)lane;
      }
      wave_lds_sync();  // the strip is rewritten by the wave's next query
    }
  } else {
    const long item = (long)blockIdx.x * wpb + w;
    const bool live = item < (long)Q * P.T;
    const int q = live ? (int)(item / P.T) : 0, t = live ? (int)(item % P.T) : 0;
    u32 code = 0;
    if constexpr (D < 0 && !OcCode<D>::GEN) {
      constexpr int C = OcCode<D>::C, OC = OcCode<D>::OC;
      const OcLanes<D> ol(P.d, lane);
      const int oc = ol.oc, rpw = ol.rpw, g = ol.g, p = ol.p;
      VT a[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        VT yv = oc_load_chunk<D, false>(y + (size_t)q * P.d, p + c * oc, P.d), mv = oc_load_chunk<D, false>(P.means, p + c * oc, P.d);
        FT *o = reinterpret_cast<FT *>(&a[c]);
        const FT *py = reinterpret_cast<const FT *>(&yv), *pm = reinterpret_cast<const FT *>(&mv);
#pragma unroll
        for (int j = 0; j < ANN_VEC; j++) o[j] = py[j] - pm[j];
      }
      for (int s0 = 0; s0 < P.ds; s0 += rpw) {
        const int sidx = s0 + g;
        const bool act = ol.valid && sidx < P.ds;
        const FT *brow = P.bases + ((size_t)t * P.ds + (act ? sidx : 0)) * P.d;
        VT b[C];
#pragma unroll
        for (int c = 0; c < C; c++) b[c] = oc_load_chunk<D, false>(brow, p + c * oc, P.d);
        FT v = row_reduce_oc<C, ROW_PRODUCT, OC>(a, b, oc, p, oc_tree_len<D>(P.d));
        u32 sign = (u32)(ft_bits(v) >> (sizeof(FT) * 8 - 1));
        if (act && p == 0 && sign) code |= 1u << (P.ds - 1 - sidx);
        if (act && p == 0) strip[sidx] = ft_mag_bits(v);
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) code |= __shfl_xor(code, m);
    } else {
      const int d = P.d;
      FT *u = reinterpret_cast<FT *>(smem) + (size_t)w * 2 * d, *m = u + d;
      for (int z = lane; z < d; z += ANN_WAVE) u[z] = y[(size_t)q * d + z] - P.means[z];
      wave_lds_sync();
      for (int s = 0; s < P.ds; s++) {
        FT v = row_reduce_generic<ROW_PRODUCT>(d, u, P.bases + ((size_t)t * P.ds + s) * d, m);
        code = code << 1 | (u32)(ft_bits(v) >> (sizeof(FT) * 8 - 1));
        if (lane == 0) strip[s] = ft_mag_bits(v);
      }
    }
    if (live && lane == 0) codes[item] = code;
    wave_lds_sync();
    if (live && lane < P.ds) {
      const int rank = probe_rank(strip, 1, P.ds, strip[lane], lane);
      if (rank < pb) pbits[(size_t)item * pb + rank] = (unsigned char)lane;
    }
  }
}

// ------------------------------------------------------------------------------------------ stage 1
// Runs of one try, in order: 0 = the query's own bucket, 1 .. ds = Hamming distance 1 (bit yy-1, as compute_which),
// then pair number pn = v (v - 1) / 2 + u for u < v < pb: the two bits of ranks u and v.  `ranked` = this try's pb ranked
// projection indices (LDS); projection s is bit ds-1-s of the code.  The result is masked to ds bits, so that a bucket
// index stays inside the table whatever the bytes hold.
__device__ __forceinline__ u32 probe_mask(u32 j, u32 ds, const unsigned char *ranked) {
  u32 m;
  if (j == 0) {
    m = 0;
  } else if (j <= ds) {
    m = 1u << (j - 1);
  } else {
    const u32 pn = j - ds - 1;
    u32 v = (u32)((1.0f + sqrtf(1.0f + 8.0f * (float)pn)) * 0.5f);  // pn < 465: exact up to the two corrections below
    while (v * (v - 1) / 2 > pn) v--;
    while ((v + 1) * v / 2 <= pn) v++;
    const u32 u = pn - v * (v - 1) / 2;
    m = (1u << ((ds - 1 - ranked[u]) & 31u)) | (1u << ((ds - 1 - ranked[v]) & 31u));
  }
  return m & ((1u << ds) - 1u);
}

// gather_select for this kernel.  The folded layouts build their FoldPlan here with constant indices: its constructor's
// loop has a run-time trip count, which puts the plan's three small arrays into scratch memory (72 bytes per lane).
template <int D, typename RT>
__device__ __forceinline__ void probe_gather(const QParams &P, const u32 *list, int cnt, int alias, u32 x,
                                             const VT (&a)[RowChunks<D>::C], const FT *yq, FT *scratch, SelState &S,
                                             const FT *yrow) {
  if constexpr (D < 0 && OcCode<D>::FOLD > 0) {
    FoldPlan fp(0);  // empty plan; filled below exactly as FoldPlan(P.d) fills it
    int s = P.d, L = 0;
#pragma unroll
    for (int l = 0; l < 5; l++) {
      const bool on = s > 16;
      fp.sprev[l] = on ? s : 0, fp.h[l] = on ? s >> 1 : 0, fp.odd[l] = on ? s & 1 : 0;
      if (on) s >>= 1, L = l + 1;
    }
    fp.L = L, fp.sL = s;
    if (fp.sL > 64) fp.L = 0;
    gather_fold<OcCode<D>::FOLD, RT>(P, fp, list, cnt, alias, x, yrow, S);
    wave_lds_sync();
  } else {
    gather_select<D, RT>(P, list, cnt, alias, x, a, yq, scratch, S, yrow);
  }
}

// ------------------------------------------------------------------------------------------ shared pieces
// What the fixed-mode bodies (stage1_fixed_body here, stage2_fixed_body in ann_filter_kernels.h, stage2_kq_kernel) have
// in common.  Everything is forced inline: an entry point compiles to the code it had when it spelled these out.

// The query row, as this lane's slice (the generic layouts read it from LDS instead: yq).
template <int D>
__device__ __forceinline__ void load_query_slice(const QParams &P, const FT *y, u32 x, int lane, VT (&a)[RowChunks<D>::C]) {
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
}

// The wave's id list: ANN_S1_CHUNK ids in LDS, cnt of them in use; vown counts the rows gathered.  list_flush gathers the
// listed rows into the selection and empties the list; list_push appends the ids of the lanes whose `own` is set
// (ballot-compacted) and flushes when another 64 might not fit.
template <int D, typename RT>
__device__ __forceinline__ void list_flush(const QParams &P, const u32 *list, int &cnt, u32 &vown, int alias, u32 x,
                                           const VT (&a)[RowChunks<D>::C], const FT *yq, FT *scratch, SelState &S,
                                           const FT *y) {
  wave_lds_sync();
  vown += cnt;
  probe_gather<D, RT>(P, list, cnt, alias, x, a, yq, scratch, S, y + (size_t)x * P.d);
  cnt = 0;
}
template <int D, typename RT>
__device__ __forceinline__ void list_push(bool own, u32 id, const QParams &P, u32 *list, int &cnt, u32 &vown, int alias,
                                          u32 x, const VT (&a)[RowChunks<D>::C], const FT *yq, FT *scratch, SelState &S,
                                          const FT *y) {
  const u64 mm = __ballot(own);
  if (own) list[cnt + mask_rank(mm)] = id;
  cnt += __popcll(mm);
  if (cnt + ANN_WAVE > ANN_S1_CHUNK) list_flush<D, RT>(P, list, cnt, vown, alias, x, a, yq, scratch, S, y);
}

// The end of a body: this wave's survivors -> mbuf / mcnt (lane 0 then runs `tally`, the workgroup's counters), barrier,
// wave 0 gathers the waves' survivors and selects.  Returns m, the number of distinct keys in S.kout, ascending (wave 0;
// 0 in the other waves).  cap >= W * K1 (the host guarantees).
template <typename Tally>
__device__ __forceinline__ int merge_waves(SelState &S, Key *mbuf, int *mcnt, int w, int W, int K1, Tally tally) {
  const int lane = lane_id();
  {
    const int m = wave_select_smallest(S.kbuf, S.kcnt, K1, S.kout);
    for (int i = lane; i < m; i += ANN_WAVE) mbuf[(size_t)w * K1 + i] = S.kout[i];
    if (lane == 0) {
      mcnt[w] = m;
      tally();
    }
  }
  __syncthreads();
  int m = 0;
  if (w == 0) {
    int total = 0;
    for (int ww = 0; ww < W; ww++) {
      const int mw = mcnt[ww];
      for (int i = lane; i < mw; i += ANN_WAVE) S.kbuf[total + i] = mbuf[(size_t)ww * K1 + i];
      total += mw;
    }
    wave_lds_sync();
    m = wave_select_smallest(S.kbuf, total, K1, S.kout);
  }
  return m;
}

// ------------------------------------------------------------------------------------------ stage 1, every family
// Admission: which valid ids of a probed bucket enter the wave's list.  A policy is built once per workgroup from the
// kernel's own arguments and x, offers operator()(id) for id < n, and says with ALWAYS whether the test is vacuous.
struct AdmitAll {
  static constexpr bool ALWAYS = true;
  __device__ __forceinline__ bool operator()(u32) const { return true; }
};

// One workgroup per query (blockIdx.x); its waves split the T * rpt (try, mask) runs.  Per wave, as stage1_select_kernel:
//   A) SEG: segment word of each run's bucket -> the owned ids into the wave's LDS list.  Admit::ALWAYS: prefix sum and
//      balanced copy, no test; otherwise the concatenation of the runs' segments, 64 ids at a time through adm(),
//      ballot-compacted: a row that is not admitted is never fetched.
//      !SEG (a table without the sorted-prefix layout): every slot of the run's bucket row, ballot-compacted.  With
//      Admit::ALWAYS the aliased query itself is not listed; otherwise it is listed when admitted, as in the segment
//      path, and probe_gather drops it -- nv_own differs accordingly.
//   B) the gather whenever the list fills, and at the end; the waves' survivors are merged by wave 0.
// Every valid id of a probed bucket is a candidate: no slot arithmetic (off, magic, P1) applies.  pb = 0 with
// rpt = 1 + ds gives the plain buckets of fixed mode.  tau0: the selection's initial admission threshold (key_max(), or
// the query's radius).  Outputs as stage1_select_kernel's: K1 ascending distinct keys padded with (+inf, ANN_ID_NONE),
// nv_tot = valid ids seen (with repeats, self included), nv_own = ids in the list = rows gathered.
//
// LDS carve-up, also of stage1_filter_kernel and stage1_radius_kernel (host mirror: stage1_probe_lds_bytes):
//   Key kbuf[W][cap], kout[W][K1], mbuf[W][K1];  TryInfo tries[T];  u32 *rptr[W][64];  u32 list[W][ANN_S1_CHUNK],
//   pref[W][64], qcode[T];  int mcnt[W];  u32 cnts[4];  u8 qbits[T][pb];  16-byte boundary;  generic d only: FT yq[d],
//   scratch[W][d]
template <int D, bool SEG, typename RT, typename Admit>
__device__ __forceinline__ void stage1_fixed_body(const QParams &P, const FT *y, int alias, const u32 *codes,
                                                  const unsigned char *pbits, int pb, u32 rpt, const Admit &adm, Key tau0,
                                                  int K1, int cap, FT *cand_dist, u32 *cand_id, u32 *nv_tot, u32 *nv_own) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
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
  S.kcnt = 0, S.K1 = K1, S.cap = cap, S.tau = tau0;
  FT *scratch = yq + (size_t)(1 + w) * P.d;
  u32 vtot = 0, vown = 0;
  VT a[RowChunks<D>::C];
  load_query_slice<D>(P, y, x, lane, a);

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
      if constexpr (Admit::ALWAYS) {
        for (u32 done = 0; done < total;) {  // balanced copy of `total` ids into the list, list-capacity pieces
          const u32 take = min((u32)ANN_S1_CHUNK - (u32)cnt, total - done);
          for (u32 e = done + lane; e < done + take; e += ANN_WAVE) {
            int lo_ = 0, hi_ = ANN_WAVE - 1;  // last run j with pref[j] <= e (it has c_j > 0)
            while (lo_ < hi_) {
              const int mid = (lo_ + hi_ + 1) >> 1;
              if (pref[mid] <= e) lo_ = mid; else hi_ = mid - 1;
            }
            list[cnt + (e - done)] = rptr[lo_][e - pref[lo_]];
          }
          cnt += take, done += take;
          if (cnt == ANN_S1_CHUNK) list_flush<D, RT>(P, list, cnt, vown, alias, x, a, yq, scratch, S, y);
        }
      } else {
        for (u32 e0 = 0; e0 < total; e0 += ANN_WAVE) {  // the `total` ids of these runs, 64 at a time, through the test
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
          list_push<D, RT>(id < P.n && adm(id), id, P, list, cnt, vown, alias, x, a, yq, scratch, S, y);
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
        bool own;
        if constexpr (Admit::ALWAYS) own = ok && id >= P.lo && id < P.hi;
        else own = id < P.n && id >= P.lo && id < P.hi && adm(id);
        vtot += __popcll(__ballot(ok));
        list_push<D, RT>(own, id, P, list, cnt, vown, alias, x, a, yq, scratch, S, y);
      }
    }
  }
  list_flush<D, RT>(P, list, cnt, vown, alias, x, a, yq, scratch, S, y);

  const int m = merge_waves(S, mbuf, mcnt, w, W, K1, [&] {
    atomicAdd(&cnts[0], vtot);
    atomicAdd(&cnts[1], vown);
  });
  if (w == 0) {
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

// Fixed mode with pair bits: every valid id of the probed buckets.
template <int D, bool SEG, typename RT>
__global__ __launch_bounds__(256) void stage1_probe_kernel(QParams P, const FT *__restrict__ y, int alias,
                                                           const u32 *__restrict__ codes,
                                                           const unsigned char *__restrict__ pbits, int pb, u32 rpt,
                                                           int K1, int cap, FT *__restrict__ cand_dist,
                                                           u32 *__restrict__ cand_id, u32 *__restrict__ nv_tot,
                                                           u32 *__restrict__ nv_own) {
  stage1_fixed_body<D, SEG, RT>(P, y, alias, codes, pbits, pb, rpt, AdmitAll{}, key_max(), K1, cap, cand_dist, cand_id, nv_tot,
                                nv_own);
}
