// ann_prune_kernels.h -- stage 1 on half the bytes with the native answer (annhip_index_set_prune; gfx950).
//
// The parity path's stage 1 gathers ~P1 candidate rows per query to learn its k+1 smallest keys.  With pruning the
// existing stage1_select_kernel reads the NARROW copy of the rows (h(p) = row p rounded to the narrow type) and returns
// the Kp > k+1 smallest keys on it; prune_rescore_kernel then
//   rescore      gathers those <= Kp NATIVE rows, one wave per query (rerank_kernel's lane map and ex_reduce: the bits
//                native stage 1 computes for the same pair), and ranks them by counting: the k+1 smallest exact keys;
//   certificate  decides whether they are provably what native stage 1 would have selected among ALL candidates:
//                  m < Kp            the preselection left nothing out, or
//                  LB > tau          tau = the (k+1)-th exact distance, B = the Kp-th preselect distance,
//                                    LB = (sqrt(B (1 - g)) - E)^2 (1 - g), g = 2^-16, E >= max_p ||p - h(p)||_2.
//                Every candidate left out has a float distance-on-h >= B, so a real one >= B (1 - g) (the float tree of
//                non-negative terms is within (1 + 2^-24)^(log2 d + 3) of the real sum); ||y - p|| >= ||y - h|| - E; and
//                its native float distance is >= the real one times (1 - g): it lies above tau and cannot be among the
//                k+1 smallest.  The test is written so that NaN, a non-positive root, a tiny B and +inf all fail;
//   finalize     a certified query takes finalize1's test on its exact keys (as FusedTail.enabled == 2 does in the
//                stage-1 workgroup): top_id / top_dist, or the flagged list.  An uncertified query is flagged: the exact
//                path answers it from the whole candidate row, on native rows.
// prune_rowerr_kernel computes max_p ||p - h(p)||^2 in double, once per index.
#pragma once
#include "ann_rerank_kernels.h"

#define ANN_PRUNE_WAVES 4
#define ANN_PRUNE_KMAX 64  // Kp at most: one preselected key per lane

struct PruneArgs {
  const FT *points, *y;
  const FT *pre_d;    // [Q][Kp] preselect distances on the narrow rows, ascending, +inf pads
  const u32 *pre_i;   // [Q][Kp] their ids, ANN_ID_NONE pads
  const u32 *nv_tot;  // [Q] valid slots of the candidate row (finalize1's prefix test)
  u32 *nv_own;        // [Q] in: narrow rows gathered; out: native-row equivalents of the bytes requested (statistics)
  u32 *top_id;        // [Q][k]
  FT *top_dist;
  u32 *flist, *fcount;
  unsigned long long *exact_total, *uncertified;
  FT *tie_d;          // [Q][k+1] a flagged query's exact candidate list for the tie path (ann_tie.h): certified = the
  u32 *tie_i;         // min(m, k+1) smallest exact keys ascending, (+inf, ANN_ID_NONE) pads; uncertified = empty.  Or NULL
  double E;
  u32 n, Q, L1, P1;
  int d, k, Kp;
};

// The second half for ONE query on ONE wave, wherever the caller has the preselection.  a: the query row as this lane's
// slice (ExLanes<D>: the gathers' lane map); myid: this lane's preselected id (lanes >= Kp and pads: ANN_ID_NONE); B: the
// Kp-th preselect distance (+inf where fewer were found); vtot / vown: the query's valid slots / narrow rows gathered;
// keys, sorted, ids: this wave's LDS scratch, Kp entries each.  (Called from wave 0 of the stage-1 workgroup on its
// kout it costs that kernel a wave per SIMD: profiles/prune_tail_devcode.md.)
template <int D>
__device__ __forceinline__ void prune_rescore_wave(const PruneArgs &A, u32 q, const VT (&a)[RowChunks<D>::C], u32 myid, FT B,
                                                   u32 vtot, u32 vown, Key *keys, Key *sorted, u32 *ids) {
  constexpr int C = RowChunks<D>::C;
  const int lane = lane_id();
  const int d = A.d, k = A.k, K1 = A.k + 1, Kp = A.Kp;
  // the preselected ids (distinct: stage 1 selects distinct keys and an id has one distance)
  const bool real = myid < A.n;
  const u64 rm = __ballot(real);
  const int m = __builtin_popcountll(rm);
  if (real) ids[mask_rank(rm)] = myid;
  const ExLanes<D> ln(d, lane);
  wave_lds_sync();
  const FT *__restrict__ points = A.points;
  auto load = [&](VT(&b)[C], int r0, u32 &id) {
    const int r = r0 + ln.g;
    id = ids[(ln.valid && r < m) ? r : r0];
    const FT *rp = points + (size_t)id * d;
#pragma unroll
    for (int c = 0; c < C; c++) {
      if constexpr (D > 0) b[c] = reinterpret_cast<const VT *>(rp)[ln.p + c * ln.oc];
      else b[c] = oc_load_chunk<D, false>(rp, ln.p + c * ln.oc, d);
    }
  };
  auto score = [&](const VT(&b)[C], int r0, u32 id) {
    const FT dist = ex_reduce<D>(a, b, ln.oc, ln.p, d);
    if (ln.valid && r0 + ln.g < m && ln.p == 0) keys[r0 + ln.g] = key_make(dist, id);
  };
  if (m) {
    VT b0[C], b1[C];
    u32 i0 = 0, i1 = 0;
    load(b0, 0, i0);
    for (int r0 = 0; r0 < m; r0 += 2 * ln.rpw) {
      const int r1 = r0 + ln.rpw, r2 = r1 + ln.rpw;
      if (r1 < m) load(b1, r1, i1);
      score(b0, r0, i0);
      if (r1 < m) {
        if (r2 < m) load(b0, r2, i0);
        score(b1, r1, i1);
      }
    }
  }
  wave_lds_sync();
  // the exact keys ascending, by counting (m <= 64 distinct keys, one per lane)
  const Key me = keys[lane < m ? lane : 0];
  int rank = 0;
  for (int t = 0; t < m; t++) rank += key_less(keys[t], me) ? 1 : 0;
  if (lane < m) sorted[rank] = me;
  wave_lds_sync();
  const int me_cnt = m < K1 ? m : K1;  // what native stage 1 hands to finalize1: min(k+1, distinct candidates)
  // ---- certificate
  bool cert = m < Kp;
  if (!cert && m >= K1) {
    const double Bd = (double)B;
    const double tau = (double)key_dist(sorted[K1 - 1]);
    const double g1 = 1.0 - 0x1p-16;
    const double r = sqrt(Bd * g1) - A.E;
    if (Bd >= 0x1p-100 && r > 0.0) {
      const double LB = (r * r) * g1 * (1.0 - 0x1p-40);  // the last factor: the roundings of this expression itself
      if (LB > tau) cert = true;
    }
  }
  // ---- finalize1's test on the exact keys (see finalize1_kernel)
  bool bad = me_cnt < k;
  for (int t = lane; t + 1 < me_cnt; t += ANN_WAVE)
    if (ft_bits(key_dist(sorted[t])) == ft_bits(key_dist(sorted[t + 1]))) bad = true;
  if (me_cnt >= k && !(key_dist(sorted[k - 1]) < ft_inf())) bad = true;
  if (A.L1 > A.P1 && vtot >= A.P1) bad = true;
  if (!cert || __ballot(bad) != 0) {
    if (lane == 0) {
      A.flist[atomicAdd(A.fcount, 1u)] = q;
      if (A.exact_total) atomicAdd(A.exact_total, 1ull);
      if (!cert && A.uncertified) atomicAdd(A.uncertified, 1ull);
    }
    // The flagged query's candidate list for the exact step's tie path.  Certified: sorted[0 .. me_cnt) are the smallest
    // keys of the WHOLE candidate row (every key left out lies strictly above the K1-th), i.e. the list native stage 1
    // writes for a rejected query.  Uncertified: nothing is known about the row, the list is empty.
    if (A.tie_d && lane < K1) {
      const bool have = cert && lane < me_cnt;
      A.tie_d[(size_t)q * K1 + lane] = have ? key_dist(sorted[lane]) : ft_inf();
      A.tie_i[(size_t)q * K1 + lane] = have ? key_id(sorted[lane]) : ANN_ID_NONE;
    }
  } else {
    for (int t = lane; t < k; t += ANN_WAVE) {
      A.top_id[(size_t)q * k + t] = key_id(sorted[t]);
      A.top_dist[(size_t)q * k + t] = key_dist(sorted[t]);
    }
  }
  if (lane == 0 && A.nv_own) A.nv_own[q] = (vown + 1) / 2 + (u32)m;
}

template <int D>
__global__ __launch_bounds__(64 * ANN_PRUNE_WAVES) void prune_rescore_kernel(PruneArgs A) {
  __shared__ Key s_keys[ANN_PRUNE_WAVES][ANN_PRUNE_KMAX], s_sorted[ANN_PRUNE_WAVES][ANN_PRUNE_KMAX];
  __shared__ u32 s_ids[ANN_PRUNE_WAVES][ANN_PRUNE_KMAX];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const u32 q = __builtin_amdgcn_readfirstlane(blockIdx.x * ANN_PRUNE_WAVES + w);
  if (q >= A.Q) return;  // no workgroup barrier below
  const ExLanes<D> ln(A.d, lane);
  VT a[RowChunks<D>::C];
  const FT *yq = A.y + (size_t)q * A.d;
#pragma unroll
  for (int c = 0; c < RowChunks<D>::C; c++) {
    if constexpr (D > 0) a[c] = reinterpret_cast<const VT *>(yq)[ln.p + c * ln.oc];
    else a[c] = oc_load_chunk<D, false>(yq, ln.p + c * ln.oc, A.d);
  }
  const u32 myid = lane < A.Kp ? A.pre_i[(size_t)q * A.Kp + lane] : ANN_ID_NONE;
  prune_rescore_wave<D>(A, q, a, myid, A.pre_d[(size_t)q * A.Kp + A.Kp - 1], A.nv_tot[q], A.nv_own ? A.nv_own[q] : 0u, s_keys[w],
                        s_sorted[w], s_ids[w]);
}

// out[0] = max over the rows of ||p - h(p)||^2 as the bits of a non-negative double (they order like the values);
// out[1] != 0: some row has a non-finite difference (NaN, or a value the narrow type turns into +-inf).  One wave per
// row at a time; out is zeroed by the caller.
__global__ __launch_bounds__(256) void prune_rowerr_kernel(size_t rows, int d, const FT *__restrict__ points,
                                                           const RN *__restrict__ narrow, unsigned long long *out) {
  const int lane = lane_id();
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((size_t)gridDim.x * blockDim.x) >> 6;
  double worst = 0;
  bool broken = false;
  for (size_t r = wave; r < rows; r += waves) {
    double acc = 0;
    for (int z = lane; z < d; z += ANN_WAVE) {
      const double df = (double)points[r * d + z] - (double)narrow[r * d + z];
      acc += df * df;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
    if (!(acc < __builtin_inf())) broken = true;  // NaN or +inf
    else if (acc > worst) worst = acc;
  }
  if (lane == 0) {
    atomicMax(out, (unsigned long long)__builtin_bit_cast(unsigned long long, worst));
    if (broken) atomicAdd(out + 1, 1ull);
  }
}
