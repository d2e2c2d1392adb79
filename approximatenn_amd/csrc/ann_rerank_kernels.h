// ann_rerank_kernels.h -- exact top-k of caller-supplied candidates on native rows (annhip_rerank; gfx950).
//
// tail_hash_merge_kernel (ann_tail_hash_kernels.h) with the bucket enumeration replaced by the caller's id list: one wave
// per query, the query in registers in the ExLanes<D> map, one ExSel buffer per wave, no workgroup barrier.  Per wave:
//   rerank_stage   the query's ccnt 64-bit entries -> 32-bit ids in LDS.  An entry >= rows (pads, -1, 2^32 + 5 ...) is
//                  dropped by the 64-bit compare before it is narrowed (ballot compaction, order kept); then an id equal
//                  to an earlier entry is dropped: ExSel / ex_compact rank keys by counting and need them distinct;
//   score          the survivors rpw rows per pass, the next pass's row loads in flight while this one is reduced.  A lane
//                  group reads row id from points (id < n) or from the tail (id - n); ex_reduce / the literal tree give
//                  the query path's distance bits;
//   tail_store     the k best ascending, pad (rows, +inf) -- after the whole list has been staged, so ids_dev may be
//                  cand_dev where ccnt == k: a wave reads the row of its own query before it writes it, and no other wave
//                  touches that row.
// Nothing is tested but id < rows: no allow list, no tags, no alias rule.  Each row is read once per (query, candidate):
// there is no reuse to stage, the loads go from HBM / L2 straight to registers.
// LDS of one workgroup: per wave one selection buffer (cap + k keys; the any-d form's query and tree scratch in front of
// it), then per wave the id list (ccnt words rounded up to 4).
#pragma once
#include "ann_tail_hash_kernels.h"

struct RerankArgs {
  TailArgs t;          // tail, y, out rows, n, m (pad = n + m), Q, d, k, cap; the rest unused
  const FT *points;    // rows [0, n)
  const size_t *cand;  // [Q][ccnt]; may be t.out_ids where ccnt == k
  int ccnt;
};
__host__ __device__ inline size_t rerank_wave_words(size_t ccnt) { return (ccnt + 3) & ~(size_t)3; }
// rerank_stage reads the id list 16 bytes at a time.  A wave's list starts 16-byte aligned because the lists are whole
// multiples of 4 words and the waves' key buffers in front of them hold 2 k + ANN_EX_SLACK keys of 8 or 16 bytes each.
static_assert(ANN_EX_SLACK % 2 == 0 && sizeof(Key) % 8 == 0, "the id lists behind the key buffers must stay 16-byte aligned");

// cand[q][0..ccnt) -> ids[0..return): the distinct entries below rows, in the order of their first occurrence
__device__ __forceinline__ int rerank_stage(const RerankArgs &A, u32 *ids, u32 q) {
  const int lane = lane_id();
  const size_t *src = A.cand + (size_t)q * A.ccnt;
  const u64 rows = (u64)A.t.n + A.t.m;
  int cnt = 0;
  for (int e0 = 0; e0 < A.ccnt; e0 += ANN_WAVE) {
    const int e = e0 + lane;
    const u64 id = e < A.ccnt ? (u64)src[e] : rows;
    const bool ok = id < rows;  // all 64 bits: 2^32 + 5 is not row 5
    const u64 mm = __ballot(ok);
    if (ok) ids[cnt + mask_rank(mm)] = (u32)id;
    cnt += __builtin_popcountll(mm);
  }
  wave_lds_sync();
  // ids[0..ns) are distinct; entry e of the block at e0 >= ns is tested against them and against the block's entries before it
  int ns = 0;
  for (int e0 = 0; e0 < cnt; e0 += ANN_WAVE) {
    const int e = e0 + lane;
    const bool live = e < cnt;
    const u32 me = ids[live ? e : e0];
    bool dup = false;
    int f = 0;
    for (; f + 4 <= ns; f += 4) {  // (ids and the offset are 16-byte aligned)
      const uint4 v = *reinterpret_cast<const uint4 *>(ids + f);
      dup |= v.x == me || v.y == me || v.z == me || v.w == me;
    }
    for (; f < ns; f++) dup |= ids[f] == me;
    const int nb = min(ANN_WAVE, cnt - e0);
    for (int g = 0; g < nb; g++) dup |= g < lane && ids[e0 + g] == me;
    const bool keep = live && !dup;
    const u64 mm = __ballot(keep);
    wave_lds_sync();  // the block has been read; ns + rank <= e
    if (keep) ids[ns + mask_rank(mm)] = me;
    ns += __builtin_popcountll(mm);
    wave_lds_sync();
  }
  return ns;
}

template <int D>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void rerank_kernel(RerankArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.t.d;
  const size_t wave_keys = (size_t)A.t.cap + A.t.k;
  Key *kbase = reinterpret_cast<Key *>(smem) + (size_t)w * wave_keys;
  u32 *ids = reinterpret_cast<u32 *>(smem + (size_t)W * wave_keys * sizeof(Key)) + (size_t)w * rerank_wave_words(A.ccnt);
  const u32 q = __builtin_amdgcn_readfirstlane(blockIdx.x * W + w);
  if (q >= A.t.Q) return;  // no workgroup barrier below
  ExSel S;
  S.init(kbase, kbase + A.t.cap, A.t.cap, A.t.k, q, A.t.Q);
  const ExLanes<D> ln(d, lane);
  VT a[C];
  const FT *yq = A.t.y + (size_t)q * d;
#pragma unroll
  for (int c = 0; c < C; c++) {
    if constexpr (D > 0) a[c] = reinterpret_cast<const VT *>(yq)[ln.p + c * ln.oc];
    else a[c] = oc_load_chunk<D, false>(yq, ln.p + c * ln.oc, d);
  }
  const int ns = rerank_stage(A, ids, q);
  const FT *__restrict__ points = A.points, *__restrict__ tail = A.t.tail;
  const u32 n = A.t.n;
  // survivors ids[0..ns): rpw rows per pass, the next pass's loads in flight while this one is reduced
  auto load = [&](VT(&b)[C], int r0, u32 &id) {
    const int r = r0 + ln.g;
    id = ids[(ln.valid && r < ns) ? r : r0];
    const FT *rp = id < n ? points + (size_t)id * d : tail + (size_t)(id - n) * d;
#pragma unroll
    for (int c = 0; c < C; c++) {
      if constexpr (D > 0) b[c] = reinterpret_cast<const VT *>(rp)[ln.p + c * ln.oc];
      else b[c] = oc_load_chunk<D, false>(rp, ln.p + c * ln.oc, d);
    }
  };
  auto offer = [&](const VT(&b)[C], int r0, u32 id) {
    const bool head = ln.valid && r0 + ln.g < ns && ln.p == 0;
    const Key key = key_make(ex_reduce<D>(a, b, ln.oc, ln.p, d), id);
    S.offer<0>(head && key_less(key, S.tau[0]), key);
  };
  if (ns) {
    VT b0[C], b1[C];
    u32 i0 = 0, i1 = 0;
    load(b0, 0, i0);
    for (int r0 = 0; r0 < ns; r0 += 2 * ln.rpw) {
      const int r1 = r0 + ln.rpw, r2 = r1 + ln.rpw;
      if (r1 < ns) load(b1, r1, i1);
      offer(b0, r0, i0);
      if (r1 < ns) {
        if (r2 < ns) load(b0, r2, i0);
        offer(b1, r1, i1);
      }
    }
  }
  tail_store<0>(S, A.t, q, true);
}

// Any d without a register layout: tail_hash_merge_generic_kernel's literal in-place tree, its rows read from points or
// the tail through the id list.  Per wave: yq[d], m[NP][d] in front of the selection buffer.
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void rerank_generic_kernel(RerankArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.t.d;
  int NP = ANN_EX_GEN_ELEMS / d;
  NP = NP < 1 ? 1 : (NP > ANN_WAVE ? ANN_WAVE : NP);
  const size_t wave_ft = ((size_t)(1 + NP) * d * sizeof(FT) + 15) & ~(size_t)15;  // yq[d], m[NP][d]
  const size_t wave_bytes = wave_ft + sizeof(Key) * ((size_t)A.t.cap + A.t.k);
  unsigned char *wb = smem + (size_t)w * wave_bytes;
  FT *yq = reinterpret_cast<FT *>(wb), *m = yq + d;
  Key *kbase = reinterpret_cast<Key *>(wb + wave_ft);
  u32 *ids = reinterpret_cast<u32 *>(smem + (size_t)W * wave_bytes) + (size_t)w * rerank_wave_words(A.ccnt);
  const u32 q = __builtin_amdgcn_readfirstlane(blockIdx.x * W + w);
  if (q >= A.t.Q) return;  // no workgroup barrier below
  ExSel S;
  S.init(kbase, kbase + A.t.cap, A.t.cap, A.t.k, q, A.t.Q);
  for (int z = lane; z < d; z += ANN_WAVE) yq[z] = A.t.y[(size_t)q * d + z];
  const int ns = rerank_stage(A, ids, q);  // (ends with a fence: yq is in LDS)
  int sh0 = 0;  // d <= 1 << sh0
  while ((1 << sh0) < d) sh0++;
  const FT zero = 0;
  const FT *__restrict__ points = A.points, *__restrict__ tail = A.t.tail;
  const u32 n = A.t.n;
  wave_lds_sync();
  for (int r0 = 0; r0 < ns; r0 += NP) {
    const int np = min(NP, ns - r0);
    for (int it = lane; it < (np << sh0); it += ANN_WAVE) {
      const int pr = it >> sh0, z = it & ((1 << sh0) - 1);
      if (z < d) {
        const u32 id = ids[r0 + pr];
        const FT *rp = id < n ? points + (size_t)id * d : tail + (size_t)(id - n) * d;
        const FT df = yq[z] - rp[z];
        m[pr * d + z] = df * df;
      }
    }
    wave_lds_sync();
    int sh = sh0;
    for (int s = d; s >> 1; s >>= 1) {
      const int h = s >> 1;
      while (sh > 0 && (1 << (sh - 1)) >= h) sh--;  // h <= 1 << sh
      for (int it = lane; it < (np << sh); it += ANN_WAVE) {
        const int pr = it >> sh, z = it & ((1 << sh) - 1);
        if (z < h) {
          FT *mp = m + pr * d;
          const FT g = ((s & 1) && z == 0) ? mp[s - 1] : zero;
          mp[z] = mp[z] + (mp[z + h] + g);
        }
      }
      wave_lds_sync();
    }
    const bool act = lane < np;
    const Key key = key_make(act ? m[lane * d] : zero, ids[act ? r0 + lane : r0]);
    wave_lds_sync();  // m is rewritten by the next batch
    S.offer<0>(act && key_less(key, S.tau[0]), key);
  }
  tail_store<0>(S, A.t, q, true);
}
