// ann_kq_kernels.h -- stage 2 of a fixed-mode query whose k is chosen per call (annhip_query_k; gfx950).
//
// kg = the index's k (QParams::k): the width of a graph row.  kq = the k of this call: the number of stage-1 results
// (top[0..kq)) and the length of an output row.  stage2_select_kernel and its filter / tag variants use one k for all
// three; this kernel is stage2_filter_kernel with the widths apart and the validity tests of all three families behind
// two nullable pointers each:
//
//   row of query x   kq + kq * kg slots: slot j < kq is stage-1 result j with the distance it already has, slot
//                    kq + p * kg + z is graph[top[p]][z], z < kg.  A pad among the stage-1 results, (n, +inf), has no
//                    neighbours: it contributes nothing.
//   ok               id < n, not x itself when aliased, bit id of `bits` when bits != NULL, qlo[x] <= (tags[id] &
//                    qmask[x]) <= qhi[x] when tags != NULL (the pair form passes qvalue twice).  Tested where an id
//                    ENTERS the wave's LDS list: a rejected row is never fetched.  NULL or not is wave-uniform: one branch each, no template axis.
//   output           the kq smallest distinct (distance, id) keys, ascending, (n, +inf) where fewer exist.
//
// The waves split the row in runs of 64 slots.  A lane needs (p, z) of its slot in every pass; dividing by the run-time
// kg there would cost a division per lane and pass.  Instead every lane divides ONCE, for its first slot, and then walks:
// one pass further is 64 slots further, i.e. z += 64 % kg, p += 64 / kg and one carry.  g = j - kq is signed and (p, z)
// is its FLOORED quotient and remainder, so the lanes that start among the stage-1 results (g < 0, p < 0) walk into the
// graph part by the same rule; exact for every kg >= 1 and every slot index below 2^31 (the host refuses longer rows).
//
// The slot walk and the kq-wide output are this kernel's own; the query-row load, the list and the merge are the pieces
// it shares with the fixed-mode bodies (ann_probe_kernels.h), probe_gather included: the arithmetic of gather_select
// without the private segment that FoldPlan's constructor costs the folded layouts.  No call but annhip_query_k and the
// radius entry points launches anything from this file.
#pragma once
#include "ann_tag_kernels.h"

// LDS carve-up (host mirror: stage2_kq_lds_bytes, which annhip_index_max_query_k evaluates):
//   Key kbuf[W][cap], kout[W][K1], mbuf[W][K1], top[kq];  u32 list[W][ANN_S1_CHUNK];  int mcnt[W];  u32 cnts[4];
//   16-byte boundary;  generic d only: FT yq[d], scratch[W][d]
template <int D, typename IdOut, typename RT>
__global__ __launch_bounds__(256) void stage2_kq_kernel(QParams P, const FT *__restrict__ y, int alias,
                                                        const u32 *__restrict__ top_id, const FT *__restrict__ top_dist, int kq,
                                                        const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                        const u32 *__restrict__ qmask, const u32 *__restrict__ qlo, const u32 *__restrict__ qhi, int K1,
                                                        int cap, IdOut *__restrict__ out_ids, FT *__restrict__ out_dist,
                                                        unsigned long long *__restrict__ rows_done) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const u32 x = blockIdx.x;
  const int kg = P.k;
  TagPred tp{0, 0, 0};  // wave-uniform: this query's predicate, read once
  if (tags) tp = tag_pred(qmask, qlo, qhi, x);
  unsigned char *sp = smem;
  Key *kbuf_all = reinterpret_cast<Key *>(sp);   sp += sizeof(Key) * (size_t)W * cap;
  Key *kout_all = reinterpret_cast<Key *>(sp);   sp += sizeof(Key) * (size_t)W * K1;
  Key *mbuf = reinterpret_cast<Key *>(sp);       sp += sizeof(Key) * (size_t)W * K1;
  Key *top = reinterpret_cast<Key *>(sp);        sp += sizeof(Key) * (size_t)kq;
  u32 *list_all = reinterpret_cast<u32 *>(sp);   sp += sizeof(u32) * (size_t)W * ANN_S1_CHUNK;
  int *mcnt = reinterpret_cast<int *>(sp);       sp += sizeof(int) * (size_t)W;
  u32 *cnts = reinterpret_cast<u32 *>(sp);       sp += sizeof(u32) * 4;  // [1] rows gathered
  sp = smem + (((sp - smem) + 15) & ~(size_t)15);
  FT *yq = reinterpret_cast<FT *>(sp);  // generic d only: [d] + W*[d]
  u32 *list = list_all + (size_t)w * ANN_S1_CHUNK;

  for (int t = threadIdx.x; t < kq; t += blockDim.x) top[t] = key_make(top_dist[(size_t)x * kq + t], top_id[(size_t)x * kq + t]);
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
  u32 vown = 0;
  int cnt = 0;
  const u32 L2q = (u32)kq + (u32)kq * (u32)kg;
  const u32 per = (((L2q + W - 1) / W) + 63u) & ~63u;  // this wave's slice of the row [0, L2q)
  const u32 s0 = min(L2q, (u32)w * per), s1 = min(L2q, s0 + per);
  // (p, z) of this lane's first slot: floored quotient and remainder of g = j - kq by kg -- the one division of the lane
  const int q64 = ANN_WAVE / kg, r64 = ANN_WAVE - q64 * kg;  // wave-uniform
  int p, z;
  {
    const int g = (int)(s0 + (u32)lane) - kq;
    p = g >= 0 ? g / kg : -((kg - 1 - g) / kg);
    z = g - p * kg;
  }
  for (u32 base = s0; base < s1; base += ANN_WAVE) {
    const u32 j = base + lane;
    bool direct = false, ok = false;
    Key dk = key_max();
    u32 id = ANN_ID_NONE;
    if (j < s1) {
      if (p < 0) {  // j < kq: the stage-1 result itself, with the distance it already has
        dk = top[j];
        direct = key_dist(dk) < ft_inf();
      } else {
        const u32 parent = key_id(top[p]);
        if (parent < P.n) {  // (a pad has no neighbours)
          id = P.graph[(size_t)parent * kg + z];
          ok = id < P.n && !(alias && id == x);
          if (ok && bits) ok = filter_allows(bits, id);
          if (ok && tags) ok = tag_match(tags[id], tp);
        }
      }
    }
    if (base < (u32)kq) {  // wave-uniform: only these passes hold direct keys
      if (S.kcnt + ANN_WAVE > S.cap) sel_shrink(S);
      const bool push = direct && key_less(dk, S.tau);
      const u64 dm = __ballot(push);
      if (push) S.kbuf[S.kcnt + mask_rank(dm)] = dk;
      S.kcnt += __popcll(dm);
    }
    list_push<D, RT>(ok, id, P, list, cnt, vown, alias, x, a, yq, scratch, S, y);
    z += r64, p += q64;  // 64 slots further
    if (z >= kg) z -= kg, p++;
  }
  list_flush<D, RT>(P, list, cnt, vown, alias, x, a, yq, scratch, S, y);

  const int m = merge_waves(S, mbuf, mcnt, w, W, K1, [&] { atomicAdd(&cnts[1], vown); });
  if (w == 0) {
    for (int t = lane; t < kq; t += ANN_WAVE) {  // the kq smallest distinct keys in (distance, id) order, (n, +inf) where fewer exist
      out_ids[(size_t)x * kq + t] = t < m ? (IdOut)key_id(S.kout[t]) : (IdOut)P.n;
      out_dist[(size_t)x * kq + t] = t < m ? key_dist(S.kout[t]) : ft_inf();
    }
    if (rows_done && lane == 0) atomicAdd(&rows_done[(x & 63u) * 8u], (unsigned long long)cnts[1]);
  }
}
