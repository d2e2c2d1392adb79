// ann_group_kernels.h -- grouped queries by collapse (annhip_collapse, annhip_query_grouped,
// annhip_index_exact_query_grouped; gfx950).
//
// The group key of row i is tags[i] & gmask.  Collapse walks a row of L entries (id, dist) in the order given and keeps a
// non-pad entry iff fewer than g earlier non-pad entries of the row have its key; the first k kept entries are the output,
// padded with (pad_id, +inf).  An entry with id >= rows is a pad: skipped, never dereferenced, the test made on all 64
// bits before the id is narrowed.  Distances are copied bit for bit and never compared.
//
//   group_collapse_kernel   one wave per row, several rows per workgroup, no workgroup barrier.  Per wave:
//     stage     the row's L <= 1024 entries 64 at a time, entry j on lane j % 64 (coalesced); the non-pad ones go to LDS in
//               order (ballot compaction) as (id narrowed to 32 bits, key gathered from tags, distance).  Every load of the
//               row has returned before anything is written: ids_out / dists_out may be the input where k == L.
//     keep      the staged entries 64 at a time: entry j counts the equal keys in front of it -- whole chunks as broadcast
//               16-byte LDS reads, its own chunk lane by lane -- and is kept iff that count is below g.  A ballot and a
//               running base give the kept entries their places in order.  The scan stops once k are kept.
//     finish    pads behind the kept entries, counts[q], short[q] = fewer than k kept although the row held no pad.
// O(L^2 / 64) compares per lane at worst and a few where the first entries already hold k groups.
// LDS of one workgroup: per wave Lr = L rounded up to 64 entries of (FT dist, u32 key, u32 id), the arrays of all waves one
// after the other (group_lds_bytes).  No call but the three grouped entry points launches anything from this file.
#pragma once
#include "ann_device.h"

#define ANN_GROUP_WAVES 4  // rows per workgroup
__host__ __device__ inline size_t group_row_entries(size_t L) { return (L + ANN_WAVE - 1) / ANN_WAVE * ANN_WAVE; }
__host__ __device__ inline size_t group_lds_bytes(size_t L) {
  return (size_t)ANN_GROUP_WAVES * group_row_entries(L) * (sizeof(FT) + 2 * sizeof(u32));
}

// ids_in / ids_out and dists_in / dists_out may alias each other (k == L): no __restrict__ on them.
__global__ __launch_bounds__(64 * ANN_GROUP_WAVES) void group_collapse_kernel(size_t Q, int L, int k, u32 g, u32 gmask,
                                                                              const u32 *__restrict__ tags, u64 rows, size_t pad_id,
                                                                              const size_t *ids_in, const FT *dists_in,
                                                                              size_t *ids_out, FT *dists_out,
                                                                              u32 *__restrict__ counts,
                                                                              unsigned char *__restrict__ shrt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const size_t q = (size_t)blockIdx.x * ANN_GROUP_WAVES + w;
  if (q >= Q) return;  // wave-uniform; no workgroup barrier below
  const size_t Lr = group_row_entries((size_t)L);
  FT *sd = reinterpret_cast<FT *>(smem) + (size_t)w * Lr;
  u32 *sk = reinterpret_cast<u32 *>(smem + (size_t)ANN_GROUP_WAVES * Lr * sizeof(FT)) + (size_t)w * Lr;
  u32 *si = reinterpret_cast<u32 *>(smem + (size_t)ANN_GROUP_WAVES * Lr * (sizeof(FT) + sizeof(u32))) + (size_t)w * Lr;

  // ---- stage: the non-pad entries, in order
  const size_t *ri = ids_in + q * (size_t)L;
  const FT *rd = dists_in + q * (size_t)L;
  int nv = 0;
  for (int e0 = 0; e0 < L; e0 += ANN_WAVE) {
    const int e = e0 + lane;
    const u64 id = e < L ? (u64)ri[e] : rows;
    const bool ok = id < rows;  // all 64 bits: 2^32 + 5 is not row 5
    const u64 mm = __ballot(ok);
    if (ok) {
      const int at = nv + (int)mask_rank(mm);
      si[at] = (u32)id;
      sk[at] = tags[id] & gmask;
      sd[at] = rd[e];
    }
    nv += __popcll(mm);
  }
  wave_lds_sync();

  // ---- keep: entry j iff fewer than g equal keys among the entries in front of it
  size_t *oi = ids_out + q * (size_t)k;
  FT *od = dists_out + q * (size_t)k;
  int base = 0;
  for (int e0 = 0; e0 < nv && base < k; e0 += ANN_WAVE) {
    const int e = e0 + lane;
    const bool live = e < nv;
    const u32 me = sk[live ? e : e0];
    u32 cnt = 0;
    for (int f = 0; f < e0; f += 4) {  // (e0 is a multiple of 64 and sk 16-byte aligned)
      const uint4 v = *reinterpret_cast<const uint4 *>(sk + f);
      cnt += (u32)(v.x == me) + (u32)(v.y == me) + (u32)(v.z == me) + (u32)(v.w == me);
    }
    const int nb = min(ANN_WAVE, nv - e0);  // the chunk's own entries: those on lower lanes
    for (int t = 0; t < nb; t += 4) {       // (up to 3 words behind entry nv - 1, inside Lr: only lanes > t + 3 >= nb read them, none live)
      const uint4 v = *reinterpret_cast<const uint4 *>(sk + e0 + t);
      cnt += (u32)(t < lane && v.x == me) + (u32)(t + 1 < lane && v.y == me) + (u32)(t + 2 < lane && v.z == me) +
             (u32)(t + 3 < lane && v.w == me);
    }
    const bool keep = live && cnt < g;
    const u64 mm = __ballot(keep);
    const int at = base + (int)mask_rank(mm);
    if (keep && at < k) {
      oi[at] = (size_t)si[e];
      od[at] = sd[e];
    }
    base += __popcll(mm);
  }

  // ---- finish
  const int kept = min(base, k);
  const FT inf = ft_inf();
  for (int t = kept + lane; t < k; t += ANN_WAVE) oi[t] = pad_id, od[t] = inf;
  if (lane == 0) {
    if (counts) counts[q] = (u32)kept;
    if (shrt) shrt[q] = (unsigned char)(kept < k && nv == L);
  }
}
