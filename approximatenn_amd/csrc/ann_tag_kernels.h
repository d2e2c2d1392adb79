// ann_tag_kernels.h -- per-query tag predicates of the fixed query mode (annhip_index_set_tags, annhip_query_tagged;
// gfx950).  The exact scan applies the same predicate in its EX_TAGS form (ann_exact_kernels.h).
//
// Rows carry a 32-bit tag word, every query a (mask, value) pair: row i competes for query q iff
// (tags[i] & qmask[q]) == qvalue[q].  The range form (annhip_query_between) gives every query a (mask, lo, hi) triple:
// qlo[q] <= (tags[i] & qmask[q]) <= qhi[q], unsigned.  It is the same kernels: they take (qmask, qlo, qhi), hold the
// predicate as a TagPred (ann_device.h) and the pair form passes its qvalue array for both bounds.
// Like the allow list (ann_filter_kernels.h, the model of every kernel here) the predicate only narrows what fixed mode
// calls a valid id, and it is tested where an id ENTERS the wave's LDS list: a row that does not match costs its 4-byte
// id and its 4-byte tag, never a row.
//
//   AdmitTags        the predicate of one query as an admission policy
//   stage1_tag / stage2_tag   stage1_fixed_body (ann_probe_kernels.h) / stage2_fixed_body (ann_filter_kernels.h) with it
//
// `bits`, the index's allow list, may be NULL: both tests apply when it is set.  NULL or not is a kernel argument, hence one
// wave-uniform branch and no second template axis.  tags, bits, qmask, qlo and qhi are separate kernel arguments, and no
// untagged call launches anything from this file.
#pragma once
#include "ann_filter_kernels.h"

// id < n (the caller's test).  The two loads are independent of each other where both tests apply.
__device__ __forceinline__ bool tag_allows(const u32 *__restrict__ tags, const u32 *__restrict__ bits, const TagPred &p, u32 id) {
  if (bits) {
    const u32 t = tags[id], wd = bits[id >> 5];
    return tag_match(t, p) && ((wd >> (id & 31u)) & 1u);
  }
  return tag_match(tags[id], p);
}

// the admission policy of query x's predicate (see stage1_fixed_body): qmask[x] / qlo[x] / qhi[x] are read once per
// workgroup and are wave-uniform
struct AdmitTags {
  static constexpr bool ALWAYS = false;
  const u32 *__restrict__ tags, *__restrict__ bits;
  TagPred p;
  __device__ __forceinline__ AdmitTags(const u32 *tags, const u32 *bits, const u32 *qmask, const u32 *qlo, const u32 *qhi, u32 x)
      : tags(tags), bits(bits), p(tag_pred(qmask, qlo, qhi, x)) {}
  __device__ __forceinline__ bool operator()(u32 id) const { return tag_allows(tags, bits, p, id); }
};

// ------------------------------------------------------------------------------------------ stage 1
// stage1_fixed_body with the predicate of query x: nv_own = matching valid ids (self included when it matches).
template <int D, bool SEG, typename RT>
__global__ __launch_bounds__(256) void stage1_tag_kernel(QParams P, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ codes,
                                                            const unsigned char *__restrict__ pbits, int pb, u32 rpt,
                                                            const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                         const u32 *__restrict__ qmask, const u32 *__restrict__ qlo, const u32 *__restrict__ qhi, int K1, int cap,
                                                            FT *__restrict__ cand_dist, u32 *__restrict__ cand_id,
                                                            u32 *__restrict__ nv_tot, u32 *__restrict__ nv_own) {
  stage1_fixed_body<D, SEG, RT>(P, y, alias, codes, pbits, pb, rpt, AdmitTags(tags, bits, qmask, qlo, qhi, blockIdx.x), key_max(),
                                K1, cap, cand_dist, cand_id, nv_tot, nv_own);
}

// ------------------------------------------------------------------------------------------ stage 2
// stage2_fixed_body over the stage-1 results and those of their graph neighbours that pass query x's test.
template <int D, typename IdOut, typename RT>
__global__ __launch_bounds__(256) void stage2_tag_kernel(QParams P, int Q, const FT *__restrict__ y, int alias,
                                                            const u32 *__restrict__ top_id, const FT *__restrict__ top_dist,
                                                            const u32 *__restrict__ tags, const u32 *__restrict__ bits,
                                                         const u32 *__restrict__ qmask, const u32 *__restrict__ qlo, const u32 *__restrict__ qhi, u32 P2, int K1, int cap,
                                                            IdOut *__restrict__ out_ids, FT *__restrict__ out_dist,
                                                            u32 *__restrict__ flist, u32 *__restrict__ fcount,
                                                            unsigned long long *__restrict__ exact_total,
                                                            unsigned long long *__restrict__ rows_done, u32 xbase) {
  stage2_fixed_body<D, IdOut, RT>(P, y, alias, top_id, top_dist, AdmitTags(tags, bits, qmask, qlo, qhi, xbase + blockIdx.x), P2, K1,
                                  cap, out_ids, out_dist, flist, fcount, exact_total, rows_done, xbase);
}
