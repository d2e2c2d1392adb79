// ann_tail_hash_kernels.h -- appended rows looked up by hash code (annhip_index_hash_tail; gfx950).
//
// annhip_index_hash_tail gives every tail row the T hash codes a fixed-mode query equal to it would get (the hash
// kernels themselves, launched over the tail) and files the rows, per try, into a CSR over the 2^ds buckets.  A query then
// fetches only the tail rows of the buckets it probes anyway: per try its own bucket, the ds buckets at Hamming distance
// 1 and the pair buckets of its ranked bits (ann_probe_kernels.h, probe_mask).
//
//   thash_count / thash_scan / thash_place   the CSR: count per (try, bucket), inclusive scan per try, place by counting
//                                            the bucket's end down to its start (the order inside a bucket is arbitrary:
//                                            the answer is a function of the candidate SET)
//   tail_hash_merge_kernel<D, V>             one wave per query: seed from R(q) (tail_seed), enumerate the (try, mask)
//                                            runs, flatten their CSR ranges into an LDS chunk, reject, gather, score,
//                                            store (tail_store)
//   tail_hash_merge_generic_kernel           the same around the literal in-place LDS tree (any d)
//
// Reject, before a row is fetched, one lane per candidate:
//   first-try rule  a row found in try t is dropped when it also hits in a try t' < t (thash_hits on its stored codes:
//                   4 T bytes against a whole row).  Buckets of one try are disjoint, so with this rule every row reaches
//                   the selection at most once: ExSel / ex_compact rank keys by counting and need them distinct;
//   validity        the allow-list bit and the tag word of id n + j.
// The distances come out of ex_reduce / the literal tree against the query in registers / LDS: the query path's bits.
#pragma once
#include "ann_probe_kernels.h"
#include "ann_tail_kernels.h"

#define ANN_THASH_CHUNK 256  // candidate rows one wave stages in LDS at a time

struct TailHashArgs {
  TailArgs t;              // tail, y, in/out rows, validity words, scored, n, m (ALL tail rows: the pad is n + m), Q, d, k, kin, cap
  const u32 *codes;        // [Q][T] the batch's hash codes
  const unsigned char *pbits;  // [Q][T][pb] ranked projection indices, or NULL (pb == 0)
  const u32 *tcodes;       // [mh][T] the hashed tail rows' codes
  const u32 *off;          // [T][nb + 1] bucket b of try t = rows[off[t][b] .. off[t][b + 1]); offsets include t * mh
  const u32 *rows;         // [T][mh] tail row numbers j
  u32 mh;
  int T, ds, pb;
};

// membership of x = cq ^ c in the probe contract's mask set; pm = OR of the ranked bits
__device__ __forceinline__ bool thash_hits(u32 x, u32 pm) {
  const int pc = __builtin_popcount(x);
  return pc <= 1 || (pc == 2 && (x & ~pm) == 0);
}

// ------------------------------------------------------------------------------------------ the CSR
__global__ void thash_count_kernel(size_t items, const u32 *__restrict__ tcodes, int T, u32 stride, u32 *__restrict__ off) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x)
    atomicAdd(&off[(size_t)(i % T) * stride + min(tcodes[i], stride - 2)], 1u);
}
// one workgroup per try: off[t][b] := t * mh + the rows of try t in buckets 0 .. b (the bucket's END)
__global__ __launch_bounds__(1024) void thash_scan_kernel(u32 *__restrict__ off, u32 stride, u32 mh) {
  __shared__ u32 wsum[16];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  u32 *a = off + (size_t)blockIdx.x * stride;
  u32 carry = blockIdx.x * mh;
  for (u32 base = 0; base < stride; base += blockDim.x) {
    const u32 i = base + threadIdx.x;
    const u32 v = i < stride ? a[i] : 0;
    const u32 incl = wave_incl_scan(v);
    if (lane == ANN_WAVE - 1) wsum[w] = incl;
    __syncthreads();
    u32 before = 0, total = 0;
    for (int ww = 0; ww < (int)(blockDim.x >> 6); ww++) {
      const u32 s = wsum[ww];
      before += ww < w ? s : 0;
      total += s;
    }
    if (i < stride) a[i] = carry + before + incl;
    carry += total;
    __syncthreads();
  }
}
// every bucket's end counts down to its start while its rows are placed
__global__ void thash_place_kernel(size_t items, const u32 *__restrict__ tcodes, int T, u32 stride, u32 *__restrict__ off,
                                   u32 *__restrict__ rows) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
    const u32 at = atomicSub(&off[(size_t)(i % T) * stride + min(tcodes[i], stride - 2)], 1u) - 1u;
    rows[at] = (u32)(i / T);
  }
}

// ------------------------------------------------------------------------------------------ the query side
// Per-wave LDS behind the selection buffers: the query's codes and pair masks, the runs of one enumeration pass, the chunk.
struct ThashWave {
  u32 *qc, *pm;            // [T]
  u32 *pref, *rst, *rtry;  // [64] per run of the pass: exclusive prefix of its length, its first index in rows, its try
  u32 *cj, *ct;            // [ANN_THASH_CHUNK] candidate tail row, the try that found it
};
__host__ __device__ inline size_t thash_wave_words(int T) { return 2 * (size_t)T + 3 * ANN_WAVE + 2 * ANN_THASH_CHUNK; }
__device__ __forceinline__ ThashWave thash_carve(u32 *p, int T) {
  ThashWave L;
  L.qc = p, L.pm = p + T, L.pref = p + 2 * T, L.rst = L.pref + ANN_WAVE, L.rtry = L.rst + ANN_WAVE;
  L.cj = L.rtry + ANN_WAVE, L.ct = L.cj + ANN_THASH_CHUNK;
  return L;
}

// the query's codes and the OR of its ranked bits per try -> LDS
__device__ __forceinline__ void thash_load_query(const TailHashArgs &A, const ThashWave &L, u32 q) {
  for (int t = lane_id(); t < A.T; t += ANN_WAVE) {
    L.qc[t] = A.codes[(size_t)q * A.T + t];
    u32 pm = 0;
    for (int u = 0; u < A.pb; u++) pm |= 1u << ((A.ds - 1 - A.pbits[((size_t)q * A.T + t) * A.pb + u]) & 31);
    L.pm[t] = pm & ((1u << A.ds) - 1u);
  }
  wave_lds_sync();
}

// cj[0..cnt) / ct: candidates as found -> cj[0..return): those that hit in no earlier try and are valid for the query
template <int V>
__device__ __forceinline__ int thash_reject(const TailHashArgs &A, const ThashWave &L, int cnt, const u32 *__restrict__ bits,
                                            const u32 *__restrict__ tags, const TagPred &tp) {
  const int lane = lane_id();
  int ns = 0;
  for (int e0 = 0; e0 < cnt; e0 += ANN_WAVE) {
    const int e = e0 + lane;
    bool ok = e < cnt;
    const u32 j = L.cj[ok ? e : e0], t = L.ct[ok ? e : e0];
    const u32 *cj = A.tcodes + (size_t)j * A.T;
    for (u32 t2 = 0; ok && t2 < t; t2++) ok = !thash_hits(L.qc[t2] ^ cj[t2], L.pm[t2]);
    if constexpr (V != EX_ALL) {
      const u32 id = A.t.n + j;
      if (ok && bits) ok = (bits[id >> 5] >> (id & 31)) & 1u;
      if (V == EX_TAGS && ok) ok = tag_match(tags[id], tp);
    }
    const u64 mm = __ballot(ok);
    wave_lds_sync();  // the pass has read its entries; ns + rank <= e
    if (ok) L.cj[ns + mask_rank(mm)] = j;
    ns += __builtin_popcountll(mm);
  }
  wave_lds_sync();
  return ns;
}

// The (try, mask) runs of query q, 64 at a time: CSR range of each run's bucket, wave prefix sum, balanced copy of the
// row numbers into the chunk (stage1_probe_kernel's idiom); score(ns) runs over cj[0..ns) whenever the chunk has filled.
template <int V, typename Score>
__device__ __forceinline__ void thash_enumerate(const TailHashArgs &A, const ThashWave &L, u32 q, const u32 *__restrict__ bits,
                                                const u32 *__restrict__ tags, const TagPred &tp, Score &&score) {
  const int lane = lane_id();
  const u32 ds = (u32)A.ds, rpt = 1u + ds + (u32)(A.pb * (A.pb - 1) / 2), runs = (u32)A.T * rpt;
  const u32 stride = (1u << ds) + 1u;
  const unsigned char *qbits = A.pbits + (size_t)q * A.T * A.pb;  // read by the pair runs only (pb >= 2)
  int cnt = 0;
  for (u32 rb = 0; rb < runs; rb += ANN_WAVE) {
    const u32 r = rb + lane;
    u32 c = 0, start = 0, t = 0;
    if (r < runs) {
      t = r / rpt;
      const u32 b = L.qc[t] ^ probe_mask(r - t * rpt, ds, qbits + (size_t)t * A.pb);
      const u32 *o = A.off + (size_t)t * stride + b;  // b < 2^ds: the codes and the masks are ds bits wide
      start = o[0];
      c = o[1] - start;
    }
    const u32 incl = wave_incl_scan(c);
    const u32 total = __shfl(incl, ANN_WAVE - 1);
    L.pref[lane] = incl - c, L.rst[lane] = start, L.rtry[lane] = t;
    wave_lds_sync();
    for (u32 done = 0; done < total;) {
      const u32 take = min((u32)ANN_THASH_CHUNK - (u32)cnt, total - done);
      for (u32 e = done + lane; e < done + take; e += ANN_WAVE) {
        int lo_ = 0, hi_ = ANN_WAVE - 1;  // last run with pref <= e (it is not empty)
        while (lo_ < hi_) {
          const int mid = (lo_ + hi_ + 1) >> 1;
          if (L.pref[mid] <= e) lo_ = mid; else hi_ = mid - 1;
        }
        L.cj[cnt + (e - done)] = A.rows[L.rst[lo_] + (e - L.pref[lo_])];
        L.ct[cnt + (e - done)] = L.rtry[lo_];
      }
      cnt += take, done += take;
      if (cnt == ANN_THASH_CHUNK) {
        wave_lds_sync();
        score(thash_reject<V>(A, L, cnt, bits, tags, tp));
        cnt = 0;
      }
    }
    wave_lds_sync();  // pref / rst / rtry are rewritten by the next pass
  }
  wave_lds_sync();
  if (cnt) score(thash_reject<V>(A, L, cnt, bits, tags, tp));
}

// LDS of one workgroup: per wave one selection buffer (cap keys + k keys of scratch), then the ThashWave words
template <int D, int V>
__global__ __launch_bounds__(64 * ExCfg<D>::WAVES) void tail_hash_merge_kernel(TailHashArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int C = RowChunks<D>::C;
  const int lane = lane_id(), w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int d = A.t.d;
  const size_t wave_keys = (size_t)A.t.cap + A.t.k;
  Key *kbase = reinterpret_cast<Key *>(smem) + (size_t)w * wave_keys;
  const ThashWave L = thash_carve(reinterpret_cast<u32 *>(smem + (size_t)W * wave_keys * sizeof(Key)) + (size_t)w * thash_wave_words(A.T), A.T);
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
  TagPred tp{0, 0, 0};
  if constexpr (V == EX_TAGS) tp = tag_pred(A.t.qmask, A.t.qlo, A.t.qhi, q);
  const u32 *__restrict__ bits = V == EX_ALL ? (const u32 *)NULL : A.t.bits;
  thash_load_query(A, L, q);
  tail_seed<0>(S, A.t, q, true);
  u32 nsc = 0;
  const FT *__restrict__ tail = A.t.tail;
  // survivors cj[0..ns): rpw rows per pass, the next pass's loads in flight while this one is reduced
  auto load = [&](VT(&b)[C], int r0, int ns, u32 &j) {
    const int r = r0 + ln.g;
    j = L.cj[(ln.valid && r < ns) ? r : r0];
    const FT *rp = tail + (size_t)j * d;
#pragma unroll
    for (int c = 0; c < C; c++) {
      if constexpr (D > 0) b[c] = reinterpret_cast<const VT *>(rp)[ln.p + c * ln.oc];
      else b[c] = oc_load_chunk<D, false>(rp, ln.p + c * ln.oc, d);
    }
  };
  auto offer = [&](const VT(&b)[C], int r0, int ns, u32 j) {
    const bool head = ln.valid && r0 + ln.g < ns && ln.p == 0;
    const Key key = key_make(ex_reduce<D>(a, b, ln.oc, ln.p, d), A.t.n + j);
    if (A.t.scored) nsc += (u32)__builtin_popcountll(__ballot(head));
    S.offer<0>(head && key_less(key, S.tau[0]), key);
  };
  auto score = [&](int ns) {
    if (!ns) return;
    VT b0[C], b1[C];
    u32 j0 = 0, j1 = 0;
    load(b0, 0, ns, j0);
    for (int r0 = 0; r0 < ns; r0 += 2 * ln.rpw) {
      const int r1 = r0 + ln.rpw, r2 = r1 + ln.rpw;
      if (r1 < ns) load(b1, r1, ns, j1);
      offer(b0, r0, ns, j0);
      if (r1 < ns) {
        if (r2 < ns) load(b0, r2, ns, j0);
        offer(b1, r1, ns, j1);
      }
    }
    wave_lds_sync();  // the chunk is refilled
  };
  thash_enumerate<V>(A, L, q, bits, A.t.tags, tp, score);
  tail_store<0>(S, A.t, q, true);
  if (A.t.scored && lane == 0 && nsc) atomicAdd(&A.t.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nsc);
}

// Any d without a register layout: tail_merge_generic_kernel's literal in-place tree, its rows read from the tail in HBM
// through the chunk.  Per wave: yq[d], m[NP][d] in front of the selection buffer.  V is a kernel argument (bits / tags).
__global__ __launch_bounds__(64 * ANN_EX_GEN_WAVES) void tail_hash_merge_generic_kernel(TailHashArgs A) {
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
  const ThashWave L = thash_carve(reinterpret_cast<u32 *>(smem + (size_t)W * wave_bytes) + (size_t)w * thash_wave_words(A.T), A.T);
  const u32 q = __builtin_amdgcn_readfirstlane(blockIdx.x * W + w);
  if (q >= A.t.Q) return;  // no workgroup barrier below
  ExSel S;
  S.init(kbase, kbase + A.t.cap, A.t.cap, A.t.k, q, A.t.Q);
  const u32 *__restrict__ tags = A.t.tags, *__restrict__ bits = A.t.bits;
  TagPred tp{0, 0, 0};
  if (tags) tp = tag_pred(A.t.qmask, A.t.qlo, A.t.qhi, q);
  for (int z = lane; z < d; z += ANN_WAVE) yq[z] = A.t.y[(size_t)q * d + z];
  thash_load_query(A, L, q);
  tail_seed<0>(S, A.t, q, true);
  int sh0 = 0;  // d <= 1 << sh0
  while ((1 << sh0) < d) sh0++;
  const FT zero = 0;
  u32 nsc = 0;
  const FT *__restrict__ tail = A.t.tail;
  auto score = [&](int ns) {
    for (int r0 = 0; r0 < ns; r0 += NP) {
      const int np = min(NP, ns - r0);
      for (int it = lane; it < (np << sh0); it += ANN_WAVE) {
        const int pr = it >> sh0, z = it & ((1 << sh0) - 1);
        if (z < d) {
          const FT df = yq[z] - tail[(size_t)L.cj[r0 + pr] * d + z];
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
      const Key key = key_make(act ? m[lane * d] : zero, A.t.n + L.cj[act ? r0 + lane : r0]);
      wave_lds_sync();  // m is rewritten by the next batch
      if (A.t.scored) nsc += (u32)np;
      S.offer<0>(act && key_less(key, S.tau[0]), key);
    }
    wave_lds_sync();  // the chunk is refilled
  };
  if (tags) thash_enumerate<EX_TAGS>(A, L, q, bits, tags, tp, score);
  else thash_enumerate<EX_BITS>(A, L, q, bits, tags, tp, score);
  tail_store<0>(S, A.t, q, true);
  if (A.t.scored && lane == 0 && nsc) atomicAdd(&A.t.scored[(blockIdx.x & 63u) * 8u], (unsigned long long)nsc);
}
