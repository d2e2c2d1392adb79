// ann_host.hip -- host side of the HIP backend: the resident index, the launch sequence of the query and
// precomp paths, and the C-ABI (include/ann_hip.h, include/algg.h, include/gpu_comp.h).
//
// Reference being replaced: the OpenCL shim /root/reference/alggp.c (buffers, kernel launches) plus the
// host orchestration /root/reference/alg.c as compiled for the GPU, and /root/reference/gpu_comp.c.
// There is no CPU fallback anywhere in this file: without a HIP device every entry point exits loudly.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <limits>
#include <mutex>
#include <vector>

#include "../../include/algg.h"
#include "../../include/ann_hip.h"
#include "../../include/gpu_comp.h"
#include "ann_hostpool.h"
#include "ann_precomp_kernels.h"
#include "ann_query_kernels.h"
#include "ann_probe_kernels.h"
#include "ann_recall_kernels.h"
#include "ann_exact_kernels.h"
#include "ann_filter_kernels.h"
#include "ann_tag_kernels.h"
#include "ann_kq_kernels.h"
#include "ann_radius_kernels.h"
#include "ann_tail_kernels.h"
#include "ann_tail_hash_kernels.h"
#include "ann_rerank_kernels.h"
#include "ann_prune_kernels.h"
#include "ann_sorted_kernels.h"
#include "ann_group_kernels.h"

static_assert(sizeof(ftype) == sizeof(FT), "ftype.h and ann_device.h disagree on the precision");

#define HIPCHECK(call)                                                                           \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      fprintf(stderr, "Error on GPU: %s (%s:%d: %s)\n", hipGetErrorString(e_), __FILE__, __LINE__, \
              #call);                                                                            \
      exit(1);                                                                                   \
    }                                                                                            \
  } while (0)

static void die(const char *msg) {
  fprintf(stderr, "approxnn_hip: %s\n", msg);
  exit(1);
}

// The HIP runtime consumes libc random() while it initialises (observed on ROCm 7.2: the first precomp after
// srandom(s) drew different rotations than the second).  The reference's callers own that stream (seeded
// drivers, compare_results.c:124-130), so every entry point parks it while HIP code runs.
// Guards nest and may be entered from several host threads: only the outermost one swaps the state.
static std::mutex g_rand_mu;
static int g_rand_depth = 0;
static char g_rand_scratch[256];
static char *g_rand_saved = NULL;
struct RandGuard {
  RandGuard() {
    std::lock_guard<std::mutex> lk(g_rand_mu);
    if (g_rand_depth++ == 0) g_rand_saved = initstate(1u, g_rand_scratch, sizeof g_rand_scratch);
  }
  ~RandGuard() {
    std::lock_guard<std::mutex> lk(g_rand_mu);
    if (--g_rand_depth == 0) setstate(g_rand_saved);
  }
};

// ----------------------------------------------------------------------------- environment switches
// A/B and test hooks ("Environment switches"), read ONCE -- at the first entry into the library and again
// whenever annhip_reload_env() is called -- never on the per-batch host path.
struct EnvCfg {
  bool loaded = false;
  bool exact = false, slot_scan = false, point_precomp = false, all_tries = false;
  int fuse = -1;      // ANN_HIP_FUSE: -1 unset, 0 never, 1 whenever possible
  int s1_waves = 0;   // ANN_HIP_S1_WAVES: 0 unset
  int s1_slots = 0;   // ANN_HIP_S1_SLOTS: annhip_query's stage 1 as a persistent grid holding that many waves per SIMD (0 = off)
  int tail = -1;      // ANN_HIP_TAIL: 0 = stage 2 as separate rows / network / widen kernels (the classic path, A/B and tests)
  int s2_threads = 64;  // ANN_HIP_S2_THREADS: workgroup size of the fused stage-2 kernel (64, or 128; cfg3: 64-66 vs 67-68 us)
  int segx = -1;      // ANN_HIP_SEGX: -1 unset (auto: shards of <= 30 % of the rows), 0 never, 1 whenever the shard qualifies
  size_t lds_row_max = 150 * 1024, exact_bytes = (size_t)1 << 30;
  int cache_mode = 0;  // ANN_HIP_CACHE: 0 sampled fingerprint (default), 1 strict (full content hash), 2 off
  size_t bk_group = 0;  // ANN_HIP_BK_GROUP: cap on the members per pass of precomp's bucket kernel (0 = what fits the LDS)
  int fin_tail = 1;     // ANN_HIP_FIN_TAIL: 0 = finalize1 as its own launch after stage 1 (A/B; default: in the stage-1 workgroups' tail)
  int s2_multi = 1;     // ANN_HIP_S2_MULTI: 0 = sharded stage-2 distances with one workgroup per query (A/B of stage2_dist_multi_kernel)
  int codes_lpq = 1;    // ANN_HIP_CODES_LPQ: 0 = the lanes-per-row hash kernel for every row length (A/B)
  int tie = 1;          // ANN_HIP_TIE: 0 = flagged rows always take the literal network (no tie path, ann_tie.h)
  int rows = 0;         // ANN_HIP_ROWS: f16 / f32 = query_gpu's resident single-device index reads narrow rows (annhip_index_set_rows)
  int exact_ranges = 0;  // ANN_HIP_EXACT_RANGES: row ranges of annhip_exact_knn's scan (0 = from n, ycnt and the CU count; tests)
  int prune = -1;        // ANN_HIP_PRUNE: annhip_index_set_prune's mode of a new index (-1 auto, 0 off, 1 on where eligible)
  int prune_k = 0;       // ANN_HIP_PRUNE_K: keys the preselection keeps per query (0 = max(16, 3 (k+1) / 2); A/B)
  bool rows_warned = false;  // ... and the one warning where it cannot (the other library's type, sharded modes) has been printed
};
static EnvCfg g_env;
static size_t env_size(const char *name, size_t dflt) {
  const char *e = getenv(name);
  return e && atoll(e) > 0 ? (size_t)atoll(e) : dflt;
}
static int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}
static void load_env() {
  EnvCfg c;
  c.loaded = true;
  c.exact = getenv("ANN_HIP_EXACT") != NULL;
  c.slot_scan = getenv("ANN_HIP_SLOT_SCAN") != NULL;
  c.point_precomp = getenv("ANN_HIP_POINT_PRECOMP") != NULL;
  c.all_tries = getenv("ANN_HIP_PRECOMP_ALL_TRIES") != NULL;
  c.fuse = env_int("ANN_HIP_FUSE", -1);
  c.s1_waves = env_int("ANN_HIP_S1_WAVES", 0);
  if (c.s1_waves < 1 || c.s1_waves > 4) c.s1_waves = 0;
  c.s1_slots = std::max(0, std::min(8, env_int("ANN_HIP_S1_SLOTS", 0)));
  c.segx = env_int("ANN_HIP_SEGX", -1);
  c.tail = env_int("ANN_HIP_TAIL", -1);
  c.s2_threads = env_int("ANN_HIP_S2_THREADS", 64) == 128 ? 128 : 64;
  c.lds_row_max = env_size("ANN_HIP_LDS_ROW_MAX", 150 * 1024);
  c.exact_bytes = env_size("ANN_HIP_EXACT_BYTES", (size_t)1 << 30);
  c.bk_group = env_size("ANN_HIP_BK_GROUP", 0);
  c.tie = env_int("ANN_HIP_TIE", 1);
  c.codes_lpq = env_int("ANN_HIP_CODES_LPQ", 1);
  c.s2_multi = env_int("ANN_HIP_S2_MULTI", 1);
  c.fin_tail = env_int("ANN_HIP_FIN_TAIL", 1);
  c.exact_ranges = std::max(0, env_int("ANN_HIP_EXACT_RANGES", 0));
  c.prune = env_int("ANN_HIP_PRUNE", -1);
  if (c.prune < -1 || c.prune > 1) c.prune = -1;
  c.prune_k = std::max(0, env_int("ANN_HIP_PRUNE_K", 0));
  const char *rw = getenv("ANN_HIP_ROWS");
  c.rows = !rw ? ANNHIP_ROWS_NATIVE : !strcmp(rw, "f16") ? ANNHIP_ROWS_F16 : !strcmp(rw, "f32") ? ANNHIP_ROWS_F32 : ANNHIP_ROWS_NATIVE;
  const char *cm = getenv("ANN_HIP_CACHE");
  c.cache_mode = !cm ? 0 : !strcmp(cm, "strict") ? 1 : !strcmp(cm, "off") ? 2 : 0;
  g_env = c;
}
static inline const EnvCfg &env() {
  if (!g_env.loaded) load_env();
  return g_env;
}
extern "C" void annhip_reload_env(void) { load_env(); }

// ----------------------------------------------------------------------------- device lifecycle
static bool g_init = false;
struct CleanupNode {
  void (*f)(void);
  CleanupNode *next;
};
static CleanupNode *g_cleanups = NULL;
static void cache_clear();

extern "C" void gpu_init(void) {
  if (g_init) return;
  RandGuard keep_callers_stream;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fprintf(stderr, "No GPU found.\n");  // same message as gpu_comp.c:85-90
    exit(1);
  }
  int dev = 0;
  const char *e = getenv("ANN_HIP_DEVICE");
  if (e) dev = atoi(e);
  if (dev < 0 || dev >= ndev) die("ANN_HIP_DEVICE out of range");
  HIPCHECK(hipSetDevice(dev));
  HIPCHECK(hipFree(0));
  g_init = true;
}

extern "C" void register_cleanup(void (*f)(void)) {
  if (g_init) {
    CleanupNode *c = (CleanupNode *)malloc(sizeof(CleanupNode));
    c->f = f;
    c->next = g_cleanups;
    g_cleanups = c;
  } else {
    f();
  }
}

extern "C" void gpu_cleanup(void) {
  if (!g_init) return;
  g_init = false;
  while (g_cleanups) {
    g_cleanups->f();
    CleanupNode *n = g_cleanups->next;
    free(g_cleanups);
    g_cleanups = n;
  }
  cache_clear();
}

extern "C" const char *annhip_precision(void) {
#ifdef USE_FLOAT
  return "f32";
#else
  return "f64";
#endif
}

// ----------------------------------------------------------------------------- small utilities
struct DevBuf {  // grow-only device workspace
  void *p = NULL;
  size_t cap = 0;
  void *need(size_t bytes) {
    if (bytes > cap) {
      if (p) HIPCHECK(hipFree(p));
      size_t want = bytes + bytes / 8 + 256;
      HIPCHECK(hipMalloc(&p, want));
      cap = want;
    }
    return p;
  }
  void release() {
    if (p) HIPCHECK(hipFree(p));
    p = NULL, cap = 0;
  }
};

struct PinBuf {  // grow-only pinned host memory
  void *p = NULL;
  size_t cap = 0;
  void *need(size_t bytes) {
    if (bytes > cap) {
      if (p) HIPCHECK(hipHostFree(p));
      size_t want = bytes + bytes / 8 + 256;
      HIPCHECK(hipHostMalloc(&p, want, hipHostMallocPortable));
      cap = want;
    }
    return p;
  }
  void release() {
    if (p) HIPCHECK(hipHostFree(p));
    p = NULL, cap = 0;
  }
};

template <typename T>
static T *dev_alloc(size_t count) {
  void *p = NULL;
  HIPCHECK(hipMalloc(&p, (count ? count : 1) * sizeof(T)));
  return (T *)p;
}

static int device_cus() {  // compute units of the current device (cached per device)
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    hipDeviceProp_t prop;
    cus[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return cus[dev];
}

static unsigned grid_for(size_t work, unsigned block, unsigned cap = 1u << 20) {
  size_t g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

#define ANN_NCOUNTERS (8 + 64 * 8)
struct EventPair {
  hipEvent_t a, b;
};

// Scratch memory of one in-flight query batch.  The index owns a default one; callers that overlap batches on
// several HIP streams give each stream its own (annhip_workspace_create).
struct annhip_workspace {
  DevBuf codes, cand_d, cand_i, nvt, nvo, top_i, top_d, flist, xids, xd, r2i, r2d, out_i, out_d;
  DevBuf pbits;  // fixed mode with pair bits: u8[Q][T][b] ranked projection indices of this batch (annhip_index_set_probe)
  DevBuf sorted;  // annhip_query_sorted: u32 start[Q], len[Q], list[Q][3], qmask[Q]
  DevBuf tie_d, tie_i;  // pruned stage 1: [Q][k+1] exact candidate lists of the flagged queries (PruneArgs::tie_d / tie_i)
  DevBuf grp_i, grp_d;  // annhip_query_grouped: the [Q][list] result that the collapse reads (size_t ids, FT dists)
  // annhip_query_sorted_set: the staging that the interval count sizes, the arrays that the entry count sizes, and the
  // pinned copy of the call's offsets with the event that says the previous call's upload has read it
  DevBuf sset, spart;
  PinBuf spin;
  hipEvent_t sset_ev = NULL;
  u32 *d_fcount = NULL;
  void release() {
    sset.release(), spart.release(), spin.release();
    if (sset_ev) HIPCHECK(hipEventDestroy(sset_ev));
    sset_ev = NULL;
    DevBuf *bufs[] = {&codes, &cand_d, &cand_i, &nvt, &nvo, &top_i, &top_d, &flist, &xids, &xd, &r2i, &r2d, &out_i, &out_d, &pbits, &sorted, &tie_d, &tie_i, &grp_i, &grp_d};
    for (DevBuf *b : bufs) b->release();
    if (d_fcount) HIPCHECK(hipFree(d_fcount));
    d_fcount = NULL;
  }
};

// the one narrow row storage this library serves (RN, ann_device.h); the other library's value is refused
#ifdef USE_FLOAT
#define ANNHIP_ROWS_NARROW ANNHIP_ROWS_F16
#define ANN_NARROW_WHAT "binary16"
#else
#define ANNHIP_ROWS_NARROW ANNHIP_ROWS_F32
#define ANN_NARROW_WHAT "binary32"
#endif

struct annhip_index {
  size_t n = 0, k = 0, d = 0, ds = 0, lo = 0, hi = 0;
  int T = 0;
  FT *d_points = NULL;
  bool own_points = false;
  std::vector<u32 *> d_tabs;  // per try
  std::vector<uint2 *> d_segs;  // per try: per-bucket (first owned position, owned count, valid count)
  std::vector<uint4 *> d_segx;  // per try: 32-byte inline records (small shards only, see build_segx_kernel)
  int use_seg = 1;              // stage-1 scan: 0 slot scan (a table without the sorted-prefix layout: foreign save_t),
                                // 1 segment words + table rows, 2 inline records
  std::vector<TryInfo> h_tries;
  TryInfo *d_tries = NULL;
  u32 *d_graph = NULL;
  FT *d_means = NULL, *d_bases = NULL;
  FT *d_graph_dists = NULL;  // precomp only: squared distances of the graph edges until the caller takes them
  u32 L1 = 0, P1 = 0, Lc1 = 0, L2 = 0, P2 = 0, Lc2 = 0;
  size_t sum_pm = 0;
  hipStream_t stream = 0;
  annhip_workspace ws;           // default workspace (annhip_query, staged calls)
  DevBuf io_y, io_ids, io_dist;  // query_gpu's staging of host inputs/outputs, reused between calls
  PinBuf io_y_pin, io_out_pin;   // ... and their pinned host-side bounce buffers
  unsigned long long *d_rows = NULL;  // [0] stage-1 gathered rows, [2] exact-path queries, [3] of those: answered by the tie path, [8..8+512) rows kernels (64 padded shards)
  // measurement
  int profile = 0;  // 1: stage-1 event pair + stage marks + row statistics; 2: the stage-1 event pair only (two events per
                    // step: what bench.py keeps inside its timed region; every event costs ~5 us of stream time)
  std::vector<EventPair> ev_used, ev_free;
  std::vector<hipEvent_t> seg_free;
  std::vector<std::vector<hipEvent_t>> seg_used;  // per call: events at the stage boundaries
  double seg_ms[6] = {0, 0, 0, 0, 0, 0};          // codes, stage1, finalize+fallback, stage-2 rows, stage-2 network, widen
  double s1_ms = 0;
  double s1_launches = 0, queries = 0;
  int gather_pieces = 1;  // annhip_sh_stage1 in this many launches (annhip_index_set_gather_pieces)
  int gather_slots = 0;   // annhip_sh_stage1 as a persistent grid holding this many waves per SIMD (0 = one workgroup per query)
  int fixed = 0;          // annhip_index_set_fixed: opt-in non-parity query mode (Q1/Q2 undone)
  int probe = 0;          // annhip_index_set_probe: pair bits b of fixed mode (0 = own bucket + Hamming distance 1 only)
  int rows = ANNHIP_ROWS_NATIVE;  // annhip_index_set_rows: which copy of the point rows the single-device query reads
  RN *d_points_h = NULL;          // narrow copy of the rows (made on the first ANNHIP_ROWS_NARROW, kept until destroy/reshard)
  // annhip_index_set_prune (ann_prune_kernels.h): parity-mode stage 1 preselects on d_points_h and rescores on native rows
  int prune = -1;                 // the mode asked for: -1 auto, 0 off, 1 on where eligible
  bool prune_ready = false;       // d_points_h and prune_E are made and the index qualifies (prune_active: and the query does)
  double prune_E = 0;             // >= max over the rows of ||p - h(p)||_2
  int prune_kp = 0;               // keys the preselection keeps per query
  u32 *filter = NULL;             // annhip_index_set_filter: the index's copy of the allow list, u32[ceil(n / 32)] (NULL = none)
  long long filter_count = -1;    // allowed rows among [0, n), taken when the filter was set (-1 = no filter)
  u32 *tags = NULL;               // annhip_index_set_tags: the index's copy of the rows' tag words, u32[n] (NULL = none)
  // annhip_index_append: rows added since the build, scanned exactly by every fixed-mode query (ann_tail_kernels.h).
  // Tail row j has id n + j.  filter and tags are allocated for n + tail_cap rows and hold n + tail_m.
  FT *d_tail = NULL;              // [tail_cap][d], owned
  size_t tail_m = 0, tail_cap = 0;
  // annhip_index_hash_tail: tail rows [0, tail_mh) are looked up by hash code (ann_tail_hash_kernels.h), [tail_mh, tail_m)
  // are scanned exactly.  The structure names rows by j, not by address: it survives a move of d_tail.
  size_t tail_mh = 0;
  u32 *tail_codes = NULL;  // [tail_mh][T]
  u32 *tail_off = NULL;    // [T][2^ds + 1], offsets into tail_rows (they include t * tail_mh)
  u32 *tail_rows = NULL;   // [T][tail_mh]
  // annhip_index_sort_tags (ann_sorted_kernels.h): the row ids [0, ord_ms) ordered by (tags & ord_mask, id) and the masked
  // words in that order; rows [ord_ms, n_total) are "fresh": appended since, scanned by the tail's kernel
  u32 *ord_perm = NULL, *ord_keys = NULL;
  size_t ord_ms = 0;
  u32 ord_mask = 0;
};
static size_t n_total(const annhip_index *ix) { return ix->n + ix->tail_m; }
static size_t filter_words(size_t rows) { return (rows + 31) / 32; }

static QParams make_params(const annhip_index *ix) {
  QParams P;
  P.points = ix->d_points;
  P.tries = ix->d_tries;
  P.graph = ix->d_graph;
  P.means = ix->d_means;
  P.bases = ix->d_bases;
  P.n = (u32)ix->n, P.lo = (u32)ix->lo, P.hi = (u32)ix->hi;
  P.d = (int)ix->d, P.k = (int)ix->k, P.T = ix->T, P.ds = (int)ix->ds;
  P.L1 = ix->L1, P.P1 = ix->P1, P.Lc1 = ix->Lc1, P.L2 = ix->L2, P.Lc2 = ix->Lc2;
  P.q0 = 0, P.qn = 0;
  P.fixed = ix->fixed ? 1u : 0u;
  if (ix->fixed) P.P1 = P.Lc1 = P.L1;  // every slot of the candidate row takes part
  return P;
}

// QParams of the single-device query path (annhip_query / _on / _slice, annhip_stream_*): the rows the index is set to
static QParams query_params(const annhip_index *ix) {
  QParams P = make_params(ix);
  if (ix->rows == ANNHIP_ROWS_NARROW) P.points_h = ix->d_points_h;
  return P;
}

static FT ft_inf_host() { return std::numeric_limits<FT>::infinity(); }
static u32 magic_for(u32 pm) { return (u32)((1ull << 32) / pm) + 1u; }

// derive row geometry (SURVEY 8 notation) once the tries are known
static void finish_geometry(annhip_index *ix) {
  size_t off = 0;
  ix->sum_pm = 0;
  for (int t = 0; t < ix->T; t++) {
    TryInfo &tr = ix->h_tries[t];
    if (tr.pm == 0) die("empty bucket table");
    tr.off = (u32)off;
    off += (size_t)tr.pm * (ix->ds + 1);
    tr.end = (u32)off;
    tr.magic = magic_for(tr.pm);
    ix->sum_pm += tr.pm;
    if ((unsigned long long)off * tr.pm >= (1ull << 32)) die("candidate row too long for 32-bit slot arithmetic");
  }
  ix->L1 = (u32)off;
  ix->P1 = 1u << ann_lg(ix->L1);
  ix->Lc1 = (u32)ann_need_len(ix->L1, ix->k);
  ix->L2 = (u32)(ix->k * (ix->k + 1));
  ix->P2 = 1u << ann_lg(ix->L2);
  ix->Lc2 = (u32)ann_need_len(ix->L2, ix->k);
  if (!ix->d_tries) ix->d_tries = dev_alloc<TryInfo>(ix->T);
  HIPCHECK(hipMemcpy(ix->d_tries, ix->h_tries.data(), sizeof(TryInfo) * ix->T, hipMemcpyHostToDevice));
  if (!ix->ws.d_fcount) ix->ws.d_fcount = dev_alloc<u32>(4);
  if (!ix->d_rows) {
    ix->d_rows = dev_alloc<unsigned long long>(ANN_NCOUNTERS);
    HIPCHECK(hipMemset(ix->d_rows, 0, ANN_NCOUNTERS * sizeof(unsigned long long)));
  }
}

// (re)build the per-bucket segment words of every try for the current owned range; decides use_seg
static void build_segments(annhip_index *ix) {
  const size_t nb = (size_t)1 << ix->ds;
  u32 *bad = dev_alloc<u32>(1);
  HIPCHECK(hipMemset(bad, 0, sizeof(u32)));
  ix->d_segs.resize(ix->T, NULL);
  for (int t = 0; t < ix->T; t++) {
    if (!ix->d_segs[t]) ix->d_segs[t] = dev_alloc<uint2>(nb);
    build_seg_kernel<<<grid_for(nb, 256, 1u << 30), 256>>>(nb, ix->h_tries[t].pm, ix->d_tabs[t], (u32)ix->n, (u32)ix->lo,
                                                           (u32)ix->hi, ix->d_segs[t], bad);
    ix->h_tries[t].seg = ix->d_segs[t];
  }
  u32 nbad = 0;
  HIPCHECK(hipMemcpy(&nbad, bad, sizeof(u32), hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(bad));
  ix->use_seg = (nbad == 0 && !env().slot_scan) ? 1 : 0;
  // a small shard (<= 30 % of the rows) scans through inline records: one 32-byte fetch per run instead of two fetches
  bool small = ix->use_seg && (double)(ix->hi - ix->lo) <= 0.3 * (double)ix->n;
  for (int t = 0; t < ix->T; t++) small = small && ix->h_tries[t].pm <= 255;
  if (env().segx >= 0) small = small && env().segx != 0;
  ix->d_segx.resize(ix->T, NULL);
  for (int t = 0; t < ix->T; t++) {
    if (small) {
      if (!ix->d_segx[t]) ix->d_segx[t] = dev_alloc<uint4>(2 * nb);
      build_segx_kernel<<<grid_for(nb, 256, 1u << 30), 256>>>(nb, ix->h_tries[t].pm, ix->d_tabs[t], ix->d_segs[t], ix->d_segx[t]);
    } else if (ix->d_segx[t]) {
      HIPCHECK(hipFree(ix->d_segx[t]));
      ix->d_segx[t] = NULL;
    }
    ix->h_tries[t].segx = ix->d_segx[t];
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  if (small) ix->use_seg = 2;
}

static void check_limits(size_t n, size_t k, size_t d, size_t ds, int T) {
  if (n >= 0xFFFFFFF0ull) die("n must fit 32-bit ids on the device");
  if (k < 1 || n <= k) die("need n > k >= 1");
  if (ds > 31) die("d_short > 31 is not supported (bucket table would not fit memory anyway)");
  if (T < 1) die("need tries >= 1");
  size_t d_max = 1;
  while (d_max < d) d_max <<= 1;
  if (d_max < 16) die("d_max < 16 is out of bounds in the reference (apply_walsh_step, compute.cl:107); not supported");
}

extern "C" void annhip_index_set_stream(annhip_index *ix, void *s) { ix->stream = (hipStream_t)s; }
extern "C" void annhip_index_set_gather_pieces(annhip_index *ix, int pieces) { ix->gather_pieces = pieces < 1 ? 1 : pieces; }
extern "C" void annhip_index_set_gather_slots(annhip_index *ix, int waves_per_simd) {
  ix->gather_slots = waves_per_simd < 0 ? 0 : waves_per_simd > 8 ? 8 : waves_per_simd;
}
static void drop_filter(annhip_index *ix) {
  if (ix->filter) HIPCHECK(hipFree(ix->filter));
  ix->filter = NULL;
  ix->filter_count = -1;
}
extern "C" void annhip_index_set_fixed(annhip_index *ix, int fixed) {
  ix->fixed = fixed ? 1 : 0;
  if (!ix->fixed && ix->filter) {  // a parity-mode query has no notion of a filter: it must not look as if one applied
    HIPCHECK(hipDeviceSynchronize());
    drop_filter(ix);
  }
}
// Row tags (annhip_index_set_tags): attributes of the rows, read by annhip_query_tagged and
// annhip_index_exact_query_tagged only.  Contract: include/ann_hip.h.  Kernels: ann_tag_kernels.h.
// the tag order goes with the tags it was sorted from (the caller has synchronised)
static void drop_order(annhip_index *ix) {
  if (ix->ord_perm) HIPCHECK(hipFree(ix->ord_perm));
  if (ix->ord_keys) HIPCHECK(hipFree(ix->ord_keys));
  ix->ord_perm = ix->ord_keys = NULL;
  ix->ord_ms = 0, ix->ord_mask = 0;
}
static void drop_tags(annhip_index *ix) {
  if (ix->tags) HIPCHECK(hipFree(ix->tags));
  ix->tags = NULL;
  drop_order(ix);
}
extern "C" int annhip_index_set_tags(annhip_index *ix, const uint32_t *tags, int tags_on_device) {
  if (!tags) {
    if (ix->tags) HIPCHECK(hipDeviceSynchronize());
    drop_tags(ix);
    return 0;
  }
  if (ix->lo != 0 || ix->hi != ix->n) {
    fprintf(stderr, "annhip_index_set_tags: the index does not hold rows [0, n) on this device (resharded)\n");
    return -1;
  }
  HIPCHECK(hipDeviceSynchronize());
  drop_order(ix);  // new tags: the order was sorted from the old ones
  if (!ix->tags) ix->tags = dev_alloc<u32>(ix->n + ix->tail_cap);
  HIPCHECK(hipMemcpy(ix->tags, tags, sizeof(u32) * n_total(ix), tags_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  return 0;
}
extern "C" int annhip_index_has_tags(const annhip_index *ix) { return ix->tags ? 1 : 0; }
// Contract: include/ann_hip.h.  Kernels: ann_sorted_kernels.h.  A stable LSD radix sort of (tags & mask, id), one pass per
// byte of the mask that has a bit set; synchronous, on the null stream.
extern "C" int annhip_index_sort_tags(annhip_index *ix, uint32_t field_mask) {
  if (!field_mask) {
    if (ix->ord_perm) HIPCHECK(hipDeviceSynchronize());
    drop_order(ix);
    return 0;
  }
  const char *why = !ix->tags ? "the index has no tags (annhip_index_set_tags)"
                    : (ix->lo != 0 || ix->hi != ix->n) ? "the index does not hold rows [0, n) on this device (resharded)" : NULL;
  if (why) {
    fprintf(stderr, "annhip_index_sort_tags: %s\n", why);
    return -1;
  }
  HIPCHECK(hipDeviceSynchronize());
  drop_order(ix);
  const size_t ms = n_total(ix);  // (below 2^32 - 16: check_limits and tail_refusal)
  const u32 nblk = (u32)((ms + ANN_SORT_ITEMS - 1) / ANN_SORT_ITEMS);
  u32 *keys = dev_alloc<u32>(ms), *perm = dev_alloc<u32>(ms), *keys2 = dev_alloc<u32>(ms), *perm2 = dev_alloc<u32>(ms);
  u32 *hist = dev_alloc<u32>((size_t)256 * nblk);
  tsort_init_kernel<<<grid_for(ms, 256, 4096), 256>>>((u32)ms, ix->tags, field_mask, keys, perm);
  for (int shift = 0; shift < 32 && nblk; shift += 8) {
    if (!((field_mask >> shift) & 255u)) continue;  // every key has digit 0: the pass would move nothing
    tsort_count_kernel<<<nblk, 64>>>(keys, (u32)ms, shift, nblk, hist);
    tsort_scan_kernel<<<1, 1024>>>(hist, (size_t)256 * nblk);
    tsort_place_kernel<<<nblk, 64>>>(keys, perm, (u32)ms, shift, nblk, hist, keys2, perm2);
    std::swap(keys, keys2), std::swap(perm, perm2);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipFree(keys2));
  HIPCHECK(hipFree(perm2));
  HIPCHECK(hipFree(hist));
  ix->ord_keys = keys, ix->ord_perm = perm, ix->ord_ms = ms, ix->ord_mask = field_mask;
  return 0;
}
extern "C" size_t annhip_index_tag_order(const annhip_index *ix, uint32_t *field_mask) {
  if (field_mask) *field_mask = ix->ord_perm ? ix->ord_mask : 0;
  return ix->ord_perm ? ix->ord_ms : 0;
}
// filter_count := the set bits among rows [0, n_total) of the index's bitmap (synchronous, null stream)
static void filter_recount(annhip_index *ix) {
  const size_t rows = n_total(ix);
  unsigned long long *cnt = dev_alloc<unsigned long long>(1), host = 0;
  HIPCHECK(hipMemset(cnt, 0, sizeof host));
  filter_count_kernel<<<grid_for(filter_words(rows), 256, 1024), 256>>>(rows, ix->filter, cnt);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(&host, cnt, sizeof host, hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(cnt));
  ix->filter_count = (long long)host;
}
// Contract: include/ann_hip.h.  Kernels: ann_filter_kernels.h.
extern "C" int annhip_index_set_filter(annhip_index *ix, const uint32_t *bits, int bits_on_device) {
  if (!bits) {
    if (ix->filter) HIPCHECK(hipDeviceSynchronize());
    drop_filter(ix);
    return 0;
  }
  if (!ix->fixed) {
    fprintf(stderr, "annhip_index_set_filter: fixed mode is off (annhip_index_set_fixed); parity-mode queries take no filter\n");
    return -1;
  }
  if (ix->lo != 0 || ix->hi != ix->n) {
    fprintf(stderr, "annhip_index_set_filter: the index does not hold rows [0, n) on this device (resharded)\n");
    return -1;
  }
  const size_t nw = filter_words(n_total(ix));
  HIPCHECK(hipDeviceSynchronize());
  if (!ix->filter) ix->filter = dev_alloc<u32>(filter_words(ix->n + ix->tail_cap));
  HIPCHECK(hipMemcpy(ix->filter, bits, sizeof(u32) * nw, bits_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  filter_recount(ix);
  return 0;
}
extern "C" long long annhip_index_filter_count(const annhip_index *ix) { return ix->filter ? ix->filter_count : -1; }
extern "C" int annhip_filter_pack(size_t n, const uint8_t *flags_dev, uint32_t *bits_dev, void *hip_stream) {
  if (!n) return 0;
  gpu_init();
  filter_pack_kernel<<<grid_for((n + 63) / 64, 4, 4096), 256, 0, (hipStream_t)hip_stream>>>(n, flags_dev, bits_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int annhip_index_set_probe(annhip_index *ix, int pair_bits) {
  if (pair_bits < ANNHIP_PROBE_ALL || pair_bits > (int)ix->ds) {
    fprintf(stderr, "annhip_index_set_probe: pair bits %d outside 0..d_short = %d (ANNHIP_PROBE_ALL = -1)\n", pair_bits, (int)ix->ds);
    return -1;
  }
  ix->probe = pair_bits == ANNHIP_PROBE_ALL ? (int)ix->ds : pair_bits;
  return 0;
}
extern "C" int annhip_index_probe(const annhip_index *ix) { return ix->probe; }

#ifdef USE_FLOAT
// rows -> binary16, round to nearest even (overflow -> +-inf, subnormals kept, NaN stays NaN)
__global__ void rows_to_half_kernel(size_t count, const float *__restrict__ in, __half *__restrict__ out) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x)
    out[e] = __float2half_rn(in[e]);
}
static void rows_to_narrow(size_t count, const FT *in, RN *out) {
  rows_to_half_kernel<<<grid_for(count, 256, 1u << 20), 256>>>(count, in, reinterpret_cast<__half *>(out));
}
#else
// rows -> binary32, round to nearest even (overflow -> +-inf, subnormals kept, NaN stays NaN): one v_cvt_f32_f64 under the
// kernel descriptor's default mode (both round modes 0 = nearest even, both denorm modes 3 = kept on input and output)
__global__ void rows_to_float_kernel(size_t count, const double *__restrict__ in, float *__restrict__ out) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x)
    out[e] = (float)in[e];
}
static void rows_to_narrow(size_t count, const FT *in, RN *out) {
  rows_to_float_kernel<<<grid_for(count, 256, 1u << 20), 256>>>(count, in, out);
}
#endif

extern "C" int annhip_index_set_rows(annhip_index *ix, int rows) {
  if (rows != ANNHIP_ROWS_NATIVE && rows != ANNHIP_ROWS_F16 && rows != ANNHIP_ROWS_F32) {
    fprintf(stderr, "annhip_index_set_rows: unknown row storage %d (ANNHIP_ROWS_NATIVE = 0, ANNHIP_ROWS_F16 = 1, "
                    "ANNHIP_ROWS_F32 = 2)\n", rows);
    return -1;
  }
  if (rows != ANNHIP_ROWS_NATIVE && rows != ANNHIP_ROWS_NARROW) {
    fprintf(stderr, "annhip_index_set_rows: %s rows are a feature of the %s library only\n",
            rows == ANNHIP_ROWS_F16 ? "binary16" : "binary32", rows == ANNHIP_ROWS_F16 ? "f32" : "f64");
    return -1;
  }
  if (rows == ANNHIP_ROWS_NARROW) {
    if (ix->tail_m) {
      fprintf(stderr, "annhip_index_set_rows: " ANN_NARROW_WHAT " rows and appended rows do not compose (annhip_index_drop_tail, or "
                      "Index.compact)\n");
      return -1;
    }
    if (!(ix->lo == 0 && ix->hi == ix->n)) {
      fprintf(stderr, "annhip_index_set_rows: " ANN_NARROW_WHAT " rows need the whole index on this device (rows [0, n))\n");
      return -1;
    }
    if (!ix->d_points_h) {  // first enable: the copy is made on the device and kept (switching back and forth is free)
      const size_t count = ix->n * ix->d;
      ix->d_points_h = dev_alloc<RN>(count);
      HIPCHECK(hipDeviceSynchronize());  // the native rows may have been written on another stream
      rows_to_narrow(count, ix->d_points, ix->d_points_h);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipDeviceSynchronize());
    }
  }
  ix->rows = rows;
  return 0;
}
extern "C" int annhip_index_rows(const annhip_index *ix) { return ix->rows; }
static void drop_half_rows(annhip_index *ix) {
  if (ix->d_points_h) HIPCHECK(hipFree(ix->d_points_h));
  ix->d_points_h = NULL;
  ix->rows = ANNHIP_ROWS_NATIVE;
  ix->prune_ready = false;
}

// ----------------------------------------------------------------------------- pruned stage 1 (annhip_index_set_prune)
// Contract: include/ann_hip.h.  Kernels: ann_prune_kernels.h.  The narrow copy is the one annhip_index_set_rows makes.
static int layout_code(size_t d, bool allow_oc);  // (the layout table, below)
static bool layout_is_generic(int code);
static int prune_keys(size_t k) {
  const int K1 = (int)k + 1;
  // measured at cfg3 (k = 10), ms per step with 16 / 24 / 32 keys: 0.859 / 0.878 / 0.894 against 1.245 native (0.943 / 1.025 /
  // 1.125 while the selection ran through an LDS buffer); every query was certified at all three, so more keys buy nothing
  int kp = env().prune_k > 0 ? env().prune_k : std::max(16, 3 * K1 / 2);
  return std::min(ANN_PRUNE_KMAX, std::max(kp, K1));
}
// what keeps this index from pruning whatever the query (NULL: nothing)
static const char *prune_refusal(const annhip_index *ix) {
#ifndef USE_FLOAT
  return "pruning is a feature of the f32 library only";
#else
  return (ix->lo != 0 || ix->hi != ix->n) ? "the index does not hold rows [0, n) on this device (resharded)"
         : ix->tail_m                     ? "the index has appended rows (annhip_index_drop_tail, or Index.compact)"
         : ix->k + 1 > 32                 ? "k + 1 must be at most 32"
         : layout_is_generic(layout_code(ix->d, true)) ? "no register layout for this row length"
                                          : NULL;
#endif
}
// queries of this index take the pruned stage 1 right now (parity mode, native rows selected, nothing appended)
static bool prune_active(const annhip_index *ix) {
  return ix->prune_ready && ix->d_points_h && !ix->fixed && ix->rows == ANNHIP_ROWS_NATIVE && !ix->tail_m && ix->lo == 0 &&
         ix->hi == ix->n;
}
// Apply `mode` to the index: the narrow copy and E are made here, never inside a query call (synchronous, null stream).
// Returns -1 -- with one line on stderr where `who` is given -- and changes nothing where mode 1 cannot be served.
static int prune_setup(annhip_index *ix, int mode, const char *who) {
  RandGuard keep_callers_stream;
  if (mode == 0) {
    ix->prune = 0, ix->prune_ready = false;  // the copy stays: annhip_index_set_rows shares it
    return 0;
  }
  const char *why = prune_refusal(ix);
  const int kp = prune_keys(ix->k);
  const size_t count = ix->n * ix->d;
  if (!why && mode < 0) {  // auto: small indexes keep the native path
    size_t free_b = 0, total_b = 0;
    if ((size_t)ix->P1 < 8 * (size_t)kp) why = "candidate rows too short";
    else if (count * sizeof(FT) < ((size_t)1 << 30)) why = "native rows below 1 GiB";
    else if (!ix->d_points_h &&
             (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < count * sizeof(RN) + ((size_t)2 << 30)))
      why = "not enough free device memory for the narrow copy";
  }
  bool made = false;
  double E = 0;
  if (!why) {
    HIPCHECK(hipDeviceSynchronize());  // the native rows may have been written on another stream
    if (!ix->d_points_h) {
      ix->d_points_h = dev_alloc<RN>(count);
      rows_to_narrow(count, ix->d_points, ix->d_points_h);
      HIPCHECK(hipGetLastError());
      made = true;
    }
    unsigned long long *acc = dev_alloc<unsigned long long>(2), host[2] = {0, 0};
    HIPCHECK(hipMemset(acc, 0, sizeof host));
    prune_rowerr_kernel<<<grid_for((ix->n + 3) / 4, 1, 8192), 256>>>(ix->n, (int)ix->d, ix->d_points, ix->d_points_h, acc);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(host, acc, sizeof host, hipMemcpyDeviceToHost));
    HIPCHECK(hipFree(acc));
    double worst;
    memcpy(&worst, &host[0], sizeof worst);
    E = sqrt(worst) * (1.0 + 0x1p-20);  // rounded up: the double sum of d squares is within d 2^-53 of the real one
    if (host[1] || !(E < std::numeric_limits<double>::infinity())) {
      why = "a row does not survive " ANN_NARROW_WHAT " (overflow or NaN): no finite error bound";
      if (made) {
        HIPCHECK(hipFree(ix->d_points_h));
        ix->d_points_h = NULL;
      }
    }
  }
  if (why) {
    if (mode == 1) {
      if (who) fprintf(stderr, "%s: %s\n", who, why);
      return -1;
    }
    ix->prune = mode, ix->prune_ready = false;  // auto: stays off, silently
    return 0;
  }
  ix->prune = mode, ix->prune_ready = true, ix->prune_E = E, ix->prune_kp = kp;
  return 0;
}
extern "C" int annhip_index_set_prune(annhip_index *ix, int mode) {
  if (mode < -1 || mode > 1) {
    fprintf(stderr, "annhip_index_set_prune: unknown mode %d (-1 auto, 0 off, 1 on where eligible)\n", mode);
    return -1;
  }
  return prune_setup(ix, mode, "annhip_index_set_prune");
}
extern "C" int annhip_index_prune(const annhip_index *ix) { return prune_active(ix) ? 1 : 0; }
extern "C" int annhip_index_prune_bound(const annhip_index *ix, double *E, int *keys) {
  if (!ix->prune_ready) return 0;
  if (E) *E = ix->prune_E;
  if (keys) *keys = ix->prune_kp;
  return 1;
}

// ----------------------------------------------------------------------------- appended rows (the tail)
// Contract: include/ann_hip.h.  Kernels: ann_tail_kernels.h.  All of it synchronous on the null stream.
static const char *tail_refusal(const annhip_index *ix, size_t count) {
  return !ix->fixed ? "fixed mode is off (annhip_index_set_fixed); parity-mode queries never see appended rows"
         : (ix->lo != 0 || ix->hi != ix->n) ? "the index does not hold rows [0, n) on this device (resharded)"
         : ix->rows != ANNHIP_ROWS_NATIVE ? "the index reads narrow rows (annhip_index_set_rows); a tail holds native rows only"
         : (n_total(ix) + count >= 0xFFFFFFF0ull || count >= 0xFFFFFFF0ull) ? "row ids must fit 32 bits"
                                                                          : NULL;
}
// mh = 0: the codes and the CSR of the hashed tail rows are freed (the caller has synchronised)
static void drop_tail_hash(annhip_index *ix) {
  for (u32 **p : {&ix->tail_codes, &ix->tail_off, &ix->tail_rows}) {
    if (*p) HIPCHECK(hipFree(*p));
    *p = NULL;
  }
  ix->tail_mh = 0;
}
// capacity >= rows: the tail buffer and the index's bitmap and tag copies move to larger allocations
static void tail_grow(annhip_index *ix, size_t rows) {
  if (rows <= ix->tail_cap) return;
  HIPCHECK(hipDeviceSynchronize());
  const size_t cap = std::max(rows, 2 * ix->tail_cap), have = n_total(ix);
  FT *nt = dev_alloc<FT>(cap * ix->d);
  if (ix->tail_m) HIPCHECK(hipMemcpy(nt, ix->d_tail, sizeof(FT) * ix->tail_m * ix->d, hipMemcpyDeviceToDevice));
  if (ix->d_tail) HIPCHECK(hipFree(ix->d_tail));
  ix->d_tail = nt;
  if (ix->filter) {
    u32 *nf = dev_alloc<u32>(filter_words(ix->n + cap));
    HIPCHECK(hipMemcpy(nf, ix->filter, sizeof(u32) * filter_words(have), hipMemcpyDeviceToDevice));
    HIPCHECK(hipFree(ix->filter));
    ix->filter = nf;
  }
  if (ix->tags) {
    u32 *ng = dev_alloc<u32>(ix->n + cap);
    HIPCHECK(hipMemcpy(ng, ix->tags, sizeof(u32) * have, hipMemcpyDeviceToDevice));
    HIPCHECK(hipFree(ix->tags));
    ix->tags = ng;
  }
  ix->tail_cap = cap;
}
extern "C" int annhip_index_reserve_tail(annhip_index *ix, size_t rows) {
  if (const char *why = tail_refusal(ix, rows > ix->tail_m ? rows - ix->tail_m : 0)) {
    fprintf(stderr, "annhip_index_reserve_tail: %s\n", why);
    return -1;
  }
  tail_grow(ix, rows);
  return 0;
}
extern "C" int annhip_index_append(annhip_index *ix, const ftype *rows, int rows_on_device, size_t count, const uint32_t *tags,
                                   int tags_on_device) {
  const char *why = tail_refusal(ix, count);
  if (!why && ix->tags && !tags) why = "the index has tags (annhip_index_set_tags): the new rows need theirs";
  if (!why && !ix->tags && tags) why = "tags were given but the index has none (annhip_index_set_tags)";
  if (!why && count && !rows) why = "rows == NULL";
  if (why) {
    fprintf(stderr, "annhip_index_append: %s\n", why);
    return -1;
  }
  if (!count) return 0;
  HIPCHECK(hipDeviceSynchronize());
  if (ix->prune_ready) drop_half_rows(ix);  // a pruned stage 1 never sees a tail: its copy and bound go (rows are native here)
  tail_grow(ix, ix->tail_m + count);
  const size_t at = n_total(ix);
  HIPCHECK(hipMemcpy(ix->d_tail + ix->tail_m * ix->d, rows, sizeof(FT) * count * ix->d,
                     rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  if (ix->tags)
    HIPCHECK(hipMemcpy(ix->tags + at, tags, sizeof(u32) * count, tags_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  if (ix->filter) {  // the new rows are allowed
    tail_set_bits_kernel<<<grid_for(filter_words(count) + 1, 256, 1024), 256>>>(ix->filter, at, at + count);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->filter_count += (long long)count;
  }
  ix->tail_m += count;
  return 0;
}
extern "C" size_t annhip_index_tail(const annhip_index *ix) { return ix->tail_m; }
extern "C" size_t annhip_index_tail_hashed(const annhip_index *ix) { return ix->tail_mh; }
extern "C" int annhip_index_fixed(const annhip_index *ix) { return ix->fixed; }
// what: 0 = the allow list, ceil(n_total/32) words; 1 = the tags, n_total words -> dst_dev; -1 where the index has none
extern "C" int annhip_index_copy_words(const annhip_index *ix, int what, uint32_t *dst_dev) {
  const u32 *src = what == 0 ? ix->filter : what == 1 ? ix->tags : NULL;
  if (!src) return -1;
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(dst_dev, src, sizeof(u32) * (what == 0 ? filter_words(n_total(ix)) : n_total(ix)), hipMemcpyDeviceToDevice));
  return 0;
}
extern "C" int annhip_index_drop_tail(annhip_index *ix) {
  if (!ix->tail_m) return 0;
  HIPCHECK(hipDeviceSynchronize());
  ix->tail_m = 0;
  drop_tail_hash(ix);
  drop_order(ix);  // it names tail rows
  if (ix->filter) filter_recount(ix);  // the bitmap and the tags are read up to n again
  return 0;
}
extern "C" int annhip_index_copy_rows(const annhip_index *ix, size_t lo, size_t hi, ftype *dst_dev) {
  if (ix->lo != 0 || ix->hi != ix->n || lo > hi || hi > n_total(ix)) {
    fprintf(stderr, "annhip_index_copy_rows: rows [%zu, %zu) outside 0..n_total = %zu, or a resharded index\n", lo, hi, n_total(ix));
    return -1;
  }
  HIPCHECK(hipDeviceSynchronize());
  FT *dst = reinterpret_cast<FT *>(dst_dev);
  const size_t d = ix->d, b_hi = std::min(hi, ix->n);
  if (lo < b_hi) HIPCHECK(hipMemcpy(dst, ix->d_points + lo * d, sizeof(FT) * (b_hi - lo) * d, hipMemcpyDeviceToDevice));
  const size_t t_lo = std::max(lo, ix->n);
  if (t_lo < hi)
    HIPCHECK(hipMemcpy(dst + (t_lo - lo) * d, ix->d_tail + (t_lo - ix->n) * d, sizeof(FT) * (hi - t_lo) * d, hipMemcpyDeviceToDevice));
  return 0;
}

extern "C" annhip_index *annhip_index_create(const save_t *save, const ftype *points, int on_device,
                                             size_t row_lo, size_t row_hi) {
  gpu_init();
  annhip_index *ix = new annhip_index();
  ix->n = save->n, ix->k = save->k, ix->d = save->d_long, ix->ds = save->d_short, ix->T = save->tries;
  check_limits(ix->n, ix->k, ix->d, ix->ds, ix->T);
  if (row_lo > row_hi || row_hi > ix->n) die("bad row range");
  ix->lo = row_lo, ix->hi = row_hi;
  const size_t rows = row_hi - row_lo;
  if (on_device) {
    ix->d_points = const_cast<FT *>(reinterpret_cast<const FT *>(points));
  } else {
    ix->d_points = dev_alloc<FT>(rows * ix->d);
    ix->own_points = true;
    HIPCHECK(hipMemcpy(ix->d_points, points, sizeof(FT) * rows * ix->d, hipMemcpyHostToDevice));
  }
  // bucket tables: size_t on the ABI, u32 in HBM
  const size_t nb = (size_t)1 << ix->ds;
  size_t max_tab = 0;
  for (int t = 0; t < ix->T; t++) max_tab = std::max(max_tab, nb * save->par_maxes[t]);
  size_t *stage = dev_alloc<size_t>(std::max(max_tab, ix->n * ix->k));
  ix->h_tries.resize(ix->T);
  ix->d_tabs.resize(ix->T);
  for (int t = 0; t < ix->T; t++) {
    const size_t cnt = nb * save->par_maxes[t];
    if (save->par_maxes[t] >= (1u << 20)) die("bucket too large");
    ix->d_tabs[t] = dev_alloc<u32>(cnt);
    HIPCHECK(hipMemcpy(stage, save->which_par[t], sizeof(size_t) * cnt, hipMemcpyHostToDevice));
    narrow_ids_kernel<<<grid_for(cnt, 256, 1u << 30), 256>>>(cnt, stage, ix->d_tabs[t]);
    ix->h_tries[t].tab = ix->d_tabs[t];
    ix->h_tries[t].pm = (u32)save->par_maxes[t];
  }
  ix->d_graph = dev_alloc<u32>(ix->n * ix->k);
  HIPCHECK(hipMemcpy(stage, save->graph, sizeof(size_t) * ix->n * ix->k, hipMemcpyHostToDevice));
  narrow_ids_kernel<<<grid_for(ix->n * ix->k, 256, 1u << 30), 256>>>(ix->n * ix->k, stage, ix->d_graph);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipFree(stage));
  ix->d_means = dev_alloc<FT>(ix->d);
  HIPCHECK(hipMemcpy(ix->d_means, save->row_means, sizeof(FT) * ix->d, hipMemcpyHostToDevice));
  ix->d_bases = dev_alloc<FT>((size_t)ix->T * ix->ds * ix->d);
  HIPCHECK(hipMemcpy(ix->d_bases, save->bases, sizeof(FT) * ix->T * ix->ds * ix->d, hipMemcpyHostToDevice));
  build_segments(ix);
  finish_geometry(ix);
  (void)prune_setup(ix, env().prune, "ANN_HIP_PRUNE=1");
  return ix;
}

extern "C" void annhip_index_reshard(annhip_index *ix, const ftype *shard_points_dev, size_t row_lo, size_t row_hi) {
  if (row_lo > row_hi || row_hi > ix->n) die("bad row range");
  HIPCHECK(hipDeviceSynchronize());
  drop_half_rows(ix);  // narrow rows are for the whole index on one device: a resharded index reads native rows
  drop_filter(ix);     // ... and so is the allow list
  drop_tags(ix);       // ... and the rows' tags
  ix->tail_m = 0;      // ... and the appended rows (the buffer stays)
  drop_tail_hash(ix);
  if (ix->own_points && ix->d_points) HIPCHECK(hipFree(ix->d_points));
  ix->own_points = false;
  ix->d_points = const_cast<FT *>(reinterpret_cast<const FT *>(shard_points_dev));
  ix->lo = row_lo, ix->hi = row_hi;
  build_segments(ix);  // the owned segment of every bucket moves with the row range
  HIPCHECK(hipMemcpy(ix->d_tries, ix->h_tries.data(), sizeof(TryInfo) * ix->T, hipMemcpyHostToDevice));
}

extern "C" void annhip_index_destroy(annhip_index *ix) {
  if (!ix) return;
  HIPCHECK(hipDeviceSynchronize());
  if (ix->own_points && ix->d_points) HIPCHECK(hipFree(ix->d_points));
  drop_half_rows(ix);
  drop_filter(ix);
  drop_tags(ix);
  if (ix->d_tail) HIPCHECK(hipFree(ix->d_tail));
  drop_tail_hash(ix);
  for (u32 *t : ix->d_tabs)
    if (t) HIPCHECK(hipFree(t));
  for (uint2 *sg : ix->d_segs)
    if (sg) HIPCHECK(hipFree(sg));
  for (uint4 *sg : ix->d_segx)
    if (sg) HIPCHECK(hipFree(sg));
  if (ix->d_tries) HIPCHECK(hipFree(ix->d_tries));
  if (ix->d_graph) HIPCHECK(hipFree(ix->d_graph));
  if (ix->d_means) HIPCHECK(hipFree(ix->d_means));
  if (ix->d_bases) HIPCHECK(hipFree(ix->d_bases));
  if (ix->d_graph_dists) HIPCHECK(hipFree(ix->d_graph_dists));
  if (ix->d_rows) HIPCHECK(hipFree(ix->d_rows));
  ix->ws.release();
  ix->io_y.release(), ix->io_ids.release(), ix->io_dist.release();
  ix->io_y_pin.release(), ix->io_out_pin.release();
  for (auto &e : ix->ev_used) (void)hipEventDestroy(e.a), (void)hipEventDestroy(e.b);
  for (auto &e : ix->ev_free) (void)hipEventDestroy(e.a), (void)hipEventDestroy(e.b);
  for (hipEvent_t e : ix->seg_free) (void)hipEventDestroy(e);
  for (auto &m : ix->seg_used)
    for (hipEvent_t e : m) (void)hipEventDestroy(e);
  delete ix;
}

extern "C" void annhip_index_info(const annhip_index *ix, size_t out[12]) {
  size_t v[12] = {ix->n, ix->k, ix->d, ix->ds, (size_t)ix->T, ix->L1, ix->P1, ix->Lc1, ix->L2, ix->P2, ix->Lc2, ix->sum_pm};
  memcpy(out, v, sizeof v);
}

extern "C" void annhip_index_export(const annhip_index *ix, save_t *save) {
  HIPCHECK(hipDeviceSynchronize());
  const size_t nb = (size_t)1 << ix->ds;
  save->tries = ix->T;
  save->n = ix->n, save->k = ix->k, save->d_short = ix->ds, save->d_long = ix->d;
  save->which_par = (size_t **)malloc(sizeof(size_t *) * ix->T);
  save->par_maxes = (size_t *)malloc(sizeof(size_t) * ix->T);
  size_t max_cnt = ix->n * ix->k;
  for (int t = 0; t < ix->T; t++) max_cnt = std::max(max_cnt, nb * ix->h_tries[t].pm);
  size_t *stage = dev_alloc<size_t>(max_cnt);
  for (int t = 0; t < ix->T; t++) {
    const size_t cnt = nb * ix->h_tries[t].pm;
    save->par_maxes[t] = ix->h_tries[t].pm;
    save->which_par[t] = (size_t *)malloc(sizeof(size_t) * cnt);
    widen_ids_kernel<<<grid_for(cnt, 256, 1u << 30), 256>>>(cnt, ix->d_tabs[t], stage);
    HIPCHECK(hipMemcpy(save->which_par[t], stage, sizeof(size_t) * cnt, hipMemcpyDeviceToHost));
  }
  save->graph = (size_t *)malloc(sizeof(size_t) * ix->n * ix->k);
  widen_ids_kernel<<<grid_for(ix->n * ix->k, 256, 1u << 30), 256>>>(ix->n * ix->k, ix->d_graph, stage);
  HIPCHECK(hipMemcpy(save->graph, stage, sizeof(size_t) * ix->n * ix->k, hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(stage));
  save->row_means = (ftype *)malloc(sizeof(FT) * ix->d);
  HIPCHECK(hipMemcpy(save->row_means, ix->d_means, sizeof(FT) * ix->d, hipMemcpyDeviceToHost));
  save->bases = (ftype *)malloc(sizeof(FT) * ix->T * ix->ds * ix->d);
  HIPCHECK(hipMemcpy(save->bases, ix->d_bases, sizeof(FT) * ix->T * ix->ds * ix->d, hipMemcpyDeviceToHost));
}

// ----------------------------------------------------------------------------- launchers
// Row layouts (ann_device.h): D > 0 = power of two (RowLay<D>); D < 0: d/VEC is oc * C chunks, C = 2^a <= 8, oc <= 64
// lanes per row (row_reduce_oc), -D = 16*OC + C with OC = oc where the layout is static (oc = 3 or 5, e.g. the reference
// drivers' default d = 80) and OC = 0 where oc comes at run time; D = 0 = any d (literal tree through LDS).
static int layout_code(size_t d, bool allow_oc = true) {
  if (d >= 16 && (d & (d - 1)) == 0 && d <= (sizeof(FT) == 4 ? 1024u : 512u)) return (int)d;
  bool static_oc = false;
  if (allow_oc && d % ANN_VEC == 0) {
    size_t nc = d / ANN_VEC, C = 1;
    while (C < 8 && nc % (2 * C) == 0) C *= 2;
    const size_t oc = nc / C;
#ifndef ANN_NO_STATIC_OC
    // 3 x 8 chunks as 6 lanes x 4 chunks, 5 x 8 as 10 x 4: half the registers per row buffer and twice as long
    // contiguous pieces per load instruction beat the lanes left idle (12 resp. 10 of the 16 lanes of a DPP row in use):
    // d = 96 float 40.5 (3 lanes x 8) -> 61.1 % of the HBM peak in stage 1, d = 160 51.7 (5 x 8) -> 69.0 % (N = 4M, Q = 10k)
    // (5 x 4 chunks as 10 x 2 -- d = 80 float -- was measured too and loses: 52.2 % against 68.7 %)
    if ((oc == 3 || oc == 5) && C == 8) return -(int)(16 * (2 * oc) + 4);
    if ((oc == 3 || oc == 5) && C >= 2) return -(int)(16 * oc + C);  // static layout, DPP-only tail (d = 80: oc = 5)
    if ((oc == 6 || oc == 10 || oc == 12) && C == 8) return -(int)(16 * oc + C);  // 3 x 16 / 5 x 16 / 3 x 32 chunks: d = 192 / 320 / 384 float
#endif
    static_oc = C > 2;  // many 16-byte chunks per lane: the aligned layout below beats the fold (d = 384: 4.0 vs 2.4 TB/s)
  }
#ifndef ANN_NO_FOLD
  // 2 or 3 tree levels folded into a lane (4 or 8 leaves; roughly 33 <= d <= 128): d = 100 float 0.76 -> 1.7 TB/s
  if (allow_oc && !static_oc && (d + ANN_VEC - 1) / ANN_VEC <= 64) {
    const int L = ann_fold_levels((int)d);
    if (L == 2) return ANN_D_FOLD2;
    if (L == 3) return ANN_D_FOLD3;
    // four levels (16 leaves) only where the rows are unaligned anyway: for aligned d the element loads of the OTHER
    // kernels cost what the gathers gain (d=136: stage 1 3.1 -> 2.8 ms but 2.7 -> 2.2 M q/s; d=250: 0.51 -> 1.0 M q/s)
    if (L == 4 && d % ANN_VEC != 0) return ANN_D_FOLD4;
  }
#endif
  if (allow_oc && d % ANN_VEC == 0) {
    size_t nc = d / ANN_VEC, C = 1;
    while (C < 8 && nc % (2 * C) == 0) C *= 2;
    const size_t oc = nc / C;
    if (oc >= 2 && oc <= 64) return -(int)C;
  }
#ifndef ANN_NO_UNALIGNED_LAYOUT
  // d not a multiple of the 16-byte chunk: ceil(d/VEC) lanes per row, element-wise loads, tree of length d
  if (allow_oc && d % ANN_VEC != 0 && (d + ANN_VEC - 1) / ANN_VEC >= 2 && (d + ANN_VEC - 1) / ANN_VEC <= 64) return ANN_D_UNALIGNED;
#endif
#ifndef ANN_NO_FOLD
  // no lanes-per-row layout at all (d = 300 float: 75 chunks; d = 150 double): the any-d code everywhere, but the
  // selection gathers fold 4 or 5 levels into a lane
  if (allow_oc) {
    const int L = ann_fold_levels((int)d);
    if (L == 4) return ANN_D_FOLD4G;
    if (L == 5) return ANN_D_FOLD5G;
  }
#endif
  return 0;
}
static bool layout_is_generic(int code) { return code == 0 || code == ANN_D_FOLD4G || code == ANN_D_FOLD5G; }

// The layout table: the codes the launchers instantiate kernels for.  A new row layout is one entry in QueryLayouts
// plus the case of layout_code() that returns it (its decoding lives in ann_device.h: RowLay / OcCode).
template <int... Vs>
struct Ints {};
template <int... A, int... B>
constexpr Ints<A..., B...> operator+(Ints<A...>, Ints<B...>) { return {}; }
// what layout_code(d, false) returns -- bucket-centric precomp, sharded stage-2 distances, recall: the powers of two
// (RowLay<D>; 4 KB rows in float only) and 0 (any d)
#ifdef USE_FLOAT
typedef Ints<16, 32, 64, 128, 256, 512, 1024, 0> Pow2Layouts;
#else
typedef Ints<16, 32, 64, 128, 256, 512, 0> Pow2Layouts;
#endif
// what layout_code(d) returns -- the query path: those and the lanes-per-row codes -(16*OC + C), element-wise and folded
typedef decltype(Pow2Layouts{} + Ints<-1, -2, -4, -8, -50, -52, -82, -84, -100, -104, -164, -168, -200, ANN_D_UNALIGNED,
                                      ANN_D_FOLD2, ANN_D_FOLD3, ANN_D_FOLD4, ANN_D_FOLD4G, ANN_D_FOLD5G>{}) QueryLayouts;

template <int V>
using Int = std::integral_constant<int, V>;
template <int... Vs>
static bool in_table(Ints<Vs...>, int v) { return ((v == Vs) || ...); }
// f(Int<V>{}) for the entry V == v: one instantiation of f per entry.  A value without an entry is a bug: it never
// falls back to another layout's kernels.
template <int... Vs, typename F>
static void with_value(Ints<Vs...>, int v, F &&f) {
  if (!((v == Vs && (f(Int<Vs>{}), true)) || ...)) die("no kernel instantiated for this layout code / template argument");
}

// The query kernels that read point rows come in two row types: f(TypeTag<RT>{}) with RT = RN (the library's narrow
// type: binary16 in the f32 library, binary32 in the f64 library) where QParams::points_h is set, and FT otherwise.
template <typename T>
struct TypeTag {
  typedef T type;
};
template <typename F>
static void with_rows(const QParams &P, F &&f) {
  if (P.points_h) return f(TypeTag<RN>{});
  f(TypeTag<FT>{});
}

// the code the query launchers dispatch for d, looked up through the table (INT_MIN: none)
extern "C" int annhip_layout_code(size_t d) {
  const int code = layout_code(d);
  return in_table(QueryLayouts{}, code) ? code : INT_MIN;
}

static bool d_is_fast(size_t d) { return layout_code(d, false) > 0; }   // power-of-two register layout
static bool d_needs_lds_row(size_t d) { return layout_is_generic(layout_code(d)); }    // literal tree through LDS

template <typename K>
static void allow_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) die("row too long for the LDS of one CU");
  if (bytes > 48 * 1024)
    HIPCHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// Qhash <= Q: only the first Qhash queries are hashed.  Stage 1 reads code[i*Q + x] for the tries i that own a
// slot below Lc1, i.e. flat indices below tries_used*Q, i.e. queries below ceil(tries_used*Q/T).
static void launch_codes(const QParams &P, size_t Qhash, const FT *y, u32 *codes, hipStream_t s, u32 *zero_me = NULL) {
  const int wpb = 4;
  const size_t Q = Qhash;
  const size_t items = Q * (size_t)P.T;
  if (!items) return;
  if (d_is_fast(P.d) && (size_t)P.d * sizeof(FT) <= 512 && env().codes_lpq) {  // a lane per query (codes_lpq_kernel)
    const size_t smem = sizeof(FT) * ((size_t)P.ds + 1) * P.d + sizeof(u32) * ANN_WAVE * ANN_LPQ_WAVES;
    const dim3 grid((unsigned)((Q + ANN_WAVE - 1) / ANN_WAVE), (unsigned)P.T);
    with_value(Pow2Layouts{}, layout_code(P.d, false), [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      if constexpr (D > 0 && D * sizeof(FT) <= 512) {
        allow_lds(codes_lpq_kernel<D>, smem);
        hipLaunchKernelGGL(codes_lpq_kernel<D>, grid, dim3(64 * ANN_LPQ_WAVES), smem, s, P, (int)Q, y, codes, zero_me);
      }
    });
  } else if (d_is_fast(P.d)) {  // workgroup = (try, run of queries); the try's projection rows live in LDS
    const size_t smem = sizeof(FT) * (size_t)P.ds * P.d;
    const dim3 grid((unsigned)((Q + ANN_CODES_QPB - 1) / ANN_CODES_QPB), (unsigned)P.T);
    with_value(Pow2Layouts{}, layout_code(P.d, false), [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      if constexpr (D > 0) {
        allow_lds(codes_kernel<D>, smem);
        hipLaunchKernelGGL(codes_kernel<D>, grid, dim3(64 * wpb), smem, s, P, (int)Q, y, codes, zero_me);
      }
    });
  } else {
    const unsigned grid = (unsigned)((items + wpb - 1) / wpb);
    const size_t smem = d_needs_lds_row(P.d) ? sizeof(FT) * wpb * 2 * (size_t)P.d : 0;
    with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      if constexpr (D <= 0) {
        allow_lds(codes_kernel<D>, smem);
        hipLaunchKernelGGL(codes_kernel<D>, dim3(grid), dim3(64 * wpb), smem, s, P, (int)Q, y, codes, zero_me);
      }
    });
  }
  HIPCHECK(hipGetLastError());
}

// waves per query: enough slots per wave to amortise the per-wave selection and merge; a shard gathers only part of
// each query's rows and sees G times the queries, and is better off with one wave per query (measured per-rank steps
// with 4 / 2 / 1 waves: 1.336 / 1.306 / 1.292 ms at 1/2 of the rows, 1.392 / 1.304 / 1.299 ms at 1/4; 1/8: 1.87 -> 1.55)
static int stage1_waves(u32 P1, double own_frac) {
  int w = (int)(P1 / ANN_S1_CHUNK);
  if (w < 1) w = 1;
  if (w > 4) w = 4;
  if (own_frac <= 0.5) w = 1;
  if (env().s1_waves) w = env().s1_waves;  // ANN_HIP_S1_WAVES; measured at cfg3: 4 = 2 (1.19 ms) < 8 (1.21) < 1 (1.28)
  return w;
}
static int stage1_cap(int W, int K1) {
  int cap = 256;
  if (cap < W * K1) cap = W * K1;
  if (cap < K1 + 128) cap = K1 + 128;
  return (cap + 63) & ~63;
}
// regs: stage1_select_kernel<..., REGS = true> -- no candidate buffers, one kout (wave 0's)
static size_t stage1_lds_bytes(const QParams &P, int W, int K1, int cap, u32 tail_len = 0, bool regs = false) {
  size_t b = sizeof(Key) * (regs ? 0 : (size_t)W * cap) + sizeof(Key) * (size_t)(regs ? 1 : W) * K1 +
             sizeof(Key) * (size_t)W * K1 + sizeof(TryInfo) * (size_t)P.T +
             sizeof(u32 *) * (size_t)W * ANN_WAVE + sizeof(u32) * (size_t)W * ANN_S1_CHUNK +
             sizeof(u32) * (size_t)W * ANN_WAVE + sizeof(u32) * (size_t)P.T + sizeof(int) * (size_t)W + sizeof(u32) * 4 +
             3 * sizeof(u32) * (size_t)tail_len;
  b = (b + 15) & ~(size_t)15;
  b += sizeof(FT) * (size_t)tail_len;
  b = (b + 15) & ~(size_t)15;
  if (d_needs_lds_row(P.d)) b += sizeof(FT) * (size_t)P.d * (1 + W);
  return b;
}

// hipMemsetAsync on 4 bytes cost ~100 us of stream time between kernels on ROCm 7.2; a one-thread kernel does not
__global__ void zero_u32_kernel(u32 *p) { *p = 0; }

__global__ void sum_u32_kernel(size_t count, const u32 *__restrict__ v, unsigned long long *out) {
  unsigned long long acc = 0;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x)
    acc += v[e];
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
  if (lane_id() == 0) atomicAdd(out, acc);
}

// the HIP-event pair around one stage-1 "launch" of a profiled index (s1_prof_end: and the gathered-row statistics)
static EventPair s1_prof_begin(annhip_index *ix, hipStream_t s) {
  EventPair ev;
  if (ix->ev_free.empty()) {
    HIPCHECK(hipEventCreate(&ev.a));
    HIPCHECK(hipEventCreate(&ev.b));
  } else {
    ev = ix->ev_free.back();
    ix->ev_free.pop_back();
  }
  HIPCHECK(hipEventRecord(ev.a, s));
  return ev;
}
static void s1_prof_end(annhip_index *ix, EventPair ev, size_t Q, const u32 *nvo, hipStream_t s) {
  HIPCHECK(hipEventRecord(ev.b, s));
  ix->ev_used.push_back(ev);
  // gathered-row statistics only while measuring: one small reduction kernel, outside the event bracket
  if (ix->profile == 1) sum_u32_kernel<<<grid_for(Q, 256, 64), 256, 0, s>>>(Q, nvo, ix->d_rows);
}

static void launch_stage1(annhip_index *ix, const QParams &P, size_t Q, const FT *y, int alias,
                          const u32 *codes, FT *cand_d, u32 *cand_i, u32 *nvt, u32 *nvo, hipStream_t s,
                          const std::vector<TryInfo> &h_tries, int use_seg, FusedTail F = FusedTail{0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL},
                          Key *cand_key = NULL, int pieces = 1, int slots = 0, size_t qstride = 0, int keys = 0,
                          bool bracket = true) {
  // qstride: stride of the try-major code array the kernel reads as codes[try * qstride + x] (0 = Q; a host that answers
  // a SLICE of a larger batch passes the whole batch's size and a code pointer offset to the slice, annhip_query_slice)
  // keys: distinct keys selected per query (0 = k + 1; the pruned stage 1 preselects more, F.enabled == 0 only)
  // bracket: false = the caller brackets this launch together with what follows it (s1_prof_begin / s1_prof_end)
  const int kq = (int)(qstride ? qstride : Q);
  if (!Q) return;
  if (keys && F.enabled) die("launch_stage1: a preselection has no fused tail");
  const int K1 = keys ? keys : P.k + 1, W = stage1_waves(P.P1, (double)(P.hi - P.lo) / (double)P.n), cap = stage1_cap(W, K1);
  // the running selection in registers where the layout's gather offers keys by ballot and the list fits two registers
  const bool regs = K1 <= ANN_SEL_REGS_KMAX && sel_regs_code(layout_code(P.d));
  const size_t smem = stage1_lds_bytes(P, W, K1, cap, F.enabled == 1 ? F.len2 : 0, regs);
  u32 runs_used = 0;  // (try, hamming neighbour) runs that start below P1, in slot order
  for (int t = 0; t < P.T; t++)
    for (int yy = 0; yy <= P.ds; yy++)
      if (h_tries[t].off + (u32)yy * h_tries[t].pm < P.P1) runs_used++;
  // slots > 0: a PERSISTENT grid that holds at most `slots` waves on every SIMD and walks the queries itself.  The
  // one-workgroup-per-query launch refills every freed wave slot at once, and a workgroup of several waves from another
  // stream -- the small kernels of the other in-flight batches, RCCL's collectives -- is then not placed until the
  // gather drains (measured: an RCCL kernel sat for 1.09 of a 1.25 ms gather, and the GPU then idled 0.45 ms per step
  // while the chain behind it ran).  With one slot per SIMD left alone they start at once.
  unsigned max_grid = 0xFFFFFFFFu;
  if (slots > 0) max_grid = std::max(1u, (unsigned)device_cus() * 4u * (unsigned)slots / (unsigned)W);
  EventPair ev;
  const bool prof = ix && ix->profile && bracket;
  if (prof) ev = s1_prof_begin(ix, s);
  // (Chaining the stage-1 launches of overlapping batches through an event was tried and is slower, 7.9 vs 8.3 M q/s:
  // letting consecutive gathers overlap is what hides the workgroup tail of each launch.)
  const size_t np = (size_t)std::max(1, std::min(pieces, 64)), per = (Q + np - 1) / np;
  with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
    with_rows(P, [&](auto rt) {
      auto launch_sel = [&](auto sg, auto fu, auto rg) {
        constexpr int D = decltype(dd)::value, SG = decltype(sg)::value;
        constexpr bool FU = decltype(fu)::value, RG = decltype(rg)::value;
        using RT = typename decltype(rt)::type;
        allow_lds(stage1_select_kernel<D, SG, FU, RT, RG>, smem);
        for (size_t a = 0; a < Q; a += per) {
          QParams Pp = P;
          Pp.q0 = (u32)a, Pp.qn = (u32)std::min(per, Q - a);
          hipLaunchKernelGGL((stage1_select_kernel<D, SG, FU, RT, RG>), dim3(std::min<unsigned>(Pp.qn, max_grid)), dim3(64 * W), smem,
                             s, Pp, kq, y, alias, codes, K1, cap, runs_used, cand_d, cand_i, nvt, nvo, F, cand_key);
        }
      };
      auto launch = [&](auto sg, auto fu) {
        if constexpr (sel_regs_layout<decltype(dd)::value>()) {
          if (regs) return launch_sel(sg, fu, std::true_type{});
        } else if (regs) {
          die("launch_stage1: register selection chosen for a layout without one");
        }
        launch_sel(sg, fu, std::false_type{});
      };
      if (use_seg == 2) launch(Int<2>{}, std::false_type{});
      else if (use_seg && F.enabled == 1) launch(Int<1>{}, std::true_type{});
      else if (use_seg) launch(Int<1>{}, std::false_type{});
      else if (F.enabled == 1) launch(Int<0>{}, std::true_type{});
      else launch(Int<0>{}, std::false_type{});
    });
  });
  HIPCHECK(hipGetLastError());
  if (prof) s1_prof_end(ix, ev, Q, nvo, s);
  if (ix) ix->s1_launches += 1;
}

#ifdef USE_FLOAT
// The second half of the pruned stage 1 (ann_prune_kernels.h): rescore the kp preselected candidates of every query on
// the native rows, certify, apply finalize1's test.  P: the native-row parameters.
static void launch_prune_rescore(annhip_index *ix, const QParams &P, size_t Q, const FT *y, int kp, const FT *pre_d,
                                 const u32 *pre_i, const u32 *nvt, u32 *nvo, u32 *top_i, FT *top_d, u32 *fl, u32 *d_fcount,
                                 FT *tie_d, u32 *tie_i, hipStream_t s) {
  if (!Q) return;
  if (kp < P.k + 1 || kp > ANN_PRUNE_KMAX || P.k + 1 > 32) die("launch_prune_rescore: preselection size out of range");
  PruneArgs A = {};
  A.points = P.points, A.y = y, A.pre_d = pre_d, A.pre_i = pre_i, A.nv_tot = nvt, A.nv_own = nvo;
  A.top_id = top_i, A.top_dist = top_d, A.flist = fl, A.fcount = d_fcount;
  A.exact_total = ix->d_rows + 2, A.uncertified = ix->d_rows + 4;
  A.tie_d = tie_d, A.tie_i = tie_i;
  A.E = ix->prune_E;
  A.n = P.n, A.Q = (u32)Q, A.L1 = P.L1, A.P1 = P.P1;
  A.d = P.d, A.k = P.k, A.Kp = kp;
  const dim3 grid((unsigned)((Q + ANN_PRUNE_WAVES - 1) / ANN_PRUNE_WAVES)), block(64 * ANN_PRUNE_WAVES);
  with_value(QueryLayouts{}, layout_code(P.d), [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    if constexpr (D != 0 && !OcCode<D>::GEN) hipLaunchKernelGGL(prune_rescore_kernel<D>, grid, block, 0, s, A);
    else die("launch_prune_rescore: no register layout for this row length");
  });
  HIPCHECK(hipGetLastError());
}
#endif

// ---- fixed mode with pair bits (annhip_index_set_probe; ann_probe_kernels.h)
// The hash kernels with the ranking: launch_codes' three forms, every query hashed; pbits u8[Q][T][pb].
static void launch_codes_probe(const QParams &P, size_t Q, const FT *y, u32 *codes, unsigned char *pbits, int pb, hipStream_t s,
                               u32 *zero_me = NULL) {
  const int wpb = ANN_PROBE_WPB;
  const size_t items = Q * (size_t)P.T;
  if (!items) return;
  if (pb < 1 || pb > P.ds || P.ds > 31) die("launch_codes_probe: pair bits outside 1..d_short");
  if (d_is_fast(P.d) && (size_t)P.d * sizeof(FT) <= 512 && env().codes_lpq) {  // a lane per query
    const size_t smem = sizeof(FT) * ((size_t)P.ds + 1) * P.d + sizeof(u32) * ANN_WAVE * ANN_LPQ_WAVES +
                        sizeof(UB) * (size_t)P.ds * ANN_WAVE;
    const dim3 grid((unsigned)((Q + ANN_WAVE - 1) / ANN_WAVE), (unsigned)P.T);
    with_value(Pow2Layouts{}, layout_code(P.d, false), [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      if constexpr (D > 0 && D * sizeof(FT) <= 512) {
        allow_lds(codes_probe_lpq_kernel<D>, smem);
        hipLaunchKernelGGL(codes_probe_lpq_kernel<D>, grid, dim3(64 * ANN_LPQ_WAVES), smem, s, P, (int)Q, y, codes, zero_me, pb, pbits);
      }
    });
  } else if (d_is_fast(P.d)) {  // workgroup = (try, run of queries); the try's projection rows live in LDS
    const size_t smem = sizeof(FT) * (size_t)P.ds * P.d;
    const dim3 grid((unsigned)((Q + ANN_CODES_QPB - 1) / ANN_CODES_QPB), (unsigned)P.T);
    with_value(Pow2Layouts{}, layout_code(P.d, false), [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      if constexpr (D > 0) {
        allow_lds(codes_probe_kernel<D>, smem);
        hipLaunchKernelGGL(codes_probe_kernel<D>, grid, dim3(64 * wpb), smem, s, P, (int)Q, y, codes, zero_me, pb, pbits);
      }
    });
  } else {
    const unsigned grid = (unsigned)((items + wpb - 1) / wpb);
    const size_t smem = d_needs_lds_row(P.d) ? sizeof(FT) * wpb * 2 * (size_t)P.d : 0;
    with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      if constexpr (D <= 0) {
        allow_lds(codes_probe_kernel<D>, smem);
        hipLaunchKernelGGL(codes_probe_kernel<D>, dim3(grid), dim3(64 * wpb), smem, s, P, (int)Q, y, codes, zero_me, pb, pbits);
      }
    });
  }
  HIPCHECK(hipGetLastError());
}

static size_t stage1_probe_lds_bytes(const QParams &P, int W, int K1, int cap, int pb) {
  size_t b = sizeof(Key) * (size_t)W * cap + 2 * sizeof(Key) * (size_t)W * K1 + sizeof(TryInfo) * (size_t)P.T +
             sizeof(u32 *) * (size_t)W * ANN_WAVE + sizeof(u32) * (size_t)W * ANN_S1_CHUNK +
             sizeof(u32) * (size_t)W * ANN_WAVE + sizeof(u32) * (size_t)P.T + sizeof(int) * (size_t)W + sizeof(u32) * 4 +
             (size_t)P.T * pb;
  b = (b + 15) & ~(size_t)15;
  if (d_needs_lds_row(P.d)) b += sizeof(FT) * (size_t)P.d * (1 + W);
  return b;
}

// The per-query tag predicate of one annhip_query_tagged call (ann_tag_kernels.h): the rows' tag words and the batch's
// (mask, lo, hi) arrays, all on the device: qlo <= (tag & qmask) <= qhi.  The pair form (mask, value) is qlo = qhi = its
// value array (tag_pair), the range form (annhip_query_between) gives the three apart; the kernels are the same.
struct TagQuery {
  const u32 *tags, *qmask, *qlo, *qhi;
};
static TagQuery tag_pair(const u32 *tags, const u32 *qmask, const u32 *qvalue) { return TagQuery{tags, qmask, qvalue, qvalue}; }

// Stage 1 of fixed mode over 1 + ds + pb (pb - 1) / 2 buckets per try (pb = 0: the plain 1 + ds, no ranked bits), for
// every family that walks the (try, mask) runs (stage1_fixed_body in ann_probe_kernels.h and its two copies): with a radius
// stage1_radius_kernel (bits and tq may each be NULL), else with tq stage1_tag_kernel (bits may be NULL), else with bits
// stage1_filter_kernel, else stage1_probe_kernel.  Waves per query from the RUN count: a run holds at most par_maxes[t]
// ids, and a wave should see about a list (ANN_S1_CHUNK) of them to amortise its selection and the merge -- the rule
// stage1_waves applies to P1, which says nothing about the pair runs.
static void launch_stage1_fixed(annhip_index *ix, const QParams &P, size_t Q, const FT *y, int alias, const u32 *codes,
                                const unsigned char *pbits, int pb, const u32 *bits, const TagQuery *tq, const FT *radius,
                                FT *cand_d, u32 *cand_i, u32 *nvt, u32 *nvo, hipStream_t s) {
  if (!Q) return;
  const u32 rpt = 1u + (u32)P.ds + (u32)(pb * (pb - 1) / 2);
  size_t slots = 0;
  for (int t = 0; t < P.T; t++) slots += (size_t)rpt * ix->h_tries[t].pm;
  int W = (int)std::min<size_t>(4, std::max<size_t>(1, slots / ANN_S1_CHUNK));
  if (env().s1_waves) W = env().s1_waves;
  const int K1 = P.k + 1, cap = stage1_cap(W, K1);
  const size_t smem = stage1_probe_lds_bytes(P, W, K1, cap, pb);
  const u32 *tags = tq ? tq->tags : NULL, *qmask = tq ? tq->qmask : NULL, *qlo = tq ? tq->qlo : NULL, *qhi = tq ? tq->qhi : NULL;
  EventPair ev;
  if (ix->profile) ev = s1_prof_begin(ix, s);
  with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
    with_rows(P, [&](auto rt) {
      auto launch = [&](auto sg) {
        constexpr int D = decltype(dd)::value;
        constexpr bool SG = decltype(sg)::value;
        using RT = typename decltype(rt)::type;
        const dim3 grid((unsigned)Q), block(64 * W);
        if (radius) {
          allow_lds(stage1_radius_kernel<D, SG, RT>, smem);
          hipLaunchKernelGGL((stage1_radius_kernel<D, SG, RT>), grid, block, smem, s, P, y, alias, codes, pbits, pb, rpt, radius,
                             tags, bits, qmask, qlo, qhi, K1, cap, cand_d, cand_i, nvt, nvo);
        } else if (tq) {
          allow_lds(stage1_tag_kernel<D, SG, RT>, smem);
          hipLaunchKernelGGL((stage1_tag_kernel<D, SG, RT>), grid, block, smem, s, P, y, alias, codes, pbits, pb, rpt, tags, bits,
                             qmask, qlo, qhi, K1, cap, cand_d, cand_i, nvt, nvo);
        } else if (bits) {
          allow_lds(stage1_filter_kernel<D, SG, RT>, smem);
          hipLaunchKernelGGL((stage1_filter_kernel<D, SG, RT>), grid, block, smem, s, P, y, alias, codes, pbits, pb, rpt, bits, K1,
                             cap, cand_d, cand_i, nvt, nvo);
        } else {
          allow_lds(stage1_probe_kernel<D, SG, RT>, smem);
          hipLaunchKernelGGL((stage1_probe_kernel<D, SG, RT>), grid, block, smem, s, P, y, alias, codes, pbits, pb, rpt, K1, cap,
                             cand_d, cand_i, nvt, nvo);
        }
      };
      if (ix->use_seg) launch(std::true_type{});
      else launch(std::false_type{});
    });
  });
  HIPCHECK(hipGetLastError());
  if (ix->profile) s1_prof_end(ix, ev, Q, nvo, s);
  ix->s1_launches += 1;
}

// bucket-centric stage 1 of precomp: returns false when the shape does not fit (caller uses the per-point kernel)
static bool launch_stage1_bucket(const QParams &P, const TryInfo &one, size_t nbuckets, FT *cand_d, u32 *cand_i, u32 *nvt,
                                 u32 *nvo, hipStream_t s, u32 brem = 0, u32 bmod = 1) {
  if (!d_is_fast(P.d) || env().point_precomp) return false;
  const int K1 = P.k + 1, W = K1 > ANN_WAVE ? ANN_BK_WAVES_HI : ANN_BK_WAVES;
  if (K1 > 2 * ANN_WAVE) return false;  // the wave-resident selection holds one or two keys per lane
  const size_t ch = P.d / ANN_VEC, trows = std::max<size_t>(ANN_BK_TILE_CHUNKS / ch, 8);
  const size_t tile = sizeof(VT) * trows * (ch + 1);
  if (P.ds + 1 > ANN_BK_MAX_RUNS) return false;
  const u32 list_cap = std::min<u32>(P.P1, (u32)(P.ds + 1) * one.pm);
  const size_t fixed = tile + sizeof(u32) * (size_t)list_cap + sizeof(u32) * (ANN_BK_MAX_RUNS + 1) + 16;
  const size_t budget = 80 * 1024;  // keep two workgroups per CU
  if (fixed + sizeof(Key) * (size_t)K1 * W > budget) return false;
  // members whose K1-key lists fit beside the tile; more members than that walk the tiles once per group
  u32 mgroup = (u32)std::min<size_t>(one.pm, (budget - fixed) / (sizeof(Key) * (size_t)K1));
  if (env().bk_group) mgroup = (u32)std::min<size_t>(mgroup, std::max<size_t>(env().bk_group, (size_t)W));
  const size_t smem = fixed + sizeof(Key) * (size_t)mgroup * K1;
  if ((u32)P.k > P.P1) return false;
  with_value(Pow2Layouts{}, layout_code(P.d, false), [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    if constexpr (D > 0) {
      auto launch = [&](auto hi) {
        constexpr bool HI = decltype(hi)::value;
        allow_lds((stage1_bucket_kernel<D, HI>), smem);
        hipLaunchKernelGGL((stage1_bucket_kernel<D, HI>), dim3((unsigned)nbuckets), dim3(64 * W), smem, s, P, K1, list_cap,
                           mgroup, cand_d, cand_i, nvt, nvo, brem, bmod);
      };
      if (K1 <= ANN_WAVE) launch(std::false_type{});
      else launch(std::true_type{});
    }
  });
  HIPCHECK(hipGetLastError());
  return true;
}

static size_t rows_lds_bytes(const QParams &P, u32 chunk) {
  size_t b = 2 * sizeof(u32) * (size_t)chunk + sizeof(TryInfo) * (size_t)P.T + sizeof(u32) * (size_t)P.T + 16;
  b = (b + 15) & ~(size_t)15;
  if (d_needs_lds_row(P.d)) b += sizeof(FT) * (size_t)P.d * (1 + 4);
  return b;
}

template <int MODE>
static void launch_rows(const QParams &P, size_t Q, const FT *y, int alias, const u32 *codes, const u32 *qidx,
                        u32 xbase, size_t nq, u32 len, const u32 *top_i, const FT *top_d, u32 *ids, FT *dist,
                        unsigned long long *rows_done, hipStream_t s, const u32 *live_rows = NULL, u32 live_off = 0,
                        size_t qstride = 0) {
  if (!nq) return;
  const int kq = (int)(qstride ? qstride : Q);  // stride of the code array (see launch_stage1)
  // long rows (exact path, a handful of rows) are split over up to 8 workgroups; short rows get one
  // (device-driven launches expect a handful of rows, each on a step's critical path: 32 workgroups per row)
  const unsigned split = len >= 1024 ? (live_rows ? 32 : 8) : 1;
  u32 chunk = len < ANN_RD_CHUNK ? ((len + 63u) & ~63u) : ANN_RD_CHUNK;  // LDS lists sized to the row
  if (split > 1) chunk = std::max<u32>(live_rows ? 128 : 256, (((len + split - 1) / split) + 63u) & ~63u);
  if (chunk > ANN_RD_CHUNK) chunk = ANN_RD_CHUNK;
  const size_t smem = rows_lds_bytes(P, chunk);
  // short rows (stage 2 at small k): fewer waves per row, more rows resident per CU
  const unsigned block = len <= 128 ? 128 : 256;
  // device-driven: a flat persistent grid over (row, part) items (see the kernel); otherwise one workgroup per (row, part)
  const unsigned flat = live_rows ? split : 0;
  const dim3 grid = live_rows ? dim3((unsigned)std::min<size_t>(nq * split, 512)) : dim3((unsigned)nq, split);
  with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
    with_rows(P, [&](auto rt) {
      constexpr int D = decltype(dd)::value;
      using RT = typename decltype(rt)::type;
      allow_lds(row_dists_kernel<D, MODE, RT>, smem);
      hipLaunchKernelGGL((row_dists_kernel<D, MODE, RT>), grid, dim3(block), smem, s, P, kq, y, alias, codes, qidx, xbase, len,
                         top_i, top_d, ids, dist, rows_done, live_rows, (u32)nq, chunk, live_off, flat);
    });
  });
  HIPCHECK(hipGetLastError());
}

// network + rdups + network on nq rows of reference length L, `len` stored entries, row stride in_stride.
// tie: stage 1's candidate lists of the rows' queries -- rows with one run of tied distances are answered from their
// class bits by wave 0 (ann_tie.h), the others by the network (ANN_HIP_TIE=0: always the network).
static void launch_exact_select(u32 L, u32 len, u32 in_stride, int k, size_t nq, u32 *ids, FT *dist,
                                const u32 *qidx, u32 xbase, u32 *out_i, FT *out_d, int ostride, int ooff,
                                hipStream_t s, const u32 *live_rows = NULL, size_t *out64 = NULL, unsigned max_block = 1024,
                                u32 live_off = 0, TieArgs tie = TieArgs{NULL, NULL, 0, NULL, 0}) {
  if (!nq) return;
  const int lk = ann_lg(L);
  unsigned npairs = 8u << (lk > 4 ? lk - 4 : 0);
  // one pair per thread up to max_block.  1024 threads is the fastest shape on an idle GPU, but a 16-wave workgroup
  // cannot be placed while a saturating kernel of 1-wave workgroups keeps taking every freed slot (measured: 0.1 ms
  // alone, 1.1 ms = until the gather drained, next to the sharded stage 1): launches that run beside gathers use 256.
  // Device-driven launches (normally nothing or a row or two to do, often beside other batches' kernels) use 256 too:
  // with the tie path's registers a 16-wave workgroup needs a nearly empty CU, and even the launch that finds nothing to
  // do has to be PLACED -- behind the stage-1 kernels of the other in-flight batches it serialised a three-lane
  // pipeline of 1k-query batches (51 -> 86 us per batch).  The tie path scans a row with four waves just as well.
  if (live_rows) max_block = std::min(max_block, 256u);
  unsigned block = npairs >= max_block ? max_block : ((npairs + 63) / 64) * 64;
  if (block < 64) block = 64;
  const size_t row_smem = (size_t)len * (sizeof(FT) + sizeof(u32));
  // device-driven: a persistent grid of 128 workgroups (a launch of 512 x 16 waves that finds nothing to do cost ~10 us)
  const unsigned grid = live_rows ? (unsigned)std::min<size_t>(nq, 128) : (unsigned)nq;
  const bool in_lds = row_smem <= env().lds_row_max;  // the whole row in LDS (a CU has 160 KB); longer rows sort in place in HBM
  const u32 Pn = (u32)1 << lk;
  int nw = 0;
  if ((tie.cand_d || tie.derive) && env().tie && L >= 16 && tie.K1 == k + 1 && tie.K1 <= ANN_WAVE && (u32)k <= Pn)
    nw = Pn <= 4096 ? 1 : Pn <= 8192 ? 2 : Pn <= 16384 ? 4 : 0;
  size_t tie_smem = nw ? ann_tie_lds_bytes(nw) : 0;
  if (nw && tie.derive) tie_smem += ann_tie_derive_bytes(Pn);  // a list derived from the row: its keys live in LDS
  if (tie_smem > 150 * 1024) nw = 0;
  if (!nw) tie = TieArgs{NULL, NULL, 0, NULL, 0}, tie_smem = 0;
  const size_t smem = std::max(in_lds ? row_smem : (size_t)0, tie_smem);
  auto launch = [&](auto lds, auto nwc) {
    constexpr bool LDS = decltype(lds)::value;
    constexpr int NW = decltype(nwc)::value;
    allow_lds((exact_select_kernel<LDS, NW>), smem);
    hipLaunchKernelGGL((exact_select_kernel<LDS, NW>), dim3(grid), dim3(block), smem, s, L, len, in_stride, k, ids, dist, qidx,
                       xbase, out_i, out_d, ostride, ooff, live_rows, (u32)nq, out64, live_off, tie);
  };
  with_value(Ints<0, 1, 2, 4>{}, nw, [&](auto nwc) {
    if (in_lds) launch(std::true_type{}, nwc);
    else launch(std::false_type{}, nwc);
  });
  HIPCHECK(hipGetLastError());
}

// the whole of stage 2 for queries [xbase, xbase + nq) in one launch (needs Lc2 <= 1024: the row lives in LDS)
template <typename IdOut>
static void launch_stage2_fused(const QParams &P, size_t Q, const FT *y, int alias, u32 xbase, size_t nq, const u32 *top_i,
                                const FT *top_d, IdOut *out_ids, FT *out_d, unsigned long long *rows_ctr, hipStream_t s) {
  if (!nq) return;
  size_t smem = sizeof(Key) * (size_t)P.k + 3 * sizeof(u32) * (size_t)P.Lc2 + 16;
  smem = (smem + 15) & ~(size_t)15;
  smem += sizeof(FT) * (size_t)P.Lc2;
  smem = (smem + 15) & ~(size_t)15;
  if (d_needs_lds_row(P.d)) smem += sizeof(FT) * (size_t)P.d * 3;
  with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
    with_rows(P, [&](auto rt) {
      constexpr int D = decltype(dd)::value;
      using RT = typename decltype(rt)::type;
      allow_lds((stage2_fused_kernel<D, IdOut, RT>), smem);
      hipLaunchKernelGGL((stage2_fused_kernel<D, IdOut, RT>), dim3((unsigned)nq), dim3(env().s2_threads), smem, s, P, (int)Q, y,
                         alias, top_i, top_d, P.Lc2, out_ids, out_d, rows_ctr, xbase);
    });
  });
  HIPCHECK(hipGetLastError());
}

// Stage 2 by selection for queries [xbase, xbase + nq) (stage2_select_kernel), then the literal path for the rows it
// flagged (device-driven: the flagged list is walked in passes of a bounded workspace, a pass beyond the device-side
// count exits at once).  out32 / out64: exactly one is non-NULL (precomp's graph rows / query() ids); both are indexed
// by the global row x.  Returns false -- nothing launched -- when the shape is not taken (the caller runs the classic path).
static bool stage2_select_with_fallback(const QParams &P, size_t Q, const FT *y, int alias, u32 xbase, size_t nq,
                                        const u32 *top_i, const FT *top_d, u32 *out32, size_t *out64, FT *out_d,
                                        DevBuf &flist, u32 *d_fcount, DevBuf &r2i, DevBuf &r2d,
                                        unsigned long long *exact_total, unsigned long long *rows_ctr, hipStream_t s,
                                        const u32 *filter = NULL, const TagQuery *tq = NULL) {
  // filter: fixed mode's allow list (stage2_filter_kernel); tq: a tagged query's predicate (stage2_tag_kernel)
  if (!nq) return true;
  if ((filter || tq) && !P.fixed) die("stage2_select_with_fallback: an allow list or a tag predicate needs fixed mode");
  const int K1 = P.k + 1, W = 4, cap = stage1_cap(W, K1);
  const u32 P2 = (P.L2 < 16 || P.fixed) ? P.L2 : (u32)1 << ann_lg(P.L2);
  size_t smem = sizeof(Key) * (size_t)W * cap + 2 * sizeof(Key) * (size_t)W * K1 + sizeof(Key) * (size_t)P.k +
                sizeof(u32) * (size_t)W * ANN_S1_CHUNK + sizeof(int) * (size_t)W + sizeof(u32) * 4;
  smem = (smem + 15) & ~(size_t)15;
  if (d_needs_lds_row(P.d)) smem += sizeof(FT) * (size_t)P.d * (1 + W);
  const size_t row_bytes = (size_t)P.Lc2 * (sizeof(FT) + sizeof(u32));
  const size_t chunk = std::max<size_t>(1, ((size_t)1 << 30) / row_bytes);
  if ((u32)P.k >= P2 || smem > 150 * 1024 || nq > 64 * chunk) return false;
  u32 *fl = (u32 *)flist.need(sizeof(u32) * nq);
  zero_u32_kernel<<<1, 1, 0, s>>>(d_fcount);
  with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
    with_rows(P, [&](auto rt) {
      auto launch = [&](auto *out) {  // the id type of the output rows: size_t (query()) or u32 (precomp's graph)
        constexpr int D = decltype(dd)::value;
        using RT = typename decltype(rt)::type;
        using TT = std::remove_pointer_t<decltype(out)>;
        if (tq) {
          allow_lds((stage2_tag_kernel<D, TT, RT>), smem);
          hipLaunchKernelGGL((stage2_tag_kernel<D, TT, RT>), dim3((unsigned)nq), dim3(64 * W), smem, s, P, (int)Q, y, alias,
                             top_i, top_d, tq->tags, filter, tq->qmask, tq->qlo, tq->qhi, P2, K1, cap, out, out_d, fl, d_fcount,
                             exact_total, rows_ctr, xbase);
          return;
        }
        if (filter) {
          allow_lds((stage2_filter_kernel<D, TT, RT>), smem);
          hipLaunchKernelGGL((stage2_filter_kernel<D, TT, RT>), dim3((unsigned)nq), dim3(64 * W), smem, s, P, (int)Q, y, alias,
                             top_i, top_d, filter, P2, K1, cap, out, out_d, fl, d_fcount, exact_total, rows_ctr, xbase);
          return;
        }
        allow_lds((stage2_select_kernel<D, TT, RT>), smem);
        hipLaunchKernelGGL((stage2_select_kernel<D, TT, RT>), dim3((unsigned)nq), dim3(64 * W), smem, s, P, (int)Q, y, alias,
                           top_i, top_d, P2, K1, cap, out, out_d, fl, d_fcount, exact_total, rows_ctr, xbase);
      };
      if (out64) launch(out64);
      else launch(out32);
    });
  });
  HIPCHECK(hipGetLastError());
  if (P.fixed) return true;  // nothing is ever flagged: the selection IS the result
  const size_t R = std::min(nq, chunk);
  u32 *ri = (u32 *)r2i.need(sizeof(u32) * R * P.Lc2);
  FT *rd = (FT *)r2d.need(sizeof(FT) * R * P.Lc2);
  for (size_t p0 = 0; p0 < nq; p0 += R) {
    const size_t np = std::min(R, nq - p0);
    launch_rows<MODE_GRAPH>(P, Q, y, alias, NULL, fl + p0, 0, np, P.Lc2, top_i, top_d, ri, rd, rows_ctr, s, d_fcount, (u32)p0);
    launch_exact_select(P.L2, P.Lc2, P.Lc2, P.k, np, ri, rd, fl + p0, 0, out32, out_d, P.k, 0, s, d_fcount, out64, 1024,
                        (u32)p0);
  }
  return true;
}

// finalize + exact fallback for the queries finalize1 rejected.  The top-k lands in top_i/top_d
// (row stride ostride, column offset ooff).  device_driven: no host read-back -- the exact-path kernels are
// launched over the worst case (every query rejected) and rows beyond the device-side count exit at once;
// used when the worst-case workspace is affordable (query batches).  Otherwise (precomp: millions of rows) the
// count is read back and the exact path runs in bounded chunks.  Returns the number of exact-path rows when it
// is known on the host (-1 when device-driven).
static long finalize_and_fallback(annhip_index *ix, const QParams &P, size_t Q, const FT *y, int alias,
                                  const u32 *codes, int mode, const FT *cand_d, const u32 *cand_i,
                                  const u32 *nvt, u32 *top_i, FT *top_d, int ostride, int ooff, DevBuf &flist,
                                  DevBuf &xids, DevBuf &xd, u32 *d_fcount, unsigned long long *rows_done,
                                  unsigned long long *exact_total, bool device_driven, hipStream_t s, size_t qstride = 0,
                                  bool prefinalized = false, bool lists_may_be_empty = false) {
  // prefinalized: stage 1 applied finalize1's test itself (FusedTail.enabled == 2, or the pruned stage 1's rescore): flist / *d_fcount / top_* are set
  // lists_may_be_empty (the pruned stage 1): a flagged query that was not certified has no exact candidate list -- its
  // list is empty and the tie path derives one from the row, as the staged API does (cand_d == NULL: for every row)
  const int K1 = P.k + 1;
  unsigned long long *tie_ctr = ix ? ix->d_rows + 3 : NULL;
  const TieArgs tie0 = cand_d ? TieArgs{cand_d, cand_i, K1, tie_ctr, lists_may_be_empty ? 1 : 0} : TieArgs{NULL, NULL, K1, tie_ctr, 1};
  u32 nflag = 0;
  u32 *fl = (u32 *)flist.need(sizeof(u32) * Q);
  const size_t row_bytes = (size_t)P.Lc1 * (sizeof(FT) + sizeof(u32));
  size_t chunk = env().exact_bytes / (row_bytes ? row_bytes : 1);
  if (chunk < 1) chunk = 1;
  if (mode == 0) {
    if (!prefinalized) {
      zero_u32_kernel<<<1, 1, 0, s>>>(d_fcount);
      hipLaunchKernelGGL(finalize1_kernel, dim3(grid_for(Q, 256, 1u << 30)), dim3(256), 0, s, (int)Q, P.k, K1, P.L1,
                         P.P1, cand_d, cand_i, nvt, top_i, top_d, ostride, ooff, fl, d_fcount, exact_total);
      HIPCHECK(hipGetLastError());
    }
    if (device_driven && Q <= 8 * chunk) {
      // The workspace holds R = min(Q, chunk) rows; the flagged list is walked in passes of R entries, each pass
      // device-driven (a pass beyond the device-side count exits at once: two empty launches).  One pass covers
      // every query batch up to 32k queries at cfg3's row length; cfg4's Q = 100k takes 4, cfg5 (196 KB rows) 2 --
      // the step stays asynchronous there too (it used to fall back to a host read-back).
      const size_t R = std::min(Q, chunk);
      u32 *ids = (u32 *)xids.need(sizeof(u32) * R * P.Lc1);
      FT *dist = (FT *)xd.need(sizeof(FT) * R * P.Lc1);
      for (size_t p0 = 0; p0 < Q; p0 += R) {
        const size_t nq = std::min(R, Q - p0);
        launch_rows<MODE_TABLE>(P, Q, y, alias, codes, fl + p0, 0, nq, P.Lc1, NULL, NULL, ids, dist, rows_done, s, d_fcount,
                                (u32)p0, qstride);
        launch_exact_select(P.L1, P.Lc1, P.Lc1, P.k, nq, ids, dist, fl + p0, 0, top_i, top_d, ostride, ooff, s, d_fcount,
                            NULL, 1024, (u32)p0, tie0);
      }
      return -1;
    }
    HIPCHECK(hipMemcpyAsync(&nflag, d_fcount, sizeof(u32), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  } else {
    nflag = (u32)Q;
    if (exact_total) {
      unsigned long long add = Q, cur = 0;
      HIPCHECK(hipMemcpyAsync(&cur, exact_total, sizeof cur, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      cur += add;
      HIPCHECK(hipMemcpyAsync(exact_total, &cur, sizeof cur, hipMemcpyHostToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
  }
  for (size_t q0 = 0; q0 < nflag; q0 += chunk) {  // exact path in bounded chunks of rows
    const size_t nq = std::min(chunk, (size_t)nflag - q0);
    u32 *ids = (u32 *)xids.need(sizeof(u32) * nq * P.Lc1);
    FT *dist = (FT *)xd.need(sizeof(FT) * nq * P.Lc1);
    const u32 *qidx = mode == 0 ? fl + q0 : NULL;
    launch_rows<MODE_TABLE>(P, Q, y, alias, codes, qidx, (u32)q0, nq, P.Lc1, NULL, NULL, ids, dist, rows_done, s, NULL, 0, qstride);
    launch_exact_select(P.L1, P.Lc1, P.Lc1, P.k, nq, ids, dist, qidx, (u32)q0, top_i, top_d, ostride, ooff, s, NULL, NULL, 1024,
                        0, mode == 0 ? tie0 : TieArgs{NULL, NULL, 0, NULL, 0});
  }
  return (long)nflag;
}

static void seg_mark(annhip_index *ix, std::vector<hipEvent_t> *marks, hipStream_t s) {
  if (!marks) return;
  hipEvent_t e;
  if (ix->seg_free.empty()) {
    HIPCHECK(hipEventCreate(&e));
  } else {
    e = ix->seg_free.back();
    ix->seg_free.pop_back();
  }
  HIPCHECK(hipEventRecord(e, s));
  marks->push_back(e);
}

// Stage 1 reads code[i*Q + x] for the tries i that own a slot below Lc1, i.e. flat indices below
// tries_used*Q of the [q*T+t] array, i.e. the codes of queries below ceil(tries_used*Q/T): only those are hashed.
static size_t codes_needed(const annhip_index *ix, size_t Q) {
  if (ix->fixed) return Q;
  int tries_used = 0;
  while (tries_used < ix->T && ix->h_tries[tries_used].off < ix->Lc1) tries_used++;
  return std::min(Q, ((size_t)tries_used * Q + ix->T - 1) / ix->T);
}

// the exact scan of the appended rows, merged into the rows a fixed-mode call has produced (defined with the exact scan)
static void launch_tail_merge(annhip_index *ix, size_t Q, const FT *y, int alias, size_t k, const TagQuery *tq, size_t kin,
                              const size_t *in_ids, const FT *in_d, size_t *ids, FT *dists, unsigned long long *scored,
                              hipStream_t s, size_t skip = 0);
// the hashed tail rows of the buckets the call probes, merged in place into the rows it has produced (likewise)
static void launch_tail_hash_merge(annhip_index *ix, size_t Q, const FT *y, size_t k, const TagQuery *tq, const u32 *codes,
                                   const unsigned char *pbits, int pb, size_t *ids, FT *dists, unsigned long long *scored,
                                   hipStream_t s);
static void launch_radius_trim(size_t Q, size_t kcap, size_t pad_id, const FT *radius, size_t *ids, FT *dists, u32 *counts,
                               hipStream_t s);
// What a grouped call adds to its list of kq = L entries: the collapse (ann_group_kernels.h) into the caller's [Q][k].
struct GroupCall {
  size_t k, per_group;
  u32 gmask;
  u32 *counts;           // may be NULL
  unsigned char *shrt;   // may be NULL
};
static void launch_collapse(size_t Q, size_t L, const GroupCall &g, const u32 *tags, size_t rows, size_t pad_id, const size_t *ids_in,
                            const FT *dists_in, size_t *ids_out, FT *dists_out, hipStream_t s);

// How a call of the query path ends: the marks padded to the seven that annhip_stats reads (a path with fewer stages
// leaves its last segments at zero) and handed over, and the index's counter.
static void finish_call(annhip_index *ix, std::vector<hipEvent_t> *marks, hipStream_t s, size_t Q) {
  while (marks && marks->size() < 7) seg_mark(ix, marks, s);
  if (marks) ix->seg_used.push_back(*marks);
  ix->queries += (double)Q;
}

// What the entries of fixed mode ask of fixed_query (defined below the stage 2 of a per-call k).
struct FixedCall {
  size_t kq;           // the k of the call: sizes K1 and every buffer
  bool stage2_kq;      // false: kq == ix->k and the index's own selection path; true: stage2_kq_kernel, whatever kq is
  const TagQuery *tq;  // the tag family of stage 1 and stage 2, or NULL
  const FT *radius;    // annhip_query_radius / _between: stage1_radius_kernel and the trim with counts; stage2_kq only
  u32 *counts;
  const GroupCall *group;  // annhip_query_grouped: the [Q][kq] result goes to the workspace, its collapse to the caller; or NULL
};
static long fixed_query(annhip_index *ix, annhip_workspace &ws, hipStream_t s, size_t Q, const ftype *y_dev, int alias,
                        const FixedCall &c, size_t *ids_dev, ftype *dists_dev, int codes_ready = 0);

// ----------------------------------------------------------------------------- query
// codes_ready: ws.codes already holds the hash codes of this batch (query_gpu computes them chunk by chunk while the
// batch is still arriving over PCIe)
// codes_ext / qstride: the batch is a SLICE of a larger one whose codes (try-major reads, stride qstride) the caller holds:
// codes_ext points at the slice's first query (annhip_query_slice).
// An index in fixed mode goes to fixed_query with its own k: what follows is the parity path.
static long query_impl(annhip_index *ix, annhip_workspace &ws, hipStream_t s, size_t Q, const ftype *y_dev, int alias,
                       int mode, size_t *ids_dev, ftype *dists_dev, int codes_ready = 0, const u32 *codes_ext = NULL,
                       size_t qstride = 0) {
  // codes_ready: 1 = ws.codes holds the batch's codes, 2 = and ws.d_fcount has been reset
  if (ix->fixed && !codes_ext)
    return fixed_query(ix, ws, s, Q, y_dev, alias, FixedCall{ix->k, false, NULL, NULL, NULL}, ids_dev, dists_dev, codes_ready);
  if (!Q) return 0;
  if (Q >= 0x7FFFFFFFull / (size_t)(ix->T > 0 ? ix->T : 1)) die("query batch too large");
  if (ix->fixed) die("annhip_query_slice: not available in fixed mode");
  const QParams P = query_params(ix);
  if (!ws.d_fcount) ws.d_fcount = dev_alloc<u32>(4);
  const FT *y = reinterpret_cast<const FT *>(y_dev);
  const int k = P.k, K1 = k + 1;
  if (env().exact) mode = 1;
  if ((u32)k > P.P1) mode = 1;
  std::vector<hipEvent_t> marks_store, *marks = ix->profile == 1 ? &marks_store : NULL;
  seg_mark(ix, marks, s);
  const u32 *codes = codes_ext;
  bool fcount_zeroed = codes_ready == 2;
  if (!codes_ext) {  // (parity-mode queries ignore the probe setting)
    u32 *own = (u32 *)ws.codes.need(sizeof(u32) * Q * P.T);
    if (!codes_ready) {
      launch_codes(P, codes_needed(ix, Q), y, own, s, ws.d_fcount);  // also resets the batch's flagged-query counter
      fcount_zeroed = codes_needed(ix, Q) > 0;
    }
    codes = own;
  }
  seg_mark(ix, marks, s);
  u32 *top_i = (u32 *)ws.top_i.need(sizeof(u32) * Q * k);
  FT *top_d = (FT *)ws.top_d.need(sizeof(FT) * Q * k);
  FT *cand_d = NULL;
  u32 *cand_i = NULL, *nvt = NULL;
  // pruned stage 1 (annhip_index_set_prune): preselect on the narrow copy, rescore on native rows -- the same answers
#ifdef USE_FLOAT
  const bool pruned = mode == 0 && !codes_ext && prune_active(ix) && K1 <= 32 && ix->prune_kp >= K1;
#else
  const bool pruned = false;
#endif
  // ---- fused path: stage 2 runs in the tail of every query's stage-1 workgroup; only rejected queries come back
  {
    const size_t xrow = (size_t)P.Lc1 * (sizeof(FT) + sizeof(u32));
    const bool whole = ix->lo == 0 && ix->hi == ix->n;
    // Measured: +5 % at Q = 1k (launch-bound), neutral at cfg3 (Q = 10k, d = 128), -6 % at Q = 10k, d = 64 -- the tail
    // keeps the workgroup's registers/LDS occupied through a chain of dependent loads.  So: small batches only.
    const bool want = !codes_ext && (env().fuse >= 0 ? env().fuse != 0 : Q <= 2048);  // ANN_HIP_FUSE: 0 = never, 1 = whenever possible
    if (mode == 0 && whole && want && !pruned && P.Lc2 <= 1024 && Q * xrow <= env().exact_bytes) {
      FT *out_d = dists_dev ? reinterpret_cast<FT *>(dists_dev) : (FT *)ws.out_d.need(sizeof(FT) * Q * k);
      u32 *fl = (u32 *)ws.flist.need(sizeof(u32) * Q);
      u32 *nvo = (u32 *)ws.nvo.need(sizeof(u32) * Q);
      if (!fcount_zeroed) zero_u32_kernel<<<1, 1, 0, s>>>(ws.d_fcount);
      FusedTail F{1, P.Lc2, ids_dev, out_d, fl, ws.d_fcount, ix->d_rows + 2, NULL, NULL};
      cand_d = (FT *)ws.cand_d.need(sizeof(FT) * Q * K1);  // written for rejected queries only
      cand_i = (u32 *)ws.cand_i.need(sizeof(u32) * Q * K1);
      launch_stage1(ix, P, Q, y, alias, codes, cand_d, cand_i, NULL, nvo, s, ix->h_tries, ix->use_seg, F);
      seg_mark(ix, marks, s);
      // rejected queries (device-side count, normally zero): exact stage 1, then the classic stage 2, for them only
      unsigned long long *rows_ctr = ix->profile == 1 ? ix->d_rows + 8 : NULL;
      u32 *xi = (u32 *)ws.xids.need(sizeof(u32) * Q * P.Lc1);
      FT *xd = (FT *)ws.xd.need(sizeof(FT) * Q * P.Lc1);
      launch_rows<MODE_TABLE>(P, Q, y, alias, codes, fl, 0, Q, P.Lc1, NULL, NULL, xi, xd, rows_ctr, s, ws.d_fcount);
      launch_exact_select(P.L1, P.Lc1, P.Lc1, k, Q, xi, xd, fl, 0, top_i, top_d, k, 0, s, ws.d_fcount, NULL, 1024, 0,
                          TieArgs{cand_d, cand_i, K1, ix->d_rows + 3, 0});
      seg_mark(ix, marks, s);
      u32 *r2i = (u32 *)ws.r2i.need(sizeof(u32) * Q * P.Lc2);
      FT *r2d = (FT *)ws.r2d.need(sizeof(FT) * Q * P.Lc2);
      launch_rows<MODE_GRAPH>(P, Q, y, alias, NULL, fl, 0, Q, P.Lc2, top_i, top_d, r2i, r2d, rows_ctr, s, ws.d_fcount);
      seg_mark(ix, marks, s);
      launch_exact_select(P.L2, P.Lc2, P.Lc2, k, Q, r2i, r2d, fl, 0, NULL, out_d, k, 0, s, ws.d_fcount, ids_dev);
      seg_mark(ix, marks, s);
      finish_call(ix, marks, s, Q);
      return -1;
    }
  }
  bool prefinalized = false;
#ifdef USE_FLOAT
  if (pruned) {
    const int kp = ix->prune_kp;
    FT *pre_d = (FT *)ws.cand_d.need(sizeof(FT) * Q * kp);
    u32 *pre_i = (u32 *)ws.cand_i.need(sizeof(u32) * Q * kp);
    nvt = (u32 *)ws.nvt.need(sizeof(u32) * Q);
    u32 *nvo = (u32 *)ws.nvo.need(sizeof(u32) * Q);
    u32 *fl = (u32 *)ws.flist.need(sizeof(u32) * Q);
    // the flagged queries' exact lists for the tie path: buffers of their own (stride K1; pre_d / pre_i have stride kp and
    // are still being read by other waves of the rescore kernel)
#ifndef ANN_PRUNE_NO_TIE_LIST  // (A/B builds: no lists, every flagged row derives its own as before)
    cand_d = (FT *)ws.tie_d.need(sizeof(FT) * Q * K1);
    cand_i = (u32 *)ws.tie_i.need(sizeof(u32) * Q * K1);
#endif
    prefinalized = true;
    if (!fcount_zeroed) zero_u32_kernel<<<1, 1, 0, s>>>(ws.d_fcount);
    QParams Pn = P;
    Pn.points_h = ix->d_points_h;
    // one stage-1 "launch" for the statistics: the event pair brackets preselection and rescoring together
    EventPair ev;
    if (ix->profile) ev = s1_prof_begin(ix, s);
    launch_stage1(ix, Pn, Q, y, alias, codes, pre_d, pre_i, nvt, nvo, s, ix->h_tries, ix->use_seg,
                  FusedTail{0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL}, NULL, 1, env().s1_slots, qstride, kp, false);
    launch_prune_rescore(ix, P, Q, y, kp, pre_d, pre_i, nvt, nvo, top_i, top_d, fl, ws.d_fcount, cand_d, cand_i, s);
    if (ix->profile) s1_prof_end(ix, ev, Q, nvo, s);
    // cand_d / cand_i: a certified flagged query's exact list; an uncertified one's is empty and the tie path derives it
  } else
#endif
  if (mode == 0) {
    cand_d = (FT *)ws.cand_d.need(sizeof(FT) * Q * K1);
    cand_i = (u32 *)ws.cand_i.need(sizeof(u32) * Q * K1);
    nvt = (u32 *)ws.nvt.need(sizeof(u32) * Q);
    u32 *nvo = (u32 *)ws.nvo.need(sizeof(u32) * Q);
    // finalize1's test runs in the tail of the stage-1 workgroups (no finalize1 launch, no counter-reset launch)
    u32 *fl = (u32 *)ws.flist.need(sizeof(u32) * Q);
    prefinalized = env().fin_tail != 0;
    if (prefinalized && !fcount_zeroed) zero_u32_kernel<<<1, 1, 0, s>>>(ws.d_fcount);
    launch_stage1(ix, P, Q, y, alias, codes, cand_d, cand_i, nvt, nvo, s, ix->h_tries, ix->use_seg,
                  FusedTail{prefinalized ? 2 : 0, 0, NULL, NULL, fl, ws.d_fcount, ix->d_rows + 2, top_i, top_d}, NULL, 1,
                  env().s1_slots, qstride);
  }
  seg_mark(ix, marks, s);
  unsigned long long *rows_ctr = ix->profile == 1 ? ix->d_rows + 8 : NULL;
  long nflag = finalize_and_fallback(ix, P, Q, y, alias, codes, mode, cand_d, cand_i, nvt, top_i, top_d, k, 0,
                                     ws.flist, ws.xids, ws.xd, ws.d_fcount, rows_ctr, ix->d_rows + 2, true, s, qstride,
                                     prefinalized, pruned);
  seg_mark(ix, marks, s);
  // stage 2 (det_results second half, alg.c:314-327)
  FT *out_d = dists_dev ? reinterpret_cast<FT *>(dists_dev) : (FT *)ws.out_d.need(sizeof(FT) * Q * k);
  if (ix->lo == 0 && ix->hi == ix->n && P.Lc2 <= 1024 && env().tail != 0) {
    // one kernel: row assembly, neighbour gathers, network and size_t ids per query (stage2_fused_kernel)
    launch_stage2_fused<size_t>(P, Q, y, alias, 0, Q, top_i, top_d, ids_dev, out_d, rows_ctr, s);
    seg_mark(ix, marks, s);  // "stage2_rows" = the whole fused stage 2; "stage2_network" and "widen" stay 0
    finish_call(ix, marks, s, Q);
    return nflag;
  }
  if (ix->lo == 0 && ix->hi == ix->n && env().tail != 0 &&
      stage2_select_with_fallback(P, Q, y, alias, 0, Q, top_i, top_d, NULL, ids_dev, out_d, ws.flist, ws.d_fcount, ws.r2i,
                                  ws.r2d, ix->d_rows + 2, rows_ctr, s)) {
    // long stage-2 rows (k >= 32): selection + proof instead of the P2-entry network; "stage2_rows" = all of it
    seg_mark(ix, marks, s);
    finish_call(ix, marks, s, Q);
    return nflag;
  }
  u32 *out_i = (u32 *)ws.out_i.need(sizeof(u32) * Q * k);
  const size_t row_bytes = (size_t)P.Lc2 * (sizeof(FT) + sizeof(u32));
  size_t chunk = ((size_t)2 << 30) / row_bytes;
  if (chunk < 1) chunk = 1;
  for (size_t q0 = 0; q0 < Q; q0 += chunk) {
    const size_t nq = std::min(chunk, Q - q0);
    u32 *r2i = (u32 *)ws.r2i.need(sizeof(u32) * nq * P.Lc2);
    FT *r2d = (FT *)ws.r2d.need(sizeof(FT) * nq * P.Lc2);
    launch_rows<MODE_GRAPH>(P, Q, y, alias, NULL, NULL, (u32)q0, nq, P.Lc2, top_i, top_d, r2i, r2d, rows_ctr, s);
    if (q0 + chunk >= Q) seg_mark(ix, marks, s);
    launch_exact_select(P.L2, P.Lc2, P.Lc2, k, nq, r2i, r2d, NULL, (u32)q0, out_i, out_d, k, 0, s);
  }
  seg_mark(ix, marks, s);
  widen_ids_kernel<<<grid_for(Q * k, 256, 1u << 30), 256, 0, s>>>(Q * k, out_i, ids_dev);
  HIPCHECK(hipGetLastError());
  seg_mark(ix, marks, s);
  finish_call(ix, marks, s, Q);
  return nflag;
}

extern "C" long annhip_query(annhip_index *ix, size_t Q, const ftype *y_dev, int alias, int mode, size_t *ids_dev,
                             ftype *dists_dev) {
  return query_impl(ix, ix->ws, ix->stream, Q, y_dev, alias, mode, ids_dev, dists_dev);
}

extern "C" int annhip_probe_bits(annhip_index *ix, void *hip_stream, size_t Q, const ftype *y_dev, uint32_t *codes_dev,
                                 uint8_t *pbits_dev) {
  if (ix->probe <= 0) return -1;
  if (Q >= 0x7FFFFFFFull / (size_t)(ix->T > 0 ? ix->T : 1)) die("query batch too large");
  launch_codes_probe(query_params(ix), Q, reinterpret_cast<const FT *>(y_dev), codes_dev, pbits_dev, ix->probe,
                     (hipStream_t)hip_stream);
  return 0;
}

extern "C" annhip_workspace *annhip_workspace_create(annhip_index *ix) {
  (void)ix;
  gpu_init();
  return new annhip_workspace();
}

extern "C" void annhip_workspace_destroy(annhip_workspace *ws) {
  if (!ws) return;
  HIPCHECK(hipDeviceSynchronize());
  ws->release();
  delete ws;
}

extern "C" long annhip_query_on(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t Q, const ftype *y_dev,
                                int alias, int mode, size_t *ids_dev, ftype *dists_dev) {
  return query_impl(ix, ws ? *ws : ix->ws, (hipStream_t)hip_stream, Q, y_dev, alias, mode, ids_dev, dists_dev);
}

// ----------------------------------------------------------------------------- the entries of fixed mode with their refusals
// What annhip_query_tagged / _k / _radius / _between refuse: fixed mode off; then, for all but annhip_query_tagged
// (resharded = false: it goes on to fixed_query's abort there, as it always did), a resharded index; then the entry's
// own reasons in its order, each its text or NULL.  Prints "who: why" for the first that holds and returns it, or NULL.
static const char *const NO_TAGS = "the index has no tags (annhip_index_set_tags)";
static const char *pair_or_neither(const uint32_t *qmask_dev, const uint32_t *qvalue_dev) {
  return (qmask_dev != NULL) != (qvalue_dev != NULL) ? "qmask_dev and qvalue_dev must both be given, or neither" : NULL;
}
static const char *fixed_refusal(const annhip_index *ix, const char *who, bool resharded, std::initializer_list<const char *> own) {
  const char *why = !ix->fixed ? "fixed mode is off (annhip_index_set_fixed)"
                    : resharded && !(ix->lo == 0 && ix->hi == ix->n) ? "the index does not hold rows [0, n) on this device (resharded)"
                                                                     : NULL;
  for (const char *w : own)
    if (!why) why = w;
  if (why) fprintf(stderr, "%s: %s\n", who, why);
  return why;
}

// Contract: include/ann_hip.h.  A refusal launches nothing and leaves the outputs untouched.
extern "C" long annhip_query_tagged(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t Q, const ftype *y_dev,
                                    int alias, const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev,
                                    ftype *dists_dev) {
  if (fixed_refusal(ix, "annhip_query_tagged", false,
                    {!ix->tags ? NO_TAGS : NULL, !qmask_dev || !qvalue_dev ? "qmask_dev and qvalue_dev must both be given" : NULL}))
    return -2;
  const TagQuery tq = tag_pair(ix->tags, qmask_dev, qvalue_dev);
  return fixed_query(ix, ws ? *ws : ix->ws, (hipStream_t)hip_stream, Q, y_dev, alias, FixedCall{ix->k, false, &tq, NULL, NULL},
                     ids_dev, dists_dev);
}

// ----------------------------------------------------------------------------- query with a per-call k (annhip_query_k)
// Contract: include/ann_hip.h.  kg = ix->k (graph width), kq = the k of the call.  Stage 1 does not depend on k in fixed
// mode (P1 = Lc1 = L1) and none of its kernels reads QParams::k: the existing launchers run on a QParams copy whose k is
// kq, which sizes K1, cap and the LDS.  Stage 2 is stage2_kq_kernel (ann_kq_kernels.h) on the index's own QParams.
static size_t stage2_kq_lds_bytes(const QParams &P, int W, int K1, int cap, size_t kq) {
  size_t b = sizeof(Key) * (size_t)W * cap + 2 * sizeof(Key) * (size_t)W * K1 + sizeof(Key) * kq +
             sizeof(u32) * (size_t)W * ANN_S1_CHUNK + sizeof(int) * (size_t)W + sizeof(u32) * 4;
  b = (b + 15) & ~(size_t)15;
  if (d_needs_lds_row(P.d)) b += sizeof(FT) * (size_t)P.d * (1 + W);
  return b;
}
#define ANN_KQ_LDS_MAX ((size_t)160 * 1024)  // what allow_lds permits
// Waves per query of stage 2 for this kq: the most of 4, 2, 1 whose carve-up fits (results do not depend on the count);
// 0 = none fits.
static int stage2_kq_waves(const QParams &P, size_t kq) {
  for (int W = 4; W >= 1; W >>= 1)
    if (stage2_kq_lds_bytes(P, W, (int)kq + 1, stage1_cap(W, (int)kq + 1), kq) <= ANN_KQ_LDS_MAX) return W;
  return 0;
}
// Does a call with this kq fit?  Stage 1 is judged by the worst of its families at the most waves a launcher takes (4, or
// ANN_HIP_S1_WAVES) and the most pair bits (d_short): the answer does not depend on the probe, filter or tag settings.
static bool query_k_fits(const QParams &P, size_t kq) {
  if (kq < 1 || kq > 1024 || (kq + 1) * ((size_t)P.k + 1) >= 0x7FFFFFFFull) return false;
  const int K1 = (int)kq + 1, W1 = env().s1_waves ? env().s1_waves : 4, cap1 = stage1_cap(W1, K1);
  const size_t s1 = std::max(stage1_lds_bytes(P, W1, K1, cap1), stage1_probe_lds_bytes(P, W1, K1, cap1, P.ds));
  return s1 <= ANN_KQ_LDS_MAX && stage2_kq_waves(P, kq) > 0;
}

extern "C" size_t annhip_index_max_query_k(const annhip_index *ix) {
  const QParams P = make_params(ix);
  size_t lo = 0, hi = 1024;  // the carve-ups grow with kq: the largest kq that fits, by bisection
  while (lo < hi) {
    const size_t mid = (lo + hi + 1) / 2;
    if (query_k_fits(P, mid)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

static void launch_stage2_kq(const QParams &P, size_t Q, const FT *y, int alias, const u32 *top_i, const FT *top_d, size_t kq,
                             const u32 *filter, const TagQuery *tq, size_t *out_ids, FT *out_d, unsigned long long *rows_ctr,
                             hipStream_t s) {
  if (!Q) return;
  const int W = stage2_kq_waves(P, kq), K1 = (int)kq + 1, cap = stage1_cap(W, K1);
  if (W < 1) die("launch_stage2_kq: kq beyond annhip_index_max_query_k");
  const size_t smem = stage2_kq_lds_bytes(P, W, K1, cap, kq);
  with_value(QueryLayouts{}, layout_code(P.d), [&](auto dd) {
    with_rows(P, [&](auto rt) {
      constexpr int D = decltype(dd)::value;
      using RT = typename decltype(rt)::type;
      allow_lds((stage2_kq_kernel<D, size_t, RT>), smem);
      hipLaunchKernelGGL((stage2_kq_kernel<D, size_t, RT>), dim3((unsigned)Q), dim3(64 * W), smem, s, P, y, alias, top_i, top_d,
                         (int)kq, tq ? tq->tags : (const u32 *)NULL, filter, tq ? tq->qmask : (const u32 *)NULL,
                         tq ? tq->qlo : (const u32 *)NULL, tq ? tq->qhi : (const u32 *)NULL, K1, cap, out_ids, out_d, rows_ctr);
    });
  });
  HIPCHECK(hipGetLastError());
}

// ----------------------------------------------------------------------------- fixed mode (annhip_index_set_fixed)
// Opt-in, NOT the reference's results: query x hashes into ITS OWN buckets (the reference reads
// code[i*Q+x] of a [Q][T] array, Q2), all L1 / L2 slots are candidates (the reference orders the first 2^floor(log2 L)
// only, Q1), and the answer is simply the kq smallest distinct (distance, id) keys -- stage 1's selection kernel,
// finalize1 without its proof, stage 2 by selection.  Single device, whole index.  The one path of every fixed-mode call:
// hash (with pair bits: the kernel that also ranks the projections), stage 1, finalize1, the stage 2 that c names, the
// appended rows, a radius call's trim.  The entries have refused what can be refused.
// codes_ready (query_gpu): 1 = ws.codes holds the batch's codes, 2 = and ws.d_fcount has been reset; a probing call
// hashes again all the same, for the ranked bits.
static long fixed_query(annhip_index *ix, annhip_workspace &ws, hipStream_t s, size_t Q, const ftype *y_dev, int alias,
                        const FixedCall &c, size_t *ids_dev, ftype *dists_dev, int codes_ready) {
  if (!Q) return 0;
  if (Q >= 0x7FFFFFFFull / (size_t)(ix->T > 0 ? ix->T : 1)) die("query batch too large");
  if (!(ix->lo == 0 && ix->hi == ix->n)) die("fixed mode needs the whole index on this device");
  const QParams P = query_params(ix);
  QParams P1 = P;  // stage 1's view: k = kq
  P1.k = (int)c.kq;
  if (!ws.d_fcount) ws.d_fcount = dev_alloc<u32>(4);
  const FT *y = reinterpret_cast<const FT *>(y_dev);
  const size_t kq = c.kq;
  const int K1 = (int)kq + 1;
  std::vector<hipEvent_t> marks_store, *marks = ix->profile == 1 ? &marks_store : NULL;
  seg_mark(ix, marks, s);
  const bool probing = ix->probe > 0;
  unsigned char *pbits = NULL;
  u32 *codes = (u32 *)ws.codes.need(sizeof(u32) * Q * P.T);
  if (probing) {
    pbits = (unsigned char *)ws.pbits.need((size_t)Q * P.T * ix->probe);
    launch_codes_probe(P, Q, y, codes, pbits, ix->probe, s, ws.d_fcount);
  } else if (!codes_ready) {
    launch_codes(P, Q, y, codes, s, ws.d_fcount);
  }
  seg_mark(ix, marks, s);
  u32 *top_i = (u32 *)ws.top_i.need(sizeof(u32) * Q * kq);
  FT *top_d = (FT *)ws.top_d.need(sizeof(FT) * Q * kq);
  FT *cand_d = (FT *)ws.cand_d.need(sizeof(FT) * Q * K1);
  u32 *cand_i = (u32 *)ws.cand_i.need(sizeof(u32) * Q * K1);
  u32 *nvt = (u32 *)ws.nvt.need(sizeof(u32) * Q);
  u32 *nvo = (u32 *)ws.nvo.need(sizeof(u32) * Q);
  if (c.radius || ix->filter || c.tq || probing)  // one kernel family each, for every pair-bit setting (b = 0: no ranked bits)
    launch_stage1_fixed(ix, P1, Q, y, alias, codes, pbits, probing ? ix->probe : 0, ix->filter, c.tq, c.radius, cand_d, cand_i, nvt,
                        nvo, s);
  else launch_stage1(ix, P1, Q, y, alias, codes, cand_d, cand_i, nvt, nvo, s, ix->h_tries, ix->use_seg);
  seg_mark(ix, marks, s);
  hipLaunchKernelGGL(finalize1_kernel, dim3(grid_for(Q, 256, 1u << 30)), dim3(256), 0, s, (int)Q, (int)kq, K1, P.L1, P.P1, cand_d,
                     cand_i, nvt, top_i, top_d, (int)kq, 0, (u32 *)NULL, (u32 *)NULL, (unsigned long long *)NULL, P.n);
  HIPCHECK(hipGetLastError());
  seg_mark(ix, marks, s);
  // (what the caller's rows hold: kq entries, or the k of a grouped call)
  FT *out_d = dists_dev ? reinterpret_cast<FT *>(dists_dev) : (FT *)ws.out_d.need(sizeof(FT) * Q * (c.group ? c.group->k : kq));
  size_t *const caller_ids = ids_dev;
  FT *const caller_d = out_d;
  if (c.group) {  // the list of kq entries stays in the workspace
    ids_dev = (size_t *)ws.grp_i.need(sizeof(size_t) * Q * kq);
    out_d = (FT *)ws.grp_d.need(sizeof(FT) * Q * kq);
  }
  unsigned long long *scored = ix->profile == 1 ? ix->d_rows + 8 : NULL;
  // two stage 2s, different kernels: a call with the index's own k keeps its selection path, annhip_query_k and the
  // radius calls keep stage2_kq_kernel even where kq == ix->k
  if (c.stage2_kq) launch_stage2_kq(P, Q, y, alias, top_i, top_d, kq, ix->filter, c.tq, ids_dev, out_d, scored, s);
  else if (!stage2_select_with_fallback(P, Q, y, alias, 0, Q, top_i, top_d, NULL, ids_dev, out_d, ws.flist, ws.d_fcount, ws.r2i,
                                        ws.r2d, NULL, scored, s, ix->filter, c.tq))
    die("fixed mode: stage-2 shape not supported");
  seg_mark(ix, marks, s);
  // the appended rows merged into stage 2's rows of kq ("stage2_network" of annhip_stage_ms): the hashed ones through the
  // buckets this call probes, the rest scanned exactly
  if (ix->tail_mh) launch_tail_hash_merge(ix, Q, y, kq, c.tq, codes, pbits, probing ? ix->probe : 0, ids_dev, out_d, scored, s);
  if (ix->tail_m > ix->tail_mh)
    launch_tail_merge(ix, Q, y, alias, kq, c.tq, kq, ids_dev, out_d, ids_dev, out_d, scored, s, ix->tail_mh);
  // (in profile mode the trim's time falls into the segment of the tail merges: annhip_stage_ms reports no tail segment,
  // so the trim is in neither the stage-1 nor the stage-2 figure)
  if (c.radius) launch_radius_trim(Q, kq, n_total(ix), c.radius, ids_dev, out_d, c.counts, s);
  // (likewise the collapse of a grouped call)
  if (c.group) launch_collapse(Q, kq, *c.group, ix->tags, n_total(ix), n_total(ix), ids_dev, out_d, caller_ids, caller_d, s);
  finish_call(ix, marks, s, Q);
  return 0;
}

// Contract: include/ann_hip.h.  A refusal launches nothing and leaves the outputs untouched; this entry never aborts on
// what it can refuse.
extern "C" long annhip_query_k(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                               size_t kq, const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev,
                               ftype *dists_dev) {
  const bool tagged = qmask_dev && qvalue_dev;
  if (fixed_refusal(ix, "annhip_query_k", true,
                    {pair_or_neither(qmask_dev, qvalue_dev), tagged && !ix->tags ? NO_TAGS : NULL,
                     !query_k_fits(make_params(ix), kq) ? "kq outside 1..annhip_index_max_query_k" : NULL}))
    return -2;
  const TagQuery tq = tag_pair(ix->tags, qmask_dev, qvalue_dev);
  return fixed_query(ix, ws ? *ws : ix->ws, (hipStream_t)hip_stream, ycnt, y_dev, alias,
                     FixedCall{kq, true, tagged ? &tq : NULL, NULL, NULL}, ids_dev, dists_dev);
}

// ----------------------------------------------------------------------------- radius queries (annhip_query_radius)
// Contract: include/ann_hip.h.  Kernels: ann_radius_kernels.h.
static void launch_radius_trim(size_t Q, size_t kcap, size_t pad_id, const FT *radius, size_t *ids, FT *dists, u32 *counts,
                               hipStream_t s) {
  if (!Q || !kcap) return;
  const size_t blocks = (Q + 3) / 4;  // one wave per row, 4 rows per workgroup
  if (blocks > 0x7FFFFFFFull) die("radius trim: batch too large");
  hipLaunchKernelGGL(radius_trim_kernel, dim3((unsigned)blocks), dim3(256), 0, s, Q, kcap, pad_id, radius, ids, dists, counts);
  HIPCHECK(hipGetLastError());
}

// A refusal launches nothing and leaves the outputs untouched; this entry never aborts on what it can refuse.
extern "C" long annhip_query_radius(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev,
                                    int alias, size_t kcap, const ftype *radius_dev, const uint32_t *qmask_dev,
                                    const uint32_t *qvalue_dev, size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev) {
  const bool tagged = qmask_dev && qvalue_dev;
  if (fixed_refusal(ix, "annhip_query_radius", true,
                    {!radius_dev ? "radius_dev must be given" : NULL, !ids_dev ? "ids_dev must be given" : NULL,
                     pair_or_neither(qmask_dev, qvalue_dev), tagged && !ix->tags ? NO_TAGS : NULL,
                     !query_k_fits(make_params(ix), kcap) ? "kcap outside 1..annhip_index_max_query_k" : NULL}))
    return -2;
  const TagQuery tq = tag_pair(ix->tags, qmask_dev, qvalue_dev);
  return fixed_query(ix, ws ? *ws : ix->ws, (hipStream_t)hip_stream, ycnt, y_dev, alias,
                     FixedCall{kcap, true, tagged ? &tq : NULL, reinterpret_cast<const FT *>(radius_dev), counts_dev}, ids_dev,
                     dists_dev);
}

// Contract: include/ann_hip.h.  The range form of annhip_query_k (radius_dev == NULL) and annhip_query_radius: the same
// launchers with the two bounds apart.  With the index's own k and no radius it takes annhip_query_tagged's path, the
// stage1_tag / stage2_tag kernels.  A refusal launches nothing and leaves the outputs untouched.
extern "C" long annhip_query_between(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev,
                                     int alias, size_t kq, const ftype *radius_dev, const uint32_t *qmask_dev,
                                     const uint32_t *qlo_dev, const uint32_t *qhi_dev, size_t *ids_dev, ftype *dists_dev,
                                     uint32_t *counts_dev) {
  const bool own_k = !radius_dev && kq == ix->k;
  if (fixed_refusal(ix, "annhip_query_between", true,
                    {!qmask_dev || !qlo_dev || !qhi_dev ? "qmask_dev, qlo_dev and qhi_dev must all be given" : NULL,
                     !ix->tags ? NO_TAGS : NULL, radius_dev && !ids_dev ? "ids_dev must be given" : NULL,
                     !own_k && !query_k_fits(make_params(ix), kq) ? "kq outside 1..annhip_index_max_query_k" : NULL}))
    return -2;
  const TagQuery tq{ix->tags, qmask_dev, qlo_dev, qhi_dev};
  return fixed_query(ix, ws ? *ws : ix->ws, (hipStream_t)hip_stream, ycnt, y_dev, alias,
                     FixedCall{kq, !own_k, &tq, reinterpret_cast<const FT *>(radius_dev), counts_dev}, ids_dev, dists_dev);
}

extern "C" int annhip_radius_trim(size_t ycnt, size_t kcap, size_t pad_id, const ftype *radius_dev, size_t *ids_dev,
                                  ftype *dists_dev, uint32_t *counts_dev, void *hip_stream) {
  if (!radius_dev || !ids_dev || !dists_dev) return -1;
  launch_radius_trim(ycnt, kcap, pad_id, reinterpret_cast<const FT *>(radius_dev), ids_dev, reinterpret_cast<FT *>(dists_dev),
                     counts_dev, (hipStream_t)hip_stream);
  return 0;
}

// ----------------------------------------------------------------------------- grouped queries (annhip_query_grouped)
// Contract: include/ann_hip.h.  Kernel: ann_group_kernels.h.
static void launch_collapse(size_t Q, size_t L, const GroupCall &g, const u32 *tags, size_t rows, size_t pad_id, const size_t *ids_in,
                            const FT *dists_in, size_t *ids_out, FT *dists_out, hipStream_t s) {
  if (!Q) return;
  const size_t blocks = (Q + ANN_GROUP_WAVES - 1) / ANN_GROUP_WAVES;  // one wave per row
  if (blocks > 0x7FFFFFFFull) die("collapse: batch too large");
  const size_t smem = group_lds_bytes(L);
  allow_lds(group_collapse_kernel, smem);
  hipLaunchKernelGGL(group_collapse_kernel, dim3((unsigned)blocks), dim3(64 * ANN_GROUP_WAVES), smem, s, Q, (int)L, (int)g.k,
                     (u32)std::min<size_t>(g.per_group, 0xFFFFFFFFull), g.gmask, tags, (u64)rows, pad_id, ids_in, dists_in, ids_out,
                     dists_out, g.counts, g.shrt);
  HIPCHECK(hipGetLastError());
}

extern "C" int annhip_collapse(size_t ycnt, size_t L, size_t k, size_t per_group, uint32_t gmask, const uint32_t *tags_dev, size_t rows,
                               size_t pad_id, const size_t *ids_in, const ftype *dists_in, size_t *ids_out, ftype *dists_out,
                               uint32_t *counts_dev, uint8_t *short_dev, void *hip_stream) {
  if (L < 1 || L > 1024 || k < 1 || k > L || !per_group || !gmask || !tags_dev || !ids_in || !dists_in || !ids_out || !dists_out ||
      rows >= 0xFFFFFFF0ull)
    return -1;
  if (!ycnt) return 0;
  gpu_init();
  launch_collapse(ycnt, L, GroupCall{k, per_group, gmask, counts_dev, short_dev}, tags_dev, rows, pad_id, ids_in,
                  reinterpret_cast<const FT *>(dists_in), ids_out, reinterpret_cast<FT *>(dists_out), (hipStream_t)hip_stream);
  return 0;
}

// what both grouped entries refuse of the grouping itself: its text or NULL
static const char *group_refusal(size_t list, size_t k, size_t per_group, uint32_t gmask) {
  return !gmask       ? "gmask must not be 0"
         : !per_group ? "per_group must be at least 1"
         : !k || k > list ? "k outside 1..list"
                          : NULL;
}
static const char *all_or_none(const uint32_t *qmask_dev, const uint32_t *qlo_dev, const uint32_t *qhi_dev) {
  const int given = (qmask_dev != NULL) + (qlo_dev != NULL) + (qhi_dev != NULL);
  return given != 0 && given != 3 ? "qmask_dev, qlo_dev and qhi_dev must all be given, or none" : NULL;
}

// A refusal launches nothing and leaves the outputs untouched; this entry never aborts on what it can refuse.
extern "C" long annhip_query_grouped(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev,
                                     int alias, size_t list, size_t k, size_t per_group, uint32_t gmask, const uint32_t *qmask_dev,
                                     const uint32_t *qlo_dev, const uint32_t *qhi_dev, size_t *ids_dev, ftype *dists_dev,
                                     uint32_t *counts_dev, uint8_t *short_dev) {
  if (fixed_refusal(ix, "annhip_query_grouped", true,
                    {!ix->tags ? NO_TAGS : NULL, group_refusal(list, k, per_group, gmask),
                     !query_k_fits(make_params(ix), list) ? "list outside 1..annhip_index_max_query_k" : NULL,
                     all_or_none(qmask_dev, qlo_dev, qhi_dev), !ids_dev ? "ids_dev must be given" : NULL}))
    return -2;
  const TagQuery tq{ix->tags, qmask_dev, qlo_dev, qhi_dev};
  const GroupCall g{k, per_group, gmask, counts_dev, short_dev};
  return fixed_query(ix, ws ? *ws : ix->ws, (hipStream_t)hip_stream, ycnt, y_dev, alias,
                     FixedCall{list, true, qmask_dev ? &tq : NULL, NULL, NULL, &g}, ids_dev, dists_dev);
}

extern "C" long annhip_query_slice(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, size_t q_lo, size_t nq,
                                   const ftype *y_slice_dev, const uint32_t *codes_all_dev, int alias, size_t *ids_dev,
                                   ftype *dists_dev) {
  if (q_lo + nq > ycnt) die("annhip_query_slice: slice outside the batch");
  if (alias && q_lo) die("annhip_query_slice: an aliased batch (y == points) cannot be sliced");
  if (!(ix->lo == 0 && ix->hi == ix->n)) die("annhip_query_slice needs all rows on this device (replica hosts)");
  return query_impl(ix, ws ? *ws : ix->ws, (hipStream_t)hip_stream, nq, y_slice_dev, alias, 0, ids_dev, dists_dev, false,
                    codes_all_dev + q_lo, ycnt);
}

// ----------------------------------------------------------------------------- host-side streaming
// query() hands over host buffers on every call (ann.h:61-62) and returns host buffers: upload, compute and download
// are serialised and each call ends in a device synchronisation.  A stream of independent host-resident batches does
// not need that: each of `lanes` in-flight batches has pinned staging buffers, a workspace and a HIP stream, so the
// upload of batch i+1 and the download of batch i-1 run beside the kernels of batch i.
struct StreamLane {
  hipStream_t stream = NULL;
  annhip_workspace ws;
  FT *y_pin = NULL, *y_dev = NULL, *d_dev = NULL, *d_pin = NULL;
  size_t *i_dev = NULL, *i_pin = NULL;
  hipEvent_t done = NULL;
  long ticket = -1;  // -1: free
  size_t ycnt = 0;
};
struct annhip_stream {
  annhip_index *ix;
  size_t max_ycnt;
  std::vector<StreamLane> lanes;
  long next_ticket = 0;
};

extern "C" annhip_stream *annhip_stream_open(annhip_index *ix, size_t max_ycnt, int lanes) {
  if (lanes < 1 || lanes > 16 || !max_ycnt) die("annhip_stream_open: need 1..16 lanes and max_ycnt > 0");
  annhip_stream *st = new annhip_stream();
  st->ix = ix, st->max_ycnt = max_ycnt;
  st->lanes.resize(lanes);
  for (StreamLane &L : st->lanes) {
    HIPCHECK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    HIPCHECK(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    HIPCHECK(hipHostMalloc((void **)&L.y_pin, sizeof(FT) * max_ycnt * ix->d, hipHostMallocDefault));
    HIPCHECK(hipHostMalloc((void **)&L.d_pin, sizeof(FT) * max_ycnt * ix->k, hipHostMallocDefault));
    HIPCHECK(hipHostMalloc((void **)&L.i_pin, sizeof(size_t) * max_ycnt * ix->k, hipHostMallocDefault));
    L.y_dev = dev_alloc<FT>(max_ycnt * ix->d);
    L.d_dev = dev_alloc<FT>(max_ycnt * ix->k);
    L.i_dev = dev_alloc<size_t>(max_ycnt * ix->k);
  }
  return st;
}

extern "C" long annhip_stream_submit(annhip_stream *st, size_t ycnt, const ftype *y_host, int alias) {
  if (ycnt > st->max_ycnt) die("annhip_stream_submit: batch larger than max_ycnt");
  StreamLane &L = st->lanes[st->next_ticket % (long)st->lanes.size()];
  if (L.ticket >= 0) return -1;  // every lane is in flight: collect the oldest ticket first
  annhip_index *ix = st->ix;
  memcpy(L.y_pin, y_host, sizeof(FT) * ycnt * ix->d);  // the caller's buffer is free again when submit returns
  HIPCHECK(hipMemcpyAsync(L.y_dev, L.y_pin, sizeof(FT) * ycnt * ix->d, hipMemcpyHostToDevice, L.stream));
  query_impl(ix, L.ws, L.stream, ycnt, reinterpret_cast<const ftype *>(L.y_dev), alias, 0, L.i_dev,
             reinterpret_cast<ftype *>(L.d_dev));
  HIPCHECK(hipMemcpyAsync(L.i_pin, L.i_dev, sizeof(size_t) * ycnt * ix->k, hipMemcpyDeviceToHost, L.stream));
  HIPCHECK(hipMemcpyAsync(L.d_pin, L.d_dev, sizeof(FT) * ycnt * ix->k, hipMemcpyDeviceToHost, L.stream));
  HIPCHECK(hipEventRecord(L.done, L.stream));
  L.ticket = st->next_ticket, L.ycnt = ycnt;
  return st->next_ticket++;
}

extern "C" int annhip_stream_collect(annhip_stream *st, long ticket, size_t *ids_host, ftype *dists_host) {
  if (ticket < 0) return -1;
  StreamLane &L = st->lanes[ticket % (long)st->lanes.size()];
  if (L.ticket != ticket) return -1;  // unknown or already collected
  HIPCHECK(hipEventSynchronize(L.done));
  memcpy(ids_host, L.i_pin, sizeof(size_t) * L.ycnt * st->ix->k);
  if (dists_host) memcpy(dists_host, L.d_pin, sizeof(FT) * L.ycnt * st->ix->k);
  L.ticket = -1;
  return 0;
}

extern "C" void annhip_stream_close(annhip_stream *st) {
  if (!st) return;
  for (StreamLane &L : st->lanes) {
    HIPCHECK(hipStreamSynchronize(L.stream));
    L.ws.release();
    HIPCHECK(hipHostFree(L.y_pin));
    HIPCHECK(hipHostFree(L.d_pin));
    HIPCHECK(hipHostFree(L.i_pin));
    HIPCHECK(hipFree(L.y_dev));
    HIPCHECK(hipFree(L.d_dev));
    HIPCHECK(hipFree(L.i_dev));
    (void)hipEventDestroy(L.done);
    (void)hipStreamDestroy(L.stream);
  }
  delete st;
}

// ----------------------------------------------------------------------------- staged API
extern "C" void annhip_stage1_rows(annhip_index *ix, size_t Q, const ftype *y_dev, int alias,
                                   const uint32_t *codes_dev, const uint32_t *qidx_dev, size_t nq,
                                   uint32_t *ids_dev, ftype *dist_dev) {
  const QParams P = make_params(ix);
  launch_rows<MODE_TABLE>(P, Q, reinterpret_cast<const FT *>(y_dev), alias, codes_dev, qidx_dev, 0, nq, P.Lc1, NULL,
                          NULL, ids_dev, reinterpret_cast<FT *>(dist_dev), ix->profile == 1 ? ix->d_rows + 8 : NULL, ix->stream);
}

extern "C" void annhip_exact_select(annhip_index *ix, int stage, size_t nq, uint32_t *ids_dev, ftype *dist_dev,
                                    const uint32_t *qidx_dev, uint32_t *out_id_dev, ftype *out_dist_dev) {
  const u32 L = stage == 1 ? ix->L1 : ix->L2, len = stage == 1 ? ix->Lc1 : ix->Lc2;
  launch_exact_select(L, len, len, (int)ix->k, nq, ids_dev, reinterpret_cast<FT *>(dist_dev), qidx_dev, 0,
                      out_id_dev, reinterpret_cast<FT *>(out_dist_dev), (int)ix->k, 0, ix->stream, NULL, NULL, 1024, 0,
                      TieArgs{NULL, NULL, (int)ix->k + 1, ix->d_rows + 3, 1});
}

// Test hook: sort_and_uniq on nq free-standing rows of reference length L (stride len = ann_need_len(L, k)), optionally
// with the tie path fed by the candidate lists cand_*_dev [nq][k+1]; *resolved_dev counts the rows it answered.
extern "C" void annhip_test_sort_rows(size_t L, size_t k, size_t nq, uint32_t *ids_dev, ftype *dist_dev,
                                      const ftype *cand_d_dev, const uint32_t *cand_i_dev, uint32_t *out_id_dev,
                                      ftype *out_dist_dev, unsigned long long *resolved_dev, int derive) {
  gpu_init();
  const u32 len = (u32)ann_need_len(L, k);
  launch_exact_select((u32)L, len, len, (int)k, nq, ids_dev, reinterpret_cast<FT *>(dist_dev), NULL, 0, out_id_dev,
                      reinterpret_cast<FT *>(out_dist_dev), (int)k, 0, NULL, NULL, NULL, 1024, 0,
                      TieArgs{reinterpret_cast<const FT *>(cand_d_dev), cand_i_dev, (int)k + 1, resolved_dev,
                              cand_d_dev ? 0 : derive});
  HIPCHECK(hipStreamSynchronize(NULL));
}

// Test hook: stage 1's running selection (test_select_kernel) on ns key streams, stream b = entries [off[b], off[b+1]).
extern "C" int annhip_test_select(size_t ns, const uint32_t *off_dev, const ftype *dist_dev, const uint32_t *id_dev, size_t K1,
                                  int W, int lds, ftype *out_dist_dev, uint32_t *out_id_dev) {
  gpu_init();
  if (K1 < 1 || K1 > 256 || W < 1 || W > 4 || (!lds && K1 > ANN_SEL_REGS_KMAX)) return -1;
  if (!ns) return 0;
  const int cap = stage1_cap(W, (int)K1);
  const size_t smem = sizeof(Key) * (lds ? (size_t)W * cap : 0) + sizeof(Key) * (size_t)(lds ? W : 1) * K1 +
                      sizeof(Key) * (size_t)W * K1 + sizeof(int) * (size_t)W;
  auto launch = [&](auto rg) {
    constexpr bool RG = decltype(rg)::value;
    allow_lds(test_select_kernel<RG>, smem);
    hipLaunchKernelGGL(test_select_kernel<RG>, dim3((unsigned)ns), dim3(64 * W), smem, NULL, off_dev,
                       reinterpret_cast<const FT *>(dist_dev), id_dev, (int)K1, cap, reinterpret_cast<FT *>(out_dist_dev), out_id_dev);
  };
  if (lds) launch(std::false_type{});
  else launch(std::true_type{});
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(NULL));
  return 0;
}

// A HIP stream whose kernels may use every compute unit except `reserve` of them (the highest-numbered ones).
// Used for the stage-1 gathers of a sharded host: that kernel would otherwise occupy every wave slot of the GPU, and
// the small kernels and RCCL collectives of the other in-flight batch wait for slots (a multi-wave workgroup can wait
// until the gather has drained).  The gather is HBM-bound and does not need the last few CUs.  NULL if unsupported.
extern "C" void *annhip_stream_create_reserving(int reserve) {
  gpu_init();
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NULL;
  const int ncu = prop.multiProcessorCount;
  if (reserve < 0 || reserve >= ncu) return NULL;
  std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
  for (int cu = 0; cu < ncu - reserve; cu++) mask[cu / 32] |= 1u << (cu % 32);
  hipStream_t st = NULL;
  if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
    (void)hipGetLastError();
    return NULL;
  }
  return st;
}
extern "C" void annhip_stream_destroy(void *hip_stream) {
  if (hip_stream) (void)hipStreamDestroy((hipStream_t)hip_stream);
}

// ---- point-sharded hosts, owner protocol (approximatenn_amd/sharded.py).  Every call is
// asynchronous on the given HIP stream and touches no index-owned scratch, so several batches can be in flight.
extern "C" size_t annhip_key_bytes(void) { return sizeof(Key); }

extern "C" void annhip_sh_codes(annhip_index *ix, void *hip_stream, size_t Q, const ftype *y_dev, size_t q_lo, size_t q_hi,
                                uint32_t *codes_slice_dev) {
  const size_t hi = std::min(std::min(q_hi, Q), codes_needed(ix, Q));
  if (hi <= q_lo) return;
  launch_codes(make_params(ix), hi - q_lo, reinterpret_cast<const FT *>(y_dev) + q_lo * ix->d, codes_slice_dev,
               (hipStream_t)hip_stream);
}

extern "C" void annhip_sh_stage1(annhip_index *ix, void *hip_stream, size_t Q, const ftype *y_dev, int alias,
                                 const uint32_t *codes_dev, void *keys_dev, uint32_t *nvalid_dev, uint32_t *nown_dev) {
  const QParams P = make_params(ix);
  if ((u32)P.k > P.P1) die("annhip_sh_stage1: k exceeds the sorted prefix; use the exact path (annhip_stage1_rows)");
  launch_stage1(ix, P, Q, reinterpret_cast<const FT *>(y_dev), alias, codes_dev, NULL, NULL, nvalid_dev, nown_dev,
                (hipStream_t)hip_stream, ix->h_tries, ix->use_seg, FusedTail{0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL},
                reinterpret_cast<Key *>(keys_dev), ix->gather_pieces, ix->gather_slots);
  ix->queries += (double)Q;
}

extern "C" void annhip_sh_merge_finalize(annhip_index *ix, void *hip_stream, int ndev, size_t Q, size_t q_lo, size_t qs,
                                         const void *keys_in_dev, const uint32_t *nvalid_dev, uint32_t *top_id_dev,
                                         ftype *top_dist_dev) {
  if (ndev < 1 || ndev > 16) die("annhip_sh_merge_finalize supports 1..16 devices");
  if (!qs) return;
  const size_t nq = q_lo < Q ? std::min(qs, Q - q_lo) : 0;
  const size_t smem = sizeof(Key) * 4 * (size_t)(ndev + 1) * (ix->k + 1);
  allow_lds(merge_finalize_kernel, smem);
  hipLaunchKernelGGL(merge_finalize_kernel, dim3((unsigned)((qs + 3) / 4)), dim3(256), smem, (hipStream_t)hip_stream, ndev,
                     (int)nq, (u32)q_lo, (u32)qs, (int)ix->k + 1, (int)ix->k, ix->L1, ix->P1,
                     reinterpret_cast<const Key *>(keys_in_dev), nvalid_dev, top_id_dev, reinterpret_cast<FT *>(top_dist_dev),
                     ix->d_rows + 2);
  HIPCHECK(hipGetLastError());
}

// Exact stage 1 of the flagged queries, device-driven (no host read-back), in two halves around one MIN all-reduce of
// rows_dist_dev (ftype[fcap][Lc1], fixed size whatever the count):
//   begin: ascending list of the flagged queries (flist_dev u32[2+fcap] = {listed, total, list...}) from the all-gathered
//          top ids; ids and owned distances of the first Lc1 slots of each listed query (+inf elsewhere);
//   end:   the reference's network on the reduced rows -> top_id_all_dev[x][0..k) (the flag disappears) and
//          top_dist_all_dev[x][0..k); the owner's slices are patched.
// Queries beyond fcap stay flagged: annhip_sh_stage2 lists them and the host repairs them after the step.
extern "C" void annhip_sh_exact1_begin(annhip_index *ix, void *hip_stream, size_t Q, const ftype *y_dev, int alias,
                                       const uint32_t *codes_dev, const uint32_t *top_id_all_dev, size_t fcap,
                                       uint32_t *flist_dev, uint32_t *rows_id_dev, ftype *rows_dist_dev) {
  const QParams P = make_params(ix);
  hipStream_t s = (hipStream_t)hip_stream;
  const unsigned nchunks = (unsigned)((Q + ANN_FLAG_CHUNK - 1) / ANN_FLAG_CHUNK);
  u32 *chunk_cnt = reinterpret_cast<u32 *>(rows_id_dev);  // scratch until the rows kernel overwrites it (stream order)
  if ((size_t)nchunks > fcap * (size_t)P.Lc1) die("annhip_sh_exact1_begin: batch too large for the flag scan scratch");
  hipLaunchKernelGGL(flag_count_kernel, dim3(nchunks), dim3(ANN_FLAG_CHUNK), 0, s, (int)Q, P.k, top_id_all_dev, chunk_cnt);
  hipLaunchKernelGGL(flag_place_kernel, dim3(nchunks), dim3(ANN_FLAG_CHUNK), 0, s, (int)Q, P.k, top_id_all_dev, chunk_cnt,
                     (u32)fcap, flist_dev);
  HIPCHECK(hipGetLastError());
  launch_rows<MODE_TABLE>(P, Q, reinterpret_cast<const FT *>(y_dev), alias, codes_dev, flist_dev + 2, 0, fcap, P.Lc1, NULL,
                          NULL, rows_id_dev, reinterpret_cast<FT *>(rows_dist_dev), ix->profile == 1 ? ix->d_rows + 8 : NULL, s,
                          flist_dev);
}

extern "C" void annhip_sh_exact1_end(annhip_index *ix, void *hip_stream, size_t Q, size_t q_lo, size_t qs, size_t fcap,
                                     const uint32_t *flist_dev, uint32_t *rows_id_dev, ftype *rows_dist_dev,
                                     uint32_t *top_id_all_dev, ftype *top_dist_all_dev, uint32_t *top_id_dev,
                                     ftype *top_dist_dev) {
  hipStream_t s = (hipStream_t)hip_stream;
  // (no rank but the owner ever held the merged candidate list of a flagged query: the tie path derives it from the
  // reduced row)
  launch_exact_select(ix->L1, ix->Lc1, ix->Lc1, (int)ix->k, fcap, rows_id_dev, reinterpret_cast<FT *>(rows_dist_dev),
                      flist_dev + 2, 0, top_id_all_dev, reinterpret_cast<FT *>(top_dist_all_dev), (int)ix->k, 0, s, flist_dev,
                      NULL, 256, 0, TieArgs{NULL, NULL, (int)ix->k + 1, ix->d_rows + 3, 1});
  hipLaunchKernelGGL(patch_owner_kernel, dim3(8), dim3(256), 0, s, flist_dev, (u32)q_lo, (u32)qs, (int)ix->k, top_id_all_dev,
                     reinterpret_cast<const FT *>(top_dist_all_dev), top_id_dev, reinterpret_cast<FT *>(top_dist_dev));
  HIPCHECK(hipGetLastError());
  (void)Q;
}

extern "C" void annhip_sh_stage2(annhip_index *ix, void *hip_stream, size_t Q, const ftype *y_dev, int alias,
                                 const uint32_t *top_id_all_dev, ftype *dist_out_dev, uint32_t *flagged_dev) {
  const QParams P = make_params(ix);
  hipStream_t s = (hipStream_t)hip_stream;
  zero_u32_kernel<<<1, 1, 0, s>>>(flagged_dev);  // flagged_dev = {count, query indices...}, Q + 1 entries
  const u32 per = P.Lc2 - (u32)P.k;
  if (d_is_fast(P.d) && env().s2_multi && per && per <= ANN_S2M_CAP && Q) {  // many queries per workgroup (stage2_dist_multi_kernel)
    // queries per workgroup: enough to fill the gather loop (a rank owns (hi - lo) / n of the slots), within the LDS lists
    const double own = std::max(1e-3, (double)(P.hi - P.lo) / (double)P.n);
    u32 qpb = (u32)std::min<double>(64.0, std::max(1.0, 128.0 / (own * per)));
    qpb = std::max<u32>(1, std::min<u32>(qpb, ANN_S2M_CAP / per));
    const unsigned grid = (unsigned)((Q + qpb - 1) / qpb);
    with_value(Pow2Layouts{}, layout_code(P.d, false), [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      if constexpr (D > 0)
        hipLaunchKernelGGL(stage2_dist_multi_kernel<D>, dim3(grid), dim3(256), 0, s, P, (int)Q, reinterpret_cast<const FT *>(y_dev),
                           alias, P.Lc2, qpb, top_id_all_dev, reinterpret_cast<FT *>(dist_out_dev), flagged_dev,
                           ix->profile == 1 ? ix->d_rows + 8 : NULL);
    });
    HIPCHECK(hipGetLastError());
    return;
  }
  launch_rows<MODE_GRAPH_DIST>(P, Q, reinterpret_cast<const FT *>(y_dev), alias, NULL, NULL, 0, Q, P.Lc2, top_id_all_dev,
                               NULL, flagged_dev, reinterpret_cast<FT *>(dist_out_dev), ix->profile == 1 ? ix->d_rows + 8 : NULL, s);
}

extern "C" void annhip_sh_final(annhip_index *ix, void *hip_stream, int ndev, size_t Q, size_t q_lo, size_t qs,
                                const uint32_t *top_id_dev, const ftype *top_dist_dev, const ftype *dist_in_dev,
                                uint32_t *out_id_dev, ftype *out_dist_dev) {
  if (!qs) return;
  const size_t nq = q_lo < Q ? std::min(qs, Q - q_lo) : 0;
  const size_t smem = (size_t)ix->Lc2 * (sizeof(FT) + sizeof(u32));
  if (smem > 150 * 1024) die("annhip_sh_final: stage-2 row does not fit LDS");
  const int lk = ann_lg(ix->L2);
  unsigned npairs = 8u << (lk > 4 ? lk - 4 : 0);
  unsigned block = npairs >= 1024 ? 1024 : ((npairs + 63) / 64) * 64;
  if (block < 64) block = 64;
  allow_lds(final_select_kernel, smem);
  hipLaunchKernelGGL(final_select_kernel, dim3((unsigned)std::min<size_t>(qs, 1u << 20)), dim3(block), smem,
                     (hipStream_t)hip_stream, ndev, (int)nq, (u32)q_lo, (u32)qs, (u32)ix->n, (int)ix->k, ix->L2, ix->Lc2,
                     ix->d_graph, top_id_dev, reinterpret_cast<const FT *>(top_dist_dev),
                     reinterpret_cast<const FT *>(dist_in_dev), out_id_dev, reinterpret_cast<FT *>(out_dist_dev));
  HIPCHECK(hipGetLastError());
}

// stage-2 rows (ids + distances, Lc2 each) of the listed queries only: the repair pass of flagged queries
extern "C" void annhip_stage2_rows_list(annhip_index *ix, size_t Q, const ftype *y_dev, int alias, const uint32_t *qidx_dev,
                                        size_t nq, const uint32_t *top_id_dev, const ftype *top_dist_dev,
                                        uint32_t *ids_dev, ftype *dist_dev) {
  const QParams P = make_params(ix);
  launch_rows<MODE_GRAPH>(P, Q, reinterpret_cast<const FT *>(y_dev), alias, NULL, qidx_dev, 0, nq, P.Lc2, top_id_dev,
                          reinterpret_cast<const FT *>(top_dist_dev), ids_dev, reinterpret_cast<FT *>(dist_dev),
                          ix->profile == 1 ? ix->d_rows + 8 : NULL, ix->stream);
}

// ---- content checksums (multi-GPU hosts prove with them that every rank holds the same index and the same batch;
// bench.py all-reduces them with MIN and MAX).  Order-sensitive per word, commutative across words, so the result does
// not depend on the launch geometry: sum over i of mix(word_i, i).
__global__ void checksum_kernel(size_t nwords, const u32 *__restrict__ w, size_t tail_bytes, unsigned long long *out) {
  unsigned long long acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x) {
    unsigned long long v = ((unsigned long long)w[i] << 32 | (u32)i) ^ ((unsigned long long)(i >> 32) * 0x9E3779B97F4A7C15ull);
    v *= 0xFF51AFD7ED558CCDull;
    v ^= v >> 29;
    v *= 0xC4CEB9FE1A85EC53ull;
    acc += v ^ (v >> 32);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && tail_bytes) {  // the last 1..3 bytes of a length that is no multiple of 4
    const unsigned char *b = reinterpret_cast<const unsigned char *>(w + nwords);
    u32 t = 0;
    for (size_t j = 0; j < tail_bytes; j++) t |= (u32)b[j] << (8 * j);
    acc += ((unsigned long long)t + 1) * 0xD6E8FEB86659FD93ull + nwords;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
  if (lane_id() == 0) atomicAdd(out, acc);
}

static unsigned long long checksum_dev(const void *p, size_t nbytes, unsigned long long *d_acc, hipStream_t s) {
  if ((uintptr_t)p % 4) die("annhip_checksum_dev: pointer must be 4-byte aligned");
  HIPCHECK(hipMemsetAsync(d_acc, 0, sizeof(unsigned long long), s));
  const size_t nwords = nbytes / 4;
  checksum_kernel<<<grid_for(nwords ? nwords : 1, 256, 4096), 256, 0, s>>>(nwords, (const u32 *)p, nbytes % 4, d_acc);
  HIPCHECK(hipGetLastError());
  unsigned long long h = 0;
  HIPCHECK(hipMemcpyAsync(&h, d_acc, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return h ^ (nbytes * 0x9E3779B97F4A7C15ull);
}

extern "C" unsigned long long annhip_checksum_dev(const void *dev_ptr, size_t nbytes, void *hip_stream) {
  RandGuard keep_callers_stream;
  gpu_init();
  unsigned long long *acc = dev_alloc<unsigned long long>(1);
  const unsigned long long h = checksum_dev(dev_ptr, nbytes, acc, (hipStream_t)hip_stream);
  HIPCHECK(hipFree(acc));
  return h;
}

// everything a query reads except the point rows: geometry, bucket tables, graph, means, projection rows
extern "C" unsigned long long annhip_index_checksum(annhip_index *ix) {
  RandGuard keep_callers_stream;
  unsigned long long *acc = dev_alloc<unsigned long long>(1);
  hipStream_t s = ix->stream;
  const size_t nb = (size_t)1 << ix->ds;
  unsigned long long h = ix->n * 0x100000001B3ull ^ ix->k << 40 ^ ix->d << 20 ^ ix->ds << 8 ^ (size_t)ix->T;
  auto fold = [&](unsigned long long v) { h = (h ^ v) * 0xFF51AFD7ED558CCDull, h ^= h >> 31; };
  for (int t = 0; t < ix->T; t++) {
    fold(ix->h_tries[t].pm);
    fold(checksum_dev(ix->d_tabs[t], sizeof(u32) * nb * ix->h_tries[t].pm, acc, s));
  }
  fold(checksum_dev(ix->d_graph, sizeof(u32) * ix->n * ix->k, acc, s));
  fold(checksum_dev(ix->d_means, sizeof(FT) * ix->d, acc, s));
  fold(checksum_dev(ix->d_bases, sizeof(FT) * (size_t)ix->T * ix->ds * ix->d, acc, s));
  HIPCHECK(hipFree(acc));
  return h;
}

extern "C" void annhip_profile(annhip_index *ix, int profile) { ix->profile = profile == 2 ? 2 : profile != 0; }

extern "C" void annhip_stats(annhip_index *ix, double out[8], int reset) {
  HIPCHECK(hipStreamSynchronize(ix->stream));
  for (auto &e : ix->ev_used) {
    float ms = 0;
    HIPCHECK(hipEventSynchronize(e.b));
    HIPCHECK(hipEventElapsedTime(&ms, e.a, e.b));
    ix->s1_ms += ms;
    ix->ev_free.push_back(e);
  }
  ix->ev_used.clear();
  for (auto &m : ix->seg_used) {
    for (size_t i = 0; i + 1 < m.size() && i < 6; i++) {
      float ms = 0;
      HIPCHECK(hipEventSynchronize(m[i + 1]));
      HIPCHECK(hipEventElapsedTime(&ms, m[i], m[i + 1]));
      ix->seg_ms[i] += ms;
    }
    for (hipEvent_t e : m) ix->seg_free.push_back(e);
  }
  ix->seg_used.clear();
  unsigned long long rows[ANN_NCOUNTERS];
  HIPCHECK(hipMemcpy(rows, ix->d_rows, sizeof rows, hipMemcpyDeviceToHost));
  unsigned long long other = 0;
  for (int i = 0; i < 64; i++) other += rows[8 + i * 8];
  out[0] = ix->s1_launches, out[1] = ix->s1_ms, out[2] = (double)rows[0], out[3] = (double)other;
  out[4] = (double)rows[2], out[5] = ix->queries, out[6] = (double)rows[3] /* answered by the tie path */;
  out[7] = (double)rows[4] /* pruned stage 1: not certified */;
  if (reset) {
    ix->s1_launches = ix->s1_ms = ix->queries = 0;
    for (double &v : ix->seg_ms) v = 0;
    HIPCHECK(hipMemset(ix->d_rows, 0, sizeof rows));
  }
}

extern "C" void annhip_stage_ms(annhip_index *ix, double out[6]) {
  double dummy[8];
  annhip_stats(ix, dummy, 0);  // resolves pending events
  for (int i = 0; i < 6; i++) out[i] = ix->seg_ms[i];
}


// ----------------------------------------------------------------------------- recall scoring
// ranks_dev[q][j] = number of points strictly closer to query q than its j-th guess (0 = it is the nearest).
// points_dev: ALL n rows; guess_dev: size_t[Q][k] as returned by query()/precomp(); self: skip point q for query q.
extern "C" void annhip_recall_ranks(size_t n, size_t d, size_t k, const ftype *points_dev, size_t Q, const ftype *y_dev,
                                    const size_t *guess_dev, int self, unsigned long long *ranks_dev) {
  gpu_init();
  if (!Q || !k) return;
  if (n >= 0xFFFFFFF0ull) die("n must fit 32 bits");
  const FT *pts = reinterpret_cast<const FT *>(points_dev), *y = reinterpret_cast<const FT *>(y_dev);
  FT *gd = dev_alloc<FT>(Q * k);
  unsigned long long *hist = dev_alloc<unsigned long long>(Q * (k + 1));
  HIPCHECK(hipMemset(hist, 0, sizeof(unsigned long long) * Q * (k + 1)));
  const int wpb = 4;
  const bool fast = d_is_fast(d);
  const size_t smem_g = fast ? 0 : sizeof(FT) * wpb * 2 * d;
  const size_t smem_s = fast ? sizeof(FT) * ANN_RECALL_TILE * d : sizeof(FT) * wpb * 2 * d;
  const unsigned tiles = (unsigned)((n + ANN_RECALL_TILE - 1) / ANN_RECALL_TILE);
  unsigned qgroups = (unsigned)std::min<size_t>((Q + wpb - 1) / wpb, tiles < 2048 ? (4096 / (tiles ? tiles : 1)) + 1 : 1);
  if (qgroups < 1) qgroups = 1;
  if (qgroups > 65535) qgroups = 65535;
  with_value(Pow2Layouts{}, layout_code(d, false), [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    allow_lds(recall_guess_dist_kernel<D>, smem_g);
    hipLaunchKernelGGL(recall_guess_dist_kernel<D>, dim3((unsigned)((Q + wpb - 1) / wpb)), dim3(64 * wpb), smem_g, 0, pts, (u32)n,
                       (int)d, (int)Q, (int)k, y, guess_dev, gd);
    allow_lds(recall_scan_kernel<D>, smem_s);
    hipLaunchKernelGGL(recall_scan_kernel<D>, dim3(tiles, qgroups), dim3(64 * wpb), smem_s, 0, pts, (u32)n, (int)d, (int)Q,
                       (int)k, y, gd, self, hist);
  });
  HIPCHECK(hipGetLastError());
  // rank[j] = #points closer than guess j = sum of hist[c] over the c's whose point is closer than gdist[j]:
  // a point counted in bin c has exactly c guesses at least as close as itself, so it is closer than guess j iff
  // guess j is not among those c, i.e. (guesses ascending) iff c <= position of j.  Done on the host: tiny.
  std::vector<unsigned long long> h(Q * (k + 1)), out(Q * k);
  std::vector<FT> g(Q * k);
  HIPCHECK(hipMemcpy(h.data(), hist, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(g.data(), gd, sizeof(FT) * g.size(), hipMemcpyDeviceToHost));
  for (size_t q = 0; q < Q; q++)
    for (size_t j = 0; j < k; j++) {
      // number of guesses strictly closer than guess j (works for unsorted guesses too)
      size_t pos = 0;
      for (size_t i = 0; i < k; i++) pos += g[q * k + i] < g[q * k + j];
      unsigned long long r = 0;
      for (size_t c = 0; c <= pos && c <= k; c++) r += h[q * (k + 1) + c];
      out[q * k + j] = r;
    }
  HIPCHECK(hipMemcpy(ranks_dev, out.data(), sizeof(unsigned long long) * out.size(), hipMemcpyHostToDevice));
  HIPCHECK(hipFree(gd));
  HIPCHECK(hipFree(hist));
}

// the same with host pointers in and out (ranks_host: unsigned long long[ycnt*k]) -- for plain-C drivers such as
// tests/harness/test_correctness.c, the counterpart of /root/reference/test_correctness.c
extern "C" void annhip_recall_ranks_host(size_t n, size_t d, size_t k, const ftype *points, size_t Q, const ftype *y,
                                         const size_t *guess, int self, unsigned long long *ranks_host) {
  RandGuard keep_callers_stream;
  gpu_init();
  if (!Q || !k) return;
  FT *dp = dev_alloc<FT>(n * d), *dy = (y == points) ? dp : dev_alloc<FT>(Q * d);
  size_t *dg = dev_alloc<size_t>(Q * k);
  unsigned long long *dr = dev_alloc<unsigned long long>(Q * k);
  HIPCHECK(hipMemcpy(dp, points, sizeof(FT) * n * d, hipMemcpyHostToDevice));
  if (dy != dp) HIPCHECK(hipMemcpy(dy, y, sizeof(FT) * Q * d, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dg, guess, sizeof(size_t) * Q * k, hipMemcpyHostToDevice));
  annhip_recall_ranks(n, d, k, reinterpret_cast<const ftype *>(dp), Q, reinterpret_cast<const ftype *>(dy), dg, self, dr);
  HIPCHECK(hipMemcpy(ranks_host, dr, sizeof(unsigned long long) * Q * k, hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(dp));
  if (dy != dp) HIPCHECK(hipFree(dy));
  HIPCHECK(hipFree(dg));
  HIPCHECK(hipFree(dr));
}

// ----------------------------------------------------------------------------- exact k nearest neighbours
// Contract: include/ann_hip.h.  Kernels: ann_exact_kernels.h.  Synchronous, on the null stream like the recall scorer.
#define ANN_EX_LDS_BUDGET (150 * 1024)       // one workgroup per CU
#define ANN_EX_WS_BYTES ((size_t)256 << 20)  // workspace cap; larger batches go in chunks of queries
#define ANN_EX_MIN_RANGE 1024                // rows per range at least: below that the merge outweighs the scan
static int exact_refuse(const char *why) {
  fprintf(stderr, "annhip_exact_knn: %s\n", why);
  return 1;
}
static int exact_check(size_t n, size_t d, size_t k, int self) {
  if (d < 1) return exact_refuse("d must be at least 1");
  if (n >= 0xFFFFFFF0ull) return exact_refuse("n must fit 32 bits");
  if (k < 1 || k > 1024) return exact_refuse("k must be in 1..1024");
  if (k > n - (self && n ? 1 : 0) || !n) return exact_refuse("k exceeds the number of rows a query can be given");
  return 0;
}
// LDS carve-up of one workgroup of the exact scan for a kernel that takes up to max_waves waves: the row tile, then per wave
// the selection buffers (and the query + tree scratch of the any-d path), then the tile's validity words.  The one source
// of this arithmetic: exact_run and launch_tail_merge (ann_tail_kernels.h) both size their launches with it.
// valid (ann_exact_kernels.h): every row, the allow list, or the tag predicate with or without an allow list.
// prefetch: the kernel moves the next tile through registers.  false: the row does not fit.
struct ExShape {
  size_t W, tile_rows, smem, cap;
  bool prefetch;
};
// sorted: the shape of sorted_scan_kernel (ann_sorted_kernels.h) -- behind the waves' buffers come the tile's ids, its
// allow-list flags (one word per row each) and the workgroup's (q, start, end) triples; never a prefetch.
static bool exact_shape(size_t d, size_t k, bool generic, int max_waves, bool prefetch, ExValid valid, ExShape &sh,
                        bool sorted = false) {
  const size_t row_bytes = d * sizeof(FT);
  const size_t cap = k + ANN_EX_SLACK;
  size_t np = ANN_EX_GEN_ELEMS / d;
  np = np < 1 ? 1 : (np > ANN_WAVE ? ANN_WAVE : np);
  const size_t wave_bytes = sizeof(Key) * (ANN_EX_QB * cap + k) + (generic ? (((1 + np) * row_bytes + 15) & ~(size_t)15) : 0);
  // tile: what the threads can keep in flight (ANN_EX_PF pieces of 16 bytes each) where the kernel prefetches
  auto tile_rows_of = [&](size_t W, bool pf) {
    return std::max<size_t>(1, (pf ? (size_t)ANN_EX_PF * 64 * W * 16 : (size_t)ANN_EX_GEN_TILE_BYTES) / row_bytes);
  };
  auto smem_of = [&](size_t W, bool pf) {  // (EX_BITS: the tile's words of the allow list behind the waves' buffers,
    if (sorted)
      return ((tile_rows_of(W, pf) * row_bytes + 15) & ~(size_t)15) + W * wave_bytes +
             sizeof(u32) * (2 * tile_rows_of(W, pf) + 3 * W * ANN_EX_QB);
    return ((tile_rows_of(W, pf) * row_bytes + 15) & ~(size_t)15) + W * wave_bytes +  // EX_TAGS: its tag words before them)
           (valid == EX_TAGS ? sizeof(u32) * tile_rows_of(W, pf) : 0) +
           (valid != EX_ALL ? sizeof(u32) * ANN_EX_TBITS(tile_rows_of(W, pf)) : 0);
  };
  size_t W = (size_t)max_waves;
  while (W > 1 && smem_of(W, prefetch) > ANN_EX_LDS_BUDGET) W--;
  if (prefetch && row_bytes > (size_t)ANN_EX_PF * 64 * W * 16) prefetch = false;  // one row is more than the threads hold
  if (prefetch && valid == EX_TAGS && tile_rows_of(W, true) > 64 * W) prefetch = false;  // ... or more tags: one per thread
  sh.W = W, sh.cap = cap, sh.prefetch = prefetch;
  sh.smem = smem_of(W, prefetch);
  sh.tile_rows = tile_rows_of(W, prefetch);
  return sh.smem <= 160 * 1024;
}
// Every instance of exact_scan_kernel / exact_scan_generic_kernel.  EX_BITS reads the allow list through the last argument,
// EX_TAGS through G (ann_exact_kernels.h).
typedef void (*ExScanKernel)(ExArgs, ExValidArgs, const u32 *);
// Shape of one annhip_exact_knn call and its launches: the scan and the merge of every chunk of queries.
static int exact_run(size_t n, size_t d, size_t k, const FT *pts, size_t ycnt, const FT *y, int self, size_t *ids_dev,
                     FT *dists_dev, bool generic, int max_waves, bool prefetch, ExValid valid, ExScanKernel kernel,
                     const ExValidArgs &G) {
  ExShape sh;
  if (!exact_shape(d, k, generic, max_waves, prefetch, valid, sh)) return exact_refuse("row too long for the LDS of one CU");
  const size_t W = sh.W, cap = sh.cap, smem = sh.smem, tile_rows = sh.tile_rows;
  prefetch = sh.prefetch;
  const size_t qpg = W * ANN_EX_QB;  // queries per workgroup
  // Row ranges: enough workgroups for several rounds over the CUs at small ycnt, one range where the query groups fill
  // the chip already; a range is long enough that its first rows (every one a survivor until k are known) do not count.
  const size_t cus = (size_t)device_cus(), qgroups_all = (ycnt + qpg - 1) / qpg;
  size_t ranges = (8 * cus + qgroups_all - 1) / qgroups_all;
  ranges = std::min(ranges, std::max<size_t>(1, n / std::max<size_t>(ANN_EX_MIN_RANGE, 256 * k)));
  if (ranges > 1) {  // the last round over the CUs should be full: of r/2..r ranges take the count that wastes least
    size_t best = ranges;
    double best_waste = 1e30;
    for (size_t r = ranges; r >= std::max<size_t>(1, ranges / 2); r--) {
      const double wgs = (double)(qgroups_all * r), rounds = ceil(wgs / (double)cus);
      const double waste = rounds * (double)cus / wgs;
      if (waste < best_waste - 1e-9) best_waste = waste, best = r;
    }
    ranges = best;
  }
  if (env().exact_ranges) ranges = (size_t)env().exact_ranges;
  ranges = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(ranges, n), std::max<size_t>(1, 16384 / k)));
  const size_t range_rows = (n + ranges - 1) / ranges;
  ranges = (n + range_rows - 1) / range_rows;  // no empty range
  size_t qchunk = ANN_EX_WS_BYTES / (ranges * k * sizeof(Key));
  qchunk = std::max(qpg, qchunk / qpg * qpg);
  qchunk = std::min(qchunk, (ycnt + qpg - 1) / qpg * qpg);
  Key *ws = dev_alloc<Key>(qchunk * ranges * k);
  ExArgs A;
  A.points = pts, A.y = y, A.ws = ws;
  A.n = (u32)n, A.range_rows = (u32)range_rows, A.d = (int)d, A.k = (int)k, A.self = self ? 1 : 0;
  A.tile_rows = (int)tile_rows, A.cap = (int)cap, A.ranges = (int)ranges, A.prefetch = prefetch ? 1 : 0;
  allow_lds(kernel, smem);
  for (size_t q0 = 0; q0 < ycnt; q0 += qchunk) {
    const size_t qn = std::min(qchunk, ycnt - q0);
    A.q0 = (u32)q0, A.qn = (u32)qn;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((qn + qpg - 1) / qpg), (unsigned)ranges), dim3((unsigned)(64 * W)), smem, 0, A, G,
                       G.bits);
    hipLaunchKernelGGL(exact_merge_kernel, dim3((unsigned)((qn + 3) / 4)), dim3(256), 0, 0, ws, (u32)qn, (int)ranges, (int)k,
                       ids_dev + q0 * k, dists_dev + q0 * k);
    if (valid != EX_ALL)  // fewer than k valid rows: the "no row" padding becomes (n, +inf)
      exact_tail_kernel<<<grid_for(qn * k, 256, 1024), 256>>>(qn * k, n, ids_dev + q0 * k, dists_dev + q0 * k);
    HIPCHECK(hipGetLastError());
  }
  HIPCHECK(hipStreamSynchronize(0));
  HIPCHECK(hipFree(ws));
  return 0;
}

// What the three entry points do once the call is valid: the kernel of the row layout and of the validity form, then
// exact_run with that kernel's waves and prefetch.
static int exact_scan(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev, int self,
                      ExValid valid, const ExValidArgs &G, size_t *ids_dev, ftype *dists_dev) {
  if (!ycnt) return 0;
  gpu_init();
  const FT *pts = reinterpret_cast<const FT *>(points_dev), *y = reinterpret_cast<const FT *>(y_dev);
  FT *dd = reinterpret_cast<FT *>(dists_dev);
  const int code = layout_code(d);
  if (layout_is_generic(code)) {
    const ExScanKernel kernel = valid == EX_TAGS   ? exact_scan_generic_kernel<EX_TAGS>
                                : valid == EX_BITS ? exact_scan_generic_kernel<EX_BITS>
                                                   : exact_scan_generic_kernel<EX_ALL>;
    return exact_run(n, d, k, pts, ycnt, y, self, ids_dev, dd, true, ANN_EX_GEN_WAVES, false, valid, kernel, G);
  }
  int rc = 1;
  with_value(QueryLayouts{}, code, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    if constexpr (D != 0 && !OcCode<D>::GEN) {
      const ExScanKernel kernel = valid == EX_TAGS   ? exact_scan_kernel<D, EX_TAGS>
                                  : valid == EX_BITS ? exact_scan_kernel<D, EX_BITS>
                                                     : exact_scan_kernel<D, EX_ALL>;
      rc = exact_run(n, d, k, pts, ycnt, y, self, ids_dev, dd, false, ExCfg<D>::WAVES, ExCfg<D>::PREFETCH, valid, kernel, G);
    }
  });
  return rc;
}

extern "C" int annhip_exact_knn(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                                int self, size_t *ids_dev, ftype *dists_dev) {
  if (const int rc = exact_check(n, d, k, self)) return rc;
  return exact_scan(n, d, k, points_dev, ycnt, y_dev, self, EX_ALL, ExValidArgs{}, ids_dev, dists_dev);
}

extern "C" int annhip_exact_knn_filtered(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt,
                                         const ftype *y_dev, int self, const uint32_t *bits_dev, size_t *ids_dev,
                                         ftype *dists_dev) {
  if (const int rc = exact_check(n, d, k, self)) return rc;
  return exact_scan(n, d, k, points_dev, ycnt, y_dev, self, bits_dev ? EX_BITS : EX_ALL, ExValidArgs{NULL, bits_dev, NULL, NULL},
                    ids_dev, dists_dev);
}

extern "C" int annhip_exact_knn_tagged(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                                       int self, const uint32_t *tags_dev, const uint32_t *bits_dev,
                                       const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev,
                                       ftype *dists_dev) {
  if (!tags_dev || !qmask_dev || !qvalue_dev) return exact_refuse("tags_dev, qmask_dev and qvalue_dev must all be given");
  if (const int rc = exact_check(n, d, k, self)) return rc;
  return exact_scan(n, d, k, points_dev, ycnt, y_dev, self, EX_TAGS, ExValidArgs{tags_dev, bits_dev, qmask_dev, qvalue_dev, qvalue_dev},
                    ids_dev, dists_dev);
}

// Contract: include/ann_hip.h.  annhip_exact_knn_tagged's scan (the EX_TAGS form) with the two bounds apart.
extern "C" int annhip_exact_knn_between(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                                        int self, const uint32_t *tags_dev, const uint32_t *bits_dev,
                                        const uint32_t *qmask_dev, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                                        size_t *ids_dev, ftype *dists_dev) {
  if (!tags_dev || !qmask_dev || !qlo_dev || !qhi_dev) return exact_refuse("tags_dev, qmask_dev, qlo_dev and qhi_dev must all be given");
  if (const int rc = exact_check(n, d, k, self)) return rc;
  return exact_scan(n, d, k, points_dev, ycnt, y_dev, self, EX_TAGS, ExValidArgs{tags_dev, bits_dev, qmask_dev, qlo_dev, qhi_dev},
                    ids_dev, dists_dev);
}

extern "C" int annhip_exact_knn_host(size_t n, size_t d, size_t k, const ftype *points, size_t ycnt, const ftype *y,
                                     int self, size_t *ids, ftype *dists) {
  if (const int rc = exact_check(n, d, k, self)) return rc;
  if (!ycnt) return 0;
  RandGuard keep_callers_stream;
  gpu_init();
  FT *dp = dev_alloc<FT>(n * d), *dy = (y == points) ? dp : dev_alloc<FT>(ycnt * d);
  size_t *di = dev_alloc<size_t>(ycnt * k);
  FT *dd = dev_alloc<FT>(ycnt * k);
  HIPCHECK(hipMemcpy(dp, points, sizeof(FT) * n * d, hipMemcpyHostToDevice));
  if (dy != dp) HIPCHECK(hipMemcpy(dy, y, sizeof(FT) * ycnt * d, hipMemcpyHostToDevice));
  const int rc = annhip_exact_knn(n, d, k, reinterpret_cast<const ftype *>(dp), ycnt, reinterpret_cast<const ftype *>(dy), self, di,
                                  reinterpret_cast<ftype *>(dd));
  if (!rc) {
    HIPCHECK(hipMemcpy(ids, di, sizeof(size_t) * ycnt * k, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(dists, dd, sizeof(FT) * ycnt * k, hipMemcpyDeviceToHost));
  }
  HIPCHECK(hipFree(dp));
  if (dy != dp) HIPCHECK(hipFree(dy));
  HIPCHECK(hipFree(di));
  HIPCHECK(hipFree(dd));
  return rc;
}

// ----------------------------------------------------------------------------- the tail's scan
// One workgroup per W x ANN_EX_QB queries streams the whole tail (ann_tail_kernels.h).  in_ids / in_d: the rows to merge
// into, kin entries per query; they may be ids / dists themselves (kin == k).  Runs on s and returns at once.
// skip: tail rows [0, skip) are already in the rows to merge into (the hashed tier); ids below n + skip count as real there.
static void launch_tail_merge(annhip_index *ix, size_t Q, const FT *y, int alias, size_t k, const TagQuery *tq, size_t kin,
                              const size_t *in_ids, const FT *in_d, size_t *ids, FT *dists, unsigned long long *scored,
                              hipStream_t s, size_t skip) {
  if (!Q || ix->tail_m <= skip) return;
  const size_t d = ix->d;
  const ExValid valid = tq ? EX_TAGS : ix->filter ? EX_BITS : EX_ALL;
  TailArgs A;
  A.tail = ix->d_tail + skip * d, A.y = y, A.in_ids = in_ids, A.in_d = in_d, A.out_ids = ids, A.out_d = dists;
  A.bits = ix->filter, A.tags = tq ? tq->tags : NULL, A.qmask = tq ? tq->qmask : NULL, A.qlo = tq ? tq->qlo : NULL,
  A.qhi = tq ? tq->qhi : NULL;
  A.scored = scored;
  A.n = (u32)(ix->n + skip), A.m = (u32)(ix->tail_m - skip), A.Q = (u32)Q;
  A.d = (int)d, A.k = (int)k, A.kin = (int)kin, A.self = alias ? 1 : 0;
  auto shape = [&](bool generic, int max_waves, bool prefetch) {
    ExShape sh;
    if (!exact_shape(d, k, generic, max_waves, prefetch, valid, sh)) die("launch_tail_merge: row too long for the LDS of one CU");
    A.tile_rows = (int)sh.tile_rows, A.cap = (int)sh.cap, A.prefetch = sh.prefetch ? 1 : 0;
    return sh;
  };
  const int code = layout_code(d);
  if (layout_is_generic(code)) {
    const ExShape sh = shape(true, ANN_EX_GEN_WAVES, false);
    allow_lds(tail_merge_generic_kernel, sh.smem);
    hipLaunchKernelGGL(tail_merge_generic_kernel, dim3((unsigned)((Q + sh.W * ANN_EX_QB - 1) / (sh.W * ANN_EX_QB))),
                       dim3((unsigned)(64 * sh.W)), sh.smem, s, A);
  } else {
    with_value(QueryLayouts{}, code, [&](auto dc) {
      constexpr int D = decltype(dc)::value;
      if constexpr (D != 0 && !OcCode<D>::GEN) {
        const ExShape sh = shape(false, ExCfg<D>::WAVES, ExCfg<D>::PREFETCH);
        const dim3 grid((unsigned)((Q + sh.W * ANN_EX_QB - 1) / (sh.W * ANN_EX_QB))), block((unsigned)(64 * sh.W));
        auto go = [&](auto kernel) {
          allow_lds(kernel, sh.smem);
          hipLaunchKernelGGL(kernel, grid, block, sh.smem, s, A);
        };
        if (valid == EX_TAGS) go(tail_merge_kernel<D, EX_TAGS>);
        else if (valid == EX_BITS) go(tail_merge_kernel<D, EX_BITS>);
        else go(tail_merge_kernel<D, EX_ALL>);
      }
    });
  }
  HIPCHECK(hipGetLastError());
}

// ----------------------------------------------------------------------------- the hashed tail
// One wave per query (ann_tail_hash_kernels.h).  LDS per wave: one selection buffer of exact_shape()'s cap plus k keys,
// the any-d form's query and tree scratch, the candidate chunk; the waves come down until the workgroup fits.
static void launch_tail_hash_merge(annhip_index *ix, size_t Q, const FT *y, size_t k, const TagQuery *tq, const u32 *codes,
                                   const unsigned char *pbits, int pb, size_t *ids, FT *dists, unsigned long long *scored,
                                   hipStream_t s) {
  if (!Q || !ix->tail_mh) return;
  const size_t d = ix->d;
  const ExValid valid = tq ? EX_TAGS : ix->filter ? EX_BITS : EX_ALL;
  TailHashArgs A;
  A.t.tail = ix->d_tail, A.t.y = y, A.t.in_ids = ids, A.t.in_d = dists, A.t.out_ids = ids, A.t.out_d = dists;
  A.t.bits = ix->filter, A.t.tags = tq ? tq->tags : NULL, A.t.qmask = tq ? tq->qmask : NULL, A.t.qlo = tq ? tq->qlo : NULL,
  A.t.qhi = tq ? tq->qhi : NULL;
  A.t.scored = scored;
  A.t.n = (u32)ix->n, A.t.m = (u32)ix->tail_m, A.t.Q = (u32)Q;
  A.t.d = (int)d, A.t.k = (int)k, A.t.kin = (int)k, A.t.self = 0, A.t.tile_rows = 0, A.t.prefetch = 0;
  A.codes = codes, A.pbits = pbits, A.pb = pbits ? pb : 0;
  A.tcodes = ix->tail_codes, A.off = ix->tail_off, A.rows = ix->tail_rows, A.mh = (u32)ix->tail_mh, A.T = ix->T, A.ds = (int)ix->ds;
  struct Shape {
    size_t W, smem;
  };
  auto shape = [&](bool generic, int max_waves) {
    ExShape sh;
    if (!exact_shape(d, k, generic, max_waves, false, valid, sh)) die("launch_tail_hash_merge: row too long for the LDS of one CU");
    A.t.cap = (int)sh.cap;
    size_t np = ANN_EX_GEN_ELEMS / d;
    np = np < 1 ? 1 : (np > ANN_WAVE ? ANN_WAVE : np);
    const size_t wave_bytes = sizeof(Key) * (sh.cap + k) + (generic ? (((1 + np) * d * sizeof(FT) + 15) & ~(size_t)15) : 0) +
                              sizeof(u32) * thash_wave_words(ix->T);
    Shape r{(size_t)max_waves, 0};
    while (r.W > 1 && r.W * wave_bytes > ANN_EX_LDS_BUDGET) r.W--;
    r.smem = r.W * wave_bytes;
    if (r.smem > 160 * 1024) die("launch_tail_hash_merge: row too long for the LDS of one CU");
    return r;
  };
  const int code = layout_code(d);
  if (layout_is_generic(code)) {
    const Shape sh = shape(true, ANN_EX_GEN_WAVES);
    allow_lds(tail_hash_merge_generic_kernel, sh.smem);
    hipLaunchKernelGGL(tail_hash_merge_generic_kernel, dim3((unsigned)((Q + sh.W - 1) / sh.W)), dim3((unsigned)(64 * sh.W)), sh.smem,
                       s, A);
  } else {
    with_value(QueryLayouts{}, code, [&](auto dc) {
      constexpr int D = decltype(dc)::value;
      if constexpr (D != 0 && !OcCode<D>::GEN) {
        const Shape sh = shape(false, ExCfg<D>::WAVES);
        const dim3 grid((unsigned)((Q + sh.W - 1) / sh.W)), block((unsigned)(64 * sh.W));
        auto go = [&](auto kernel) {
          allow_lds(kernel, sh.smem);
          hipLaunchKernelGGL(kernel, grid, block, sh.smem, s, A);
        };
        if (valid == EX_TAGS) go(tail_hash_merge_kernel<D, EX_TAGS>);
        else if (valid == EX_BITS) go(tail_hash_merge_kernel<D, EX_BITS>);
        else go(tail_hash_merge_kernel<D, EX_ALL>);
      }
    });
  }
  HIPCHECK(hipGetLastError());
}

// Contract: include/ann_hip.h.  Codes by the hash launch itself, then count / scan / place per try.
extern "C" int annhip_index_hash_tail(annhip_index *ix) {
  const char *why = tail_refusal(ix, 0);
  if (!why && (unsigned long long)ix->T * ix->tail_m >= 0xFFFFFFF0ull) why = "tries x tail rows must fit 32 bits";
  if (why) {
    fprintf(stderr, "annhip_index_hash_tail: %s\n", why);
    return -1;
  }
  const size_t m = ix->tail_m;
  if (!m) return 0;
  HIPCHECK(hipDeviceSynchronize());
  drop_tail_hash(ix);
  const size_t items = m * (size_t)ix->T;
  const u32 stride = (u32)(((size_t)1 << ix->ds) + 1);
  ix->tail_codes = dev_alloc<u32>(items);
  ix->tail_off = dev_alloc<u32>((size_t)ix->T * stride);
  ix->tail_rows = dev_alloc<u32>(items);
  // the code of a non-aliased fixed-mode query equal to the row: the query path's own hash launch over the tail
  launch_codes(query_params(ix), m, ix->d_tail, ix->tail_codes, 0);
  HIPCHECK(hipMemsetAsync(ix->tail_off, 0, sizeof(u32) * (size_t)ix->T * stride, 0));
  thash_count_kernel<<<grid_for(items, 256, 4096), 256>>>(items, ix->tail_codes, ix->T, stride, ix->tail_off);
  thash_scan_kernel<<<ix->T, 1024>>>(ix->tail_off, stride, (u32)m);
  thash_place_kernel<<<grid_for(items, 256, 4096), 256>>>(items, ix->tail_codes, ix->T, stride, ix->tail_off, ix->tail_rows);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  ix->tail_mh = m;
  return 0;
}

// What the annhip_index_exact_query* entries refuse before they scan, in their order: a resharded index; then the entry's
// own test of its pointers (args: its text or NULL) and, for a tagged call, an index without tags -- the other way round
// for annhip_index_exact_query_tagged (tags_first).
static int index_exact_refusal(const annhip_index *ix, const char *args, bool tagged, bool tags_first = false) {
  const char *no_tags = tagged && !ix->tags ? NO_TAGS : NULL;
  const char *why = ix->lo != 0 || ix->hi != ix->n ? "the index does not hold rows [0, n) (resharded)"
                    : tags_first && no_tags        ? no_tags
                    : args                         ? args
                                                   : no_tags;
  return why ? exact_refuse(why) : 0;
}

// The three exact scans of an index (its entries have refused what index_exact_refusal names): over the built rows as
// before, then -- where rows have been appended -- the tail's scan merged in.  kq = the k of the call.  qmask_dev == NULL:
// untagged; the pair form passes its value array for both bounds.
static int index_exact(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t kq, const uint32_t *qmask_dev,
                       const uint32_t *qlo_dev, const uint32_t *qhi_dev, size_t *ids_dev, ftype *dists_dev) {
  const ftype *pts = reinterpret_cast<const ftype *>(ix->d_points);
  auto built = [&](size_t k, size_t *ids, ftype *dists) {
    if (!qmask_dev) return annhip_exact_knn_filtered(ix->n, ix->d, k, pts, ycnt, y_dev, alias, ix->filter, ids, dists);
    return annhip_exact_knn_between(ix->n, ix->d, k, pts, ycnt, y_dev, alias, ix->tags, ix->filter, qmask_dev, qlo_dev, qhi_dev, ids,
                                    dists);
  };
  if (!ix->tail_m) return built(kq, ids_dev, dists_dev);
  if (const int rc = exact_check(n_total(ix), ix->d, kq, alias)) return rc;
  if (!ycnt) return 0;
  const size_t kin = std::min(kq, ix->n - (alias && ix->n ? 1 : 0));  // what the built rows can fill
  const TagQuery tq{ix->tags, qmask_dev, qlo_dev, qhi_dev};
  const FT *y = reinterpret_cast<const FT *>(y_dev);
  FT *dd = reinterpret_cast<FT *>(dists_dev);
  int rc = 0;
  if (kin == kq) {
    if ((rc = built(kq, ids_dev, dists_dev))) return rc;
    launch_tail_merge(ix, ycnt, y, alias, kq, qmask_dev ? &tq : NULL, kq, ids_dev, dd, ids_dev, dd, NULL, 0);
  } else {  // fewer built rows than kq: their scan goes to a buffer of its own
    size_t *ti = kin ? dev_alloc<size_t>(ycnt * kin) : NULL;
    FT *td = kin ? dev_alloc<FT>(ycnt * kin) : NULL;
    if (kin) rc = built(kin, ti, reinterpret_cast<ftype *>(td));
    if (!rc) launch_tail_merge(ix, ycnt, y, alias, kq, qmask_dev ? &tq : NULL, kin, ti, td, ids_dev, dd, NULL, 0);
    HIPCHECK(hipStreamSynchronize(0));
    if (ti) HIPCHECK(hipFree(ti));
    if (td) HIPCHECK(hipFree(td));
  }
  HIPCHECK(hipStreamSynchronize(0));
  return rc;
}

extern "C" int annhip_index_exact_query(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t *ids_dev,
                                        ftype *dists_dev) {
  if (const int rc = index_exact_refusal(ix, NULL, false)) return rc;
  return index_exact(ix, ycnt, y_dev, alias, ix->k, NULL, NULL, NULL, ids_dev, dists_dev);
}

extern "C" int annhip_index_exact_query_tagged(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias,
                                               const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev,
                                               ftype *dists_dev) {
  const char *args = !qmask_dev || !qvalue_dev ? "tags_dev, qmask_dev and qvalue_dev must all be given" : NULL;
  if (const int rc = index_exact_refusal(ix, args, true, true)) return rc;
  return index_exact(ix, ycnt, y_dev, alias, ix->k, qmask_dev, qvalue_dev, qvalue_dev, ids_dev, dists_dev);
}

// Contract: include/ann_hip.h.  The three exact scans with a k of the call's own; their refusals.
extern "C" int annhip_index_exact_query_k(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t kq,
                                          const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev,
                                          ftype *dists_dev) {
  if (const int rc = index_exact_refusal(ix, pair_or_neither(qmask_dev, qvalue_dev), qmask_dev != NULL)) return rc;
  return index_exact(ix, ycnt, y_dev, alias, kq, qmask_dev, qvalue_dev, qvalue_dev, ids_dev, dists_dev);
}

// The end of the exact radius calls: the rows cut at the radius (ann_radius_kernels.h), then the null stream drained.
static int exact_trim(const annhip_index *ix, size_t ycnt, size_t kcap, const ftype *radius_dev, size_t *ids_dev, ftype *dists_dev,
                      uint32_t *counts_dev) {
  launch_radius_trim(ycnt, kcap, n_total(ix), reinterpret_cast<const FT *>(radius_dev), ids_dev, reinterpret_cast<FT *>(dists_dev),
                     counts_dev, 0);
  HIPCHECK(hipStreamSynchronize(0));
  return 0;
}

// Contract: include/ann_hip.h.  annhip_index_exact_query_k's path, then the trim: the ground truth of annhip_query_radius.
// Synchronous, on the null stream.
extern "C" int annhip_index_exact_query_radius(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t kcap,
                                               const ftype *radius_dev, const uint32_t *qmask_dev, const uint32_t *qvalue_dev,
                                               size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev) {
  const char *args = pair_or_neither(qmask_dev, qvalue_dev);
  if (!args && (!radius_dev || !ids_dev || !dists_dev)) args = "radius_dev, ids_dev and dists_dev must all be given";
  if (const int rc = index_exact_refusal(ix, args, qmask_dev != NULL)) return rc;
  if (const int rc = index_exact(ix, ycnt, y_dev, alias, kcap, qmask_dev, qvalue_dev, qvalue_dev, ids_dev, dists_dev)) return rc;
  return exact_trim(ix, ycnt, kcap, radius_dev, ids_dev, dists_dev, counts_dev);
}

// Contract: include/ann_hip.h.  annhip_index_exact_query_k's scans under the range predicate, then -- with a radius --
// annhip_index_exact_query_radius' trim.  Synchronous, on the null stream.
extern "C" int annhip_index_exact_query_between(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t kq,
                                                const ftype *radius_dev, const uint32_t *qmask_dev, const uint32_t *qlo_dev,
                                                const uint32_t *qhi_dev, size_t *ids_dev, ftype *dists_dev,
                                                uint32_t *counts_dev) {
  const char *args = !qmask_dev || !qlo_dev || !qhi_dev       ? "qmask_dev, qlo_dev and qhi_dev must all be given"
                     : radius_dev && (!ids_dev || !dists_dev) ? "radius_dev needs ids_dev and dists_dev"
                                                              : NULL;
  if (const int rc = index_exact_refusal(ix, args, true)) return rc;
  if (const int rc = index_exact(ix, ycnt, y_dev, alias, kq, qmask_dev, qlo_dev, qhi_dev, ids_dev, dists_dev)) return rc;
  return radius_dev ? exact_trim(ix, ycnt, kq, radius_dev, ids_dev, dists_dev, counts_dev) : 0;
}

// Contract: include/ann_hip.h.  annhip_index_exact_query_k / _between with kq = list into a buffer of the call's own, then
// the collapse into the caller's arrays: the ground truth of annhip_query_grouped.  Synchronous, on the null stream.
extern "C" int annhip_index_exact_query_grouped(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t list, size_t k,
                                                size_t per_group, uint32_t gmask, const uint32_t *qmask_dev, const uint32_t *qlo_dev,
                                                const uint32_t *qhi_dev, size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev,
                                                uint8_t *short_dev) {
  const char *args = all_or_none(qmask_dev, qlo_dev, qhi_dev);
  if (!args) args = group_refusal(list, k, per_group, gmask);
  if (!args && (!ids_dev || !dists_dev)) args = "ids_dev and dists_dev must both be given";
  if (const int rc = index_exact_refusal(ix, args, true)) return rc;  // (tagged: the group key needs the tags)
  if (const int rc = exact_check(n_total(ix), ix->d, list, alias)) return rc;
  if (!ycnt) return 0;
  size_t *li = dev_alloc<size_t>(ycnt * list);
  FT *ld = dev_alloc<FT>(ycnt * list);
  const int rc = index_exact(ix, ycnt, y_dev, alias, list, qmask_dev, qlo_dev, qhi_dev, li, reinterpret_cast<ftype *>(ld));
  if (!rc)
    launch_collapse(ycnt, list, GroupCall{k, per_group, gmask, counts_dev, short_dev}, ix->tags, n_total(ix), n_total(ix), li, ld,
                    ids_dev, reinterpret_cast<FT *>(dists_dev), 0);
  HIPCHECK(hipStreamSynchronize(0));
  HIPCHECK(hipFree(li));
  HIPCHECK(hipFree(ld));
  return rc;
}

// ----------------------------------------------------------------------------- the sorted scan (annhip_query_sorted)
// Contract: include/ann_hip.h.  Kernels: ann_sorted_kernels.h.  Everything goes to the call's stream; nothing waits.
static void launch_tag_runs(const annhip_index *ix, size_t Q, const u32 *qlo, const u32 *qhi, u32 *start, u32 *len, hipStream_t s) {
  if (!Q) return;
  hipLaunchKernelGGL(tag_runs_kernel, dim3(grid_for(Q, 256, 1u << 30)), dim3(256), 0, s, ix->ord_keys, (u32)ix->ord_ms, (u32)Q, qlo,
                     qhi, start, len);
  HIPCHECK(hipGetLastError());
}
extern "C" int annhip_tag_runs(annhip_index *ix, void *hip_stream, size_t ycnt, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                               uint32_t *start_dev, uint32_t *len_dev) {
  if (!ix->ord_perm || !qlo_dev || !qhi_dev || !start_dev || !len_dev || ycnt >= 0xFFFFFFF0ull) return -1;
  launch_tag_runs(ix, ycnt, qlo_dev, qhi_dev, start_dev, len_dev, (hipStream_t)hip_stream);
  return 0;
}

// the scan's launch for this index's row length: false where a row is too long for the LDS of one CU
// part != NULL: the set form -- list has four words per entry and entry e's result goes to part[slot(e)][k]
static bool launch_sorted_scan(annhip_index *ix, size_t Q, const FT *y, int alias, size_t k, const u32 *list, size_t *ids, FT *dists,
                               hipStream_t s, bool dry, Key *part = NULL) {
  const size_t d = ix->d;
  const ExValid valid = ix->filter ? EX_BITS : EX_ALL;
  SortedArgs SA;
  TailArgs &A = SA.t;
  A.tail = ix->d_tail, A.y = y, A.in_ids = NULL, A.in_d = NULL, A.out_ids = ids, A.out_d = dists;
  A.bits = ix->filter, A.tags = NULL, A.qmask = A.qlo = A.qhi = NULL;
  A.scored = ix->profile == 1 ? ix->d_rows + 8 : NULL;
  A.n = (u32)ix->n, A.m = (u32)ix->tail_m, A.Q = (u32)Q;
  A.d = (int)d, A.k = (int)k, A.kin = 0, A.self = alias ? 1 : 0, A.prefetch = 0;
  SA.points = ix->d_points, SA.perm = ix->ord_perm, SA.list = list;
  bool ok = true;
  auto shape = [&](bool generic, int max_waves) {
    ExShape sh;
    ok = exact_shape(d, k, generic, max_waves, false, valid, sh, true);
    A.tile_rows = (int)sh.tile_rows, A.cap = (int)sh.cap;
    return sh;
  };
  const int code = layout_code(d);
  if (layout_is_generic(code)) {
    const ExShape sh = shape(true, ANN_EX_GEN_WAVES);
    if (!ok || dry) return ok;
    const dim3 grid((unsigned)((Q + sh.W * ANN_EX_QB - 1) / (sh.W * ANN_EX_QB))), block((unsigned)(64 * sh.W));
    if (part) {
      allow_lds(sorted_scan_generic_kernel<true>, sh.smem);
      hipLaunchKernelGGL(sorted_scan_generic_kernel<true>, grid, block, sh.smem, s, SortedSetArgs{SA, part});
    } else {
      allow_lds(sorted_scan_generic_kernel<false>, sh.smem);
      hipLaunchKernelGGL(sorted_scan_generic_kernel<false>, grid, block, sh.smem, s, SA);
    }
  } else {
    with_value(QueryLayouts{}, code, [&](auto dc) {
      constexpr int D = decltype(dc)::value;
      if constexpr (D != 0 && !OcCode<D>::GEN) {
        const ExShape sh = shape(false, ExCfg<D>::WAVES);
        if (!ok || dry) return;
        const dim3 grid((unsigned)((Q + sh.W * ANN_EX_QB - 1) / (sh.W * ANN_EX_QB))), block((unsigned)(64 * sh.W));
        auto go = [&](auto kernel, auto args) {
          allow_lds(kernel, sh.smem);
          hipLaunchKernelGGL(kernel, grid, block, sh.smem, s, args);
        };
        if (part && valid == EX_BITS) go(sorted_scan_kernel<D, EX_BITS, true>, SortedSetArgs{SA, part});
        else if (part) go(sorted_scan_kernel<D, EX_ALL, true>, SortedSetArgs{SA, part});
        else if (valid == EX_BITS) go(sorted_scan_kernel<D, EX_BITS, false>, SA);
        else go(sorted_scan_kernel<D, EX_ALL, false>, SA);
      }
    });
  }
  if (ok && !dry) HIPCHECK(hipGetLastError());
  return ok;
}

extern "C" long annhip_query_sorted(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                                    size_t kq, const ftype *radius_dev, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                                    size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev) {
  const size_t nt = n_total(ix);
  const char *why = !(ix->lo == 0 && ix->hi == ix->n) ? "the index does not hold rows [0, n) on this device (resharded)"
                    : !ix->ord_perm ? "the index has no tag order (annhip_index_sort_tags)"
                    : !y_dev || !qlo_dev || !qhi_dev || !ids_dev || !dists_dev ? "y_dev, qlo_dev, qhi_dev, ids_dev and dists_dev must all be given"
                    : kq < 1 || kq > 1024 ? "kq must be in 1..1024"
                    : kq > nt - (alias && nt ? 1 : 0) ? "kq exceeds the number of rows a query can be given"
                    : ycnt >= 0xFFFFFFF0ull / 3 ? "query batch too large"
                    : !launch_sorted_scan(ix, ycnt, NULL, alias, kq, NULL, NULL, NULL, 0, true) ? "row too long for the LDS of one CU" : NULL;
  if (why) {
    fprintf(stderr, "annhip_query_sorted: %s\n", why);
    return -2;
  }
  if (!ycnt) return 0;
  hipStream_t s = (hipStream_t)hip_stream;
  annhip_workspace &w = ws ? *ws : ix->ws;
  const FT *y = reinterpret_cast<const FT *>(y_dev);
  FT *dd = reinterpret_cast<FT *>(dists_dev);
  u32 *start = (u32 *)w.sorted.need(sizeof(u32) * ycnt * 6), *len = start + ycnt, *list = len + ycnt, *qmask = list + 3 * ycnt;
  launch_tag_runs(ix, ycnt, qlo_dev, qhi_dev, start, len, s);
  hipLaunchKernelGGL(sorted_order_kernel, dim3((unsigned)((ycnt + 255) / 256)), dim3(256), 0, s, (u32)ycnt, start, len, list);
  HIPCHECK(hipGetLastError());
  launch_sorted_scan(ix, ycnt, y, alias, kq, list, ids_dev, dd, s, false);
  if (nt > ix->ord_ms) {  // the rows appended since the sort: the tail's own scan under the same predicate, merged in place
    sorted_fill_kernel<<<grid_for(ycnt, 256, 1024), 256, 0, s>>>((u32)ycnt, ix->ord_mask, qmask);
    HIPCHECK(hipGetLastError());
    const TagQuery tq{ix->tags, qmask, qlo_dev, qhi_dev};
    launch_tail_merge(ix, ycnt, y, alias, kq, &tq, kq, ids_dev, dd, ids_dev, dd, NULL, s, ix->ord_ms - ix->n);
  }
  if (radius_dev) launch_radius_trim(ycnt, kq, nt, reinterpret_cast<const FT *>(radius_dev), ids_dev, dd, counts_dev, s);
  return 0;
}

// ----------------------------------------------------------------------------- sets of intervals (annhip_query_sorted_set)
// Contract: include/ann_hip.h.  Kernels: the end of ann_sorted_kernels.h.
static const char *set_offsets_refusal(size_t ycnt, const uint32_t *off) {
  if (off[0] != 0) return "off_host[0] must be 0";
  for (size_t q = 0; q < ycnt; q++) {
    if (off[q + 1] < off[q]) return "off_host must not decrease";
    if (off[q + 1] - off[q] > ANN_SET_MAX) return "a query has more than 256 intervals";
  }
  return NULL;
}
// the call's offsets -> doff on s, through the workspace's pinned buffer: waits for the previous call's upload only
static void set_upload_offsets(annhip_workspace &w, size_t ycnt, const uint32_t *off_host, u32 *doff, hipStream_t s) {
  if (w.sset_ev) HIPCHECK(hipEventSynchronize(w.sset_ev));
  else HIPCHECK(hipEventCreateWithFlags(&w.sset_ev, hipEventDisableTiming));
  const size_t bytes = sizeof(u32) * (ycnt + 1);
  void *pin = w.spin.need(bytes);
  memcpy(pin, off_host, bytes);
  HIPCHECK(hipMemcpyAsync(doff, pin, bytes, hipMemcpyHostToDevice, s));
  HIPCHECK(hipEventRecord(w.sset_ev, s));
}
static void launch_set_runs(const annhip_index *ix, size_t Q, const u32 *doff, const u32 *lo, const u32 *hi, u32 S, u32 *nlo, u32 *nhi,
                            u32 *start, u32 *len, u32 *qof, u32 *cnt, hipStream_t s) {
  hipLaunchKernelGGL(set_runs_kernel, dim3(grid_for(Q, 64, 1u << 30)), dim3(64), 0, s, ix->ord_keys, (u32)ix->ord_ms, (u32)Q, doff, lo, hi,
                     S, nlo, nhi, start, len, qof, cnt);
  HIPCHECK(hipGetLastError());
}

extern "C" int annhip_tag_runs_set(annhip_index *ix, void *hip_stream, size_t ycnt, const uint32_t *off_host, const uint32_t *lo_dev,
                                   const uint32_t *hi_dev, uint32_t *start_dev, uint32_t *len_dev) {
  const char *why = !ix->ord_perm ? "the index has no tag order (annhip_index_sort_tags)"
                    : !off_host || !lo_dev || !hi_dev || !start_dev || !len_dev ? "off_host, lo_dev, hi_dev, start_dev and len_dev must all be given"
                    : ycnt >= 0xFFFFFFF0ull ? "query batch too large" : set_offsets_refusal(ycnt, off_host);
  if (why) {
    fprintf(stderr, "annhip_tag_runs_set: %s\n", why);
    return -1;
  }
  if (!ycnt || !off_host[ycnt]) return 0;
  hipStream_t s = (hipStream_t)hip_stream;
  u32 *doff = (u32 *)ix->ws.sset.need(sizeof(u32) * (ycnt + 1));
  set_upload_offsets(ix->ws, ycnt, off_host, doff, s);
  launch_set_runs(ix, ycnt, doff, lo_dev, hi_dev, 0, NULL, NULL, start_dev, len_dev, NULL, NULL, s);
  return 0;
}

extern "C" long annhip_query_sorted_set(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev,
                                        int alias, size_t kq, const ftype *radius_dev, const uint32_t *off_host,
                                        const uint32_t *lo_dev, const uint32_t *hi_dev, size_t split_rows, size_t *ids_dev,
                                        ftype *dists_dev, uint32_t *counts_dev) {
  const size_t nt = n_total(ix), slots_max = (size_t)1 << 27;
  const char *why = !(ix->lo == 0 && ix->hi == ix->n) ? "the index does not hold rows [0, n) on this device (resharded)"
                    : !ix->ord_perm ? "the index has no tag order (annhip_index_sort_tags)"
                    : !y_dev || !off_host || !lo_dev || !hi_dev || !ids_dev || !dists_dev
                        ? "y_dev, off_host, lo_dev, hi_dev, ids_dev and dists_dev must all be given"
                    : kq < 1 || kq > 1024 ? "kq must be in 1..1024"
                    : kq > nt - (alias && nt ? 1 : 0) ? "kq exceeds the number of rows a query can be given"
                    : ycnt >= 0xFFFFFFF0ull / 4 ? "query batch too large"
                    : (split_rows && split_rows < 64) || split_rows > 0xFFFFFFFFull ? "split_rows must be 0 or in 64..2^32-1"
                    : !launch_sorted_scan(ix, ycnt, NULL, alias, kq, NULL, NULL, NULL, 0, true) ? "row too long for the LDS of one CU"
                                                                                                 : set_offsets_refusal(ycnt, off_host);
  const size_t T = why ? 0 : off_host[ycnt];  // interval slots
  if (!why && !split_rows && T * kq > slots_max) why = "more than 2^27 partial slots (entries x kq)";
  if (why) {
    fprintf(stderr, "annhip_query_sorted_set: %s\n", why);
    return -2;
  }
  if (!ycnt) return 0;
  hipStream_t s = (hipStream_t)hip_stream;
  annhip_workspace &w = ws ? *ws : ix->ws;
  const FT *y = reinterpret_cast<const FT *>(y_dev);
  FT *dd = reinterpret_cast<FT *>(dists_dev);
  const u32 S = (u32)split_rows;
  size_t maxset = 0;
  for (size_t q = 0; q < ycnt; q++) maxset = std::max<size_t>(maxset, off_host[q + 1] - off_host[q]);
  // staging sized by the interval count: off[Q + 1], nlo / nhi / start / len / qof [T], cnt -> eoff [T + 1], qmask / rlo / rhi [Q]
  u32 *doff = (u32 *)w.sset.need(sizeof(u32) * ((ycnt + 1) + 6 * T + 1 + 3 * ycnt));
  u32 *nlo = doff + ycnt + 1, *nhi = nlo + T, *start = nhi + T, *len = start + T, *qof = len + T, *cnt = qof + T;
  u32 *qmask = cnt + T + 1, *rlo = qmask + ycnt, *rhi = rlo + ycnt;
  set_upload_offsets(w, ycnt, off_host, doff, s);
  size_t E = T;
  if (T) {
    launch_set_runs(ix, ycnt, doff, lo_dev, hi_dev, S, nlo, nhi, start, len, qof, cnt, s);
    if (S) {  // eoff := the exclusive prefix sums of the piece counts; E = eoff[T] comes back to the host
      u32 e32 = 0;
      HIPCHECK(hipMemsetAsync(cnt + T, 0, sizeof(u32), s));
      hipLaunchKernelGGL(tsort_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, T + 1);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(&e32, cnt + T, sizeof e32, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      E = e32;
      if (E * kq > slots_max || E >= 0xFFFFFFF0ull / 4) {
        fprintf(stderr, "annhip_query_sorted_set: more than 2^27 partial slots (entries x kq)\n");
        return -2;
      }
    }
  }
  const u32 *eoff = S ? cnt : NULL;
  Key *part = NULL;
  u32 *head = NULL;
  // sized by the entry count and the batch (w.spart): the partial lists first (16-byte aligned), then -- where rows have
  // been appended since the sort -- two rows of kq per query twice (a second result and one rank's fresh rows), then eq /
  // es / ee / head [E], two (key, slot) pairs of arrays for the sort, its histogram, the list
  const bool fresh = nt > ix->ord_ms && maxset;
  const u32 nblk = (u32)((E + ANN_SORT_ITEMS - 1) / ANN_SORT_ITEMS);
  const size_t part_bytes = (sizeof(Key) * E * kq + 15) & ~(size_t)15;
  const size_t row_i = sizeof(size_t) * ycnt * kq, row_d = (sizeof(FT) * ycnt * kq + 15) & ~(size_t)15;
  unsigned char *base = (unsigned char *)w.spart.need(part_bytes + (fresh ? 2 * (row_i + row_d) : 0) +
                                                      sizeof(u32) * (12 * E + (size_t)256 * nblk));
  size_t *tmp_i = reinterpret_cast<size_t *>(base + part_bytes), *fr_i = reinterpret_cast<size_t *>(base + part_bytes + row_i);
  FT *tmp_d = reinterpret_cast<FT *>(base + part_bytes + 2 * row_i), *fr_d = reinterpret_cast<FT *>(base + part_bytes + 2 * row_i + row_d);
  if (E) {
    part = reinterpret_cast<Key *>(base);
    u32 *eq = reinterpret_cast<u32 *>(base + part_bytes + (fresh ? 2 * (row_i + row_d) : 0)), *es = eq + E, *ee = es + E;
    head = ee + E;
    u32 *k0 = head + E, *v0 = k0 + E, *k1 = v0 + E, *v1 = k1 + E, *hist = v1 + E, *list = hist + (size_t)256 * nblk;
    hipLaunchKernelGGL(set_pieces_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, (u32)T, start, len, qof, eoff, S, eq, es, ee);
    HIPCHECK(hipMemsetAsync(head, 0, sizeof(u32) * E, s));
    hipLaunchKernelGGL(tsort_init_kernel, dim3(grid_for(E, 256, 4096)), dim3(256), 0, s, (u32)E, es, 0xFFFFFFFFu, k0, v0);
    for (int shift = 0; shift < 32 && ((u64)ix->ord_ms >> shift); shift += 8) {  // a start is at most ord_ms
      hipLaunchKernelGGL(tsort_count_kernel, dim3(nblk), dim3(64), 0, s, k0, (u32)E, shift, nblk, hist);
      hipLaunchKernelGGL(tsort_scan_kernel, dim3(1), dim3(1024), 0, s, hist, (size_t)256 * nblk);
      hipLaunchKernelGGL(tsort_place_kernel, dim3(nblk), dim3(64), 0, s, k0, v0, (u32)E, shift, nblk, hist, k1, v1);
      std::swap(k0, k1), std::swap(v0, v1);
    }
    hipLaunchKernelGGL(set_list_kernel, dim3(grid_for(E, 256, 4096)), dim3(256), 0, s, (u32)E, v0, eq, es, ee, list);
    HIPCHECK(hipGetLastError());
    launch_sorted_scan(ix, E, y, alias, kq, list, NULL, NULL, s, false, part);
  }
  // The rows appended since the sort compete once per interval rank (the intervals of a query are disjoint): their scan
  // under rank r's intervals, from nothing, then a two-row merge into the running result.  The result alternates between
  // the output and a second buffer; the merge of the partial lists starts where an even count of steps is left.
  size_t *cur_i = fresh && (maxset & 1) ? tmp_i : ids_dev, *oth_i = cur_i == ids_dev ? tmp_i : ids_dev;
  FT *cur_d = cur_i == ids_dev ? dd : tmp_d, *oth_d = cur_i == ids_dev ? tmp_d : dd;
  hipLaunchKernelGGL(sorted_set_merge_kernel, dim3((unsigned)((ycnt + 3) / 4)), dim3(256), 0, s, part, head, (u32)ycnt, doff, eoff,
                     (int)kq, nt, cur_i, cur_d);
  HIPCHECK(hipGetLastError());
  if (fresh) {
    sorted_fill_kernel<<<grid_for(ycnt, 256, 1024), 256, 0, s>>>((u32)ycnt, ix->ord_mask, qmask);
    const TagQuery tq{ix->tags, qmask, rlo, rhi};
    for (size_t r = 0; r < maxset; r++) {
      hipLaunchKernelGGL(set_rank_kernel, dim3(grid_for(ycnt, 256, 1u << 30)), dim3(256), 0, s, (u32)ycnt, (u32)r, doff, nlo, nhi, rlo, rhi);
      HIPCHECK(hipGetLastError());
      launch_tail_merge(ix, ycnt, y, alias, kq, &tq, 0, NULL, NULL, fr_i, fr_d, NULL, s, ix->ord_ms - ix->n);
      hipLaunchKernelGGL(set_merge2_kernel, dim3((unsigned)((ycnt + 3) / 4)), dim3(256), 0, s, (u32)ycnt, (int)kq, nt, cur_i, cur_d, fr_i,
                         fr_d, oth_i, oth_d);
      HIPCHECK(hipGetLastError());
      std::swap(cur_i, oth_i), std::swap(cur_d, oth_d);
    }
  }
  if (radius_dev) launch_radius_trim(ycnt, kq, nt, reinterpret_cast<const FT *>(radius_dev), ids_dev, dd, counts_dev, s);
  return (long)E;
}

// ----------------------------------------------------------------------------- rerank (annhip_rerank)
// Contract: include/ann_hip.h.  Kernels: ann_rerank_kernels.h.  One wave per query; LDS per wave: one selection buffer of
// exact_shape()'s cap plus k keys, the any-d form's query and tree scratch, the id list; the waves come down until the
// workgroup fits.  No workspace, nothing synchronised: the launch goes to s and the call returns.
static int rerank_refuse(const char *who, const char *why) {
  fprintf(stderr, "%s: %s\n", who, why);
  return -1;
}
static int launch_rerank(const char *who, size_t n, size_t m, size_t d, const FT *points, const FT *tail, size_t Q, const FT *y,
                         size_t ccnt, const size_t *cand, size_t k, size_t *ids, FT *dists, hipStream_t s) {
  if (k < 1 || k > 1024) return rerank_refuse(who, "k must be in 1..1024");
  if (ccnt < 1 || ccnt > 1024) return rerank_refuse(who, "ccnt must be in 1..1024");
  if (d < 1) return rerank_refuse(who, "d must be at least 1");
  if (n + m >= 0xFFFFFFF0ull || n + m < n) return rerank_refuse(who, "row ids must fit 32 bits");
  if (Q >= 0xFFFFFFF0ull) return rerank_refuse(who, "ycnt must fit 32 bits");
  const int code = layout_code(d);
  const bool generic = layout_is_generic(code);
  struct Shape {
    size_t W, smem, cap;
  };
  auto shape = [&](int max_waves) {
    ExShape sh;
    (void)exact_shape(d, k, generic, max_waves, false, EX_ALL, sh);  // for cap: no row tile here, the fit is tested below
    size_t np = ANN_EX_GEN_ELEMS / d;
    np = np < 1 ? 1 : (np > ANN_WAVE ? ANN_WAVE : np);
    const size_t wave_bytes = sizeof(Key) * (sh.cap + k) + (generic ? (((1 + np) * d * sizeof(FT) + 15) & ~(size_t)15) : 0) +
                              sizeof(u32) * rerank_wave_words(ccnt);
    Shape r{(size_t)max_waves, 0, sh.cap};
    while (r.W > 1 && r.W * wave_bytes > ANN_EX_LDS_BUDGET) r.W--;
    r.smem = r.W * wave_bytes;
    return r;
  };
  int max_waves = ANN_EX_GEN_WAVES;
  if (!generic)
    with_value(QueryLayouts{}, code, [&](auto dc) {
      constexpr int D = decltype(dc)::value;
      if constexpr (D != 0 && !OcCode<D>::GEN) max_waves = ExCfg<D>::WAVES;
    });
  const Shape sh = shape(max_waves);
  if (sh.smem > 160 * 1024) return rerank_refuse(who, "row too long for the LDS of one CU");
  if (!Q) return 0;
  gpu_init();
  RerankArgs A = {};
  A.t.tail = tail, A.t.y = y, A.t.out_ids = ids, A.t.out_d = dists;
  A.t.n = (u32)n, A.t.m = (u32)m, A.t.Q = (u32)Q;
  A.t.d = (int)d, A.t.k = (int)k, A.t.kin = 0, A.t.cap = (int)sh.cap;
  A.points = points, A.cand = cand, A.ccnt = (int)ccnt;
  const dim3 grid((unsigned)((Q + sh.W - 1) / sh.W)), block((unsigned)(64 * sh.W));
  if (generic) {
    allow_lds(rerank_generic_kernel, sh.smem);
    hipLaunchKernelGGL(rerank_generic_kernel, grid, block, sh.smem, s, A);
  } else {
    with_value(QueryLayouts{}, code, [&](auto dc) {
      constexpr int D = decltype(dc)::value;
      if constexpr (D != 0 && !OcCode<D>::GEN) {
        allow_lds(rerank_kernel<D>, sh.smem);
        hipLaunchKernelGGL(rerank_kernel<D>, grid, block, sh.smem, s, A);
      }
    });
  }
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int annhip_rerank(size_t n, size_t d, const ftype *points_dev, size_t ycnt, const ftype *y_dev, size_t ccnt,
                             const size_t *cand_dev, size_t k, size_t *ids_dev, ftype *dists_dev, void *hip_stream) {
  return launch_rerank("annhip_rerank", n, 0, d, reinterpret_cast<const FT *>(points_dev), NULL, ycnt,
                       reinterpret_cast<const FT *>(y_dev), ccnt, cand_dev, k, ids_dev, reinterpret_cast<FT *>(dists_dev),
                       (hipStream_t)hip_stream);
}

// The built rows, then the tail (id n + j, hashed or not): always the NATIVE rows, fixed mode on or off.
extern "C" int annhip_index_rerank(annhip_index *ix, void *hip_stream, size_t ycnt, const ftype *y_dev, size_t ccnt,
                                   const size_t *cand_dev, size_t k, size_t *ids_dev, ftype *dists_dev) {
  if (ix->lo != 0 || ix->hi != ix->n)
    return rerank_refuse("annhip_index_rerank", "the index does not hold rows [0, n) on this device (resharded)");
  return launch_rerank("annhip_index_rerank", ix->n, ix->tail_m, ix->d, ix->d_points, ix->d_tail, ycnt,
                       reinterpret_cast<const FT *>(y_dev), ccnt, cand_dev, k, ids_dev, reinterpret_cast<FT *>(dists_dev),
                       (hipStream_t)hip_stream);
}

// ----------------------------------------------------------------------------- precomp
// rand_pr.c:8: uniform [0,1) from libc random()
static double unit_draw(void) { return (double)(unsigned long)random() / ((double)RAND_MAX + 1); }
// rand_perm, rand_pr.c:17-30 (partial Fisher-Yates; always d_pre draws)
static std::vector<u32> draw_perm(size_t d_pre, size_t d_post) {
  std::vector<u32> p(d_post);
  for (size_t i = 0; i < d_post; i++) p[i] = (u32)i;
  for (size_t i = 0; i < d_pre; i++) {
    size_t j = (unsigned long)random() % (d_post - i) + i;
    std::swap(p[i], p[j]);
  }
  return p;
}
struct HostGivens {
  std::vector<u32> ci, cj;
  std::vector<FT> c, s;
};
// rand_rot x rots (alg.c:37-56, rand_pr.c:10-16); cos/sin by double libm, rounded to ftype (ocl2c.h:10, Q11)
static HostGivens draw_givens(size_t rots, size_t len, size_t dim) {
  HostGivens g;
  for (size_t r = 0; r < rots; r++) {
    std::vector<u32> sel = draw_perm(2 * len, dim);
    for (size_t i = 0; i < len; i++) {
      g.ci.push_back(sel[2 * i]);
      g.cj.push_back(sel[2 * i + 1]);
      FT ang = (FT)(unit_draw() * M_PI);
      // The reference's CPU path computes `s = sincos(ang, &c)` = (c = cos(a), sin(a)) (ocl2c.h:10, compute.cl:63), which
      // gcc -O2 -- its build and the oracle's -- fuses into ONE glibc sincos() call; that call differs from cos()/sin()
      // in the last bit for ~0.1 % of the arguments.  Invisible after rounding to float, but in the double build it
      // showed as 1-ulp differences in `bases` for ~7 % of the seeds: call sincos() so that the index is the reference
      // binary's bit for bit.
      double sn, cs;
      sincos((double)ang, &sn, &cs);
      g.c.push_back((FT)cs);
      g.s.push_back((FT)sn);
    }
  }
  return g;
}
struct HostXform {
  HostGivens before, after;
  std::vector<u32> perm_b, perm_ai;
};

template <typename T>
static T *upload_vec(const std::vector<T> &v, std::vector<void *> &owned) {
  T *p = dev_alloc<T>(v.size());
  if (!v.empty()) HIPCHECK(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  owned.push_back(p);
  return p;
}

// precomp() in phases (alg.c:342-434).  A single device runs them back to back (annhip_precomp_index); a sharded host
// (one process per GPU, every rank holding ALL n rows during the build) puts three collectives between them:
//   begin                      draws (Q12), means, centring                                   -- every rank, identical
//   per try:  hash(rows)       run_initial on this rank's row slice           -> ALL-GATHER of the codes (4 B / point)
//             try              bucket table (all ranks), then second_half's distance pass for THIS RANK'S BUCKETS
//                              (bucket b belongs to rank b mod G) into its members' columns of merged_i / merged_d
//   after the tries                                                          -> MIN ALL-REDUCE of merged_i, merged_d
//                              (entries nobody computed hold INT32_MAX / +inf; every entry has one writer)
//   merge                      det_results' first network over the merged rows -- every rank, all rows (17 ms at cfg3)
//   graph(rows)                supercharge + distances + network for this rank's rows -> ALL-GATHER of the graph rows
//   finish                     the resident index
struct annhip_precomp {
  size_t n = 0, k = 0, d = 0, ds = 0, d_max = 0, nb = 0, W = 0, need_W = 0, Wn = 0;
  int T = 0, tries_scored = 0, rank = 0, world = 1;
  size_t rots_before = 0, rot_len_before = 0, rots_after = 0, rot_len_after = 0;
  std::vector<HostXform> hx;
  annhip_index *ix = NULL;
  FT *centred = NULL;
  u32 *cnt = NULL, *cursor = NULL, *d_max_cnt = NULL, *d_bad = NULL, *top_i = NULL;
  FT *top_d = NULL;
  TryInfo *solo = NULL;
  DevBuf cand_d, cand_i, nvt, nvo, flist, xids, xd;
  bool exact_all = false;
  hipStream_t s = 0;
};

// reuse != NULL: the transforms another handle of the same build has drawn (a host that drives several shards from one
// process draws once); otherwise they are drawn here from the caller's random() stream.
static annhip_precomp *precomp_begin_impl(size_t n, size_t k, size_t d, const ftype *points, int on_device, int tries,
                                          size_t rots_before, size_t rot_len_before, size_t rots_after,
                                          size_t rot_len_after, int rank, int world, const std::vector<HostXform> *reuse) {
  if (n <= k || k < 1) die("need n > k >= 1");
  if (world < 1 || rank < 0 || rank >= world) die("annhip_precomp_begin: bad rank/world");
  // alg.c:347-357 (Q13: evaluated in ftype)
  size_t ds = (size_t)ceil(log2((FT)n / k));
  size_t d_max = 1;
  while (d_max < d) d_max <<= 1;
  if (ds > d_max) ds = d_max;
  check_limits(n, k, d, ds, tries);
  if (world > 1 && n >= (1ull << 30)) die("sharded precomp exchanges ids as 32-bit signed values: n < 2^30");
  if ((rots_before && 2 * rot_len_before > d) || (rots_after && 2 * rot_len_after > ds))
    die("rotation length exceeds dimension (rand_rot needs 2*len <= dim; the reference divides by zero there)");
  annhip_precomp *h = new annhip_precomp();
  const int T = tries;
  h->n = n, h->k = k, h->d = d, h->ds = ds, h->d_max = d_max, h->T = T, h->rank = rank, h->world = world;
  h->rots_before = rots_before, h->rot_len_before = rot_len_before, h->rots_after = rots_after, h->rot_len_after = rot_len_after;
  // Every transform is drawn up front, in the reference's order (alg.c:387-392, Q12), and BEFORE any HIP call:
  // these draws are the only use this path makes of the caller's random() stream.
  if (reuse) {
    h->hx = *reuse;
  } else {
    h->hx.resize(T);
    for (int t = 0; t < T; t++) {
      h->hx[t].before = draw_givens(rots_before, rot_len_before, d);
      h->hx[t].after = draw_givens(rots_after, rot_len_after, ds);
      h->hx[t].perm_b = draw_perm(d, d_max);
      h->hx[t].perm_ai = draw_perm(ds, d_max);
    }
  }
  RandGuard keep_callers_stream;
  gpu_init();
  h->exact_all = env().exact;
  hipStream_t s = h->s;

  annhip_index *ix = h->ix = new annhip_index();
  ix->n = n, ix->k = k, ix->d = d, ix->ds = ds, ix->T = T, ix->lo = 0, ix->hi = n;
  if (on_device) {
    ix->d_points = const_cast<FT *>(reinterpret_cast<const FT *>(points));
  } else {
    ix->d_points = dev_alloc<FT>(n * d);
    ix->own_points = true;
    HIPCHECK(hipMemcpy(ix->d_points, points, sizeof(FT) * n * d, hipMemcpyHostToDevice));
  }
  const FT *pts = ix->d_points;

  // column means + centring (alg.c:360-369)
  ix->d_means = dev_alloc<FT>(d);
  h->centred = dev_alloc<FT>(n * d);
  {
    FT *acc = dev_alloc<FT>((n / 2) * d);
    rows_add0_kernel<<<grid_for((n / 2) * d, 256, 8192), 256, 0, s>>>(n, d, pts, acc);
    for (size_t m = n >> 1; m >> 1; m >>= 1)
      rows_addn_kernel<<<grid_for((m / 2) * d, 256, 8192), 256, 0, s>>>(m, d, acc);
    means_finish_kernel<<<grid_for(d, 256), 256, 0, s>>>(n, d, acc, ix->d_means);
    centre_kernel<<<grid_for(n * d, 256, 16384), 256, 0, s>>>(n, d, pts, ix->d_means, h->centred);
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipFree(acc));
  }
  ix->d_bases = dev_alloc<FT>((size_t)T * ds * d);

  // The merge over tries (det_results, alg.c:308-312) sorts a row of W = k*T entries, i.e. only its first
  // ann_need_len(W, k) columns are ever read: a try whose column block starts at or beyond that length
  // contributes its bucket table (query() probes every table) but its distance pass would be computed and never
  // looked at -- tries 7..9 of 10 at cfg3, 6..9 at cfg5.  Those tries skip the pass, and the merged rows are stored
  // with the shorter stride Wn (cfg5: 61 GB instead of 120 GB).  ANN_HIP_PRECOMP_ALL_TRIES=1 runs every pass (A/B).
  h->nb = (size_t)1 << ds, h->W = k * (size_t)T;
  h->need_W = ann_need_len(h->W, k);
  h->tries_scored = env().all_tries ? T : (int)std::min<size_t>((size_t)T, (h->need_W + k - 1) / k);
  h->Wn = (size_t)h->tries_scored * k;
  h->cnt = dev_alloc<u32>(h->nb), h->cursor = dev_alloc<u32>(h->nb), h->d_max_cnt = dev_alloc<u32>(1);
  ix->h_tries.resize(T);
  ix->d_tabs.resize(T);
  ix->d_segs.assign(T, NULL);
  ix->d_segx.assign(T, NULL);
  h->d_bad = dev_alloc<u32>(1);
  HIPCHECK(hipMemset(h->d_bad, 0, sizeof(u32)));
  ix->ws.d_fcount = dev_alloc<u32>(4);
  ix->d_rows = dev_alloc<unsigned long long>(ANN_NCOUNTERS);
  HIPCHECK(hipMemset(ix->d_rows, 0, ANN_NCOUNTERS * sizeof(unsigned long long)));
  h->solo = dev_alloc<TryInfo>(1);
  return h;
}

extern "C" annhip_precomp *annhip_precomp_begin(size_t n, size_t k, size_t d, const ftype *points, int on_device, int tries,
                                                size_t rots_before, size_t rot_len_before, size_t rots_after,
                                                size_t rot_len_after, int rank, int world) {
  return precomp_begin_impl(n, k, d, points, on_device, tries, rots_before, rot_len_before, rots_after, rot_len_after, rank,
                            world, NULL);
}

// out[0..5] = d_short, merged row stride Wn (entries), tries whose distance pass runs, tries, n, k
extern "C" void annhip_precomp_info(const annhip_precomp *h, size_t out[6]) {
  size_t v[6] = {h->ds, h->Wn, (size_t)h->tries_scored, (size_t)h->T, h->n, h->k};
  memcpy(out, v, sizeof v);
}

// merged_i (u32, as int32 INT32_MAX) / merged_d (+inf) = "nobody computed this entry": the neutral elements of the MIN
// all-reduce that follows the tries on a sharded host
extern "C" void annhip_precomp_init_merged(annhip_precomp *h, uint32_t *merged_i_dev, ftype *merged_d_dev) {
  RandGuard keep_callers_stream;
  const size_t cnt = h->n * h->Wn;
  fill_u32_kernel<<<grid_for(cnt, 256, 16384), 256, 0, h->s>>>(cnt, 0x7FFFFFFFu, merged_i_dev);
  fill_ft_kernel<<<grid_for(cnt, 256, 16384), 256, 0, h->s>>>(cnt, ft_inf_host(), reinterpret_cast<FT *>(merged_d_dev));
  HIPCHECK(hipGetLastError());
}

// run_initial of try t (alg.c:154-183) for rows [row_lo,row_hi): codes_dev[x - row_lo]; also save_vecs (alg.c:189-217)
extern "C" void annhip_precomp_hash(annhip_precomp *h, int t, size_t row_lo, size_t row_hi, uint32_t *codes_dev) {
  RandGuard keep_callers_stream;
  if (t < 0 || t >= h->T || row_lo > row_hi || row_hi > h->n) die("annhip_precomp_hash: bad arguments");
  const size_t d = h->d, ds = h->ds, d_max = h->d_max;
  hipStream_t s = h->s;
  std::vector<void *> owned;
  const HostXform &hx = h->hx[t];
  XformDev X;
  X.b_i = upload_vec(hx.before.ci, owned), X.b_j = upload_vec(hx.before.cj, owned);
  X.b_c = upload_vec(hx.before.c, owned), X.b_s = upload_vec(hx.before.s, owned);
  X.a_i = upload_vec(hx.after.ci, owned), X.a_j = upload_vec(hx.after.cj, owned);
  X.a_c = upload_vec(hx.after.c, owned), X.a_s = upload_vec(hx.after.s, owned);
  X.perm_b = upload_vec(hx.perm_b, owned), X.perm_ai = upload_vec(hx.perm_ai, owned);
  X.rots_b = (int)h->rots_before, X.rlb = (int)h->rot_len_before, X.rots_a = (int)h->rots_after, X.rla = (int)h->rot_len_after;
  X.d = (int)d, X.d_max = (int)d_max, X.ds = (int)ds, X.l = ann_lg(d_max);
  const int wpb = 4;
  const size_t rows = row_hi - row_lo;
  size_t smem = sizeof(FT) * wpb * ANN_HASH_ROWS * (d + d_max + ds);
  if (rows) {
    const size_t per_wg = (size_t)wpb * ANN_HASH_ROWS;
    allow_lds(hash_rows_kernel, smem);
    hipLaunchKernelGGL(hash_rows_kernel, dim3((unsigned)((rows + per_wg - 1) / per_wg)), dim3(64 * wpb), smem, s, X, rows,
                       h->centred + row_lo * d, codes_dev);
    HIPCHECK(hipGetLastError());
  }
  if (ds) {
    smem = sizeof(FT) * wpb * (d + d_max);
    allow_lds(bases_rows_kernel, smem);
    hipLaunchKernelGGL(bases_rows_kernel, dim3((unsigned)((ds + wpb - 1) / wpb)), dim3(64 * wpb), smem, s, X,
                       h->ix->d_bases + (size_t)t * ds * d);
    HIPCHECK(hipGetLastError());
  }
  HIPCHECK(hipStreamSynchronize(s));
  for (void *p : owned) HIPCHECK(hipFree(p));
}

// second_half of try t (alg.c:245-290) from the codes of ALL n points: bucket table, then -- for the tries whose merged
// columns are read at all -- each point's candidates -> its k best, into columns [t*k, (t+1)*k) of merged_i / merged_d
// (row stride Wn).  On a sharded host only the members of this rank's buckets are scored (bucket b: rank b mod world).
extern "C" void annhip_precomp_try(annhip_precomp *h, int t, const uint32_t *codes_dev, uint32_t *merged_i_dev,
                                   ftype *merged_d_dev) {
  RandGuard keep_callers_stream;
  annhip_index *ix = h->ix;
  const size_t n = h->n, k = h->k, d = h->d, ds = h->ds, nb = h->nb;
  hipStream_t s = h->s;
  const FT *pts = ix->d_points;
  FT *merged_d = reinterpret_cast<FT *>(merged_d_dev);
  HIPCHECK(hipMemsetAsync(h->cnt, 0, sizeof(u32) * nb, s));
  HIPCHECK(hipMemsetAsync(h->cursor, 0, sizeof(u32) * nb, s));
  HIPCHECK(hipMemsetAsync(h->d_max_cnt, 0, sizeof(u32), s));
  bucket_count_kernel<<<grid_for(n, 256, 4096), 256, 0, s>>>(n, codes_dev, h->cnt);
  max_u32_kernel<<<grid_for(nb, 256, 1024), 256, 0, s>>>(nb, h->cnt, h->d_max_cnt);
  u32 pm = 0;
  HIPCHECK(hipMemcpyAsync(&pm, h->d_max_cnt, sizeof(u32), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (pm == 0 || pm >= (1u << 20)) die("degenerate bucket table");
  u32 *tab = dev_alloc<u32>(nb * pm);
  fill_u32_kernel<<<grid_for(nb * pm, 256, 16384), 256, 0, s>>>(nb * pm, (u32)n, tab);
  bucket_place_kernel<<<grid_for(n, 256, 4096), 256, 0, s>>>(n, pm, codes_dev, h->cursor, tab);
  bucket_order_kernel<<<grid_for(nb, 256, 1u << 30), 256, 0, s>>>(nb, pm, h->cnt, tab);
  HIPCHECK(hipGetLastError());
  ix->d_tabs[t] = tab;
  ix->h_tries[t].tab = tab;
  ix->h_tries[t].pm = pm;
  if (pm > 0xFFFFu) die("bucket too large");
  ix->d_segs[t] = dev_alloc<uint2>(nb);
  build_seg_kernel<<<grid_for(nb, 256, 1u << 30), 256, 0, s>>>(nb, pm, tab, (u32)n, 0u, (u32)n, ix->d_segs[t], h->d_bad);
  ix->h_tries[t].seg = ix->d_segs[t];
  ix->h_tries[t].segx = NULL;
  if (t >= h->tries_scored) {  // table, pm and segments are kept; nothing reads this try's merged columns
    HIPCHECK(hipStreamSynchronize(s));
    return;
  }
  // a one-try view of the index: candidate row = [ds+1][pm], codes are the points' own (no scramble)
  TryInfo one;
  one.seg = ix->d_segs[t];
  one.segx = NULL;
  one.tab = tab, one.pm = pm, one.off = 0, one.end = (u32)((ds + 1) * pm), one.magic = magic_for(pm);
  if ((unsigned long long)one.end * pm >= (1ull << 32)) die("candidate row too long");
  HIPCHECK(hipMemcpyAsync(h->solo, &one, sizeof one, hipMemcpyHostToDevice, s));
  QParams P;
  P.points = pts, P.tries = h->solo, P.graph = NULL, P.means = NULL, P.bases = NULL;
  P.n = (u32)n, P.lo = 0, P.hi = (u32)n, P.d = (int)d, P.k = (int)k, P.T = 1, P.ds = (int)ds;
  P.L1 = one.end, P.P1 = 1u << ann_lg(P.L1), P.Lc1 = (u32)ann_need_len(P.L1, k);
  P.L2 = P.Lc2 = 0;
  int mode = (h->exact_all || (u32)k > P.P1) ? 1 : 0;
  FT *cd = NULL;
  u32 *ci = NULL, *nv = NULL;
  if (mode == 0) {
    cd = (FT *)h->cand_d.need(sizeof(FT) * n * (k + 1));
    ci = (u32 *)h->cand_i.need(sizeof(u32) * n * (k + 1));
    nv = (u32 *)h->nvt.need(sizeof(u32) * n);
    u32 *no = (u32 *)h->nvo.need(sizeof(u32) * n);
    // sharded: rows whose bucket belongs to another rank keep this marker and are skipped by finalize1
    if (h->world > 1) mark_rows_kernel<<<grid_for(n, 256, 16384), 256, 0, s>>>(n, (u32)(k + 1), ANN_ID_SKIP, ci);
    if (!launch_stage1_bucket(P, one, nb, cd, ci, nv, no, s, (u32)h->rank, (u32)h->world)) {
      // shapes the bucket kernel does not take: every rank scores every row (the exchange is then a no-op for this try)
      launch_stage1(NULL, P, n, pts, 1, codes_dev, cd, ci, nv, no, s, std::vector<TryInfo>(1, one), env().slot_scan ? 0 : 1);
    }
  }
  finalize_and_fallback(NULL, P, n, pts, 1, codes_dev, mode, cd, ci, nv, merged_i_dev, merged_d, (int)h->Wn, (int)(t * k),
                        h->flist, h->xids, h->xd, ix->ws.d_fcount, NULL, NULL, false, s);
  HIPCHECK(hipStreamSynchronize(s));
}

// det_results on the merged rows (alg.c:419-422), part 1: the network over each point's k*T' merged entries (distances
// are reused, not recomputed, alg.c:308-312) -- every rank, all rows.
extern "C" void annhip_precomp_merge(annhip_precomp *h, uint32_t *merged_i_dev, ftype *merged_d_dev) {
  RandGuard keep_callers_stream;
  annhip_index *ix = h->ix;
  const size_t n = h->n, k = h->k;
  hipStream_t s = h->s;
  u32 nbad = 0;
  HIPCHECK(hipMemcpy(&nbad, h->d_bad, sizeof(u32), hipMemcpyDeviceToHost));
  if (nbad) die("internal error: a bucket table built by precomp is not in sorted-prefix layout");
  ix->use_seg = env().slot_scan ? 0 : 1;
  h->cand_d.release(), h->cand_i.release(), h->nvt.release(), h->nvo.release(), h->flist.release(), h->xids.release(),
      h->xd.release();
  if (h->centred) HIPCHECK(hipFree(h->centred));
  h->centred = NULL;
  finish_geometry(ix);
  h->top_i = dev_alloc<u32>(n * k);
  h->top_d = dev_alloc<FT>(n * k);
  launch_exact_select((u32)h->W, (u32)std::min(h->need_W, h->Wn), (u32)h->Wn, (int)k, n, merged_i_dev,
                      reinterpret_cast<FT *>(merged_d_dev), NULL, 0, h->top_i, h->top_d, (int)k, 0, s);
  HIPCHECK(hipStreamSynchronize(s));
}

// part 2 for rows [row_lo,row_hi): neighbour rows = the first k entries of the OTHER points' merged, sorted rows (Q16),
// distances, network -> graph_dev u32[(row_hi-row_lo)][k] and graph_dists_dev (may be NULL)
extern "C" void annhip_precomp_graph(annhip_precomp *h, size_t row_lo, size_t row_hi, uint32_t *graph_dev,
                                     ftype *graph_dists_dev) {
  RandGuard keep_callers_stream;
  annhip_index *ix = h->ix;
  const size_t n = h->n, k = h->k;
  if (row_lo > row_hi || row_hi > n) die("annhip_precomp_graph: bad row range");
  hipStream_t s = h->s;
  QParams P = make_params(ix);
  P.graph = h->top_i;
  FT *gd_own = graph_dists_dev ? NULL : dev_alloc<FT>((row_hi - row_lo) * k + 1);
  FT *gd = graph_dists_dev ? reinterpret_cast<FT *>(graph_dists_dev) : gd_own;
  if (P.Lc2 <= 1024 && env().tail != 0) {  // the fused stage-2 kernel: the [rows][Lc2] rows never travel through HBM
    for (size_t q0 = row_lo; q0 < row_hi; q0 += (size_t)1 << 30) {
      const size_t nq = std::min((size_t)1 << 30, row_hi - q0);
      launch_stage2_fused<u32>(P, n, ix->d_points, 1, (u32)q0, nq, h->top_i, h->top_d, graph_dev - row_lo * k, gd - row_lo * k,
                               NULL, s);
    }
    HIPCHECK(hipStreamSynchronize(s));
    if (gd_own) HIPCHECK(hipFree(gd_own));
    return;
  }
  DevBuf r2i, r2d;
  if (env().tail != 0 && row_hi > row_lo) {  // long rows: selection + proof, the literal path for the flagged rows only
    DevBuf fl;
    u32 *fc = dev_alloc<u32>(4);
    bool done = true;
    // rows per call: what the fallback's bounded workspace walks in at most 64 passes (stage2_select_with_fallback)
    const size_t step = std::min<size_t>((size_t)1 << 22, 64 * std::max<size_t>(1, ((size_t)1 << 30) / ((size_t)P.Lc2 * (sizeof(FT) + sizeof(u32)))));
    for (size_t q0 = row_lo; q0 < row_hi && done; q0 += step)
      done = stage2_select_with_fallback(P, n, ix->d_points, 1, (u32)q0, std::min(step, row_hi - q0), h->top_i, h->top_d,
                                         graph_dev - row_lo * k, NULL, gd - row_lo * k, fl, fc, r2i, r2d, NULL, NULL, s);
    HIPCHECK(hipStreamSynchronize(s));
    fl.release();
    HIPCHECK(hipFree(fc));
    if (done) {
      r2i.release(), r2d.release();
      if (gd_own) HIPCHECK(hipFree(gd_own));
      return;
    }
  }
  const size_t row_bytes = (size_t)P.Lc2 * (sizeof(FT) + sizeof(u32));
  size_t chunk = ((size_t)2 << 30) / row_bytes;
  if (chunk < 1) chunk = 1;
  for (size_t q0 = row_lo; q0 < row_hi; q0 += chunk) {
    const size_t nq = std::min(chunk, row_hi - q0);
    u32 *ri = (u32 *)r2i.need(sizeof(u32) * nq * P.Lc2);
    FT *rd = (FT *)r2d.need(sizeof(FT) * nq * P.Lc2);
    launch_rows<MODE_GRAPH>(P, n, ix->d_points, 1, NULL, NULL, (u32)q0, nq, P.Lc2, h->top_i, h->top_d, ri, rd, NULL, s);
    // outputs are indexed by the global row x: offset the slices so that row x lands at (x - row_lo)
    launch_exact_select(P.L2, P.Lc2, P.Lc2, (int)k, nq, ri, rd, NULL, (u32)q0, graph_dev - row_lo * k, gd - row_lo * k,
                        (int)k, 0, s);
  }
  HIPCHECK(hipStreamSynchronize(s));
  r2i.release(), r2d.release();
  if (gd_own) HIPCHECK(hipFree(gd_own));
}

// the resident index; graph_dev u32[n][k] is copied in
extern "C" annhip_index *annhip_precomp_finish(annhip_precomp *h, const uint32_t *graph_dev) {
  RandGuard keep_callers_stream;
  annhip_index *ix = h->ix;
  ix->d_graph = dev_alloc<u32>(h->n * h->k);
  HIPCHECK(hipMemcpy(ix->d_graph, graph_dev, sizeof(u32) * h->n * h->k, hipMemcpyDeviceToDevice));
  if (h->top_i) HIPCHECK(hipFree(h->top_i));
  if (h->top_d) HIPCHECK(hipFree(h->top_d));
  if (h->centred) HIPCHECK(hipFree(h->centred));
  HIPCHECK(hipFree(h->cnt));
  HIPCHECK(hipFree(h->cursor));
  HIPCHECK(hipFree(h->d_max_cnt));
  HIPCHECK(hipFree(h->d_bad));
  HIPCHECK(hipFree(h->solo));
  delete h;
  (void)prune_setup(ix, env().prune, "ANN_HIP_PRUNE=1");
  return ix;
}

extern "C" annhip_index *annhip_precomp_index(size_t n, size_t k, size_t d, const ftype *points, int on_device,
                                              int tries, size_t rots_before, size_t rot_len_before,
                                              size_t rots_after, size_t rot_len_after, ftype *graph_dists_dev) {
  annhip_precomp *h = annhip_precomp_begin(n, k, d, points, on_device, tries, rots_before, rot_len_before, rots_after,
                                           rot_len_after, 0, 1);
  RandGuard keep_callers_stream;
  u32 *merged_i = dev_alloc<u32>(n * h->Wn);
  FT *merged_d = dev_alloc<FT>(n * h->Wn);
  u32 *codes = dev_alloc<u32>(n);
  for (int t = 0; t < tries; t++) {
    annhip_precomp_hash(h, t, 0, n, codes);
    annhip_precomp_try(h, t, codes, merged_i, reinterpret_cast<ftype *>(merged_d));
  }
  HIPCHECK(hipFree(codes));
  annhip_precomp_merge(h, merged_i, reinterpret_cast<ftype *>(merged_d));
  HIPCHECK(hipFree(merged_i));
  HIPCHECK(hipFree(merged_d));
  u32 *graph = dev_alloc<u32>(n * k);
  FT *gd = graph_dists_dev ? reinterpret_cast<FT *>(graph_dists_dev) : dev_alloc<FT>(n * k);
  annhip_precomp_graph(h, 0, n, graph, reinterpret_cast<ftype *>(gd));
  annhip_index *ix = annhip_precomp_finish(h, graph);
  HIPCHECK(hipFree(graph));
  if (!graph_dists_dev) ix->d_graph_dists = gd;
  return ix;
}

// ----------------------------------------------------------------------------- residency cache
// query() receives host pointers on every call (ann.h:61-62) and the reference re-wraps every buffer per call
// (alg.c:444-445,503-508).  Re-uploading a multi-GB point matrix per call would make the path PCIe-bound, so indexes
// stay resident, keyed by the host pointers plus a content fingerprint; gpu_cleanup(), annhip_cache_clear() or
// annhip_cache_drop(save) release them.
//
// Contract: the fingerprint covers par_maxes, row_means and bases IN FULL and strided
// samples (1 024 elements each) of points, graph and every which_par[t].  A caller that edits points / graph /
// which_par IN PLACE between two query() calls on the same addresses must either call annhip_cache_drop(save) /
// annhip_cache_clear(), or run with ANN_HIP_CACHE=strict (every call hashes the full content: exact, ~1 s per call
// at cfg3) or ANN_HIP_CACHE=off (every call uploads, the reference's behaviour).
static bool g_host_profile = false;
#include "ann_multi_host.h"

struct CacheEntry {
  const save_t *save;
  const ftype *points;
  const size_t *graph;
  size_t n, k, d;
  int T;
  u64 fp;
  annhip_index *ix;      // the whole index on one device, or
  annhip_multi *multi;   // ... its rows sharded over several (ANN_HIP_DEVICES / ANN_HIP_VIRTUAL_SHARDS)
};
static std::vector<CacheEntry> g_cache;
static void entry_destroy(CacheEntry &e) {
  if (e.multi) multi_destroy(e.multi);
  else annhip_index_destroy(e.ix);
}
#define ANN_CACHE_SLOTS 4
#define ANN_FP_SAMPLES 1024

struct FpHash {  // four independent multiply lanes over 64-bit words: a few GB/s per core, order-sensitive
  u64 h[4] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull};
  size_t cnt = 0;
  inline void word(u64 v) {
    u64 &x = h[cnt++ & 3];
    x = (x ^ v) * 0xFF51AFD7ED558CCDull;
    x ^= x >> 29;
  }
  void bytes(const void *p, size_t nbytes) {
    const unsigned char *b = (const unsigned char *)p;
    size_t i = 0;
    if (nbytes >= 4096) {
      // bulk: eight independent multiply-add lanes over 64-byte lines (x = x*K + word, K odd: any changed word changes
      // its lane), enough instruction-level parallelism to hash at memory speed; folded into the four lanes at the end
      u64 x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
      for (; i + 64 <= nbytes; i += 64) {
        u64 v[8];
        memcpy(v, b + i, 64);
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = x[j] * 0x9E3779B97F4A7C15ull + v[j];
      }
      for (int j = 0; j < 8; j++) word(x[j]);
    }
    for (; i + 8 <= nbytes; i += 8) {
      u64 v;
      memcpy(&v, b + i, 8);
      word(v);
    }
    if (i < nbytes) {
      u64 v = 0;
      memcpy(&v, b + i, nbytes - i);
      word(v);
    }
    word(nbytes);
  }
  template <typename T>
  void sampled(const T *p, size_t count) {  // ANN_FP_SAMPLES strided elements incl. first and last; everything if short
    if (count <= ANN_FP_SAMPLES) return bytes(p, count * sizeof(T));
    for (size_t i = 0; i < ANN_FP_SAMPLES; i++) {
      u64 v = 0;
      memcpy(&v, &p[(size_t)((unsigned __int128)(count - 1) * i / (ANN_FP_SAMPLES - 1))], sizeof(T));
      word(v);
    }
  }
  u64 done() const { return (h[0] * 3 + h[1] * 5 + h[2] * 7 + h[3] * 11) ^ (u64)cnt; }
};

// strict mode: the full content, hashed in 4 MB blocks by the host pool (block hashes combined in order).  One core
// hashes ~10 GB/s; the ~8 GB of a cfg3 index (points 5.1 GB, size_t tables 2.3 GB, graph 0.8 GB) take ~1 s on one
// thread and are memory-bound on the pool.
static u64 hash_region(const void *p, size_t nbytes) {
  const size_t BL = (size_t)4 << 20, nblocks = (nbytes + BL - 1) / BL;
  std::vector<u64> part(nblocks ? nblocks : 1, 0);
  HostPool::get().run(nblocks, [&](size_t b) {
    FpHash H;
    const size_t a = b * BL;
    H.bytes((const char *)p + a, std::min(BL, nbytes - a));
    part[b] = H.done();
  });
  FpHash H;
  H.bytes(part.data(), sizeof(u64) * nblocks);
  H.word(nbytes);
  return H.done();
}

static u64 fingerprint(const save_t *sv, const ftype *points) {
  const bool full = env().cache_mode == 1;
  const size_t nb = (size_t)1 << sv->d_short;
  FpHash H;
  H.bytes(sv->par_maxes, sizeof(size_t) * sv->tries);
  H.bytes(sv->row_means, sizeof(ftype) * sv->d_long);
  H.bytes(sv->bases, sizeof(ftype) * (size_t)sv->tries * sv->d_short * sv->d_long);
  if (full) {
    H.word(hash_region(points, sizeof(ftype) * sv->n * sv->d_long));
    H.word(hash_region(sv->graph, sizeof(size_t) * sv->n * sv->k));
    for (int t = 0; t < sv->tries; t++) H.word(hash_region(sv->which_par[t], sizeof(size_t) * nb * sv->par_maxes[t]));
  } else {
    H.sampled(points, sv->n * sv->d_long);
    H.sampled(sv->graph, sv->n * sv->k);
    for (int t = 0; t < sv->tries; t++) H.sampled(sv->which_par[t], nb * sv->par_maxes[t]);
  }
  return H.done();
}

// ANN_HIP_CACHE=strict costs this much per query() call: exported so that harnesses can print it (time_results -F)
extern "C" double annhip_fingerprint_ms(const save_t *save, const ftype *points, int strict) {
  const int keep = g_env.loaded ? g_env.cache_mode : 0;
  env();
  g_env.cache_mode = strict ? 1 : 0;
  struct timespec a, b;
  clock_gettime(CLOCK_MONOTONIC, &a);
  volatile u64 fp = fingerprint(save, points);
  (void)fp;
  clock_gettime(CLOCK_MONOTONIC, &b);
  g_env.cache_mode = keep;
  return (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6;
}

static void cache_clear() {
  for (auto &e : g_cache) entry_destroy(e);
  g_cache.clear();
}
extern "C" void annhip_cache_clear(void) { cache_clear(); }

// forget every resident index built for this save_t (free_save() of the bundled dispatcher calls it)
extern "C" void annhip_cache_drop(const save_t *save) {
  for (size_t i = 0; i < g_cache.size();) {
    if (g_cache[i].save == save) {
      entry_destroy(g_cache[i]);
      g_cache.erase(g_cache.begin() + i);
    } else {
      i++;
    }
  }
}
extern "C" size_t annhip_cache_size(void) { return g_cache.size(); }

// Measurement through the host-pointer ABI (tests/harness/time_results): the resident indexes behind
// query_gpu() record their stage-1 launches like annhip_profile() does; annhip_host_stats() = annhip_stats() of the
// index resident for `save` (0, or -1 if none), with out[6] = P1 and out[7] = L1 added.
extern "C" void annhip_host_profile(int on) {
  g_host_profile = on != 0;
  for (auto &e : g_cache) {
    if (e.ix) e.ix->profile = g_host_profile ? 1 : 0;
    if (e.multi)
      for (auto &S : e.multi->sh) S.ix->profile = g_host_profile ? 1 : 0;
  }
}
// shard < 0: the whole resident index (a sharded one: launches and milliseconds of the slowest shard, rows summed)
static int host_stats(const save_t *save, int shard, double out[8], int reset) {
  for (auto &e : g_cache)
    if (e.save == save) {
      if (e.ix) {
        if (shard > 0) return -1;
        annhip_stats(e.ix, out, reset);
        out[6] = (double)e.ix->P1, out[7] = (double)e.ix->L1;
        return 0;
      }
      annhip_multi *M = e.multi;
      if (shard >= M->G) return -1;
      double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int g = 0; g < M->G; g++) {
        if (shard >= 0 && g != shard) continue;
        DevScope ds(M->sh[g].dev);
        double v[8];
        annhip_stats(M->sh[g].ix, v, reset);
        acc[0] = std::max(acc[0], v[0]), acc[1] = std::max(acc[1], v[1]);
        acc[2] += v[2], acc[3] += v[3];
        acc[5] = std::max(acc[5], v[5]);
      }
      acc[4] = M->exact_queries;
      if (reset) M->exact_queries = 0;
      memcpy(out, acc, sizeof acc);
      out[6] = (double)M->sh[0].ix->P1, out[7] = (double)M->sh[0].ix->L1;
      return 0;
    }
  return -1;
}
extern "C" int annhip_host_stats(const save_t *save, double out[8], int reset) { return host_stats(save, -1, out, reset); }
extern "C" int annhip_host_stats_shard(const save_t *save, int shard, double out[8], int reset) {
  return shard < 0 ? -1 : host_stats(save, shard, out, reset);
}
// number of devices / virtual shards the index resident for `save` is spread over (1 = one device; 0 = none resident)
extern "C" int annhip_host_shards(const save_t *save) {
  for (auto &e : g_cache)
    if (e.save == save) return e.multi ? e.multi->G : 1;
  return 0;
}

static bool same_key(const CacheEntry &e, const save_t *sv, const ftype *points) {
  return e.save == sv && e.points == points;
}

// insert, replacing any entry with the same (save, points) key; oldest entry evicted when full
static void cache_put(const save_t *sv, const ftype *points, u64 fp, annhip_index *ix, annhip_multi *multi = NULL) {
  for (size_t i = 0; i < g_cache.size();) {
    if (same_key(g_cache[i], sv, points)) {
      entry_destroy(g_cache[i]);
      g_cache.erase(g_cache.begin() + i);
    } else {
      i++;
    }
  }
  if (g_cache.size() >= ANN_CACHE_SLOTS) {
    entry_destroy(g_cache.front());
    g_cache.erase(g_cache.begin());
  }
  if (ix) ix->profile = g_host_profile ? 1 : 0;
  g_cache.push_back(CacheEntry{sv, points, sv->graph, sv->n, sv->k, sv->d_long, sv->tries, fp, ix, multi});
}

static bool multi_matches(const CacheEntry &e, const MultiCfg &mc) {
  return mc.G > 0 ? (e.multi && e.multi->G == mc.G && e.multi->virt == mc.virt) : e.multi == NULL;
}

// the entry resident for these addresses whose geometry is the save_t's (no look at the content), or -1
static int cache_find(const save_t *sv, const ftype *points, const MultiCfg &mc) {
  for (size_t i = 0; i < g_cache.size(); i++) {
    const CacheEntry &e = g_cache[i];
    if (!same_key(e, sv, points) || e.graph != sv->graph || e.n != sv->n || e.k != sv->k || e.d != sv->d_long ||
        e.T != sv->tries || !multi_matches(e, mc))
      continue;
    const annhip_index *ix = e.ix ? e.ix : e.multi->sh[0].ix;
    bool same = ix->ds == sv->d_short;
    for (int t = 0; same && t < sv->tries; t++) same = ix->h_tries[t].pm == sv->par_maxes[t];
    if (same) return (int)i;
  }
  return -1;
}

static void annhip_cache_drop_key(const save_t *sv, const ftype *points) {
  for (size_t i = 0; i < g_cache.size();) {
    if (same_key(g_cache[i], sv, points)) {
      entry_destroy(g_cache[i]);
      g_cache.erase(g_cache.begin() + i);
    } else {
      i++;
    }
  }
}

static CacheEntry cache_get(const save_t *sv, const ftype *points) {
  const u64 fp = fingerprint(sv, points);
  const MultiCfg mc = multi_cfg();
  for (size_t i = 0; i < g_cache.size();) {
    CacheEntry &e = g_cache[i];
    if (!same_key(e, sv, points)) {
      i++;
      continue;
    }
    if (e.fp == fp && e.graph == sv->graph && e.n == sv->n && e.k == sv->k && e.d == sv->d_long && e.T == sv->tries &&
        multi_matches(e, mc))
      return e;
    entry_destroy(e);  // same addresses, different content (or another device set): stale
    g_cache.erase(g_cache.begin() + i);
  }
  if (mc.G > 0)
    cache_put(sv, points, fp, NULL, multi_create(mc, sv, points));
  else
    cache_put(sv, points, fp, annhip_index_create(sv, points, 0, 0, sv->n));
  return g_cache.back();
}

// ----------------------------------------------------------------------------- drop-in symbols
// query_gpu on one device, in two halves.  begin: the batch arrives in pageable host memory (ann.h:61-62); ONE job of the
// host pool copies it into a pinned bounce buffer in pieces of >= 256 KB, in order, and this thread sends each piece --
// and launches the hash of its queries (the codes are per query; only stage 1 needs all of them, Q2) -- as soon as the
// piece is there; then the rest of the step and the copies of the results into a pinned buffer, all asynchronous.
// end: wait, hand the results over in malloc'd memory.  Between the two the host is idle: query_gpu verifies the
// residency fingerprint there.
static double g_tmark[8];
static int g_tmark_on = -1;
static inline void tmark(int i) {
  if (g_tmark_on < 0) g_tmark_on = getenv("ANN_HIP_HOST_TIMING") != NULL;
  if (!g_tmark_on) return;
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  g_tmark[i] = t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
// 16 bytes per thread and step from pinned HOST memory (the GPU reads it across PCIe) to device memory: a kernel, not a
// DMA command -- each switch between the copy engine and the compute queue costs ~25 us of stream time (measured: the
// batch sent as 20 hipMemcpyAsync pieces with a hash launch after each took 0.65 ms longer than the kernels themselves)
typedef unsigned int copy_vec4 __attribute__((ext_vector_type(4)));
__global__ void copy_in_kernel(size_t n16, const copy_vec4 *__restrict__ src, copy_vec4 *__restrict__ dst, size_t tail, size_t nbytes) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = __builtin_nontemporal_load(src + i);
  if (blockIdx.x == 0 && threadIdx.x < tail)
    reinterpret_cast<unsigned char *>(dst)[nbytes - tail + threadIdx.x] = reinterpret_cast<const unsigned char *>(src)[nbytes - tail + threadIdx.x];
}

static void *pinned_dev_ptr(void *host) {
  void *dp = NULL;
  HIPCHECK(hipHostGetDevicePointer(&dp, host, 0));
  return dp;
}

static void query_single_begin(annhip_index *ix, size_t ycnt, const ftype *y, int alias, bool want_d) {
  tmark(0);
  const size_t k = ix->k, d = ix->d;
  FT *y_dev = (FT *)ix->io_y.need(sizeof(FT) * ycnt * d);
  char *y_pin = (char *)ix->io_y_pin.need(sizeof(FT) * ycnt * d);
  const char *y_pin_dev = (const char *)pinned_dev_ptr(y_pin);
  hipStream_t s = ix->stream;
  const QParams P = make_params(ix);
  const size_t row = sizeof(FT) * d, hashed = codes_needed(ix, ycnt);
  static const int io_pieces = env_int("ANN_HIP_IO_PIECES", 4);
  const size_t pieces = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, std::min(io_pieces, 16)), ycnt * row >> 20));
  const size_t per = (ycnt + pieces - 1) / pieces;
  u32 *codes = (u32 *)ix->ws.codes.need(sizeof(u32) * ycnt * P.T);
  if (!ix->ws.d_fcount) ix->ws.d_fcount = dev_alloc<u32>(4);
  // Everything of the call runs on ONE stream: the pieces' copy kernels back to back (PCIe stays busy while the host
  // threads copy the next piece into pinned memory), one hash launch, the step.  A copy stream of its own with the
  // hashes on the main stream an event away was built and measured: a cross-stream event wait takes ~40 us to take
  // effect -- longer than the 28 us of hashing it was meant to hide (stage 1 started 193-204 us into the call either
  // way) -- and a process has only four hardware queues: the extra stream serialised an annhip_stream pipeline of small
  // batches (51 -> 72 us per batch).
  hipStream_t cs = s;
  std::vector<std::atomic<int>> copied(pieces);
  for (auto &c : copied) c.store(0, std::memory_order_relaxed);
  // every piece is itself copied by several pool threads: items = pieces x lanes, taken in order
  const size_t lanes = std::max<size_t>(1, std::min<size_t>(HostPool::get().threads(), per * row >> 16));
  const std::function<void(size_t)> copy_part = [&](size_t it) {
    const size_t i = it / lanes, l = it % lanes;
    const size_t q0 = i * per, nq = q0 < ycnt ? std::min(per, ycnt - q0) : 0;
    const size_t bytes = nq * row, a = (bytes * l / lanes) & ~(size_t)63, b = l + 1 == lanes ? bytes : (bytes * (l + 1) / lanes) & ~(size_t)63;
    if (b > a) memcpy(y_pin + q0 * row + a, (const char *)y + q0 * row + a, b - a);
    copied[i].fetch_add(1, std::memory_order_release);
  };
  HostPool::get().begin(pieces * lanes, copy_part);
  // ONE hash launch behind the last piece (stage 1 reads the codes of the first `hashed` queries only, Q1/Q2)
  bool zeroed = false;
  for (size_t i = 0; i < pieces; i++) {
    const size_t q0 = i * per, nq = q0 < ycnt ? std::min(per, ycnt - q0) : 0;
    while ((size_t)copied[i].load(std::memory_order_acquire) < lanes) {
    }
    if (nq) {
      const size_t bytes = nq * row;  // rows are multiples of 4 bytes at least; the tail handles what is not 16
      copy_in_kernel<<<grid_for(bytes / 16 ? bytes / 16 : 1, 256, 512), 256, 0, cs>>>(
          bytes / 16, reinterpret_cast<const copy_vec4 *>(y_pin_dev + q0 * row), reinterpret_cast<copy_vec4 *>((char *)y_dev + q0 * row),
          bytes % 16, bytes);
    }
    if (i + 1 == pieces) {
      launch_codes(P, hashed, y_dev, codes, s, ix->ws.d_fcount);
      zeroed = hashed > 0;
    }
  }
  HIPCHECK(hipGetLastError());
  HostPool::get().end();
  tmark(1);
  // the final kernels write ids and distances straight into pinned host memory: no copy command at the end either
  const size_t ib = sizeof(size_t) * ycnt * k, db = sizeof(FT) * ycnt * k;
  char *out_pin = (char *)ix->io_out_pin.need(ib + db);
  char *out_dev = (char *)pinned_dev_ptr(out_pin);
  query_impl(ix, ix->ws, s, ycnt, reinterpret_cast<const ftype *>(y_dev), alias, 0, reinterpret_cast<size_t *>(out_dev),
             reinterpret_cast<ftype *>(out_dev + ib), zeroed ? 2 : 1);
  (void)want_d;
  tmark(2);
}

static void query_single_end(annhip_index *ix, size_t ycnt, size_t *result, ftype *dists) {
  const size_t ib = sizeof(size_t) * ycnt * ix->k, db = dists ? sizeof(FT) * ycnt * ix->k : 0;
  tmark(3);
  // the caller's result arrays are fresh mmap'd memory: their first touch (a page fault per 4 KB, ~50 us for a cfg3
  // batch) happens here, while the GPU works, instead of inside the copy below
  for (size_t o = 0; o < ib; o += 4096) reinterpret_cast<volatile char *>(result)[o] = 0;
  for (size_t o = 0; o < db; o += 4096) reinterpret_cast<volatile char *>(dists)[o] = 0;
  HIPCHECK(hipStreamSynchronize(ix->stream));
  tmark(4);
  const char *out_pin = (const char *)ix->io_out_pin.p;
  HostPool::get().copy(result, out_pin, ib);
  if (db) HostPool::get().copy(dists, out_pin + ib, db);
  tmark(5);
  if (g_tmark_on > 0)
    fprintf(stderr, "query_gpu host timeline (ms): batch in + hashes enqueued %.3f, step enqueued %.3f, fingerprint %.3f, "
            "wait %.3f, results out %.3f\n", g_tmark[1] - g_tmark[0], g_tmark[2] - g_tmark[1], g_tmark[3] - g_tmark[2],
            g_tmark[4] - g_tmark[3], g_tmark[5] - g_tmark[4]);
}

// ANN_HIP_ROWS before each query_gpu() step: the resident single-device index (ix; NULL = a sharded mode) is set to the
// switch's row storage -- idempotent, so annhip_reload_env() takes effect on the next call.  Where the narrow rows asked
// for do not exist (the other library's type, sharded modes) one warning per reading of the environment, and the rows
// stay native.
static void env_rows_apply(annhip_index *ix) {
  const int want = env().rows;
  if (want != ANNHIP_ROWS_NATIVE && (want != ANNHIP_ROWS_NARROW || !ix)) {
    if (!g_env.rows_warned)
      fprintf(stderr, "ANN_HIP_ROWS=%s: %s rows need the %s library and one device (not ANN_HIP_DEVICES / "
                      "ANN_HIP_VIRTUAL_SHARDS > 1); the rows stay native\n", want == ANNHIP_ROWS_F16 ? "f16" : "f32",
              want == ANNHIP_ROWS_F16 ? "binary16" : "binary32", want == ANNHIP_ROWS_F16 ? "f32" : "f64");
    g_env.rows_warned = true;
    if (ix) annhip_index_set_rows(ix, ANNHIP_ROWS_NATIVE);  // "stay native" also after a switch this library did serve
    return;
  }
  if (ix && annhip_index_set_rows(ix, want) != 0) die("ANN_HIP_ROWS: annhip_index_set_rows failed");
}

extern "C" size_t *query_gpu(const save_t *save, const ftype *points, size_t ycnt, const ftype *y,
                             ftype **dists_o) {
  RandGuard keep_callers_stream;
  gpu_init();
  const bool resident = env().cache_mode != 2;  // ANN_HIP_CACHE=off: upload per call, as the reference does
  const MultiCfg mc = multi_cfg();
  const size_t k = save->k;
  size_t *result = (size_t *)malloc(sizeof(size_t) * (ycnt * k ? ycnt * k : 1));
  if (dists_o) *dists_o = (ftype *)malloc(sizeof(ftype) * (ycnt * k ? ycnt * k : 1));
  ftype *dists = dists_o ? *dists_o : NULL;
  const int alias = y == points;
  // An index resident for these addresses with this geometry is used OPTIMISTICALLY: the step is enqueued first, the
  // content fingerprint (sampled by default, everything under ANN_HIP_CACHE=strict) is computed while the GPU works,
  // and only a mismatch -- the caller edited the index or the points in place -- costs anything: the results are
  // discarded, the index is uploaded again and the step repeated.  (Running a step on a stale resident index is
  // harmless: it is self-contained in device memory and its geometry equals the new one's.)
  for (int attempt = 0;; attempt++) {
    const int hit = resident && attempt == 0 ? cache_find(save, points, mc) : -1;
    CacheEntry e;
    if (hit >= 0) e = g_cache[hit];
    else if (resident) e = cache_get(save, points);  // uploads (and replaces a stale entry)
    else {
      e = CacheEntry{save, points, save->graph, save->n, save->k, save->d_long, save->tries, 0, NULL, NULL};
      if (mc.G > 0) e.multi = multi_create(mc, save, points);
      else e.ix = annhip_index_create(save, points, 0, 0, save->n);
    }
    bool stale = false;
    const std::function<void()> verify = [&] {
      if (hit >= 0) stale = fingerprint(save, points) != e.fp;
    };
    if (ycnt) {
      env_rows_apply(e.ix);
      if (e.multi) {  // rows sharded over several devices (or virtual shards): the owner protocol, ann_multi_host.h
        multi_query(e.multi, ycnt, y, alias, result, dists, &verify);
      } else {
        query_single_begin(e.ix, ycnt, y, alias, dists != NULL);
        verify();
        query_single_end(e.ix, ycnt, result, dists);
      }
    } else {
      verify();
    }
    if (!resident) entry_destroy(e);
    if (!stale) break;
    annhip_cache_drop_key(save, points);  // the next attempt uploads the current content
  }
  return result;
}

extern "C" size_t *precomp_gpu(size_t n, size_t k, size_t d, const ftype *points, int tries,
                               size_t rots_before, size_t rot_len_before, size_t rots_after,
                               size_t rot_len_after, save_t *save, ftype **dists_o) {
  if (multi_cfg().G > 0) {  // the build spread over the devices; each keeps its row slice resident afterwards
    size_t *graph = NULL;
    annhip_multi *M = multi_precomp(multi_cfg(), n, k, d, points, tries, rots_before, rot_len_before, rots_after,
                                    rot_len_after, &graph, dists_o);
    RandGuard keep_callers_stream;
    if (save) {
      {
        DevScope ds(M->sh[0].dev);
        annhip_index_export(M->sh[0].ix, save);
      }
      if (env().cache_mode != 2) cache_put(save, points, fingerprint(save, points), NULL, M);
      else multi_destroy(M);
    } else {
      multi_destroy(M);
    }
    return graph;
  }
  // (annhip_precomp_index draws from the caller's random() stream first, then parks it)
  annhip_index *ix = annhip_precomp_index(n, k, d, points, 0, tries, rots_before, rot_len_before, rots_after,
                                          rot_len_after, NULL);
  RandGuard keep_callers_stream;
  FT *gd = ix->d_graph_dists;
  size_t *result = (size_t *)malloc(sizeof(size_t) * n * k);
  size_t *wide = dev_alloc<size_t>(n * k);
  widen_ids_kernel<<<grid_for(n * k, 256, 1u << 30), 256>>>(n * k, ix->d_graph, wide);
  HIPCHECK(hipMemcpy(result, wide, sizeof(size_t) * n * k, hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(wide));
  if (dists_o) {
    *dists_o = (ftype *)malloc(sizeof(ftype) * n * k);
    HIPCHECK(hipMemcpy(*dists_o, gd, sizeof(FT) * n * k, hipMemcpyDeviceToHost));
  }
  HIPCHECK(hipFree(gd));
  ix->d_graph_dists = NULL;
  if (save) {
    annhip_index_export(ix, save);
    // keep the freshly built index resident for the queries that normally follow (time_results.c:95-105); an older
    // index built for the same save_t / points addresses (the reference's drivers reuse them in a loop) is replaced
    if (env().cache_mode != 2)
      cache_put(save, points, fingerprint(save, points), ix);
    else
      annhip_index_destroy(ix);
  } else {
    annhip_index_destroy(ix);
  }
  return result;
}
