/* ann_hip.h -- the resident / staged C-ABI of the HIP backend.
 *
 * query_gpu()/precomp_gpu() (algg.h) are the drop-in symbols; they are thin wrappers over the calls
 * below, which keep the index resident in HBM between calls and expose the stages of the query path
 * so that a multi-GPU host (one process per GPU, point rows sharded) can put its RCCL exchanges between
 * them.  Plain pointers and sizes only; "dev" pointers are HIP device pointers of the current device.
 *
 * The reference has no counterpart for residency: its GPU path re-wraps points, graph and every bucket
 * table as CL_MEM_USE_HOST_PTR buffers on every call (/root/reference/alg.c:444-445,503-508).
 */
#ifndef APPROXNN_HIP_ANN_HIP_H
#define APPROXNN_HIP_ANN_HIP_H
#include <stddef.h>
#include <stdint.h>
#include "ann.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct annhip_index annhip_index;

/* "f32" or "f64": the precision this library was built for (ftype.h). */
const char *annhip_precision(void);
/* The row-layout code the query kernels are dispatched with for rows of d elements, looked up through the library's
 * layout table (positive: power of two; negative: lanes-per-row / element-wise / folded forms; 0: any d), or INT_MIN
 * if the table has no entry for it.  Host only: needs no device. */
int annhip_layout_code(size_t d);

/* ---- index lifecycle ------------------------------------------------------------------------- */
/* Upload an index.  `points` holds rows [row_lo,row_hi) only (row-major, save->d_long each): the rows
 * this device owns.  points_on_device != 0: `points` is a device pointer that the index borrows (the
 * caller keeps it alive); otherwise it is host memory and is copied.  Single GPU: row_lo=0,row_hi=n. */
annhip_index *annhip_index_create(const save_t *save, const ftype *points, int points_on_device,
                                  size_t row_lo, size_t row_hi);
void annhip_index_destroy(annhip_index *ix);
/* out[0..11] = n, k, d, d_short, tries, L1, P1, Lc1, L2, P2, Lc2, sum(par_maxes)  (SURVEY 8 notation) */
void annhip_index_info(const annhip_index *ix, size_t out[12]);
/* All launches of this index go to `hip_stream` (a hipStream_t; NULL = the default stream). */
void annhip_index_set_stream(annhip_index *ix, void *hip_stream);
/* annhip_sh_stage1 launches its gather in `pieces` kernels over consecutive query ranges (default 1).  Same results;
 * the launch boundaries are where workgroups of other streams -- RCCL's in particular -- find free compute units. */
void annhip_index_set_gather_pieces(annhip_index *ix, int pieces);
/* annhip_sh_stage1 as a PERSISTENT grid: at most waves_per_simd of the gather's waves on every SIMD, the workgroups walk
 * the queries themselves (0 = one workgroup per query, the default).  The gather kernel fits 4 waves per SIMD; with 3
 * one slot per SIMD is always free, so workgroups of other streams (the other batches' small kernels, RCCL) start at
 * once instead of waiting for the gather to drain.  Same results. */
void annhip_index_set_gather_slots(annhip_index *ix, int waves_per_simd);
/* Opt-in "fixed" query mode (default 0 = the reference's results, bit for bit).  With 1, annhip_query / annhip_query_on
 * on this index (whole index on one device) undo two accidents of the reference that cost most of its recall: a query
 * looks up the buckets of ITS OWN hash codes (the reference reads code[i*Q+x] from an array written as [x*T+i],
 * alg.c:489-499 vs compute.cl:223-231) and every slot of the candidate row competes (the reference orders only the
 * first 2^floor(log2 L) slots, alg.c:137-144).  Results: the k smallest distinct (squared distance, id) pairs among the
 * candidates, stage 2 likewise; (n, +inf) where fewer than k exist.  Not comparable with the reference -- checked
 * against a brute force over the same candidate sets (tests/test_gpu_fixed_mode.py).  precomp is unaffected. */
void annhip_index_set_fixed(annhip_index *ix, int fixed);
/* Query-directed multi-probe: the recall knob of fixed mode (default 0 = fixed mode as described above, bit for bit).
 * For query x and try t let p[s], s = 0 .. d_short-1, be the projections the hash kernel computes (centred query .
 * bases[t][s] in the reference's tree order: the value whose sign bit is bit d_short-1-s of the code).  Order the s by
 * the key (|p[s]| as raw bits with the sign cleared, then s ascending): o[0], o[1], ...  With pair bits b
 * (0 <= b <= d_short) the buckets probed for (x, t) are code ^ m for m in
 *     {0}  u  {1 << z : 0 <= z < d_short}  u  {bit(o[u]) | bit(o[v]) : 0 <= u < v < b},   bit(s) = 1 << (d_short-1-s)
 * i.e. 1 + d_short + b(b-1)/2 buckets: the two-bit flips among the b LEAST CERTAIN hash bits; b <= 1 adds nothing.
 * Stage 1 returns the k smallest distinct (distance, id) keys among the valid ids of those buckets over all tries (self
 * excluded when aliased), exactly as fixed mode defines its result; stage 2 is fixed mode's, unchanged.  +-0 projections
 * have magnitude 0 and sort first; the order of NaN projections is unspecified.  The setting has an effect only while
 * fixed mode is on: parity-mode queries ignore it and stay bit-identical to the reference.  Composes with
 * annhip_index_set_rows, annhip_query_on (the ranked bits live in the batch's workspace) and annhip_stream_*.
 * annhip_index_set_probe: 0 on success; -1 with one line on stderr and the setting unchanged for pair_bits < -1 or
 * > d_short; ANNHIP_PROBE_ALL (-1) means d_short, the whole Hamming-2 ball.  annhip_index_probe: the current value (the
 * resolved one, never -1).
 * annhip_probe_bits runs the ranking hash kernel alone on hip_stream and returns what a query of this batch would use:
 * codes_dev u32[ycnt][tries] (code[q*T+t], the same bits as the plain hash kernels write) and pbits_dev
 * u8[ycnt][tries][b] = o[0..b); -1 (nothing launched) while the setting is 0. */
enum { ANNHIP_PROBE_ALL = -1 };
int annhip_index_set_probe(annhip_index *ix, int pair_bits);
int annhip_index_probe(const annhip_index *ix);
int annhip_probe_bits(annhip_index *ix, void *hip_stream, size_t ycnt, const ftype *y_dev, uint32_t *codes_dev,
                      uint8_t *pbits_dev);
/* Allow-list row filter of fixed mode (default: none).  Format: uint32_t bits[ceil(n/32)]; row i is allowed iff
 * bits[i >> 5] >> (i & 31) & 1; bits at or beyond n are ignored.  With a filter set, annhip_query / annhip_query_on /
 * annhip_stream_* return fixed mode's result with "valid id" read as "id < n, allowed, and not the query itself when
 * aliased": stage 1 = the k smallest distinct (distance, id) keys among the allowed valid ids of the probed buckets (with
 * pair bits b the same buckets as without a filter); stage 2 considers the stage-1 results and the ALLOWED graph
 * neighbours of those results (no traversal through disallowed rows); (n, +inf) where fewer than k candidates exist.  An
 * all-ones filter returns exactly the unfiltered result, bit for bit.  The bit test happens before a row is fetched: a
 * disallowed row costs 4 bytes of bitmap, not a row.  Composes with annhip_index_set_probe, annhip_index_set_rows, alias,
 * workspaces and the host stream; the annhip_sh_* staged calls, precomp, the recall scorer and query_gpu never see it.
 * annhip_index_set_filter: bits == NULL clears the filter (always accepted, returns 0).  Otherwise the index takes its OWN
 * copy of ceil(n/32) words (bits_on_device: device or host pointer; the caller's buffer is not borrowed), freed by
 * annhip_index_destroy.  Synchronous, on the null stream: device words written on another stream (annhip_filter_pack's
 * hip_stream) must be complete -- synchronise that stream -- before this call.  The caller must not change the filter while batches on this index are in flight.
 * Returns 0; -1 with one line on stderr and the setting unchanged while fixed mode is off (a parity-mode query that
 * silently returned filtered-out rows would be worse than a refusal) and for an index that does not hold rows [0, n) on
 * this device (resharded).  annhip_index_set_fixed(ix, 0) and annhip_index_reshard drop a filter that is set.
 * annhip_index_filter_count: the allowed rows among [0, n), counted when the filter was set; -1 when none is set.
 * annhip_filter_pack: one small kernel on hip_stream, u8 flags_dev[n] (non-zero = allowed: what a torch bool tensor holds)
 * -> bits_dev[ceil(n/32)], the tail bits of the last word zero; returns 0.
 * annhip_stats out[2] counts, with a filter, only the allowed ids handed to the gather: the sum over the probed buckets
 * of allowed valid ids, repeats across tries counted, the query itself counted when it is allowed. */
int annhip_index_set_filter(annhip_index *ix, const uint32_t *bits, int bits_on_device);
long long annhip_index_filter_count(const annhip_index *ix);
int annhip_filter_pack(size_t n, const uint8_t *flags_dev, uint32_t *bits_dev, void *hip_stream);
/* Per-query tag predicates of fixed mode (default: no tags).  The allow list above is one set for the whole index and
 * every query of a batch; tags let every query of a batch carry its own predicate.  Rows carry a 32-bit tag word
 * (uint32_t tags[n]), every query a (mask, value) pair (uint32_t qmask[ycnt], qvalue[ycnt]), and row i competes for query
 * q iff (tags[i] & qmask[q]) == qvalue[q].  Examples: tenant equality (mask 0xFFFFFFFF), equality on a packed field
 * (tenant in the low 24 bits, flags above), "this tenant and not deleted", everything (mask 0, value 0).  A query with
 * qvalue & ~qmask != 0 matches nothing.
 * annhip_index_set_tags: tags == NULL clears the tags (always accepted, returns 0).  Otherwise the index takes its OWN copy
 * of n words (tags_on_device: device or host pointer), freed by annhip_index_destroy.  Synchronous, on the null stream, as
 * annhip_index_set_filter is: device words written on another stream must be complete before the call, and the tags must
 * not change while batches on this index are in flight.  Returns 0; -1 with one line on stderr and the setting unchanged
 * for an index that does not hold rows [0, n) on this device (resharded).  annhip_index_reshard drops the tags.  Tags are
 * row attributes, not a filter: they may be set in parity mode, they survive annhip_index_set_fixed(ix, 0), and no
 * untagged call (annhip_query, annhip_query_on, annhip_stream_*, ...) ever reads them or returns anything else because
 * they are set.  annhip_index_has_tags: 0 or 1.
 * annhip_query_tagged: annhip_query_on (ws == NULL = the index's workspace; the stream handled the same way; mode 0) plus
 * the two device arrays u32[ycnt].  The result is fixed mode's with "valid id" read, for query q, as all of: id < n;
 * (tags[id] & qmask[q]) == qvalue[q]; allowed by the index's allow list when one is set (both tests apply, ANDed); not the
 * query itself when aliased.  Stage 1 = the k smallest distinct (distance, id) keys among those ids of the probed buckets
 * -- the same buckets as without tags, for every pair-bit setting; stage 2 considers the stage-1 results and those of
 * their graph neighbours that pass the same test; (n, +inf) pads, so a query that matches nothing returns k pads.  The
 * test happens before a row is fetched: a row that does not match costs its 4-byte id and its 4-byte tag.  Returns 0;
 * -2, with one line on stderr, nothing launched and the outputs untouched, while fixed mode is off, while the index has
 * no tags, and when either array is NULL (-1 stays annhip_query_on's "asynchronous" return).  Composes with
 * annhip_index_set_probe, annhip_index_set_rows, alias, and several workspaces on several streams.  NOT covered:
 * annhip_stream_*, annhip_sh_*, annhip_query_slice, query_gpu and parity mode take no predicate.
 * annhip_stats out[2] counts, for a tagged query, the ids handed to the gather: the matching (and allowed) valid ids over
 * the probed buckets, repeats across tries counted, the query itself counted when it matches.
 * (annhip_query_tagged is declared below, beside annhip_query_on, where the workspace type is known.)
 * Range predicates on the tag word (annhip_query_between, annhip_index_exact_query_between, annhip_exact_knn_between;
 * declared below, after the radius calls).  Every query carries a (mask, lo, hi) triple (uint32_t qmask[ycnt], qlo[ycnt],
 * qhi[ycnt]) and row i competes for query q iff qlo[q] <= (tags[i] & qmask[q]) <= qhi[q], both compares UNSIGNED 32-bit: a
 * tag word with bit 31 set is large, not negative.  With fields packed high to low one interval is equality on the upper
 * fields and a range on the lowest: tenant in bits 16-27, day in bits 0-15, mask 0x0FFFFFFF, lo = tenant << 16 | day_a,
 * hi = tenant << 16 | day_b is "this tenant, this window".  The identities, all bit for bit on ids and distances:
 *   qlo[q] == qhi[q]       the row of the pair-form call (annhip_query_tagged, annhip_query_k, annhip_query_radius,
 *                          annhip_exact_knn_tagged, ...) with qvalue = qlo;
 *   (qmask, qlo, qhi) = (0, 0, 0) and (m, 0, 0xFFFFFFFF)   the row of the untagged call, and the same number of rows
 *                          handed to the gather (annhip_stats out[2]);
 *   qlo[q] > qhi[q]        matches nothing (the interval never wraps); so does qlo[q] > qmask[q], which no masked word
 *                          can reach: all pads.
 * Everything else is the pair form's: the test happens before a row is fetched; the index's allow list is ANDed in; the
 * alias rule, annhip_index_set_probe, annhip_index_set_rows, workspaces and streams, a k of the call's own, a radius, the
 * scanned tail and the hashed tail compose; NOT covered are annhip_stream_*, annhip_sh_*, annhip_query_slice, query_gpu and
 * parity mode.  The pair-form calls and the range calls launch the same kernels: a pair is the interval [value, value]. */
int annhip_index_set_tags(annhip_index *ix, const uint32_t *tags, int tags_on_device);
int annhip_index_has_tags(const annhip_index *ix);
/* Appended rows of fixed mode: the tail (default: none).  A built index is frozen; annhip_index_append adds rows to it
 * without a rebuild.  Throughout, n = the rows the index was built from (what annhip_index_info keeps reporting), m = the
 * current tail length, n_total = n + m; tail row j has id n + j.  The rows go into a flat buffer the index owns, and every
 * fixed-mode query scans ALL of it exactly and merges the result into the index's answer (ann_tail_kernels.h): appended
 * rows have no bucket entries and no graph edges and need neither.  The cost of a step grows with ycnt * m; rebuild over
 * all n_total rows (Index.compact in the Python package) when the tail has grown.
 * annhip_index_append: the index copies `count` rows of d values (native ftype; rows_on_device: device or host pointer)
 * into its tail buffer, 16-byte aligned like the point rows; capacity doubles on growth; annhip_index_destroy frees it.
 * Synchronous, on the null stream, as annhip_index_set_filter is; the caller must not append while batches on this index are
 * in flight (growth moves the buffer).  Returns 0; count == 0 returns 0 and does nothing.  Refused -- -1, one line on stderr,
 * nothing changed -- while fixed mode is off; on a resharded index; while annhip_index_rows() != ANNHIP_ROWS_NATIVE; when
 * n_total + count >= 0xFFFFFFF0; when the index has tags and tags == NULL; when tags != NULL and the index has no tags.
 * With an allow list set the new rows are allowed: the index extends its bitmap with one-bits and adds count to
 * annhip_index_filter_count.  With tags set the index appends the `count` tag words (tags_on_device as above).
 * annhip_index_reserve_tail: capacity >= rows, so that later appends do not reallocate; 0, or -1 for the refusals above.
 * annhip_index_tail: m.
 * annhip_index_copy_rows: native rows [lo, hi) of the combined row set (built rows, then tail) -> dst_dev (device);
 * synchronous; -1 when the range is outside 0..n_total or the index is resharded.
 * annhip_index_drop_tail: m = 0, the bitmap and tag copies are read up to n again; the capacity is kept.  Always returns 0.
 * With m == 0 every entry point launches exactly what it launched before this feature and returns the same bits.
 * With m > 0:
 *   Fixed-mode queries -- annhip_query, annhip_query_on and annhip_stream_* while fixed mode is on, annhip_query_tagged and
 *   annhip_query_k: let R(q) be the result row as computed without the tail, its pads (entries with id >= n) dropped.  The
 *   call returns the k (or kq) smallest (distance, id) keys among R(q) and {(dist(q, n+j), n+j) : tail row j valid for
 *   q}, ascending, padded with (n_total, +inf).  dist is the query path's squared L2 bit for bit (the contract of
 *   annhip_exact_knn).  A tail row is valid under the rules of any row id: allowed by the allow list when one is set;
 *   passing the query's tag test in a tagged call; not row q when the call is aliased (query q leaves out row id q,
 *   wherever it lives).  The tail does not depend on the probe setting.  The merge runs on the call's stream.
 *   annhip_index_set_filter expects ceil(n_total/32) words and annhip_index_set_tags n_total words: one array serves both
 *   halves (the index's kernels only ever test ids < n).  annhip_index_filter_count counts rows among [0, n_total).
 *   annhip_index_exact_query, _tagged and _k return the exact neighbours over all n_total rows under the same validity
 *   rules; k > n_total - alias is refused where k > n - alias was.
 *   annhip_index_set_rows with a narrow type is refused (-1): narrow rows and a tail do not compose.
 *   annhip_index_reshard drops the tail.  annhip_index_set_fixed(ix, 0) keeps it stored.
 *   NOT covered -- these never see the tail: parity-mode queries, annhip_sh_*, annhip_query_slice, query_gpu,
 *   annhip_index_export, annhip_index_checksum and index files (annhip_save_write).
 * annhip_stats out[3] additionally counts, while profile = 1, the (query, valid tail row) pairs the tail's scan scored.
 *
 * Hashed tail rows (opt-in; default: none).  The exact scan costs ycnt * m row pairs per step.  annhip_index_hash_tail
 * files the current tail rows under their hash codes, so that a query fetches only the tail rows of the buckets it probes
 * anyway; those rows are then found approximately, like built rows, and no longer exactly.  mh = hashed tail rows, 0 <= mh
 * <= m.  The three tiers: built index | hashed tail [0, mh) | fresh tail [mh, m).
 * annhip_index_hash_tail: hashes ALL current tail rows and builds the bucket structure over rows [0, m); afterwards mh = m.
 * Synchronous, on the null stream, as annhip_index_append is.  Returns 0; -1, one line on stderr, nothing changed, wherever
 * annhip_index_append would refuse a call without rows: fixed mode off, a resharded index (and tries * m >= 0xFFFFFFF0).
 * m == 0: returns 0 and launches nothing.  Calling it again after more appends rebuilds over all m rows.
 * annhip_index_tail_hashed: mh.
 * Rows appended after the call land in [mh, m) and are scanned exactly as before; annhip_index_append does not change.
 * The code of tail row j in try t, c[j][t], is the hash code a non-aliased fixed-mode query equal to that row gets (the
 * query path's hash launch over the tail rows).  Hit test: for query q let cq[t] be its codes and, with pair bits b > 0,
 * o[q][t][0..b) its ranked bits (annhip_probe_bits); bit(s) = 1 << (ds-1-s); PM[q][t] = OR of bit(o[u]), u < b (0 when b = 0);
 * x = cq[t] ^ c[j][t].  Tail row j HITS in try t iff x == 0, or popcount(x) == 1, or popcount(x) == 2 and (x & ~PM[q][t]) ==
 * 0: exactly membership of x in the mask set of the probe setting (the last case is empty while b <= 1).  Row j < mh is a
 * tail candidate of q iff it hits in some try and is valid: allowed by the allow list, passing q's tag test in a tagged
 * call (the aliased test concerns ids < n only).
 * With mh > 0 a fixed-mode call (annhip_query, annhip_query_on, annhip_stream_*, annhip_query_tagged, annhip_query_k)
 * returns the k (or kq) smallest distinct (distance, id) keys among R(q) (pads dropped), the tail candidates among rows
 * [0, mh), and ALL valid rows of [mh, m); padded with (n_total, +inf); distances are the query path's bits.  With mh == 0
 * every entry point launches exactly what it launched before.
 * annhip_index_drop_tail and annhip_index_reshard set mh = 0.  annhip_index_reserve_tail and reallocating appends keep the
 * structure (it names rows by j).  annhip_index_set_fixed(ix, 0) keeps it.  A change of the probe setting needs no rebuild:
 * the masks are applied at query time.  Unchanged: annhip_index_exact_query* cover all n_total rows exactly;
 * annhip_index_copy_rows, export, checksum and index files.  Memory: 8 * tries * mh + 4 * tries * (2^ds + 1) bytes.
 * annhip_stats out[3] counts the (query, candidate) pairs the hashed lookup scored as well; annhip_stage_ms out[4] spans
 * both tail launches. */
int annhip_index_hash_tail(annhip_index *ix);
size_t annhip_index_tail_hashed(const annhip_index *ix);
int annhip_index_append(annhip_index *ix, const ftype *rows, int rows_on_device, size_t count, const uint32_t *tags,
                        int tags_on_device);
int annhip_index_reserve_tail(annhip_index *ix, size_t rows);
size_t annhip_index_tail(const annhip_index *ix);
int annhip_index_copy_rows(const annhip_index *ix, size_t lo, size_t hi, ftype *dst_dev);
int annhip_index_drop_tail(annhip_index *ix);
/* What Index.compact carries over to the rebuilt index.  annhip_index_fixed: 0 or 1 (annhip_index_set_fixed).
 * annhip_index_copy_words: the index's own copy of the allow list (what = 0: ceil(n_total/32) words) or of the tags (what =
 * 1: n_total words) -> dst_dev (device), synchronous; -1 where the index has none, or for another `what`. */
int annhip_index_fixed(const annhip_index *ix);
int annhip_index_copy_words(const annhip_index *ix, int what, uint32_t *dst_dev);
/* Opt-in binary16 point rows (default ANNHIP_ROWS_NATIVE = the reference's results, bit for bit).  With ANNHIP_ROWS_F16,
 * annhip_query / annhip_query_on / annhip_query_slice / annhip_stream_* on this index return exactly what the reference
 * returns for query(save, h(P), y), where h(P) is the point matrix rounded to IEEE binary16 (round to nearest even;
 * overflow -> +-inf, subnormals kept, NaN stays NaN) and widened back to float -- numpy's
 * P.astype(np.float16).astype(np.float32).  Everything else is unchanged: save (built from the float rows), the queries,
 * hashing, candidate slots, the reference's quirks, the network, rdups and the tie path; every distance is computed in
 * float, in the reference's tree order, without FMA, from the exactly widened halves.  alias = 1 still excludes point x
 * from query x.  A query moves half the row bytes (d = 128: 256 instead of 512 per candidate).
 * The first enable converts the rows on the device into a copy owned by the index (n*d*2 bytes; the native rows stay
 * where they are, so switching back is free and returns the old results bit for bit); annhip_index_destroy frees it.
 * precomp is unaffected (it builds from the float rows), and so are fixed mode's inputs: set_fixed + ANNHIP_ROWS_F16 gives
 * the exact top-k of the candidate sets on h(P).  Scope: the f32 library and a whole index on one device.  Returns 0, or
 * -1 with one line on stderr for ANNHIP_ROWS_F16 in the f64 library, ANNHIP_ROWS_F16 on an index whose rows are not
 * [0, n) (resharded), or an unknown value; ANNHIP_ROWS_NATIVE is accepted everywhere.  annhip_index_reshard returns the
 * index to native rows and frees the copy; the annhip_sh_* staged calls always read the native rows.
 * annhip_index_rows() = the current setting.  Drop-in path: ANN_HIP_ROWS=f16.
 *
 * ANNHIP_ROWS_F32 is the same mode for the f64 library, whose narrow row type is IEEE binary32: the results are exactly
 * the reference's for query(save, f(P), y), f(P) = the double rows rounded to binary32 (round to nearest even; overflow
 * -> +-inf, binary32 subnormals kept, NaN stays NaN) and widened back -- numpy's P.astype(np.float32).astype(np.float64).
 * save is built from the double rows, the queries stay double, every distance is computed in double, in the reference's
 * tree order, without FMA, from the exactly widened floats.  The copy takes n*d*4 bytes and a query moves half the row
 * bytes (d = 256: 1024 instead of 2048 per candidate).  All the rules above hold alike: first enable converts, native
 * rows stay, destroy and reshard free the copy, rows [0, n) on this device, annhip_sh_* / precomp / the recall scorer
 * read native rows, fixed mode composes.  Each library serves its own narrow type only: -1 with one line on stderr for
 * ANNHIP_ROWS_F32 in the f32 library, as for ANNHIP_ROWS_F16 in the f64 library.  Drop-in path: ANN_HIP_ROWS=f32. */
#define ANNHIP_ROWS_NATIVE 0
#define ANNHIP_ROWS_F16 1
#define ANNHIP_ROWS_F32 2
int annhip_index_set_rows(annhip_index *ix, int rows);
int annhip_index_rows(const annhip_index *ix);
/* Pruned stage 1 of the parity path (f32 library; csrc/ann_prune_kernels.h): the SAME ids and distance bits for fewer
 * bytes.  Stage 1 preselects K' > k + 1 keys per query on the binary16 copy of the rows (the copy annhip_index_set_rows
 * makes), rescores those K' candidates on the native rows with the query path's distance tree, and tests per query
 * whether the k + 1 smallest exact keys are provably the ones native stage 1 selects among all candidates (the
 * preselection left nothing out, or every candidate it left out lies above the (k+1)-th exact distance by a bound built
 * from E = max over the rows of ||p - binary16(p)||_2).  A query that cannot be certified takes the exact path that
 * flagged queries take; stage 2 reads native rows.  K' = max(16, 3 (k + 1) / 2), at most 64.
 * mode: 0 off; 1 on where eligible; -1 auto (the default of a new index; ANN_HIP_PRUNE sets another one): on where
 * eligible AND the index is large enough to gain (P1 >= 8 K', native rows of 1 GiB or more, free device memory for the
 * copy).  Eligible: f32 library, rows [0, n) on this device, no appended rows, k + 1 <= 32, a row length with a register
 * layout, and E finite (no row overflows binary16).  The copy (n*d*2 bytes) and E are made by this call -- or when the
 * index is created / precomp finishes, under the auto rule -- never by a query; reshard, append and destroy drop them.
 * A query is pruned only in parity mode with native rows selected: fixed mode, annhip_index_set_rows(F16) (which keeps
 * meaning what it says), annhip_query_slice and mode = 1 queries take their usual path.  Returns 0, or -1 with one line
 * on stderr and nothing changed where mode 1 cannot be served (always in the f64 library) or mode is unknown.
 * annhip_index_prune() = 1 while annhip_query / annhip_query_on on this index are pruned, else 0.
 * Statistics: annhip_stats out[7] counts the uncertified queries; out[2] counts native-row equivalents of the bytes
 * requested (narrow rows / 2 + rescored rows); the stage-1 event pair brackets preselection and rescoring together.
 * annhip_index_prune_bound() reads what annhip_index_set_prune (or the auto rule) fixed for this index and changes
 * nothing: where the index holds a narrow copy and a bound it returns 1 and stores the E of the certificate in *E and
 * the K' of the preselection in *keys (either may be NULL); otherwise -- pruning off or refused, the copy dropped by
 * reshard or append -- it returns 0 and stores nothing.  It says what a pruned query WOULD use, whether or not queries
 * are pruned right now (annhip_index_prune).  K' is fixed by the call that made the bound (ANN_HIP_PRUNE_K is read then,
 * not by a query). */
int annhip_index_set_prune(annhip_index *ix, int mode);
int annhip_index_prune(const annhip_index *ix);
int annhip_index_prune_bound(const annhip_index *ix, double *E, int *keys);
/* Point-shard an index that was built from all n rows: from now on this device owns rows [row_lo,row_hi) only
 * and reads them from shard_points_dev (device pointer to those rows, borrowed).  Tables and graph stay. */
void annhip_index_reshard(annhip_index *ix, const ftype *shard_points_dev, size_t row_lo, size_t row_hi);
/* Download the index into a save_t whose fields are malloc'd (free_save() releases it). */
void annhip_index_export(const annhip_index *ix, save_t *save);

/* ---- index files (the reference's save_t is memory-only) ------------------------------------ */
/* Write / read a save_t (format: approximatenn_amd/csrc/ann_saveio.cpp; checksummed; ids stored as 32 bit when
 * they fit).  Host-only.  Return 0 on success; on failure print to stderr and return -1 (read leaves *save zeroed).
 * A file is tied to the precision of the library that wrote it.  Read fills malloc'd fields (free_save()).        */
int annhip_save_write(const save_t *save, const char *path);
int annhip_save_read(const char *path, save_t *save);

/* ---- residency cache behind query_gpu()/precomp_gpu() ------------------------------------------------------------ */
/* The reference re-wraps points, graph and every table per call (alg.c:444-445,503-508); query_gpu() instead keeps up
 * to four indexes resident, keyed by (save, points) addresses plus a content fingerprint: par_maxes, row_means and
 * bases in full, 1 024 strided samples each of points, graph and every which_par[t].  In-place edits that miss the
 * samples are NOT seen: call annhip_cache_drop(save) (the bundled free_save() does) or annhip_cache_clear() after
 * editing, or set ANN_HIP_CACHE=strict (full content hash per call) / ANN_HIP_CACHE=off (upload per call).
 * annhip_cache_size() = resident indexes.  annhip_reload_env() re-reads the ANN_HIP_* switches (they are read once). */
void annhip_cache_clear(void);
/* Milliseconds one fingerprint of (save, points) takes on this host: strict != 0 = the full content hash that
 * ANN_HIP_CACHE=strict pays on every query() call (spread over the host thread pool, ANN_HIP_HOST_THREADS, default
 * min(cores, 16)), 0 = the sampled default.  Measurement only. */
double annhip_fingerprint_ms(const save_t *save, const ftype *points, int strict);
void annhip_cache_drop(const save_t *save);
size_t annhip_cache_size(void);
void annhip_reload_env(void);

/* ---- point rows sharded over several devices behind query_gpu()/precomp_gpu() (the reference is
 * single-device, gpu_comp.c:60-75) -------------------------------------------------------------------------------- */
/* ndev > 1: from now on precomp_gpu() builds across devices 0..ndev-1 of this process and query_gpu() keeps one resident
 * index per device -- rows [g*n/ndev,(g+1)*n/ndev) on device g, tables and graph replicated -- and answers by the owner
 * protocol (the annhip_sh_* sequence below; exchanges over RCCL: ncclCommInitAll, one group per exchange; librccl.so is
 * loaded on first use).  virtual_shards > 0 instead: that many shards on the CURRENT device with loop-back exchanges
 * (same host code and kernels; for single-GPU boxes and tests).  (0, 0) = one device, the default.  Results are
 * bit-identical in every mode.  The environment does the same without a code change: ANN_HIP_DEVICES=G,
 * ANN_HIP_VIRTUAL_SHARDS=G; a call to this function overrides it. */
void annhip_set_devices(int ndev, int virtual_shards);

/* ---- precomp on the device (alg.c:342-434) ----------------------------------------------------- */
/* Builds the index from ALL n rows on this device and keeps it resident.  Consumes libc random() in the
 * reference's order.  graph_dists_dev (device, ftype[n*k]) may be NULL. */
annhip_index *annhip_precomp_index(size_t n, size_t k, size_t d, const ftype *points,
                                   int points_on_device, int tries, size_t rots_before,
                                   size_t rot_len_before, size_t rots_after, size_t rot_len_after,
                                   ftype *graph_dists_dev);

/* precomp() in phases, for point-sharded hosts (one process per GPU; EVERY rank holds all n rows during the build and
 * draws the same rotations from the same random() seed).  Between the phases the host runs three collectives:
 *     h = annhip_precomp_begin(..., rank, world);  annhip_precomp_info(h, info);  annhip_precomp_init_merged(h, mi, md);
 *     for t in tries:  annhip_precomp_hash(h, t, lo, hi, codes_slice)     -> ALL-GATHER codes_all u32[n]
 *                      annhip_precomp_try(h, t, codes_all, mi, md)        (this rank's buckets: b mod world == rank)
 *     MIN ALL-REDUCE of mi (as int32) and md                               (every entry has exactly one writer)
 *     annhip_precomp_merge(h, mi, md);  annhip_precomp_graph(h, lo, hi, graph_slice, dists_slice)
 *                                                                          -> ALL-GATHER graph u32[n][k] (+ distances)
 *     ix = annhip_precomp_finish(h, graph_all);
 * mi u32[n][Wn], md ftype[n][Wn] with Wn = info[1]; info = {d_short, Wn, tries scored, tries, n, k}.
 * annhip_precomp_index() is exactly this sequence with world = 1.  Results are identical for any world size. */
typedef struct annhip_precomp annhip_precomp;
annhip_precomp *annhip_precomp_begin(size_t n, size_t k, size_t d, const ftype *points, int points_on_device, int tries,
                                     size_t rots_before, size_t rot_len_before, size_t rots_after, size_t rot_len_after,
                                     int rank, int world);
void annhip_precomp_info(const annhip_precomp *h, size_t out[6]);
void annhip_precomp_init_merged(annhip_precomp *h, uint32_t *merged_i_dev, ftype *merged_d_dev);
void annhip_precomp_hash(annhip_precomp *h, int t, size_t row_lo, size_t row_hi, uint32_t *codes_dev);
void annhip_precomp_try(annhip_precomp *h, int t, const uint32_t *codes_dev, uint32_t *merged_i_dev, ftype *merged_d_dev);
void annhip_precomp_merge(annhip_precomp *h, uint32_t *merged_i_dev, ftype *merged_d_dev);
void annhip_precomp_graph(annhip_precomp *h, size_t row_lo, size_t row_hi, uint32_t *graph_dev, ftype *graph_dists_dev);
annhip_index *annhip_precomp_finish(annhip_precomp *h, const uint32_t *graph_dev);

/* ---- whole query on one device (alg.c:458-519) ------------------------------------------------- */
/* y_dev: ftype[ycnt][d]; alias != 0: query x excludes point x (the y == points case, compute.cl:144-146).
 * mode 0: selection path with exact fallback; mode 1: exact path for every query.
 * ids_dev: size_t[ycnt][k], dists_dev: ftype[ycnt][k] (may be NULL).  Fully asynchronous on the index's
 * stream (the exact fallback is driven by a device-side count, no host read-back); returns -1 in that case, or
 * the number of exact-path queries when it is known on the host (mode 1, very large batches).  The running
 * count is in annhip_stats(). */
long annhip_query(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, int mode,
                  size_t *ids_dev, ftype *dists_dev);

/* ---- overlapping independent batches ---------------------------------------------------------- */
/* annhip_query keeps its scratch in the index, so calls on one index are serial.  A caller that has several
 * independent batches gives each in-flight batch its own workspace and HIP stream: the small latency-bound stages of
 * batch i (hash, finalize, stage 2) then run underneath the HBM-bound stage-1 gather of batch i+1.
 * annhip_query_on = annhip_query with explicit workspace (NULL = the index's) and stream (a hipStream_t). */
typedef struct annhip_workspace annhip_workspace;
annhip_workspace *annhip_workspace_create(annhip_index *ix);
void annhip_workspace_destroy(annhip_workspace *ws);
long annhip_query_on(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev,
                     int alias, int mode, size_t *ids_dev, ftype *dists_dev);
/* annhip_query_on with a per-query tag predicate: the contract is with annhip_index_set_tags above. */
long annhip_query_tagged(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                         const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev, ftype *dists_dev);

/* A fixed-mode query whose k is chosen by the call.  Let kg be the index's k -- the width of its neighbour graph -- and kq
 * the k of this call.  annhip_query_k returns, for query q:
 *   stage 1: the kq smallest distinct (distance, id) keys among the valid ids of the probed buckets over all tries.  The
 *     buckets are the same as in annhip_query for every pair-bit setting (annhip_index_set_probe), and "valid" is read
 *     exactly as there: id < n; allowed by the allow list when one is set (annhip_index_set_filter); passing the query's
 *     tag test when the call is tagged; not the query itself when aliased.
 *   stage 2: the kq smallest distinct keys among the stage-1 results and the valid graph neighbours graph[p][z], z < kg,
 *     of the real (id < n) stage-1 results p.  A pad among the stage-1 results contributes nothing.
 *   output: ids_dev size_t[ycnt][kq], dists_dev ftype[ycnt][kq] (may be NULL), rows ascending by (distance, id), with
 *     (n, +inf) where fewer exist.
 * kq == kg returns the bits of today's call: annhip_query / annhip_query_on in fixed mode and, tagged, annhip_query_tagged.
 * ws and hip_stream behave as in annhip_query_tagged.  qmask_dev and qvalue_dev both NULL: an untagged call; both non-NULL
 * (u32[ycnt] each): a tagged call, the predicate as in annhip_query_tagged.  Asynchronous; returns 0.  Returns -2, with one
 * line on stderr, nothing launched and the outputs untouched: while fixed mode is off; for kq == 0 or
 * kq > annhip_index_max_query_k(ix); when exactly one of the two predicate arrays is given; for a tagged call on an index
 * without tags; for an index that does not hold rows [0, n) on this device (resharded) -- this entry validates before it
 * launches and never aborts on any of these.  ycnt == 0 returns 0.  Composes with annhip_index_set_probe,
 * annhip_index_set_filter, annhip_index_set_rows, alias, and several workspaces on several streams.  NOT covered: parity
 * mode, annhip_stream_*, annhip_sh_*, annhip_query_slice and query_gpu answer the index's k only; every existing entry
 * point launches exactly what it launched before.
 * annhip_index_max_query_k: the largest kq this index accepts -- at most 1024, lower where the LDS carve-up of stage 1
 * (the worst of its kernel families, at the most waves per query and pair bits they take) or of stage 2 would exceed what
 * one workgroup may have (160 KB).  It depends on d, tries, d_short and the precision, not on the probe, filter, tag or
 * row settings; at least 256 for the row lengths the library's register layouts serve.  Stage 2 runs fewer waves per
 * query for a large kq; results do not depend on the wave count. */
long annhip_query_k(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                    size_t kq, const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev, ftype *dists_dev);
size_t annhip_index_max_query_k(const annhip_index *ix);

/* Query-sharded ("replica") hosts: every device holds ALL rows and the whole index, and answers a contiguous slice of every
 * batch.  Results depend on the whole batch (query x reads hash codes of other queries), so the codes of all
 * ycnt queries must be known everywhere: each device hashes its slice (annhip_sh_codes), ONE all-gather makes
 * codes_all_dev u32[ycnt*tries] ([q*tries+t]) -- the only exchange of the step -- and annhip_query_slice answers queries
 * [q_lo, q_lo+nq): y_slice_dev = their rows, ids_dev size_t[nq][k], dists_dev ftype[nq][k].  Same results as annhip_query
 * on the whole batch.  alias only with q_lo == 0.  SURVEY 8(e) names this split as the alternative to row sharding. */
long annhip_query_slice(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, size_t q_lo, size_t nq,
                        const ftype *y_slice_dev, const uint32_t *codes_all_dev, int alias, size_t *ids_dev, ftype *dists_dev);

/* Host-resident batches, pipelined: `lanes` batches may be in flight, each with pinned staging buffers, a workspace
 * and a HIP stream, so uploads, kernels and downloads of consecutive batches overlap (query_gpu serialises them and
 * synchronises on every call).  submit copies y_host (ftype[ycnt][d], ycnt <= max_ycnt) and returns a ticket >= 0, or
 * -1 when every lane is in flight (collect the oldest ticket first).  collect waits for that batch and copies
 * size_t[ycnt][k] ids and ftype[ycnt][k] squared distances (may be NULL) out; returns 0, or -1 for an unknown ticket.
 * alias != 0 as in annhip_query.  One host thread drives a stream object. */
typedef struct annhip_stream annhip_stream;
annhip_stream *annhip_stream_open(annhip_index *ix, size_t max_ycnt, int lanes);
long annhip_stream_submit(annhip_stream *st, size_t ycnt, const ftype *y_host, int alias);
int annhip_stream_collect(annhip_stream *st, long ticket, size_t *ids_host, ftype *dists_host);
void annhip_stream_close(annhip_stream *st);

/* ---- staged query, for point-sharded multi-GPU hosts (approximatenn_amd/sharded.py) ---------- */
/* One process per GPU; device g owns point rows [row_lo,row_hi) (annhip_index_create / annhip_index_reshard), tables
 * and graph are replicated.  Queries are dealt to OWNER devices in contiguous slices of qs = ceil(ycnt/G); the owner
 * merges its queries' candidates and runs their networks.  The host puts one collective between consecutive calls
 * (all-gather, all-to-all, all-gather, all-to-all, all-gather).  Every annhip_sh_* call is asynchronous on `hip_stream`
 * (a hipStream_t) and uses caller-provided buffers only, so several batches can be in flight on several streams.
 * "keys" are packed (squared distance bits, id) pairs of annhip_key_bytes() bytes each (8 for float, 16 for double). */
size_t annhip_key_bytes(void);
/* A HIP stream (hipStream_t) that may use every compute unit but `reserve` of them -- for the stage-1 gathers, so that
 * the small kernels and the RCCL collectives of the other in-flight batch always find free wave slots.  NULL if the
 * runtime refuses; release with annhip_stream_destroy. */
void *annhip_stream_create_reserving(int reserve);
void annhip_stream_destroy(void *hip_stream);
/* 0. hash codes of queries [q_lo,q_hi) of the batch: codes_slice_dev u32[(q-q_lo)*tries+t] (alg.c:462-492).  The
 *    all-gather of the slices is the [q*tries+t] array of the whole batch that stage 1 reads as [t*ycnt+q] (Q2).
 *    Only the codes stage 1 can read are computed (Q1). */
void annhip_sh_codes(annhip_index *ix, void *hip_stream, size_t ycnt, const ftype *y_dev, size_t q_lo, size_t q_hi,
                     uint32_t *codes_slice_dev);
/* 1. stage 1 of ALL ycnt queries over the rows this device owns: keys_dev key[ycnt][k+1] = its k+1 smallest distinct
 *    candidates per query, ascending, padded with (+inf, 0xFFFFFFFF); nvalid_dev u32[ycnt] = valid slots in the sorted
 *    prefix on ANY device (identical everywhere); nown_dev u32[ycnt] = rows gathered here.  Needs k <= P1. */
void annhip_sh_stage1(annhip_index *ix, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                      const uint32_t *codes_dev, void *keys_dev, uint32_t *nvalid_dev, uint32_t *nown_dev);
/* 2. owner of queries [q_lo, q_lo+qs): keys_in_dev key[ndev][qs][k+1] (what the all-to-all of step 1 delivers) ->
 *    the k globally best, top_id_dev u32[qs][k] / top_dist_dev ftype[qs][k], if the selection proof holds; otherwise
 *    top_id[.][0] = 0xFFFFFFFE ("flagged": exact ties between different ids, < k candidates).
 *    Slots of queries >= ycnt (ragged last slice) are filled with padding.  ndev <= 16. */
void annhip_sh_merge_finalize(annhip_index *ix, void *hip_stream, int ndev, size_t ycnt, size_t q_lo, size_t qs,
                              const void *keys_in_dev, const uint32_t *nvalid_dev, uint32_t *top_id_dev,
                              ftype *top_dist_dev);
/* 2b. exact stage 1 of the flagged queries, device-driven, around ONE fixed-size MIN all-reduce of rows_dist_dev
 *    (ftype[fcap][Lc1]):  begin = ascending list of the flagged queries, flist_dev u32[2+fcap] = {listed, total, list},
 *    derived from top_id_all_dev (identical on every device), + ids / owned distances of their first Lc1 slots;
 *    end = the reference's network on the reduced rows -> top_id_all_dev[x] (the flag disappears), top_dist_all_dev
 *    ftype[>=ycnt][k], and the owner's slices.  Flagged queries beyond fcap stay flagged (step 3 lists them). */
void annhip_sh_exact1_begin(annhip_index *ix, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                            const uint32_t *codes_dev, const uint32_t *top_id_all_dev, size_t fcap,
                            uint32_t *flist_dev, uint32_t *rows_id_dev, ftype *rows_dist_dev);
void annhip_sh_exact1_end(annhip_index *ix, void *hip_stream, size_t ycnt, size_t q_lo, size_t qs, size_t fcap,
                          const uint32_t *flist_dev, uint32_t *rows_id_dev, ftype *rows_dist_dev,
                          uint32_t *top_id_all_dev, ftype *top_dist_all_dev, uint32_t *top_id_dev,
                          ftype *top_dist_dev);
/* 3. every device, all queries: top_id_all_dev u32[>=ycnt][k] (the all-gather of step 2) -> dist_out_dev
 *    ftype[ycnt][Lc2-k] = distances of the stage-2 slots k..Lc2-1 this device owns, +inf elsewhere (supercharge,
 *    compute.cl:252-263 + compdists, alg.c:314-326).  Flagged queries are skipped and listed:
 *    flagged_dev u32[1+ycnt] = {count, query indices in no particular order}. */
void annhip_sh_stage2(annhip_index *ix, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                      const uint32_t *top_id_all_dev, ftype *dist_out_dev, uint32_t *flagged_dev);
/* 4. owner: dist_in_dev ftype[ndev][qs][Lc2-k] (the all-to-all of step 3), its own top_id/top_dist slices ->
 *    min over devices, the reference's network + rdups + network on the stage-2 row (alg.c:224-230,327), first k
 *    entries to out_id_dev u32[qs][k] / out_dist_dev ftype[qs][k] (flagged queries: 0xFFFFFFFE / +inf). */
void annhip_sh_final(annhip_index *ix, void *hip_stream, int ndev, size_t ycnt, size_t q_lo, size_t qs,
                     const uint32_t *top_id_dev, const ftype *top_dist_dev, const ftype *dist_in_dev,
                     uint32_t *out_id_dev, ftype *out_dist_dev);
/* Exact path, used for the flagged queries (on the index's stream, annhip_index_set_stream):
 * ids u32[nq][Lc1] and distances ftype[nq][Lc1] of the first Lc1 stage-1 slots of the queries listed in qidx_dev
 * (NULL = queries 0..nq-1); slots not owned here get +inf (MIN-reduce the distance rows across devices). */
void annhip_stage1_rows(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias,
                        const uint32_t *codes_dev, const uint32_t *qidx_dev, size_t nq,
                        uint32_t *ids_dev, ftype *dist_dev);
/* stage-2 rows of the listed queries: ids u32[nq][Lc2], distances ftype[nq][Lc2] from top_id_dev u32[ycnt][k] /
 * top_dist_dev ftype[ycnt][k] (rows indexed by query). */
void annhip_stage2_rows_list(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, const uint32_t *qidx_dev,
                             size_t nq, const uint32_t *top_id_dev, const ftype *top_dist_dev, uint32_t *ids_dev,
                             ftype *dist_dev);
/* the reference's network+rdups+network on rows of reference length L (stage: 1 -> L1, 2 -> L2),
 * first k entries to out_id u32[.][k] / out_dist at row qidx_dev[i] (NULL = i). */
void annhip_exact_select(annhip_index *ix, int stage, size_t nq, uint32_t *ids_dev, ftype *dist_dev,
                         const uint32_t *qidx_dev, uint32_t *out_id_dev, ftype *out_dist_dev);

/* Test hook: sort_and_uniq (alg.c:224-230) on nq free-standing rows of reference length L (row stride
 * min(L, max(2^floor(log2 L), k) + 1)); with cand_d_dev / cand_i_dev [nq][k+1] (the k+1 smallest distinct keys of each
 * row's sorted prefix, ascending, padded with (+inf, 0xFFFFFFFF)) rows with a single run of tied distances are answered
 * by the tie path instead of the network; *resolved_dev (device counter, may be NULL) counts them.  derive != 0 with
 * cand_d_dev == NULL: the kernel derives those lists from the rows itself (what sharded hosts use).  Synchronous. */
void annhip_test_sort_rows(size_t L, size_t k, size_t nq, uint32_t *ids_dev, ftype *dist_dev, const ftype *cand_d_dev,
                           const uint32_t *cand_i_dev, uint32_t *out_id_dev, ftype *out_dist_dev,
                           unsigned long long *resolved_dev, int derive);

/* Test hook: stage 1's running selection of the K1 smallest distinct (distance, id) keys, run by the device functions the
 * stage-1 kernel itself calls, on ns free-standing key streams: stream b is dist_dev / id_dev [off_dev[b], off_dev[b+1])
 * (off_dev: ns + 1 ascending offsets), split over W waves (1..4) whose results wave 0 merges.  lds == 0: the register
 * list (K1 <= 128); lds != 0: the LDS candidate buffer (K1 <= 256).  out_*_dev [ns][K1]: the keys ascending, padded with
 * (+inf, 0xFFFFFFFF).  Synchronous.  Returns 0, or -1 for arguments outside those ranges. */
int annhip_test_select(size_t ns, const uint32_t *off_dev, const ftype *dist_dev, const uint32_t *id_dev, size_t K1, int W,
                       int lds, ftype *out_dist_dev, uint32_t *out_id_dev);

/* ---- content checksums (device memory in, 64-bit value out; synchronous) ------------------------------------------- */
/* annhip_checksum_dev: checksum of nbytes of device memory (4-byte aligned), independent of the launch geometry.
 * annhip_index_checksum: geometry, every bucket table, graph, means and projection rows of a resident index -- everything
 * a query reads except the point rows.  A multi-GPU host all-reduces both with MIN and MAX at start-up: ranks that do not
 * hold the same index and the same batch would return different answers (or hang in mismatched collectives). */
unsigned long long annhip_checksum_dev(const void *dev_ptr, size_t nbytes, void *hip_stream);
unsigned long long annhip_index_checksum(annhip_index *ix);

/* ---- recall scoring (counterpart of /root/reference/test_correctness.c:169-262) --------------- */
/* ranks_dev[q][j] (u64) = number of the n points strictly closer to query q than its j-th guessed neighbour, by one
 * tiled brute-force pass with the exact distance arithmetic of the query path.  points_dev holds ALL n rows;
 * guess_dev is size_t[ycnt][k] as query()/precomp() return it; self != 0 skips point q for query q (scoring the
 * graph precomp returns).  Synchronous. */
void annhip_recall_ranks(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                         const size_t *guess_dev, int self, unsigned long long *ranks_dev);
/* The same with HOST pointers in and out (uploads, scores, downloads): for plain-C drivers (tests/harness/test_correctness.c). */
void annhip_recall_ranks_host(size_t n, size_t d, size_t k, const ftype *points, size_t ycnt, const ftype *y,
                              const size_t *guess, int self, unsigned long long *ranks_host);

/* ---- exact k nearest neighbours (ground truth for recall@k) ------------------------------------------- */
/* For every query q of y[0..ycnt), over the n rows of points: dist(q, i) is the squared L2 distance exactly as the query
 * path computes it (df = y[q][z] - p[i][z], df * df, no contraction, summed by the reference's in-place halving tree with
 * the odd element folded into z == 0): bit-identical to what query() returns for the same pair, for every d >= 1.
 * ids[q][0..k) / dists[q][0..k) are the k smallest pairs under the total order (distance ascending, then id ascending),
 * written in that order.  This tie rule is this function's own: the reference orders equal distances by the comparator
 * sequence of its sort network over a candidate row, which has no meaning for a full scan.  +inf distances (overflow) are
 * ordinary values and sort last, by id.  Rows or queries holding NaN: unspecified.
 * self != 0: point q is left out for query q (the exact k-NN graph of the points themselves, as in annhip_recall_ranks).
 * Refused on the host with a message on stderr and a non-zero return code, nothing launched, outputs untouched:
 * k outside 1..1024, k > n - (self ? 1 : 0), n >= 0xFFFFFFF0.  ycnt == 0 returns 0 and does nothing.
 * Device pointers; synchronous; 0 = done. */
int annhip_exact_knn(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                     int self, size_t *ids_dev, ftype *dists_dev);
/* annhip_exact_knn over the ALLOWED rows only (bits_dev: device bitmap in annhip_index_set_filter's format): the same
 * arithmetic, the same (distance, id) order, the same refusals (k > n - self is refused as before, whatever the bitmap
 * holds).  A query with fewer than k allowed rows gets (n, +inf) in the tail.  bits_dev == NULL behaves as
 * annhip_exact_knn. */
int annhip_exact_knn_filtered(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                              int self, const uint32_t *bits_dev, size_t *ids_dev, ftype *dists_dev);
/* annhip_exact_knn_filtered with a per-query tag predicate (device arrays tags_dev[n], qmask_dev[ycnt], qvalue_dev[ycnt]):
 * row i competes for query q iff (tags_dev[i] & qmask_dev[q]) == qvalue_dev[q] and, where bits_dev != NULL, row i is
 * allowed by that bitmap.  The same arithmetic, (distance, id) order and refusals (k > n - self is refused as before,
 * whatever the tags hold; a NULL tags_dev, qmask_dev or qvalue_dev is refused too).  A query with fewer than k matching
 * rows gets (n, +inf) in the tail. */
int annhip_exact_knn_tagged(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                            int self, const uint32_t *tags_dev, const uint32_t *bits_dev /* may be NULL */,
                            const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev, ftype *dists_dev);
/* The same with HOST pointers in and out, for plain-C drivers. */
int annhip_exact_knn_host(size_t n, size_t d, size_t k, const ftype *points, size_t ycnt, const ftype *y,
                          int self, size_t *ids, ftype *dists);
/* The same over the rows an index already holds, with the index's own k; alias as in annhip_query (query q leaves out
 * point q).  Always reads the NATIVE rows, whatever annhip_index_set_rows says.  An index that does not hold rows [0, n)
 * (a resharded one) is refused with a non-zero return code.  Honours the index's allow list when one is set
 * (annhip_index_set_filter): ground truth and query share one allowed set. */
int annhip_index_exact_query(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias,
                             size_t *ids_dev, ftype *dists_dev);
/* annhip_exact_knn_tagged over the index's native rows and its tags (annhip_index_set_tags), honouring the index's allow
 * list when one is set: the ground truth of annhip_query_tagged.  Non-zero for an index without tags or a resharded one. */
int annhip_index_exact_query_tagged(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias,
                                    const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev,
                                    ftype *dists_dev);
/* annhip_index_exact_query / annhip_index_exact_query_tagged with a k of the call's own: the exact kq nearest of the
 * index's native rows, ids_dev size_t[ycnt][kq], dists_dev ftype[ycnt][kq].  Honours the allow list when one is set, and
 * the tag test when both predicate arrays are given (both NULL: untagged; exactly one: refused).  The refusals of
 * annhip_exact_knn*: kq outside 1..1024, kq > n - alias, a resharded index, a tagged call on an index without tags --
 * non-zero, outputs untouched.  The ground truth of annhip_query_k. */
int annhip_index_exact_query_k(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t kq,
                               const uint32_t *qmask_dev, const uint32_t *qvalue_dev, size_t *ids_dev, ftype *dists_dev);

/* ---- rerank: the exact top-k of caller-supplied candidates on native rows ------------------------------ */
/* The second step of "search cheap rows for a few more candidates than needed, re-score them on the full-precision rows",
 * and the scorer of any id list the caller brings (a keyword index's hits, ids saved from an earlier query).
 * `rows` below is n for annhip_rerank and n_total = n + m for annhip_index_rerank, which covers the built rows and then the
 * tail: tail row j has id n + j, whether or not it is hashed.
 * Candidates: cand_dev[q * ccnt + c] is a row id in the size_t / int64 layout the query calls return.  An entry >= rows
 * is skipped and never dereferenced -- pads and any other value, an int64 -1 included; the comparison is made on all 64
 * bits before anything is narrowed (2^32 + 5 is not row 5).  An id that occurs more than once in a query's list counts
 * once.
 * Output: per query the k smallest (distance, id) keys among its distinct in-range candidates, ascending, ties broken by
 * id, padded with (rows, +inf) where there are fewer than k.  k may exceed ccnt.
 * Distances come out of the same trees as annhip_exact_knn: bit for bit what the query calls and annhip_exact_knn return
 * for the same (query, row) pair on native rows.  +inf (overflow) is an ordinary value and ranks before the pads.  NaN:
 * unspecified, as in annhip_exact_knn.
 * annhip_index_rerank always reads the NATIVE rows, whatever annhip_index_set_rows says (as annhip_index_exact_query
 * does), with fixed mode on or off.  Neither call consults the allow list, the tags, the probe setting or any alias rule:
 * the caller chose the candidates.
 * Runs on hip_stream (NULL: the null stream), needs no workspace, synchronises nothing and may run beside query batches on
 * other streams.  ids_dev may be cand_dev itself where ccnt == k (query, then rerank in place).  Device pointers; 0 = the
 * launch is queued.
 * Returns -1, with one line on stderr, nothing launched and the outputs untouched: k outside 1..1024; ccnt outside
 * 1..1024; d == 0; rows >= 0xFFFFFFF0; a row too long for the LDS of one CU; annhip_index_rerank on a resharded index.
 * ycnt == 0 (with arguments that pass these tests) returns 0 and launches nothing. */
int annhip_rerank(size_t n, size_t d, const ftype *points_dev, size_t ycnt, const ftype *y_dev,
                  size_t ccnt, const size_t *cand_dev, size_t k, size_t *ids_dev, ftype *dists_dev, void *hip_stream);
int annhip_index_rerank(annhip_index *ix, void *hip_stream, size_t ycnt, const ftype *y_dev,
                        size_t ccnt, const size_t *cand_dev, size_t k, size_t *ids_dev, ftype *dists_dev);

/* ---- radius queries: every candidate within r, capped --------------------------------------------------------------- */
/* All distances and radii are squared L2 in ftype, like every distance the library returns.  Row i is IN RANGE for query q
 * iff dist(q, i) <= radius[q], compared as floating-point values: -0.0 counts as 0; a negative or NaN radius puts nothing
 * in range; +inf puts every row in range, including rows whose distance overflowed to +inf.  A row whose distance is NaN
 * (inf - inf on rows that overflowed) is in range for no radius, +inf included.
 * annhip_query_radius: a fixed-mode call with the shape of annhip_query_k.  "Valid" is read exactly as there (id < n, the
 * allow list, the tag test, not the query itself when aliased) and the probed buckets are the same, for every pair-bit
 * setting.  With "smallest" meaning smallest distinct (distance, id) keys:
 *   S1 = the kcap smallest among the valid in-range ids of the probed buckets;
 *   S2 = the kcap smallest among S1 and the valid in-range graph neighbours graph[p][z], z < kg, of the members p of S1;
 *   S3 = the kcap smallest among S2 and the in-range tail candidates (hashed tier: the rows that pass the hit test of
 *        "Hashed tail rows"; fresh tier: all valid rows);
 *   output: ids_dev size_t[ycnt][kcap], dists_dev ftype[ycnt][kcap] (may be NULL) = S3 ascending, padded with
 *        (n_total, +inf); counts_dev u32[ycnt] (may be NULL), counts[q] = |S3|.  counts[q] == kcap means "there may be
 *        more: ask again with a larger kcap".
 * Two equalities follow and are part of the contract: with radius[q] = +inf the row is, bit for bit, the row of
 * annhip_query_k(kq = kcap), and counts[q] is its number of non-pad entries; with kcap == kg as well, it is the row of the
 * plain fixed-mode call.  The one exception: a row whose distance is NaN, which annhip_query_k keeps behind every other key
 * and which no radius admits -- the equalities hold for every query without such a row among its candidates.
 * radius_dev ftype[ycnt]; qmask_dev / qvalue_dev both NULL (untagged) or both given (u32[ycnt] each).  ws and hip_stream
 * as in annhip_query_k.  Asynchronous; returns 0.  Returns -2, with one line on stderr, nothing launched and the outputs
 * untouched: while fixed mode is off; on a resharded index; for kcap == 0 or kcap > annhip_index_max_query_k(ix); for
 * radius_dev == NULL or ids_dev == NULL, whatever ycnt is; when exactly one predicate array is given; for a tagged call on
 * an index without tags.  ycnt == 0 (with arguments that pass these tests) returns 0.  Composes with annhip_index_set_probe, annhip_index_set_filter, tags, annhip_index_set_rows,
 * alias, and several workspaces on several streams.  NOT covered: parity mode, annhip_stream_*, annhip_sh_*,
 * annhip_query_slice, query_gpu.  Every existing entry point launches exactly what it launched before.
 * Only in-range keys ever enter a selection buffer of stage 1 (its admission threshold starts at the radius), and stage 2
 * loads graph rows for the in-range results only (a pad has no neighbours).  What a step costs beside annhip_query_k
 * followed by annhip_radius_trim is measured, not promised: DESIGN.md section 6, tools/radius_bench.py.
 * annhip_index_exact_query_radius: the ground truth -- the kcap smallest (distance, id) among ALL valid in-range rows of
 * the n_total rows, i.e. annhip_index_exact_query_k(kq = kcap) trimmed.  Non-zero with the outputs untouched: that call's
 * refusals (a resharded index and exactly one predicate array are tested first, then NULL arrays, then kcap and the tags),
 * and a NULL radius_dev, ids_dev or dists_dev, whatever ycnt is.  Pads and counts as above.  Synchronous.
 * annhip_radius_trim: the one small kernel both calls end with, exported so that any [ycnt][kcap] result in (distance, id)
 * order can be trimmed (annhip_exact_knn's included).  An entry stays iff id != pad_id and it is in range; everything
 * after the last kept entry becomes (pad_id, +inf); counts_dev[q] (may be NULL) = entries kept.  A pad is told by its id,
 * not by its distance.  In place, on hip_stream; returns 0.  ids_dev, dists_dev and radius_dev must be non-NULL, whatever
 * ycnt and kcap are: -1 otherwise, nothing launched.  ycnt == 0 or kcap == 0 launches nothing and returns 0. */
long annhip_query_radius(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                         size_t kcap, const ftype *radius_dev, const uint32_t *qmask_dev, const uint32_t *qvalue_dev,
                         size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev);
int annhip_index_exact_query_radius(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t kcap,
                                    const ftype *radius_dev, const uint32_t *qmask_dev, const uint32_t *qvalue_dev,
                                    size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev);
int annhip_radius_trim(size_t ycnt, size_t kcap, size_t pad_id, const ftype *radius_dev, size_t *ids_dev, ftype *dists_dev,
                       uint32_t *counts_dev, void *hip_stream);

/* ---- range predicates on the tag word: qlo[q] <= (tags[i] & qmask[q]) <= qhi[q] ---------------------------------------- */
/* The predicate and its identities: "Range predicates on the tag word" in the tag section above.
 * annhip_query_between: radius_dev == NULL is annhip_query_k(kq) under the range predicate (kq may be the index's own k:
 * the row is then annhip_query_tagged's where qlo == qhi); radius_dev != NULL is annhip_query_radius with kcap = kq, and
 * counts_dev is written iff radius_dev != NULL.  ws, hip_stream, outputs and pads as in those calls.  Asynchronous;
 * returns 0 -- except that with radius_dev == NULL and kq equal to the index's k the call IS annhip_query_tagged's path
 * and returns what that call returns (0 in fixed mode; kq is the index's own, so annhip_index_max_query_k is not asked).
 * Returns -2, with one line on stderr, nothing launched and the outputs untouched: while fixed mode is off; on
 * a resharded index; when any of qmask_dev, qlo_dev, qhi_dev is NULL; on an index without tags; for kq == 0 or
 * kq > annhip_index_max_query_k(ix); with a radius, for ids_dev == NULL.
 * annhip_index_exact_query_between: the ground truth, annhip_index_exact_query_k (radius_dev == NULL) or
 * annhip_index_exact_query_radius (kcap = kq) under the range predicate, over all n_total rows.  Synchronous.  Non-zero
 * with the outputs untouched: those calls' refusals, and a NULL predicate array.
 * annhip_exact_knn_between: annhip_exact_knn_tagged with the two bounds apart; its refusals, and a NULL qlo_dev or qhi_dev. */
long annhip_query_between(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                          size_t kq, const ftype *radius_dev /* NULL: the kq nearest; else annhip_query_radius' rule, kq = kcap */,
                          const uint32_t *qmask_dev, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                          size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev /* written iff radius_dev != NULL */);
int annhip_index_exact_query_between(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias, size_t kq,
                                     const ftype *radius_dev, const uint32_t *qmask_dev, const uint32_t *qlo_dev,
                                     const uint32_t *qhi_dev, size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev);
int annhip_exact_knn_between(size_t n, size_t d, size_t k, const ftype *points_dev, size_t ycnt, const ftype *y_dev, int self,
                             const uint32_t *tags_dev, const uint32_t *bits_dev /* may be NULL */,
                             const uint32_t *qmask_dev, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                             size_t *ids_dev, ftype *dists_dev);

/* ---- grouped queries: at most per_group results per tag group, by collapse ----------------------------- */
/* "The k nearest documents, not the k nearest chunks": rows that share a document, product or author carry the same value
 * in a bit field of their tag word, and a grouped call returns at most per_group rows of each value.
 * Group key: the key of row i for a call is tags[i] & gmask; gmask is one u32 per call, not per query.  tags is the index's
 * tag array (annhip_index_set_tags, annhip_index_append): one array over the built rows and then the tail rows, tail row j
 * has id n + j.
 * Collapse takes a list of L entries (id, dist) per query in the order given -- for the query calls ascending
 * (distance, id), pads last -- and works as follows with per_group = g:
 *   - an entry with id >= rows is a pad: it is skipped and never dereferenced.  The test is made on all 64 bits before
 *     anything is narrowed, as annhip_rerank does: an int64 -1 and 2^32 + 5 are pads;
 *   - a non-pad entry j is KEPT iff fewer than g earlier non-pad entries i < j have the same key;
 *   - the output row is the first k kept entries in list order, padded with (pad_id, +inf);
 *   - counts[q] = the number of kept entries written, at most k;
 *   - short[q] = 1 iff counts[q] < k and the input list was full, i.e. none of its L entries was a pad: a longer list might
 *     have found more groups, ask again with more candidates.  Otherwise 0;
 *   - distances are never compared or recomputed: they are copied bit for bit, NaN and +inf are ordinary values;
 *   - a repeated id is an ordinary second entry (query results have none).
 * Prefix stability: whether an entry is kept depends on the entries in front of it only.  Hence
 *   collapse(first L entries of an ordering)[:k] == collapse(the whole ordering)[:k]
 * whenever the left side has k entries or the prefix was not full -- with short[q] == 0 the row of a grouped query is
 * EXACTLY the collapse of the whole ordering its list is a prefix of, not a heuristic cut of it.
 * annhip_collapse: the stand-alone pass for any [ycnt][L] list: ids_in size_t[ycnt][L], dists_in ftype[ycnt][L] ->
 * ids_out size_t[ycnt][k], dists_out ftype[ycnt][k], counts_dev u32[ycnt] (may be NULL), short_dev u8[ycnt] (may be NULL).
 * Input stride L, output stride k; the outputs may be the inputs themselves only where k == L (a row is read whole before
 * any of it is written).  Runs on hip_stream (NULL: the null stream), needs no workspace and synchronises nothing; 0 = the
 * launch is queued.  Returns -1 with nothing launched and the outputs untouched: L outside 1..1024; k outside 1..L;
 * per_group == 0; gmask == 0; a NULL tags_dev, ids_in, dists_in, ids_out or dists_out; rows >= 0xFFFFFFF0.  ycnt == 0 (with
 * arguments that pass these tests) returns 0 and launches nothing.
 * annhip_query_grouped: a fixed-mode call.  Its row is, bit for bit, annhip_collapse applied to the row of
 * annhip_query_between(kq = list) -- with the three predicate arrays NULL, of annhip_query_k(kq = list) -- with the index's
 * tags and rows = pad_id = n_total.  The list of `list` entries stays in the workspace; ids_dev size_t[ycnt][k], dists_dev
 * ftype[ycnt][k] (may be NULL), counts_dev, short_dev (each may be NULL) are all the call writes.  Stage 2 is that of
 * annhip_query_k whatever list is, and the tail merges run before the collapse: appended rows are grouped too, hashed or
 * fresh.  ws and hip_stream as in annhip_query_k.  Asynchronous; returns 0.  Returns -2, with one line on stderr, nothing
 * launched and the outputs untouched: while fixed mode is off; on a resharded index; on an index without tags; for
 * gmask == 0; per_group == 0; k == 0 or k > list; list outside 1..annhip_index_max_query_k(ix); when some but not all of
 * qmask_dev, qlo_dev, qhi_dev are given; for ids_dev == NULL.  ycnt == 0 (with arguments that pass these tests) returns 0.
 * Composes with annhip_index_set_probe, annhip_index_set_filter, annhip_index_set_rows, alias, and several workspaces on
 * several streams.  NOT covered: a radius, parity mode, annhip_stream_*, annhip_sh_*, query_gpu, the sorted scans
 * (annhip_query_sorted / _sorted_set: collapse their result with annhip_collapse).  Every existing entry point launches
 * exactly what it launched before.
 * annhip_index_exact_query_grouped: the ground truth -- the same collapse over the row of
 * annhip_index_exact_query_between / _k with kq = list: native rows, the allow list honoured, all n_total rows.
 * Synchronous.  Non-zero with the outputs untouched: that call's refusals (a resharded index, list outside 1..1024 or
 * beyond the rows a query can be given, a row too long for the LDS of one CU) and the grouped ones above (no tags, gmask,
 * per_group, k, some but not all predicate arrays, a NULL ids_dev) and a NULL dists_dev.
 * What the collapse costs beside the step that feeds it is measured, not promised: DESIGN.md §6, tools/group_bench.py. */
int annhip_collapse(size_t ycnt, size_t L, size_t k, size_t per_group, uint32_t gmask,
                    const uint32_t *tags_dev, size_t rows, size_t pad_id,
                    const size_t *ids_in, const ftype *dists_in, size_t *ids_out, ftype *dists_out,
                    uint32_t *counts_dev /* may be NULL */, uint8_t *short_dev /* may be NULL */, void *hip_stream);
long annhip_query_grouped(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt,
                          const ftype *y_dev, int alias, size_t list /* K' */, size_t k, size_t per_group, uint32_t gmask,
                          const uint32_t *qmask_dev, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                          size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev, uint8_t *short_dev);
int annhip_index_exact_query_grouped(annhip_index *ix, size_t ycnt, const ftype *y_dev, int alias,
                                     size_t list, size_t k, size_t per_group, uint32_t gmask,
                                     const uint32_t *qmask_dev, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                                     size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev, uint8_t *short_dev);

/* ---- the tag order: exact answers for selective predicates by sorted scan ----------------------------- */
/* Where a predicate is selective, do not search the ANN structure: scan exactly the rows that match.  If the row ids are
 * sorted by tags & field_mask, every pair or range predicate on that mask matches a contiguous run of the sorted order.
 *
 * annhip_index_sort_tags: over the ms = n_total rows present at the call, perm[ms] = the row ids ordered by
 * (tags[id] & field_mask, id) and keys[ms] = the masked words in that order (8 * ms bytes of device memory).  The order is
 * deterministic: equal masked words are ordered by id.  Synchronous, on the null stream, as annhip_index_set_tags is.
 * Fixed mode need not be on: tags are row attributes.  field_mask == 0 drops the order.  Returns 0; -1, with one line on
 * stderr and nothing changed: the index has no tags; the index is resharded.
 * Drops the order: annhip_index_set_tags (with new tags or with NULL), annhip_index_drop_tail, annhip_index_reshard;
 * annhip_index_destroy frees the arrays.  Keeps the order: annhip_index_set_filter (the bit is tested at scan time),
 * annhip_index_append -- rows appended after the call are "fresh": ids in [ms, n_total), scanned by the tail's kernel --,
 * annhip_index_set_fixed, annhip_index_set_rows, annhip_index_set_probe and annhip_index_hash_tail.
 * annhip_index_tag_order: the rows the order covers (ms), 0 = none; *field_mask (may be NULL) = its mask, 0 without one.
 *
 * annhip_tag_runs: per query the run of the order that its interval selects: start = lower_bound(keys, qlo),
 * len = upper_bound(keys, qhi) - start; (0, 0) where qlo > qhi.  Asynchronous on hip_stream.  Returns 0; -1 without an
 * order (or for a NULL array), nothing launched.
 *
 * annhip_query_sorted returns what annhip_index_exact_query_between(ix, ycnt, y, alias, kq, radius, M, qlo, qhi, ...)
 * returns when M[q] = field_mask for every q, bit for bit: per query the kq smallest (distance, id) keys, ascending,
 * padded with (n_total, +inf), among the rows with qlo[q] <= (tags[i] & field_mask) <= qhi[q] -- built rows and tail rows
 * both compete, the allow list applies when one is set, row q is left out for query q when aliased.  Distances are the
 * query path's bits on the NATIVE rows, whatever annhip_index_set_rows says (as annhip_index_exact_query and
 * annhip_index_rerank).  With a radius, annhip_radius_trim's rule and counts apply; counts_dev is written iff
 * radius_dev != NULL.  Asynchronous on hip_stream / ws, as annhip_query_between is.  The cost is proportional to the
 * matching rows: queries whose runs coincide or overlap share the fetch of those rows.
 * Returns 0.  Returns -2, with one line on stderr, nothing launched and the outputs untouched: without an order; on a
 * resharded index; for a NULL array (y_dev, qlo_dev, qhi_dev, ids_dev, dists_dev); for kq outside 1..1024 or larger than
 * n_total - alias; for a row too long for the LDS of one CU.
 * With annhip_profile(ix, 1), annhip_stats' out[3] additionally counts the rows the scan fetched into tiles (one count
 * per row and tile fill).
 * Limits: one order and one mask per index; native rows only; the order is not saved in index files; parity mode,
 * sharded indexes and annhip_stream_* do not use it; long runs are not split -- one workgroup streams a whole span of
 * overlapping runs, so a single query whose run is millions of rows runs on one CU: keep such queries on the ANN path, or
 * give them to annhip_query_sorted_set with split_rows > 0, which splits. */
int annhip_index_sort_tags(annhip_index *ix, uint32_t field_mask /* 0: drop the order */);
size_t annhip_index_tag_order(const annhip_index *ix, uint32_t *field_mask /* may be NULL */);
int annhip_tag_runs(annhip_index *ix, void *hip_stream, size_t ycnt, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                    uint32_t *start_dev, uint32_t *len_dev);
long annhip_query_sorted(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                         size_t kq, const ftype *radius_dev /* may be NULL */, const uint32_t *qlo_dev, const uint32_t *qhi_dev,
                         size_t *ids_dev, ftype *dists_dev, uint32_t *counts_dev /* written iff radius_dev != NULL */);

/* ---- the tag order: sets of intervals per query, long runs split over workgroups --------------------- */
/* annhip_query_sorted_set is annhip_query_sorted for a query whose predicate is a UNION of intervals: query q owns the
 * intervals j in [off[q], off[q + 1]) of (lo[j], hi[j]), and row i competes for it iff
 * lo[j] <= (tags[i] & field_mask) <= hi[j] for some such j.  Every other rule is annhip_query_sorted's: the allow list,
 * alias, the NATIVE rows, the pads (n_total, +inf), the rows appended after the sort (they compete exactly once), the
 * radius trim and its counts, the workspace and the stream.  A query with no interval matches nothing and gets all pads.
 * off_host is a HOST array [ycnt + 1], off_host[0] = 0, non-decreasing; lo_dev / hi_dev are device arrays [off[ycnt]].
 *
 * Normalisation (on the device, one thread per query): the query's intervals are ordered by (lo, hi); empty ones
 * (lo > hi) are dropped; each later one is clipped to start above the largest hi before it, or dropped where nothing is
 * left (nothing follows hi = 0xFFFFFFFF).  The survivors are pairwise disjoint, so no row is offered twice to one query.
 * annhip_tag_runs_set writes the (start, len) of the normalised intervals, in that order, into the query's slice of
 * start_dev / len_dev [off[ycnt]] -- lower_bound and upper_bound as annhip_tag_runs finds them -- and (0, 0) for the slots
 * that the normalisation emptied.  Asynchronous on hip_stream; it stages its offsets in the index's own workspace, so
 * do not overlap it with a batch that uses that workspace.  Returns 0; -1, with one line on stderr and nothing
 * launched: without an order, for a NULL array, for offsets that decrease or do not start at 0, for a set of more than 256
 * intervals.
 *
 * Pieces: with split_rows = S > 0 every run is cut at the GLOBAL positions S, 2S, 3S, ... of the order (not at offsets
 * from its own start), so the queries of one tenant produce identical pieces and overlapping windows aligned ones, whose
 * fetch the scan shares as before; the pieces of a run go to different workgroups: the set call splits long runs over
 * the CUs.  Each piece, and with S = 0 each interval slot, is one entry of the scan's list; a per-query merge of the
 * entries' partial lists writes the output row.
 * Returns the entry count E >= 0.  With S > 0 E is the number of pieces, which depends on the data: the call
 * SYNCHRONISES hip_stream once to read it (after the runs are known, before the scan is launched).  With S = 0 the call
 * does not synchronise: everything goes to hip_stream and E = off[ycnt], one entry per interval slot -- a slot whose
 * interval is empty, was dropped or matches no row is an entry with an empty run, which fetches nothing.
 * Returns -2, with one line on stderr and the outputs untouched: in every case in which annhip_query_sorted refuses; for
 * a NULL off_host, lo_dev or hi_dev; for offsets that decrease or do not start at 0; for a set of more than 256 intervals;
 * for 0 < S < 64; for E * kq > 2^27 partial slots (with S > 0 this one is known only after the runs have been computed:
 * those small launches have happened, the scan has not).
 * With annhip_profile(ix, 1), annhip_stats' out[3] counts the rows fetched into tiles, as for annhip_query_sorted.
 * Limits: at most 256 intervals per query; one order and one mask per index; no router, no sharded form. */
int annhip_tag_runs_set(annhip_index *ix, void *hip_stream, size_t ycnt, const uint32_t *off_host /* [ycnt + 1] */,
                        const uint32_t *lo_dev, const uint32_t *hi_dev /* [off[ycnt]] */, uint32_t *start_dev,
                        uint32_t *len_dev /* [off[ycnt]] */);
long annhip_query_sorted_set(annhip_index *ix, annhip_workspace *ws, void *hip_stream, size_t ycnt, const ftype *y_dev, int alias,
                             size_t kq, const ftype *radius_dev /* may be NULL */, const uint32_t *off_host,
                             const uint32_t *lo_dev, const uint32_t *hi_dev, size_t split_rows, size_t *ids_dev,
                             ftype *dists_dev, uint32_t *counts_dev /* written iff radius_dev != NULL */);

/* ---- synthetic data of the reference's drivers------------------------------------------------------ */
/* out[0..count) = iid N(0,1) by Box-Muller on the CALLER's libc random() stream, value for value what genRand /
 * rand_norm produce (/root/reference/time_results.c:10-13, randNorm.c:9-21), incl. the pending second value of a pair
 * that the reference keeps between calls (annhip_synth_reset() forgets it, as a fresh process would).  Host memory;
 * the draws are sequential, the libm part runs on several host threads. */
void annhip_synth_randnorm(size_t count, ftype *out);
void annhip_synth_reset(void);

/* ---- measurement ---------------------------------------------------------------------------------- */
/* profile = 1: bracket every stage-1 launch with HIP events on its stream, drop events at annhip_query's stage
 * boundaries and count the gathered rows (one more small kernel per step).  profile = 2: the stage-1 event pair ONLY
 * (two events per step; every event record costs ~5 us of stream time -- what bench.py keeps inside its timed region).
 * 0: off. */
void annhip_profile(annhip_index *ix, int profile);
/* out[0]=stage-1 launches, out[1]=their total ms (events; only while profiling), out[2]=rows gathered in stage 1
 * (owned valid slots; only with profile = 1), out[3]=rows gathered in stage-2/exact rows kernels (only with profile =
 * 1), out[4]=queries flagged for the exact path, out[5]=queries seen, out[6]=of the flagged ones: answered by the tie
 * path (ann_tie.h) instead of the literal network, out[7]=queries a pruned stage 1 could not certify (they are among
 * out[4]); counters accumulate since the last reset (reset != 0 clears them
 * after reading). */
void annhip_stats(annhip_index *ix, double out[8], int reset);
/* While profiling, annhip_query also drops HIP events at its stage boundaries; out[0..5] = accumulated ms of
 * hash codes, stage-1 kernel, finalize + exact fallback, stage-2 rows, stage-2 network, id widening.  Fixed mode has no
 * stage-2 network: there out[4] is the scan of the appended rows (annhip_index_append), 0 while the tail is empty. */
void annhip_stage_ms(annhip_index *ix, double out[6]);
/* The same through the host-pointer ABI: annhip_host_profile(1) makes the indexes resident behind query_gpu() /
 * precomp_gpu() record their stage-1 launches; annhip_host_stats() = annhip_stats() of the index resident for `save`
 * plus out[6] = P1, out[7] = L1 (returns 0, or -1 when no index is resident for it). */
void annhip_host_profile(int on);
int annhip_host_stats(const save_t *save, double out[8], int reset);
/* A sharded resident index (annhip_set_devices): annhip_host_shards() = the devices / virtual shards the index resident
 * for `save` is spread over (1 = one device, 0 = none resident); annhip_host_stats_shard() = annhip_host_stats() of one
 * shard (annhip_host_stats() itself then reports the slowest shard's launches / milliseconds and the rows summed). */
int annhip_host_shards(const save_t *save);
int annhip_host_stats_shard(const save_t *save, int shard, double out[8], int reset);

#ifdef __cplusplus
}
#endif
#endif
