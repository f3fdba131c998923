/*
 * haconvdr.h — C ABI of the MI355X-native dense-retrieval hot path for HAConvDR.
 *
 * Drop-in boundary.  The reference has no FFI; its seams are two
 * duck-typed Python objects.  Each entry point below cites the reference call
 * site it replaces (paths are into the upstream repo fengranMark/HAConvDR):
 *
 *   Index   = the object returned by build_faiss_index()
 *             src/test_HAConvDR_topiocqa.py:39-71 (faiss.IndexFlatIP(768) :52,
 *             sharded over GPUs :55-66) and used by search_one_by_one_with_faiss()
 *             :74-162 through .add (:98) / .search (:102) / .reset (:122).
 *   Encoder = model(input_ids, attention_mask) -> float32 [B,768]
 *             src/models.py:39-64 (ANCE.forward/query_emb), called at
 *             src/test_HAConvDR_topiocqa.py:211 and gen_doc_embeddings.py:110.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function
 * returns 0 on success or a non-zero hac_status, never throws; the message of the
 * last failure on the calling thread is hac_last_error().  A handle is not
 * re-entrant; distinct handles may be used from distinct threads.  "_device"
 * variants take HIP device pointers and a hipStream_t (as void*), enqueue work on
 * that stream and return without synchronising; host variants are synchronous
 * like the faiss calls they replace.  There is NO CPU fallback: with no HIP
 * device every call fails with HAC_ERR_HIP.
 *
 * Canonical semantics (shared with oracle/flat_ip_oracle.c): score(q, x) is the
 * k-ordered fp32 fma chain acc = fmaf(x[k], q[k], acc), k = 0..d-1 (what the
 * gfx950 fp32 MFMA computes natively); results are ordered by (score descending,
 * row ascending); NaN scores are never returned; short result lists are padded
 * with D = -FLT_MAX, I = -1 (faiss's convention).
 */
#ifndef HACONVDR_H
#define HACONVDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    HAC_OK = 0,
    HAC_ERR_INVALID = 1,   /* bad argument (null handle, d not a multiple of 32, k out of range, ...) */
    HAC_ERR_HIP = 2,       /* a HIP runtime call failed / no device */
    HAC_ERR_OOM = 3,       /* device or pinned-host allocation failed */
    HAC_ERR_UNSUPPORTED = 4,
    HAC_ERR_INTERNAL = 5   /* the device detected a broken invariant of the library itself (a candidate loop ran past the pass
                              count no legal input reaches): the affected queries' lists are returned EMPTY (-FLT_MAX / -1), never
                              wrong, and the call (host entry points) or hac_index_last_status (after *_device calls) says so */
} hac_status;

#define HAC_MAX_K 2048      /* faiss-gpu 1.7.2 has the same top-k ceiling */
#define HAC_MAX_D 1024
#define HAC_MAX_AMONG 4096  /* candidates per query of hac_index_search_among*: one LDS sort block (range search's sort_lds) */

/* ------------------------------------------------------------------ errors */
/* Message of the last failing call on this thread ("" if none).  Never NULL. */
const char *hac_last_error(void);
/* Library version string, e.g. "haconvdr-amd 0.6.0 (gfx950)". */
const char *hac_version(void);


/* ------------------------------------------------------------------- index */
typedef struct hac_index hac_index;

/* faiss.IndexFlatIP(d) [+ index_cpu_to_gpu_multiple(shard=True)]:
 * src/test_HAConvDR_topiocqa.py:52,55-66.  d must be a multiple of 32, <= HAC_MAX_D
 * (the reference fixes d = 768).  A d with d % 64 == 32 (32, 96, ..., 992) always takes
 * scan16_kernel, at every query count, and never the half-precision prefilter (both the
 * many-query kernel and the prefilter stage the queries in whole 64-element slices); results
 * are the same bits, only slower for many queries.  device_ids[0..n_dev) are HIP ordinals; with
 * n_dev > 1 the rows of every add() are split contiguously across the devices and
 * search() merges the per-device top-k (faiss IndexShards semantics; the devices are
 * searched concurrently, one host thread per device, rows stay numbered by insertion
 * order over the whole index).  The scalable path is one process per GPU
 * (haconvdr_amd.sharded). */
int hac_index_create(int d, const int *device_ids, int n_dev, hac_index **out);
void hac_index_destroy(hac_index *idx);

/* index.add(passage_embedding) — src/test_HAConvDR_topiocqa.py:98.
 * x: host pointer, float32 row-major [n, d]; copied (and re-tiled for the MFMA
 * scan) before return — the caller may free it (the reference does, :123). */
int hac_index_add(hac_index *idx, const float *x, int64_t n);
/* Same, x already in device memory of the index's (single) device. */
int hac_index_add_device(hac_index *idx, const float *x_dev, int64_t n, void *hip_stream);

/* D, I = index.search(query_embeddings, topN) — src/test_HAConvDR_topiocqa.py:102.
 * q: host float32 [nq, d]; D: host float32 [nq, k]; I: host int64 [nq, k]
 * (rows numbered by insertion order since the last reset, whatever the number of devices).
 * Synchronous.
 *
 * Result contract of every search entry point: score = k-ordered fp32 fma chain, order =
 * (score desc, row asc), NaN scores never returned, short lists padded -FLT_MAX / -1.
 * A query is held to no more than a row is: one with a NaN component scores NaN against every row and returns a list of padding
 * only, one with +-Inf components returns its +Inf rows in row order, then its -Inf rows, never a row whose chain met Inf * 0 or
 * Inf - Inf, on every route, and neither costs the other queries of the call anything (tests/test_search_nonfinite_queries_gpu.py).
 * Where it is faster (k <= 192, d % 64 == 0, d >= 192; at once with >= 48 queries and >= 1e8 (query, row) pairs; for fewer --
 * down to ONE query on >= 750 k rows, >= 17 on >= 500 k, >= 2.5e7 pairs on >= 40 k -- when the fp16 image of the rows exists
 * already, or from the third such search after the last add / reset on, which builds it: +50 % of the corpus in HBM) the
 * rows are first screened on the fp16 matrix pipe under a proven error bound, the few
 * candidates are rescored exactly and each query's list is certified complete; queries
 * that cannot be certified are searched again by the exact fp32 kernels ("Prefilter with a certificate").
 * The results are the same bits either way.  hac_index_set_option(idx, "split", "0") disables
 * the screen, "1" applies it whenever the shape allows (tests), "auto" decides by size.
 * The host entry point reads the certificates back (and may retry many failures with three
 * fp16 products per score before the exact kernels); the *_device entry points leave the
 * decision on the device -- failed queries are compacted, searched again by the exact kernels
 * and scattered back by launches sized for every query and cut down by a device-side count --
 * and never synchronize or read back: they can be captured into a HIP graph once workspaces,
 * the segment table (re-uploaded by the first search after an add / reset, which does
 * synchronize once) and the fp16 image exist.  That image (+50 % of the corpus bytes in HBM)
 * is built by the first search that takes the screen and lives as long as the segment it belongs to (reset() keeps both;
 * destroying the handle frees them); an index that never takes it (small, searched once or twice per add, or split = "0")
 * never allocates it.  A search that is being captured never builds it (nor the rescoring's row-major copy): it runs what
 * the call before it ran.  With split = "auto", when the image does not fit beside the corpus the
 * exact fp32 kernels answer instead (same bits) and no search tries again until the next add / reset; split = "1"
 * reports HAC_ERR_OOM.
 * Before capturing a *_device search into a graph, run one search of the LARGEST shape (nq, k) you will capture: a call that
 * has to grow a workspace allocates, zero-fills it on the null stream and waits for that fill (once per growth).
 * Cost of the device-decided route: per chunk of 1024 queries a re-tiling of the failed queries, two memsets, a full-grid scan,
 * a select and a scatter are launched even when no query failed (their workgroups exit at once), and failed queries go
 * straight to the exact fp32 kernels, without the host route's three-product retry and threshold seeding: on tie-heavy or
 * degenerate corpora, where many certificates fail, hac_index_search (host route) is the faster entry point. */
int hac_index_search(hac_index *idx, const float *q, int64_t nq, int k, float *D, int64_t *I);
/* Device/stream variant (single-device index).  id_map_dev (optional, int64
 * [ntotal]) maps row -> external id, fusing `passage_embedding2id[I]` (:110). */
int hac_index_search_device(hac_index *idx, const float *q_dev, int64_t nq, int k, float *D_dev,
                            int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream);
/* Top-k as packed 64-bit keys, [nq, k] sorted descending, 0 = empty slot:
 *   key = (orderable(score) << 32) | (0xFFFFFFFF - (pos_base + row)).
 * This is the unit exchanged between corpus shards (one all-gather of keys). */
int hac_index_search_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k,
                                 uint64_t *keys_dev, uint32_t pos_base, void *hip_stream);

/* ---- search with per-query excluded rows --------------------------------------------------------------------------------
 * The search contract above over (rows minus the query's excluded rows): canonical fp32 fma-chain score, order (score desc,
 * row asc), NaN scores never returned, short lists padded -FLT_MAX / -1.  faiss users know it as
 * SearchParameters(sel=IDSelectorNot(IDSelectorBatch(ids))), here with one id list per query: a query's gold passages when
 * mining dense hard negatives, the passages a conversation has already shown.
 *
 * excl: int64 [nq, e] row ids of the index (its own numbering, as in "rows by id" below -- not id_map's external ids); -1 is
 * padding, duplicates are allowed.  With e == 0, or lists that name no row of the query's top-(k + e), the result equals
 * hac_index_search*'s bit for bit.
 *
 * How: for an exclusion set E, |E| <= e, the top-k of (rows minus E) is contained in the top-(k + e) of the rows, in the same
 * order.  The call therefore searches k' = k + e keys with the kernels of search and filters the sorted key lists on the
 * device (hac_filter_keys_device) before they become (D, I).  Consequences:
 *   - k >= 1, e >= 0 and k + e <= HAC_MAX_K, otherwise HAC_ERR_INVALID (the message names k, e and the ceiling);
 *   - every route decision of search is made for k', not k: the half-precision prefilter needs k + e <= 192, and a k' that
 *     does not fit the LDS candidate buffers fails as it does for search, naming k';
 *   - the cost is that of a search at k' plus one pass over nq * k' keys.
 *
 * Ids outside [0, ntotal), as for the rows-by-id calls: the *_device entry point ignores them (it cannot look); the host entry
 * point ignores -1 and returns HAC_ERR_INVALID for any other, naming the first offending id and its (query, column).
 *
 * Host variant: synchronous, works on a multi-device index (the shards search k' keys, which are remapped and merged at k'
 * exactly as in hac_index_search; the filter then runs once, on the first device); status words of the scans are reported as
 * hac_index_search reports them.  Device variant: single-device index (HAC_ERR_UNSUPPORTED otherwise); enqueues on hip_stream,
 * never reads back; the k' keys and the filtered keys live in workspaces of the index, which grow by the rule above: run one
 * call of the largest (nq, k + e) before capturing it into a HIP graph; id_map_dev fuses the remap of the RESULT as in
 * hac_index_search_device.  nq == 0 is HAC_OK and touches nothing. */
int hac_index_search_excluding(hac_index *idx, const float *q, int64_t nq, int k, const int64_t *excl, int e, float *D, int64_t *I);
int hac_index_search_excluding_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *excl_dev, int e,
                                      float *D_dev, int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream);

/* index.reset() — src/test_HAConvDR_topiocqa.py:122.  Keeps allocations for reuse. */
int hac_index_reset(hac_index *idx);
/* index.ntotal */
int64_t hac_index_ntotal(const hac_index *idx);
/* ---- rows by id: the faiss read-back calls, and exact scores of named rows --------------------------------------------
 * Row ids are the index's own numbering: insertion order since the last reset(), over the whole index whatever the number
 * of devices, int64.  After reset() and a smaller add() the old content is unreachable: ids >= the new ntotal are outside.
 *
 * Reconstruct returns the float32 row exactly as it was added, bit for bit (NaN payloads, +-Inf, -0.0 and denormals
 * included): add() only moves bits into the tiles and these calls only move them back.  The fp16 image is never a source;
 * a segment's row-major rescoring copy ("rescore_rows") is where it is current, the tiles otherwise -- same bits.
 *
 * Score by id: D[i][j] is the canonical score of (q[i], row ids[i][j]): the k-ordered fp32 chain acc = fmaf(x[k], q[k], acc),
 * k = 0..d-1 from acc = 0, followed by the "+ 0.0f" every search applies when it packs a key.  So score_ids(q, I) of any
 * search result reproduces that search's D bit for bit, on every route.  This is not a top-k: nothing is dropped, and a NaN
 * score is returned as NaN.
 *
 * Ids outside [0, ntotal):
 *   *_device entry points  any such id (-1 included): no error, nothing is read out of bounds; reconstruct writes a row of
 *                          all-ones words (0xFFFFFFFF per float, the NaN faiss's search_and_reconstruct writes for a -1
 *                          label), score writes -FLT_MAX (the padding score of search);
 *   host entry points      -1: the same outputs; any other id outside: HAC_ERR_INVALID, the message names the first
 *                          offending id and its position.
 * A range [i0, i0 + n) that is not inside [0, ntotal] is HAC_ERR_INVALID.  n == 0 / nq == 0 / m == 0 are HAC_OK and touch
 * nothing.
 *
 * Host variants are synchronous, run on the index's own stream and work on a multi-device index (ids are translated to
 * (shard, local row) on the host, every shard gathers its share on a host thread of its own); rows and scores are staged
 * through a bounded (~64 MiB) device workspace in chunks.  *_device variants take a single-device index
 * (HAC_ERR_UNSUPPORTED otherwise) and 16-byte aligned q_dev / out_dev (HAC_ERR_INVALID otherwise); they enqueue on the
 * caller's stream and return, never read back, take no slot of the status ring and need no workspace; they synchronize at
 * most once, for the segment-table upload that the first search after an add / reset also does, and can be captured into
 * a HIP graph once that table is up (run one call outside the capture first).
 *
 * Out of scope: reconstruct through haconvdr_amd.sharded.ShardedSearcher (one process per GPU: reading a row another rank
 * holds would need a collective; its rank() below needs only two all-reduces of [nq, m] words); and nothing here changes
 * how search routes or what it returns. */
/* index.reconstruct_n(i0, n): host float32 [n, d]. */
int hac_index_reconstruct(hac_index *idx, int64_t i0, int64_t n, float *out);
/* index.reconstruct(i) / index.reconstruct_batch(ids): ids host int64 [n]; out host float32 [n, d]. */
int hac_index_reconstruct_ids(hac_index *idx, const int64_t *ids, int64_t n, float *out);
/* Device form of both (and the second half of index.search_and_reconstruct: pass a search's I): ids_dev int64 [n], or
 * NULL for the range [i0, i0 + n) (i0 is not read when ids_dev is given); out_dev float32 [n, d]. */
int hac_index_reconstruct_device(hac_index *idx, const int64_t *ids_dev, int64_t i0, int64_t n, float *out_dev, void *hip_stream);
/* Exact scores of named rows -- what IndexFlatIP users compute as (q[i] * index.reconstruct_batch(ids[i])).sum(-1), in the
 * canonical order: q host float32 [nq, d]; ids host int64 [nq, m]; D host float32 [nq, m]. */
int hac_index_score_ids(hac_index *idx, const float *q, int64_t nq, const int64_t *ids, int64_t m, float *D);
int hac_index_score_ids_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ids_dev, int64_t m, float *D_dev,
                               void *hip_stream);

/* ---- rank of named rows: at what position does the WHOLE corpus put this row for this query? ---------------------------
 * Every other question the index answers is bounded by HAC_MAX_K; this one is not.  One definition, for a query q, a
 * reference score s_ref and a bound b (an int64 row number in the numbering of the rows being counted):
 *   count_ahead(q, s_ref, b) = #{ rows r in [0, ntotal) : s(q, r) is not NaN and (s(q, r) > s_ref or (s(q, r) == s_ref and r < b)) }
 * with s the canonical score above (the k-ordered fmaf chain and the "+ 0.0f" of a packed key) and float comparisons: -0.0
 * == +0.0, +-Inf are ordinary scores.  That is "key(s, r) > key(s_ref, b)" over the rows a search can return.  A NaN s_ref
 * gives -1, a b below 0 gives -1, a b above ntotal behaves like ntotal.
 *   rank_ids(q, ids)[i][j] = count_ahead(q[i], score_ids(q[i], ids[i][j]), ids[i][j])
 * is the 0-based position row ids[i][j] takes in an unbounded search of q[i]: for D, I = search(q, k) on any route,
 * rank_ids(q, I)[i][j] == j wherever I[i][j] >= 0.  It is -1 for the id -1 and for a row whose own score is NaN (no search
 * ever returns it).  Ids outside [0, ntotal) follow the rows-by-id rule: *_device entry points give -1 and no error, the
 * host entry point ignores -1 and returns HAC_ERR_INVALID for any other, naming the first offending id and its (query, column).
 *
 * How: score_ids gives the reference; count_ahead_kernel (csrc/rank.inc) then streams the rows once in the shape of
 * scan16_kernel -- same tiles, same bit-exact MFMA chain -- and counts in its epilogue; integer sums, no candidate lists,
 * no thresholds, so no pass bound and nothing for the status word; the result is a pure function of the inputs.  Rows behind
 * ntotal (zeros, or stale rows after reset() and a smaller add()) and NaN scores never count.
 * Cost: the corpus is read once per (tile of 16 queries, chunk of 8 references): ceil(nq / 16) * ceil(m / 8) passes at the
 * exact scan's stream rate, whatever the ranks turn out to be.  Typical m is 1..4 (a query's gold passages): one pass per 16
 * queries.  A GEMM-shaped many-query form (scanq's query staging) does not exist yet.  Nothing here changes how search routes
 * or what it returns.
 *
 * *_device entry points: single-device index (HAC_ERR_UNSUPPORTED otherwise), 16-byte aligned q_dev; they enqueue on
 * hip_stream, never read back and take no slot of the status ring.  Their workspace (counters and reference scores, nq * m * 12
 * bytes) grows by the rule of the search workspaces: run one call of the largest (nq, m) before capturing into a HIP graph.
 * nq == 0 or m == 0 is HAC_OK and touches nothing.  hac_index_last_plan afterwards reads
 * "count_ahead_kernel<MT=8> grid=(P,T) QT=.. chunks=.. lds=..".  Queries go out in launches of 1024; the text is the last
 * launch's (1025 queries: QT=1, T=1).
 * count_ahead is the primitive shards add up: ref_score_dev float32 [nq, m], ref_bound_dev int64 [nq, m], count_dev int64
 * [nq, m] over THIS index's rows (haconvdr_amd.sharded: the owner's score, bounds clamp(id - shard_base, 0, n_local), a sum).
 * Host rank_ids: synchronous, on the index's own stream, staged in chunks like score_ids; on a multi-device index the scores
 * come from the shard that owns the row, every shard counts its rows on a host thread of its own ahead of (score, the bound
 * translated into its numbering) and the host adds the counts. */
int hac_index_count_ahead_device(hac_index *idx, const float *q_dev, int64_t nq, const float *ref_score_dev, const int64_t *ref_bound_dev,
                                 int64_t m, int64_t *count_dev, void *hip_stream);
int hac_index_rank_ids(hac_index *idx, const float *q, int64_t nq, const int64_t *ids, int64_t m, int64_t *rank);
int hac_index_rank_ids_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ids_dev, int64_t m, int64_t *rank_dev,
                              void *hip_stream);

/* ---- range search: every row scoring above a per-query radius (faiss: index.range_search) -------------------------------
 * For a query q and a radius r (float32, one per query):
 *   range(q, r) = { rows x in [0, ntotal) : s(q, x) is not NaN and s(q, x) > r }
 * with s the canonical score above and a strict float comparison, as in faiss's inner-product range search: -0.0 == +0.0,
 * +-Inf are ordinary scores, a NaN or +Inf radius gives an empty list, r = -Inf gives every row whose score is neither NaN
 * nor -Inf.  Rows behind ntotal (zeros, or stale rows after reset() and a smaller add()) are never returned.  faiss leaves
 * the order inside a query's list unspecified; here it is the key order, (score desc, row asc), so that
 *   len(range(q, r)) == count_ahead(q, r, 0);
 *   range(q, r) is the first len entries of an unbounded search of q: for any k <= HAC_MAX_K the entries of search(q, k) with
 *     D > r equal the first min(k, len) entries of the range result bit for bit, D and I, on every search route;
 *   rank_ids(q, I_range)[j] == j for every position j.
 * Result, in faiss's layout: lims int64 [nq + 1], lims[0] = 0; query i owns D[lims[i] : lims[i + 1]] (float32) and
 * I[lims[i] : lims[i + 1]] (int64 rows; the device form: id_map_dev[row] when id_map_dev is given).
 *
 * The size of the result is not known before the call: both entry points take a capacity `cap`, in results, and are all or
 * nothing.  lims is always complete and exact, whatever cap is.  If lims[nq] <= cap, D and I are filled in [0, lims[nq]) and
 * nothing behind that is touched.  If lims[nq] > cap, the host form leaves D and I untouched and the device form may leave
 * anything in [0, cap) and writes nothing outside it.  Either way the call returns HAC_OK -- an overflow is an answer, not an
 * error: compare lims[nq] with cap and call again.  cap == 0 with D == I == NULL is a pure count.  The result is a pure
 * function of the inputs (two identical calls return identical bytes); there is no candidate buffer, no threshold and no
 * pass bound, so nothing goes to the status ring.
 *
 * How (csrc/range.inc): range_emit_kernel streams the rows once per tile of 16 queries in the shape of count_ahead_kernel --
 * same tiles, same bit-exact MFMA chain -- and, for the groups that have a hit at all, adds to the per-query counters and
 * appends (query, key) pairs to a staging buffer through one cursor (one atomic per wave and group; pairs at or behind cap are
 * dropped, counting never stops).  range_offsets_kernel turns the counters into lims and decides fits / overflows on the
 * device; the kernels behind it read that word and exit on an overflow.  range_scatter_kernel moves the pairs into their
 * query's segment, range_sort_kernel sorts blocks of 4096 keys in LDS, range_merge_kernel merges longer segments in
 * ceil(log2(cap / 4096)) passes between two buffers, range_results_kernel writes D and I.
 * Cost: ceil(nq / 16) passes over the rows at the exact scan's stream rate, whether or not the result fits, plus the sort;
 * by arithmetic that is 63 passes of 77 GB for 1000 queries over 25M rows (not measured).  A segment of millions of keys
 * (a radius far below the scores) is sorted correctly but may be slow: every merge pass moves all of it.  The workspace is 20
 * bytes per result of min(cap, nq * ntotal).
 *
 * Host form: q float32 [nq, d], radius float32 [nq]; synchronous, on the index's own stream; works on a multi-device index
 * (every shard answers for its rows on a host thread of its own, positions are remapped to the index's numbering as search
 * does, the host adds the shards' counts into lims and, when the total fits, merges each query's per-shard lists by key).  A
 * device workspace that cannot be allocated is HAC_ERR_OOM.
 * Device form: single-device index (HAC_ERR_UNSUPPORTED otherwise), 16-byte aligned q_dev (HAC_ERR_INVALID otherwise);
 * enqueues on hip_stream and never reads back.  The workspace grows by the rule of the search workspaces: run one call of
 * the largest (nq, cap) before capturing into a HIP graph.  The launches depend on (nq, cap) and the index's size, never on
 * the data.
 * Both: nq == 0 is HAC_OK, writes lims[0] = 0 and touches nothing else; HAC_ERR_INVALID for a null q / radius / lims with
 * nq > 0, for cap < 0 and for cap > 0 with a null D or I.  hac_index_last_plan afterwards reads
 * "range_emit_kernel grid=(P,T) QT=.. cap=.. sort_lds=4096 merge_passes=.. lds=..".  Queries go out in launches of 1024;
 * grid, QT and lds are the last launch's (1025 queries: QT=1, T=1), cap is the caller's, merge_passes is the call's.
 * Out of scope: haconvdr_amd.sharded.ShardedSearcher (one process per GPU: the lists would need a variable-length gather)
 * and a GEMM-shaped many-query form. */
int hac_index_range_search(hac_index *idx, const float *q, int64_t nq, const float *radius, int64_t cap, int64_t *lims, float *D,
                           int64_t *I);
int hac_index_range_search_device(hac_index *idx, const float *q_dev, int64_t nq, const float *radius_dev, int64_t cap,
                                  int64_t *lims_dev, float *D_dev, int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream);

/* ---- search among named rows: exact top-k over each query's candidate rows ---------------------------------------------
 * faiss: SearchParameters(sel=IDSelectorBatch(ids)), one selector per query -- the positive form of search_excluding, and the
 * ranking behind score_ids (dense re-ranking of another system's run, a BM25 top-1000).  For a query q and a candidate list c
 * (int64 row ids in the index's own numbering, as in "rows by id"; m per query):
 *   among(q, c, k) = the first k entries of { rows r in set(c), 0 <= r < ntotal, s(q, r) not NaN }
 *                    ordered by (s desc, r asc), padded with D = -FLT_MAX, I = -1
 * s is the canonical score: the k-ordered fmaf chain plus the "+ 0.0f" of a packed key, the same bits score_ids and every
 * search route return.  The list is a SET: a row named twice appears once.  -1 is padding and may stand anywhere in the list.
 * A NaN query gives padding only; +-Inf scores are ordinary scores, as in search.  Three consequences:
 *   - for D, I = search(q, k') on any route and k <= k': among(q, any permutation of I[i] with repeats and -1 mixed in, k)
 *     == search(q, k), D bit for bit;
 *   - D_among[i][j] has the bits of score_ids(q, I_among)[i][j] wherever I_among >= 0;
 *   - with E the complement of set(c) and k + |E| <= HAC_MAX_K: among(q, c, k) == search_excluding(q, k, E).
 * Limits: 1 <= k <= HAC_MAX_K (k may exceed m: the tail is padding) and 0 <= m <= HAC_MAX_AMONG = 4096, one LDS sort block;
 * anything else is HAC_ERR_INVALID, and the message names k, m and the ceiling.  Longer lists would need a block merge that
 * removes repeats across blocks: out of scope.  nq == 0 is HAC_OK and touches nothing; m == 0 with nq > 0 is HAC_OK and
 * writes lists of padding only (cand may then be NULL).
 * Ids outside [0, ntotal) follow the rows-by-id rule: the *_device forms ignore them; the host form ignores -1 and returns
 * HAC_ERR_INVALID for any other, names the first offending id with its (query, column), and writes nothing.
 *
 * How (csrc/among.inc): among_keys_kernel has score_ids_kernel's grid and gather -- one workgroup per (query, 256 candidates),
 * the query row in LDS, the row read from the row-major rescoring copy where it is current and from the tiles otherwise -- and
 * writes the packed key of (score, pos_base + row) into a [nq][P] workspace, P the power of two >= m; 0 for an id outside the
 * rows, a NaN score and the slots m..P.  among_select_kernel, one workgroup per query, sorts the P keys in LDS (bitonic,
 * descending; 32 KiB at the ceiling), drops repeats (equal non-zero keys are the same row and, sorted, neighbours) and compacts
 * the first k distinct non-zero keys by a block prefix count into [nq][k], the rest 0.  No atomics: the result is a pure
 * function of the inputs (two identical calls return identical bytes); nothing goes to the status ring.
 * Cost, by arithmetic (not measured): per query m gathered rows of 4d bytes -- contiguous out of the row-major copy, one useful
 * 16-byte piece per 64-byte sector out of the tiles -- plus one LDS sort of P keys; 1000 queries x 1000 candidates at d = 768
 * gather 3.1 GB (12.3 GB of sectors out of the tiles).  The corpus size does not enter.
 *
 * Host form: synchronous, on the index's own stream; one id check before the first kernel, queries and lists staged in chunks
 * of ~64 MiB.  It works on a multi-device index: the ids are translated to (shard, local row), every shard produces its
 * [nq, k] keys on a host thread of its own, positions are remapped as search does, and the slabs are merged at k on the first
 * device (a row lives in one shard, so no repeat crosses shards).
 * Device forms: single-device index (HAC_ERR_UNSUPPORTED otherwise), 16-byte aligned q_dev (HAC_ERR_INVALID otherwise); they
 * enqueue on hip_stream, never read back and take no slot of the status ring.  id_map_dev as in hac_index_search_device.  The
 * keys form writes the sorted packed keys [nq, k] with positions pos_base + row, the unit hac_merge_keys_device merges.  The
 * key workspace grows by the rule of the search workspaces: run one call of the largest (nq, m, k) before capturing into a
 * HIP graph; capturable once the segment table is up.  hac_index_last_plan afterwards reads
 * "among_keys_kernel grid=G among_select_kernel P=.. k=.. lds=..". */
int hac_index_search_among(hac_index *idx, const float *q, int64_t nq, int k, const int64_t *cand, int64_t m, float *D, int64_t *I);
int hac_index_search_among_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *cand_dev, int64_t m,
                                  float *D_dev, int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream);
int hac_index_search_among_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *cand_dev, int64_t m,
                                       uint64_t *keys_dev, uint32_t pos_base, void *hip_stream);

/* ---- search inside a bitmap: exact top-k over the rows a bitmap selects ---------------------------------------------------
 * faiss: SearchParameters(sel=IDSelectorBitmap(n, bitmap)), and IDSelectorRange / IDSelectorNot over large sets -- what lies
 * between search_among (at most HAC_MAX_AMONG named rows) and search_excluding (at most HAC_MAX_K - k rows left out): a tenth
 * of the corpus, one block, everything but 50 000 rows.  For a query q and a mask M:
 *   masked(q, M, k) = the first k entries of { rows r : 0 <= r < ntotal, bit r of M set, s(q, r) not NaN }
 *                     ordered by (s desc, r asc), padded with D = -FLT_MAX, I = -1
 * s is the canonical score: the k-ordered fmaf chain plus the "+ 0.0f" of a packed key, the same bits search returns.
 * Mask layout: masks is uint64 [n_masks][words], words = ceil(ntotal / 64); row r is bit r & 63 of word r >> 6, so a word is
 * exactly one 64-row group of the tiles.  Viewed as bytes on a little-endian host the words are faiss's IDSelectorBitmap bitmap,
 * np.packbits(bool, bitorder="little").  Bits at or above ntotal are ignored.
 * Which mask a query uses: mask_of is int64 [nq], the mask of each query.  A NULL mask_of means mask 0 for every query when
 * n_masks == 1 and mask i for query i when n_masks == nq; any other NULL case is HAC_ERR_INVALID.
 * Identities (proved on the CPU over the oracle by tests/test_index_masked.py):
 *   - an all-ones mask: masked(q, M, k) == search(q, k);
 *   - M the mask of a set S, |S| <= HAC_MAX_AMONG: masked(q, M, k) == search_among(q, k, S);
 *   - M the complement of a set E, k + |E| <= HAC_MAX_K: masked(q, M, k) == search_excluding(q, k, E);
 *   - masked(q, M, k) == the rows of range_search(q, -inf) that M selects, cut at k (then, if there is room, the selected rows
 *     scoring -Inf, which the strict comparison of a radius leaves out and every search lists last).
 * Arguments: words must equal ceil(ntotal / 64), otherwise HAC_ERR_INVALID -- which refuses a mask packed before an add or a
 * remove changed the size; 1 <= k <= HAC_MAX_K; n_masks >= 1 when nq > 0.  nq == 0 is HAC_OK and touches nothing; ntotal == 0
 * gives lists of padding only (words is then 0 and masks may be NULL).
 * mask_of out of range: the host form returns HAC_ERR_INVALID for an entry outside [0, n_masks), names the query and writes
 * nothing; in the *_device forms that query gets an empty list, all padding, and no error -- the split the by-id calls make.
 *
 * How (csrc/masked.inc, csrc/scan16_filter.inc): mask_groups_kernel builds, per query tile, the list of the 64-row groups in which the OR of the tile's
 * queries' mask words is non-zero (clipped to ntotal in the last group; ballot + prefix, one atomic per wave; the order of a
 * list is unspecified and does not matter).  scan16_masked_kernel is the list form of the one filtered body
 * (scan16_filter<LIST, CURSOR>, built like scan16_kernel from the shared row loop of csrc/scan16_core.inc) whose work items are that list:
 * the same row stream, the same bit-exact MFMA chain, the same candidate buffers and compaction; its epilogue appends a row
 * only if the lane's own query's mask word has the row's bit.  A row is tested before it becomes a candidate, so every
 * threshold comes from selected rows and is a proven lower bound of the masked k-th score: the result does not depend on the
 * number of row streams, the list order or the launch cuts (two identical calls return identical bytes).  No threshold
 * seeding: a sample of unmasked rows would give bounds the masked set cannot meet.  select_keys_kernel finishes, as in search.
 * Cost: one pass over nq x words mask words, then ceil(nq / QT) passes (QT = 16 queries, fewer at large k), each streaming its
 * tile's selected groups from the fp32 tiles -- a selective mask costs its own rows, not the corpus.  Built for selective masks
 * or few queries: a dense mask under many queries costs one corpus pass per 16 queries, the price of rank_ids; for a small
 * complement use search_excluding.  The queries are cut into launches of whole tiles so that the list workspace
 * (uint32 [tiles][groups]) stays within 64 MiB.
 *
 * Host form: synchronous, on the index's own stream; queries and the masks they name are staged in chunks of ~64 MiB.  It
 * works on a multi-device index: each shard searches its own rows under its own slice of every mask (the host copies the bit
 * ranges span by span), the lists are remapped and merged at k on the first device like search's.
 * Device forms: single-device index (HAC_ERR_UNSUPPORTED otherwise), 16-byte aligned q_dev; they enqueue on hip_stream and
 * never read back.  id_map_dev as in hac_index_search_device.  The keys form writes the sorted packed keys [nq, k] with
 * positions pos_base + row.  The workspaces grow by the rule of the search workspaces: run one call of the largest
 * (nq, k, n_masks) before capturing into a HIP graph.  Test switches (hac_index_set_option): "masked_p" = "auto" | 1..4096 row
 * streams per query tile, "debug_masked_tiles" = 0 | the most query tiles per launch.  hac_index_last_plan afterwards reads
 * "mask_groups_kernel grid=(..) scan16_masked_kernel<W=4> grid=(P,tiles) QT=.. C=.. lds=.. launches=..". */
int hac_index_search_masked(hac_index *idx, const float *q, int64_t nq, int k, const uint64_t *masks, int64_t n_masks, int64_t words,
                            const int64_t *mask_of, float *D, int64_t *I);
int hac_index_search_masked_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks, int64_t words,
                                   const int64_t *mask_of_dev, float *D_dev, int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream);
int hac_index_search_masked_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks, int64_t words,
                                        const int64_t *mask_of_dev, uint64_t *keys_dev, uint32_t pos_base, void *hip_stream);

/* ---- search by group: exact top-k groups of rows, each by its best row -----------------------------------------------------
 * faiss: grouped search (IDGrouper, since 1.8) -- a run of distinct passages where several rows share a passage id, page-level
 * retrieval over chunk rows, MaxP scoring, hard negatives from distinct documents.  For a query q, labels g[r] (one per row)
 * and k:
 *   rep(q, G)        = the row of group G with the greatest key (score desc, row asc) among its rows whose score is not NaN;
 *                      a group with no such row has none
 *   grouped(q, g, k) = the first k of { rep(q, G) : G a label that occurs } by (score desc, row asc),
 *                      padded with D = -FLT_MAX, I = -1
 * s is the canonical score: the k-ordered fmaf chain plus the "+ 0.0f" of a packed key, the same bits search returns.  Rows
 * behind ntotal, and stale rows after reset() plus a smaller add(), belong to no group.  +-Inf scores are ordinary scores and a
 * NaN query gives padding only, as everywhere else.  In other words: an unbounded search of q, reduced to the first row of every
 * label and cut at k.  search(q, k') followed by a de-dup is NOT this: it stops being exact as soon as one group owns more than
 * k' - k of the leading rows, and k' ends at HAC_MAX_K.
 * Identities (proved on the CPU over the oracle by tests/test_index_grouped.py, asserted on the GPU):
 *   - labels all distinct (arange(ntotal)): grouped(q, g, k) == search(q, k), bit for bit on every k;
 *   - one label for every row: search(q, 1) followed by padding;
 *   - grouped(q, g, k) == search_masked(q, k, M_q), M_q the per-query mask of { rep(q, G) };
 *   - rank_ids(q, I_grouped)[j] is strictly increasing in j and >= j, and score_ids of I_grouped has the bits of D_grouped;
 *   - grouped is the rows of range_search(q, -inf) kept at their label's first occurrence and cut at k, then the -Inf-scoring
 *     representatives if there is room.
 * Labels: group_of is int64 [n_labels], values in [0, 2^32) -- what offset2pid / passage_embedding2id hold, and 32 bits let a
 * (label, list position) pair fit one 64-bit LDS word.  n_labels must equal ntotal, otherwise HAC_ERR_INVALID -- which refuses
 * labels made before an add or a remove.  The array is a per-call argument like id_map_dev: the index holds no new state, and
 * add, remove_ids and reset need no new rule.  A label outside the range: the host form returns HAC_ERR_INVALID, names the first
 * offending row and writes nothing; the *_device form cannot look, so there such a row is in no list -- it is dropped before it
 * can contribute to any threshold, and a group that loses its best row this way is represented by its next.
 * Results: D, I as search; G (may be NULL) receives G[i][j] = group_of[row of slot j], the row's own label and never id_map's
 * value, -1 in padding slots.  1 <= k <= HAC_MAX_K; a k whose buffers do not fit LDS fails as search does, naming k.  nq == 0 is
 * HAC_OK and touches nothing; ntotal == 0 gives padding only.
 *
 * How (csrc/grouped.inc): scan16_grouped_kernel is built from the row loop scan16_kernel is built from
 * (csrc/scan16_core.inc) -- the same row stream, the same bit-exact MFMA
 * chain, the same candidate buffers -- and its own compaction sorts the buffer, gathers each entry's label, keeps only the best entry
 * of every label (a second sort, of (label << 32 | list position) words in a scratch LDS array) and cuts to k.  Only when k
 * distinct labels remain does the k-th key become the query's threshold: it is then the k-th best of k distinct groups' entries,
 * a proven lower bound of the k-th group score, so the result does not depend on the number of row streams, the launch cuts or
 * the order of work.  A buffer full of one group's rows shrinks to one entry and the scan goes on.  No threshold seeding and no
 * fp16 prefilter: a sample of rows says nothing about groups.  grouped_select_kernel (one workgroup per query, no atomics)
 * reduces the workgroups' survivors the same way; it is also the merge of the multi-device host form.
 * Cost (by arithmetic, NOT measured here; DESIGN.md records one timing): ceil(nq / QT) passes over the rows at the exact scan's
 * stream rate, QT = 16 queries and fewer at large k (the scratch array takes LDS: QT = 2 at k = 2048, d = 768), plus two LDS
 * sorts and one ordered pass per compaction where scan16 has one sort.  Until k distinct groups have been seen every row is a
 * candidate: a corpus led by one giant group compacts every (C - k) / 256 rounds throughout.
 *
 * Host form: synchronous, on the index's own stream.  Labels (8 bytes per row) and queries are staged to the device on EVERY
 * call: a caller that searches the same labels repeatedly should hold them on the device and use the device form.  It works on
 * a multi-device index: every shard searches its rows under its slice of the labels, the per-shard lists (at most k distinct
 * groups each) are remapped as search does and merged on the first device by grouped_select_kernel, reading the whole label
 * array there.
 * Device form: single-device index (HAC_ERR_UNSUPPORTED otherwise), 16-byte aligned q_dev; enqueues on hip_stream and never
 * reads back; id_map_dev as in hac_index_search_device.  The workspaces grow by the rule of the search workspaces: run one call
 * of the largest (nq, k) before capturing into a HIP graph.  Test switches (hac_index_set_option): "grouped_p" = "auto" |
 * 1..4096 row streams per query tile, "debug_grouped_tiles" = 0 | the most query tiles per launch.  hac_index_last_plan
 * afterwards reads "scan16_grouped_kernel<W=4> grid=(P,T) QT=.. C=.. lds=.. grouped_select_kernel n_in=.. launches=..".
 * Out of scope: haconvdr_amd.sharded.ShardedSearcher (a group may span ranks: the merge would need the labels of other ranks'
 * rows); a keys form; a GEMM-shaped many-query form; a certified fast path (search at k' > k through the prefilter, accepted
 * when k distinct labels appear, the grouped scan only for the rest). */
int hac_index_search_grouped(hac_index *idx, const float *q, int64_t nq, int k, const int64_t *group_of, int64_t n_labels, float *D, int64_t *I,
                             int64_t *G /* may be NULL */);
int hac_index_search_grouped_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *group_of_dev, int64_t n_labels, float *D_dev,
                                    int64_t *I_dev, int64_t *G_dev /* may be NULL */, const int64_t *id_map_dev, void *hip_stream);

/* ---- search behind a cursor: exact top-k resuming at a per-query (score, row) position ---------------------------------------
 * Every list of the calls above ends at HAC_MAX_K; rank_ids gives positions, not lists, and range_search a list only for a
 * radius known beforehand.  This call gives the NEXT page: more results in a conversation, hard negatives from a rank window
 * deeper than HAC_MAX_K, the rows right behind a gold passage, a corpus listed in pieces that fit memory -- at a cost per page
 * that does not grow with the depth.  For a query q, a cursor (s_ref, b) and k:
 *   after(q, s_ref, b, k) = the first k of { rows r in [0, ntotal) : s(q, r) not NaN and
 *                                            (s(q, r) < s_ref or (s(q, r) == s_ref and r > b)) }
 *                           by (score desc, row asc), padded with D = -FLT_MAX, I = -1
 * s is the canonical score: the k-ordered fmaf chain plus the "+ 0.0f" of a packed key, the same bits search returns.  The
 * comparisons are float comparisons: -0.0 == +0.0, and +-Inf are ordinary scores.  The condition is
 * make_key(s, r) < make_key(s_ref, b), with key = ord(score) << 32 | ~position: the complement of count_ahead's predicate minus
 * the cursor's own slot.
 * Cursor values:
 *   b >= 0                  as above.  b need not be a row of the index; at or above ntotal no row tying s_ref is eligible.
 *   b == -1                 a padding slot of an earlier list: that list had ended.  The result is padding only, whatever s_ref
 *                           is -- so (D[:, -1], I[:, -1]) of any page is a valid cursor for the next one (a padding cursor
 *                           (-FLT_MAX, -1) taken literally would list the rows scoring -FLT_MAX or -Inf a second time).
 *   b == HAC_AFTER_START    from the start: every row whose score is not NaN is eligible, s_ref is not read.
 *   b < -2                  a mistake: the host form returns HAC_ERR_INVALID, names the query and writes nothing; the *_device
 *                           forms give that query an empty list and no error -- the split the by-id calls make.
 *   s_ref NaN               an empty list.
 *   both pointers NULL      every query starts from the start (only one of them NULL: HAC_ERR_INVALID).
 * Key form of the cursor, one uint64 per query in the position space of pos_base: row r is eligible iff
 * make_key(s, pos_base + r) < after_key.  0, the empty slot of a key list, is an exhausted list and gives an empty result;
 * all-ones is the start (no row packs to either value); a NULL after_keys_dev starts every query from the start.  The last
 * column of any sorted key list is therefore the cursor of the next page: of hac_index_search_keys_device, of a merged list of
 * shards, of this call's own keys form.
 * Identities (proved on the CPU over the oracle by tests/test_index_after.py, asserted on the GPU):
 *   - with a start cursor, after == search(q, k), bit for bit at every k;
 *   - D, I = search(q, K) on any route, I[j] >= 0: after(q, D[j], I[j], k) is the entries j+1 .. j+k of an unbounded search,
 *     search(q, K)[j+1 : j+1+k] wherever that fits in K;
 *   - pages chained through their last entries, concatenated up to the first padding slot, are the unbounded search:
 *     range_search(q, -inf) followed by the rows scoring -Inf; no NaN-scoring row, no row twice, the page after the end is
 *     padding only;
 *   - rank_ids(q, I_page)[j] == rank_ids(q, cursor row) + 1 + j when the cursor names a row with a non-NaN score;
 *   - after(q, s_ref, b, k) == search_masked(q, k, M), M the per-query mask of { r : key(s(q, r), r) < key(s_ref, b) };
 *   - count_ahead(q, s_ref, b) + [row b exists and scores s_ref] + len(after(q, s_ref, b, unbounded)) == the number of rows
 *     whose score is not NaN.
 * 1 <= k <= HAC_MAX_K; nq == 0 is HAC_OK and touches nothing; ntotal == 0 gives padding only.
 *
 * How (csrc/after.inc, csrc/scan16_filter.inc): after_bounds_kernel turns the cursors into each query's exclusive upper key bound (NaN score, row -1 or
 * row < -2: 0; row -2: all-ones; otherwise the key of (s_ref + 0.0f, min(row, 2^32 - 1))).  scan16_after_kernel is the cursor form of
 * the filtered body (scan16_filter<LIST, CURSOR>: scan16_masked_after_kernel is both forms at once), over every 64-row group -- scan16_kernel's row loop
 * (csrc/scan16_core.inc): the same row stream, the same bit-exact MFMA chain, the same candidate buffers and
 * compaction -- whose epilogue appends a row only if its key is below the lane's own query's bound.  A row is tested before it
 * becomes a candidate, so every threshold comes from eligible rows and is a proven lower bound of the answer's k-th score: the
 * result does not depend on the number of row streams, the launch cuts or the order of work.  No threshold seeding: a sample of
 * rows would give bounds the rows behind the cursor cannot meet.  select_keys_kernel finishes, as in search.
 * Cost (by arithmetic, NOT measured here; DESIGN.md records one timing): a page costs ceil(nq / QT) passes over the rows at the exact scan's stream rate,
 * QT = 16 queries and fewer at large k (QT = 4 at k = 2048, d = 768), whatever the depth of the cursor; a listing to depth K
 * costs ceil(K / k) pages.
 *
 * Host form: synchronous, on the index's own stream; queries and their bounds are staged in chunks of ~64 MiB.  It works on a
 * multi-device index: the cursor is in the index's numbering, and each shard searches behind a bound of its own,
 * (ord(s_ref) << 32) + (2^32 - 1 - b_local) in 64 bits, b_local = (the shard's rows at global positions <= b) - 1 -- with
 * b_local = -1 that is (ord + 1) << 32, every row of the shard tying s_ref.  The lists are remapped and merged at k on the first
 * device like search's.
 * Device forms: single-device index (HAC_ERR_UNSUPPORTED otherwise), 16-byte aligned q_dev; they enqueue on hip_stream and
 * never read back.  id_map_dev remaps the RESULT only, as in hac_index_search_device: cursor rows are always the index's own
 * rows, so a caller that maps ids pages with the keys form.  The keys form writes the sorted packed keys [nq, k] with positions
 * pos_base + row.  The workspaces grow by the rule of the search workspaces: run one call of the largest (nq, k) before
 * capturing into a HIP graph.  Test switches (hac_index_set_option): "after_p" = "auto" | 1..4096 row streams per query tile,
 * "debug_after_tiles" = 0 | the most query tiles per launch.  hac_index_last_plan afterwards reads
 * "scan16_after_kernel<W=4> grid=(P,T) QT=.. C=.. lds=.. launches=..".
 * Out of scope: an fp16 prefilter or a GEMM-shaped many-query route for cursor searches (the first page of a listing may take
 * search's: its last key is a cursor); cursors for the excluding / among / grouped variants (the masked one: the next section). */
#define HAC_AFTER_START (-2)
int hac_index_search_after(hac_index *idx, const float *q, int64_t nq, int k, const float *after_score, const int64_t *after_row, float *D, int64_t *I);
int hac_index_search_after_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const float *after_score_dev, const int64_t *after_row_dev,
                                  float *D_dev, int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream);
int hac_index_search_after_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *after_keys_dev, uint64_t *keys_dev,
                                       uint32_t pos_base, void *hip_stream);

/* ---- search inside a bitmap, behind a cursor: exact pages of the rows a bitmap selects ---------------------------------------
 * "More results, but only from this topic"; hard negatives from ranks 2000 .. 4999 of the passages of one source; the n passages
 * right behind the gold passage that the user has not seen.  For a query q, its mask M, a cursor (s_ref, b) and k:
 *   masked_after(q, M, s_ref, b, k) = the first k of
 *       { r in [0, n_rows) : bit r of M set, s(q, r) not NaN, make_key(s(q, r), pos_base + r) < bound }
 *       by (score desc, row asc), padded with -FLT_MAX / -1
 * bound is search_after's per-query exclusive upper key bound: make_key(s_ref, b) by after_bounds_kernel's rule (a NaN score,
 * row -1 and a row below -2 give 0, an exhausted list; HAC_AFTER_START gives all-ones, the start), or the key form's after_key
 * as it stands.  M is the query's own mask by search_masked's rule (mask_of; or one mask for every query; or mask i for query
 * i), in search_masked's layout; bits at or above ntotal select nothing.  s is the canonical score, the bits search, score_ids
 * and every other route return.
 * What follows (proved on the CPU over the oracle by tests/test_index_masked_after.py, asserted on the GPU):
 *   - the cursor row need not be selected by the mask, and need not exist: the bound is a key, not a row;
 *   - an all-ones mask gives search_after; the start cursor gives search_masked, bit for bit at every k;
 *   - pages chained with cursor = (D[:, -1], I[:, -1]) under the same masks list exactly the unbounded masked list, in order:
 *     nothing twice, nothing missing, ties continued by row, and a padding cursor (row -1) gives padding.
 * Arguments: the union of the two parents' -- words == ceil(ntotal / 64), n_masks >= 1 when nq > 0, 1 <= k <= HAC_MAX_K,
 * after_score and after_row both given or both NULL (the start for every query).  nq == 0 is HAC_OK and touches nothing;
 * ntotal == 0 gives padding only.  The host form refuses, with the query named and nothing written, a mask_of entry outside
 * [0, n_masks), a cursor row below -2, and one cursor pointer without the other; the *_device forms give such a query an empty
 * list and no error.
 *
 * How (csrc/scan16_filter.inc): mask_groups_kernel's lists and after_bounds_kernel's bounds as they are;
 * scan16_masked_after_kernel is scan16_masked_kernel with the lane's own query's bound loaded once.  Its epilogue appends a row
 * only if s >= th, row < rows_valid, the lane's own mask bit is set AND key < bound: every test before the append, so every
 * threshold is the k-th key of some rows that are selected and behind the cursor -- a proven lower bound of the answer's k-th
 * score, whatever the row streams, the list order or the launch cuts.  No threshold seeding.  select_keys_kernel finishes.
 * Cost (by arithmetic; DESIGN.md records one timing): what search_masked costs at that mask -- the tile's selected groups per
 * ceil(nq / QT) tiles -- at any depth; the extra work is one u64 comparison per candidate that already passed s >= th.
 *
 * Host form: synchronous; works on a multi-device index: every shard searches its own rows under its slice of the masks
 * (search_masked's chunks, 8 more bytes per query for the bound) behind a bound of its own (search_after's rule, computed by
 * the same function), remapped and merged at k on the first device.
 * Device forms: single-device index, 16-byte aligned q_dev, enqueue on hip_stream and never read back.  id_map_dev remaps the
 * RESULT only.  The keys form takes after_keys_dev (NULL: the start) and writes sorted packed keys [nq, k] in the position
 * space of pos_base; its last column is the cursor of the next page.  Capturable after one call of the largest
 * (nq, k, n_masks).  Test switches: search_masked's "masked_p" and "debug_masked_tiles".  hac_index_last_plan afterwards reads
 * "mask_groups_kernel grid=(..) scan16_masked_after_kernel<W=4> grid=(P,tiles) QT=.. C=.. lds=.. launches=..".
 * Out of scope: cursors for grouped, among and excluding; a masked entries_at / search_at; a prefilter-backed or many-query
 * masked scan; skipping groups by cursor. */
int hac_index_search_masked_after(hac_index *idx, const float *q, int64_t nq, int k, const uint64_t *masks, int64_t n_masks, int64_t words,
                                  const int64_t *mask_of, const float *after_score, const int64_t *after_row, float *D, int64_t *I);
int hac_index_search_masked_after_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks, int64_t words,
                                         const int64_t *mask_of_dev, const float *after_score_dev, const int64_t *after_row_dev, float *D_dev,
                                         int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream);
int hac_index_search_masked_after_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks,
                                              int64_t words, const int64_t *mask_of_dev, const uint64_t *after_keys_dev, uint64_t *keys_dev,
                                              uint32_t pos_base, void *hip_stream);

/* ---- entry at a rank: what sits at position t of a query's unbounded ranking? -------------------------------------------------
 * rank_ids answers row -> rank, count_ahead (score, row) -> rows ahead, search_after cursor -> next page, range_search radius ->
 * list.  This is the missing inverse, rank -> entry, at a cost that does not grow with the rank: hard negatives from a rank
 * window without the pages in front of it, page 57 of a listing without pages 1 - 56, the score at a rank (the radius that makes
 * range_search return exactly n rows; score quantiles of a corpus), an independent check of rank_ids.
 * For a query q let L(q) be the rows r in [0, ntotal) whose canonical score s(q, r) is not NaN, ordered by make_key(s, r)
 * descending, i.e. by (score desc with -0.0 == +0.0, row asc).  s is the canonical score: the k-ordered fmaf chain plus the
 * "+ 0.0f" of a packed key, the same bits search returns.
 *   entry_at(q, t) = the t-th entry of that order (0-based) when 0 <= t < |L(q)|;
 *                    otherwise padding: key 0, D = -FLT_MAX, I = -1.
 * No ceiling at HAC_MAX_K.  A NaN-scoring row is never an entry; +-Inf are ordinary scores; a row scoring exactly -FLT_MAX is a
 * real entry (I >= 0), not padding.  ntotal == 0 gives padding only; nq == 0 or m == 0 is HAC_OK and touches nothing.  ranks
 * [nq][m] are VALUES, not ids: any rank outside [0, |L(q)|), negative ones included, gives padding and is never an error, on
 * the host form too.
 * Identities (proved on the CPU over the oracle by tests/test_index_at_rank.py, asserted on the GPU):
 *   - entries_at(q, 0 .. k-1) == search(q, k) bit for bit on any route, padding included;
 *   - rank_ids(q, I_at)[i][j] == ranks[i][j] wherever I_at >= 0;
 *   - entries_at(q, rank_ids(q, ids)) returns ids and score_ids(q, ids) wherever the rank is >= 0;
 *   - search_after(q, k, entries_at(q, t)) == the entries t+1 .. t+k of the unbounded search;
 *   - with c = range_count(q, radius): D_at(c-1) > radius >= D_at(c) when both exist;
 *   - |L(q)| is the smallest t that gives padding.
 *
 * How (csrc/at_rank.inc): a radix selection over the 64-bit key, 8 bits at a time from the top, per (query, rank) pair.  A pair
 * takes one query slot of a 16-wide tile -- a query with m ranks appears m times -- and carries, on the device, the key prefix
 * found so far and the rank that remains inside it.  rank_hist_kernel is count_ahead_kernel's pass (the same row stream, the same
 * bit-exact MFMA chain) with an epilogue that, for every row whose key agrees with the pair's prefix, adds 1 to the bin of the
 * key's next digit: histograms in LDS, flushed with integer atomics, so the result is a pure function of the inputs whatever
 * the row streams, launch cuts and order.  rank_narrow_kernel walks a pair's 256 bins from the top, extends the prefix by the
 * bin that holds the remaining rank and subtracts the rows above it.  A rank outside [0, total of the first histogram) marks
 * the pair dead: key 0.  After the last digit the prefix is the key; hac_keys_to_results_device's kernel makes D / I.
 * Passes over the rows per tile of 16 pairs: 4 score digits + the position digits in which two rows of the index can differ,
 *   passes = 4 + ceil(bit_length(pos_base ^ (pos_base + ntotal - 1)) / 8)        (pos_base = 0 outside the keys form)
 * i.e. 5 up to 256 rows, 6 up to 65 536, 7 up to 16.7M, 8 beyond; the higher position digits are the same for every row and
 * the host fills them in.  Pairs go out in launches of 1024.  There is one path: no shortcut through search for shallow ranks.
 * Cost (by arithmetic, NOT measured here; DESIGN.md section 2 records the one timing taken): ceil(nq * m / 16) * passes passes
 * over the rows at the exact scan's stream rate -- 16 ranks of one query cost what 16 queries with one rank each cost; the
 * epilogue looks at every group in the first pass and, behind the second digit, at almost none.  search_at = one entries_at of
 * one rank per query plus one search_after page, at any depth.
 *
 * Host form: synchronous, on the index's own stream; queries, ranks and keys are staged in chunks of ~64 MiB like rank_ids.
 * Device forms: 16-byte aligned q_dev; they enqueue on hip_stream and never read back; the number and shape of the launches
 * depend on (nq, m) and the index's size only.  id_map_dev remaps I as in hac_index_search_device.  The keys form writes the
 * packed keys [nq][m] with positions pos_base + row, in the key space of hac_index_search_keys_device and of
 * hac_index_search_after_keys_device's cursors: an entry's key is the cursor of the page behind it.  The rule of the other keys
 * forms holds for pos_base: pos_base + ntotal > 2^32 - 1 is HAC_ERR_UNSUPPORTED ("row positions exceed 32 bits") and nothing
 * is enqueued.  The workspace (1040 bytes per pair of a launch, 8 more per pair of the call for the forms that return D / I)
 * grows by the rule of the search workspaces: run one call of the largest (nq, m) before capturing into a HIP graph.
 * Test switches (hac_index_set_option): "at_rank_p" = "auto" | 1..4096 row streams per pair tile, "debug_at_rank_tiles" = 0 | the
 * most pair tiles per launch.  hac_index_last_plan afterwards reads "rank_hist_kernel<BITS=8> grid=(P,T) QT=.. passes=.. lds=..".
 * Out of scope: multi-device (in-process sharded) indexes -- the position digits of shards whose rows map to index rows through
 * several spans do not line up: all three entry points return HAC_ERR_UNSUPPORTED and write nothing;
 * haconvdr_amd.sharded.ShardedSearcher -- with one contiguous shard_base per rank the histograms of the ranks simply add, which
 * is why the keys form takes pos_base, but the per-pass all-reduce is not built; an fp16-prefilter or GEMM-shaped many-query
 * route; ranks inside the masked / grouped / among / excluding variants. */
int hac_index_entries_at(hac_index *idx, const float *q, int64_t nq, const int64_t *ranks, int64_t m, float *D, int64_t *I);
int hac_index_entries_at_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ranks_dev, int64_t m, float *D_dev, int64_t *I_dev,
                                const int64_t *id_map_dev, void *hip_stream);
int hac_index_entries_at_keys_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ranks_dev, int64_t m, uint64_t *keys_dev,
                                     uint32_t pos_base, void *hip_stream);

/* ---- removing rows: faiss's IndexFlat::remove_ids(IDSelectorBatch(ids)), in place ------------------------------------------
 * The rows named by ids disappear; every surviving row keeps its bits and its relative order; the survivors are renumbered
 * densely from 0 -- survivor number j is row j of np.delete(x, unique(ids), axis=0) --; ntotal drops by the number of DISTINCT
 * rows removed, which is what *n_removed receives (n_removed may be NULL); rows added afterwards continue at the new ntotal.
 * After the call every entry point (search on every route, search_excluding, reconstruct, score_ids, rank_ids, count_ahead,
 * range_search) behaves exactly as an index that had been built by adding the surviving rows: the result bits are the same.
 *
 * ids: host int64 [n], the rule of the host entry points above: duplicates are allowed, -1 is a padding slot and is ignored,
 * any other id outside [0, ntotal) is HAC_ERR_INVALID, the message names the first offending id and its position, and NOTHING
 * is changed.  n == 0, or only padding, is HAC_OK, removes 0 rows and leaves the segment table alone (a captured search stays
 * valid).
 *
 * How (csrc/remove.inc, csrc/rows_host.inc): the ids are sorted and made unique on the host.  Groups of 64 rows in front of the
 * first removed row are not touched.  Behind it compact_rows_kernel -- one workgroup per destination group, one binary search
 * per lane over the removed rows, whole 1-KiB chunks out -- gathers ascending chunks of ~64 MiB of destination rows into the
 * add path's staging buffer, and device-to-device copies put them in place; a destination row never lies behind its source,
 * so a chunk only overwrites rows that no later chunk reads.  No allocation grows with the corpus.  Segments left empty are
 * freed with their images; add() continues in the partial last segment.  An fp16 image or a row-major rescoring copy that was
 * complete before the call is complete when it returns (rebuilt from the tiles over the changed groups); a segment without
 * one gets none.  Only bits move: NaN payloads, +-Inf, -0.0 and denormals survive.
 * Cost, with the first removed row at local row f of a shard of n rows: 4 * (n - f) * d * 4 bytes of HBM traffic (every moved
 * row is read and written twice), plus the image rebuilds over the same groups; removing rows near the end is nearly free,
 * removing row 0 moves the shard.
 *
 * A host call: synchronous, on the index's own stream like add / reset (synchronize your own streams first, as for those); the
 * segment table changes, so a search captured into a HIP graph before the call must be captured again.  It works on a
 * multi-device index: the ids are split by shard, every shard compacts its rows on a host thread of its own, and the spans
 * that translate shard rows to index rows are rewritten.  Everything that can fail cheaply (the id check, the workspaces of
 * every shard) happens before the first kernel; if a shard still fails after another has finished, the error is reported and
 * the index must be reset() before it is used again.  There is no *_device form: ntotal has to reach the host.
 * Out of scope: haconvdr_amd.sharded.ShardedSearcher (removing on one rank moves every later rank's shard_base). */
int hac_index_remove_ids(hac_index *idx, const int64_t *ids, int64_t n, int64_t *n_removed);

/* Device-detected failures of searches enqueued so far (the host entry points report them themselves; the *_device entry
 * points cannot, they never read back).  Waits for the index's own streams only: synchronize YOUR stream first, then call
 * this.  Returns HAC_OK, or HAC_ERR_INTERNAL with the details in hac_last_error(); reading clears the device's error word
 * (hac_index_reset clears it too).  Every scan kernel bounds its candidate-compaction loop by the number of passes the
 * worst legal input needs; a workgroup that reaches the bound sets the word, drops what it still held, and the queries of
 * its tile come back with EMPTY lists: an invariant slip is an error code, not a hang and not wrong bits. */
int hac_index_last_status(hac_index *idx);

/* Tuning and test switches of a live handle: "split" = "0" | "1" | "auto", "split_terms" = "1" | "3",
 * "force_scan16" = "0" | "1", "scanq_nt" = "0".."4", "scanq_waves" = "4" | "8", "scan_no_p8" = "0" | "1",
 * "seed_groups_max" = cap of the prefilter's seeding pass in 64-row groups (integer >= 0; 0 = by size: 14 sqrt(groups),
 * or 1024 groups when the scan is cut into passes),
 * "split_decide" = "auto" (host entry point: host, *_device: device) | "host" | "device": who reads the certificates,
 * "scan_passes" = "auto" | "1" .. "5" (prefilter: passes of the main scan, the thresholds refreshed from everything found so
 * far between them; auto: 3 from 1.6M rows, 4 from 8.4M), "scan_pass_cuts" = "auto" | "a,b" (where the first two passes end, in
 * thousandths of the rows; auto: the first after ~6k 64-row groups, the others in geometric progression towards the corpus), "debug_max_pass" = integer >= 0 (tests: the pass bound of the
 * candidate loops; 0 = the bound no legal input reaches),
 * "scan_halfq" = "1" (default) | "0" (development: a prefilter search of one tile with <= 128 / <= 64 queries runs an instantiation
 * that leaves out the empty query tiles' matrix work -- "tiles=half" / "tiles=quarter" in the plan text; "0" pins the full-tile form; same bits),
 * "fp16_image" = "lazy" (default) | "eager": when the fp16 image of the rows (what the prefilter streams) is made: by the first
 * search that wants it, or by add() while it tiles the rows of a new segment (a resident index that will serve few queries per call
 * is then fast from its first search; best effort, +50 % of the corpus in HBM either way),
 * "rescore_rows" = "auto" | "0" | "1": the prefilter's exact rescoring reads ~130 scattered rows per query; out of the T64 tiles
 * that is one useful 16-byte piece per 64-byte sector.  Small indexes (auto: <= 12M rows) therefore keep their rows once more,
 * row-major, for the rescoring alone (+100 % of a small corpus, built lazily by the THIRD prefilter search after the last add /
 * reset of an index that has none -- an index searched once per block, the reference's add / search / reset loop, never pays for
 * it --, kept current across later adds, best effort: when the allocation fails the tiles are read as before); "1" builds it with the
 * first such search at any size, "0" never (and frees one that exists, as does growing past the size).  Same bits either way.
 * "masked_p" = "auto" | "1" .. "4096" and "debug_masked_tiles" = integer >= 0: tests of hac_index_search_masked* ("search inside a
 * bitmap": row streams per query tile; the most query tiles per launch, 0 = by the list workspace).  Same bits either way.
 * "grouped_p" = "auto" | "1" .. "4096" and "debug_grouped_tiles" = integer >= 0: the same two switches of hac_index_search_grouped*
 * ("search by group").  Same bits either way.
 * "after_p" / "debug_after_tiles" and "at_rank_p" / "debug_at_rank_tiles": the same pairs of hac_index_search_after* ("search behind
 * a cursor") and hac_index_entries_at* ("entry at a rank").  Same bits either way.
 * Any other name or value is HAC_ERR_INVALID (never a silent default), hac_last_error() naming the option, the value and the
 * allowed set; a rejected value changes nothing.
 * Six environment variables give the defaults of the first six options and are read once, leniently (a value outside the set
 * falls to a default), in hac_index_create: HAC_SPLIT, HAC_SPLIT_TERMS, HAC_FORCE_SCAN16, HAC_SCANQ_NT, HAC_SCANQ_WAVES and
 * HAC_SCAN_NO_P8 (set to anything: "1").  The other options have no variable. */
int hac_index_set_option(hac_index *idx, const char *name, const char *value);

/* Profiling aid for bench.py: when enabled, the main scan kernel of every search is
 * bracketed by a hipEvent pair recorded on the launch stream (no host sync).
 * hac_index_profile_drain() waits for the recorded pairs, writes up to cap kernel
 * durations (ms, in launch order) to ms_out, sets *n_out and clears the record. */
int hac_index_set_profiling(hac_index *idx, int enable);
int hac_index_profile_drain(hac_index *idx, float *ms_out, int cap, int *n_out);
/* Human-readable description of the kernel configuration of the most recent search
 * (kernel name, grid, queries per workgroup, candidate slots, LDS bytes). */
const char *hac_index_last_plan(const hac_index *idx);

/* ------------------------------------------------------- top-k list merging */
/* K9: merge L per-block / per-shard key lists into one.  lists_dev: uint64
 * [L, nq, k] (each [nq,k] slab sorted descending, 0 = empty); out_dev: [nq, k].
 * Equals the reference's sequential `>=` block merge (:131-149) when slabs are in
 * block order and positions increase with the block index. */
int hac_merge_keys_device(int device, const uint64_t *lists_dev, int n_lists, int64_t nq, int k,
                          uint64_t *out_dev, void *hip_stream);
/* keys -> (D float32, I int64); id_map_dev optional (position -> external id). */
int hac_keys_to_results_device(int device, const uint64_t *keys_dev, int64_t n_keys,
                               const int64_t *id_map_dev, float *D_dev, int64_t *I_dev,
                               void *hip_stream);

/* Per query, the first kout keys of a sorted list whose position is not excluded.  keys_dev: uint64 [nq, kin], every row sorted
 * descending, 0 = empty slot (what hac_index_search_keys_device and hac_merge_keys_device write); excl_pos_dev: int64 [nq, e]
 * GLOBAL positions, pos_base + row, the numbering the keys carry (may be NULL when e == 0) -- a value < 0 or > 0xFFFFFFFF is
 * padding and matches nothing, duplicates are allowed; out_dev: uint64 [nq, kout], the surviving keys in their order, then 0.
 * 1 <= kout <= kin <= HAC_MAX_K, 0 <= e < HAC_MAX_K, out_dev must not alias keys_dev (the row strides differ): otherwise
 * HAC_ERR_INVALID.  One launch on hip_stream, no atomics: the output is a pure function of the inputs.  nq == 0 is HAC_OK. */
int hac_filter_keys_device(int device, const uint64_t *keys_dev, int64_t nq, int kin, const int64_t *excl_pos_dev, int e, int kout,
                           uint64_t *out_dev, void *hip_stream);

/* ----------------------------------------------------------------- encoder */
/* model(input_ids, attention_mask) -> float32 [B,768]: ANCE.forward, src/models.py:39-64
 * (RobertaModel -> last_hidden_state[:,0] -> embeddingHead -> norm), called at
 * src/test_HAConvDR_topiocqa.py:211 and gen_doc_embeddings.py:110.  RoBERTa-base geometry. */
typedef struct hac_encoder hac_encoder;
typedef struct {
    int n_layers;      /* 12 for ANCE */
    int hidden;        /* 768 */
    int n_heads;       /* 12 */
    int ffn;           /* 3072 */
    int vocab;         /* 50265 */
    int max_pos;       /* 514 */
    int type_vocab;    /* 1 */
    int pad_token_id;  /* 1: position ids are cumsum(id != pad)*(id != pad) + pad (HF RoBERTa); not read with "model" = "bert" (pos = t) */
    float ln_eps;      /* 1e-5 */
} hac_encoder_config;

int hac_encoder_create(const hac_encoder_config *cfg, int device, hac_encoder **out);
void hac_encoder_destroy(hac_encoder *enc);
/* One tensor of the checkpoint, by its state-dict name (ANCE.from_pretrained keys, :170):
 * "roberta.embeddings.*", "roberta.encoder.layer.N.*", "embeddingHead.*", "norm.*"
 * ("classifier.*" exists in the checkpoint but is unused by forward: do not pass it); with "model" = "bert" (hac_encoder_set_option)
 * the first two are "bert.embeddings.*", "bert.encoder.layer.N.*".
 * data: host float32, copied before return. */
int hac_encoder_set_weight(hac_encoder *enc, const char *name, const float *data, size_t count);
/* Checks that every tensor is present and packs the GEMM weights to bf16. */
int hac_encoder_finalize(hac_encoder *enc);
/* ids, mask: host int32 [B, L]; mask must be a prefix mask (first len >= 1 ones) as both
 * reference pipelines produce (gen_doc_embeddings.py:38-40, src/data.py:8-23), attended ids in
 * [0, vocab); out: host float32 [B, 768].  Synchronous.  HAC_ERR_INVALID names the first bad sequence. */
int hac_encoder_forward(hac_encoder *enc, const int32_t *ids, const int32_t *mask, int B, int L, float *out);
/* Device/stream variant: ids/mask device pointers of elem_bytes 4 (int32) or 8 (int64, what the
 * reference passes); out_dev float32 [B,768].  Work is enqueued on hip_stream.  A batch of more than
 * 524288 padded rows (B * roundup(L,32); option "max_tokens") runs as several sub-batches sized by the real lengths: that
 * costs ONE read-back of B ints, i.e. the call synchronizes hip_stream once (not capturable); smaller
 * batches never synchronize.  Errors the device finds are reported per sequence: a mask that is not
 * a non-empty prefix mask, or an attended token id outside [0, vocab) (nn.Embedding would raise),
 * yields a NaN row for THAT sequence only; the host variant turns such a row into HAC_ERR_INVALID. */
int hac_encoder_forward_device(hac_encoder *enc, const void *ids_dev, const void *mask_dev, int elem_bytes,
                               int B, int L, float *out_dev, void *hip_stream);
/* Tuning and test switches of a live handle: "gemm" = "auto" (by batch size) | "classic" (128^2 / 256^2 two-stage
 * kernels with separate LayerNorm passes) | "8phase" (the large-batch ping-pong kernel with folded LayerNorms whenever
 * the batch has a whole 256-row tile); "attn" = "stream" (persistent single-pass attention kernels, the default) |
 * "twopass" (one workgroup per (sequence, head), exact row maxima first: the cross-check of the tests);
 * "graph" = "auto" (default) | "off": batches of at most 16384 padded rows (the reference's own call shape is 4 queries per GPU,
 * src/test_HAConvDR_topiocqa.py:173,406: ~110 launches for ~0.4 TFLOP) are captured ONCE per (B, L, elem_bytes, options) into a HIP
 * graph over private input / output buffers and replayed -- per call one graph launch and three small device copies; the first call
 * of a shape runs plain launches (it sizes the workspaces), the second captures, later ones replay; results are the same bits as
 * with "off" (at most 64 shapes are kept per encoder; beyond that the cache starts over).  Not used while profiling is on or while
 * the caller's stream is itself capturing;
 * "ksplit" = "auto" (default) | "off": with few rows (the classic 128^2 kernels) the two residual GEMMs of a layer split their
 * K loop over 2..6 work items per tile where that pays (by a measured cost model of rows and K), the partial sums being added in a fixed order by
 * the LayerNorm pass behind them: deterministic, but the summation order -- hence the last bits of an embedding -- then depends
 * on the batch's row count (as it does between the "gemm" families); "off" restores one summation order for every small batch;
 * "ksplit_pin" = "a/b" (development, tools/ks_sweep.py: the slices of out-proj / FFN-down pinned; "0/0" = by the model);
 * "attn_qs_pin" = "0" | "1" | "2" | "4" | "8" | "16" (development, tools/opt_sweep.py: the streaming attention's query split pinned; "0" = by the rule);
 * "max_tokens" = packed rows per sub-batch (integer >= 4096); "attn_qsplit" = "auto" (default) | "off" (with few sequences the streaming
 * attention kernel deals the query rows of a (sequence, head) item to 2..16 workgroups and runs both length classes in one launch;
 * same bits); "attn_pipe" = "auto" (default) | "off" | "all" (whole (sequence, head) items -- no query split, not the <s>-only last layer -- of sequences
 * longer than 256 rows go through the kernel with two query blocks per wave, the softmax of one woven into the MFMAs of the
 * other, followed by a fix-up pass of the one-block kernel over the items whose softmax reference has to move; in "auto" a layer whose items mostly needed
 * that pass in an earlier forward goes through the one-block kernel directly, with a retry every 64th forward; "off": the one-block kernel
 * everywhere; "all" (tests): the woven form for every whole item of either length class, always; same bits); "g8_stagger" = "auto" (default) | "off" (the workgroups of the large-batch
 * QKV and out-projection GEMMs start in four phases, one per pair of XCDs, so that their epilogues do not reach HBM all at once;
 * timing only, same bits).  Any other name or value is HAC_ERR_INVALID (never a
 * silent default).  HAC_ENC_GEMM gives the default of "gemm" and is read once, in hac_encoder_create.
 * "auto" decides ONCE per forward call, from the rows of the whole batch: every sub-batch of a call runs the same
 * GEMM family and tile size, so a sequence's embedding does not depend on the sub-batch it fell into.
 *
 * "precision" = "bf16" (default) | "split".  "bf16": every operand of every matrix product is rounded to bf16 (2^-9 relative);
 * whether a checkpoint stays inside the 1e-3 cosine contract then depends on its weights.  "split": every
 * matrix product of the forward -- QKV / out-projection / FFN, Q.K^T, P.V and the last layer's <s>-row tail -- takes both
 * operands as a pair hi = bf16(v), lo = bf16(v - hi) and accumulates a_lo.b_hi + a_hi.b_lo + a_hi.b_hi in fp32, in one fixed
 * order (deterministic; eager launches, capture and replay give the same bits): operand error 2^-17 relative, GELU by an erf
 * good to fp32, fp32 residual stream, LayerNorm, softmax and head.  The forward then always has the structure of the classic
 * family with 128^2 tiles ("gemm" is ignored; "ksplit", "graph", "max_tokens" work as usual; hac_encoder_last_plan reports
 * gemm=split128 ... attn_form=split precision=split).  Cost: three MFMAs per product and twice the staged operand bytes --
 * several times the bf16 forward's time ("Precision") -- plus one more copy of the bf16 layer weights and
 * of the bf16 activation workspaces in HBM, allocated by the first forward that runs in the mode, not by hac_encoder_finalize.
 * Use it for a checkpoint whose embeddings differ between the two modes by more than a small fraction of 1e-3 in 1-cos
 * (INTEGRATION.md).  Switching back to "bf16" restores the default path bit for bit.
 *
 * "pooling" = "first" (default) | "mean": the two arms of the reference's masked_mean_or_first (src/models.py:52-61).  "first"
 * is use_mean = False, emb_all[:, 0]: the last layer computes keys and values of every row but everything else for the <s>
 * rows only.  "mean" is use_mean = True, sum(t * mask) / sum(mask) over each sequence's attended tokens: the last layer runs on
 * every row like the others (full QKV, full attention, out-projection, FFN, statistics) in all three forward structures (gemm8,
 * classic, "precision" = "split"), pool_mean_kernel then averages the len valid rows of each sequence under the last layer's
 * output LayerNorm in fp32, in an order fixed by the sequence's length alone (deterministic: eager launches, capture and replay
 * and any batch around the sequence give the same bits), and the fp32 head follows unchanged.  Cost: the last layer's full
 * price instead of a third of its QKV GEMM plus a B-row tail, about one layer in n_layers more per forward, and one pass over
 * the last layer's rows ("Pooling").  Family choice, "ksplit", "graph" (the mode is part of a captured
 * shape's key), "max_tokens" and the profiling classes work as in "first" (the pool kernel counts in HAC_ENC_CLASS_LN);
 * hac_encoder_last_plan appends " pool=mean"; hac_encoder_layer_state accepts the last layer, n_layers - 1, in this mode only.
 * A sequence the device flags is a NaN row in either mode.  Switching back to "first" restores the default path bit for bit.
 *
 * "model" = "roberta" (default) | "bert": which arm of the reference's load_model (src/models.py:112-136) the handle serves.
 * Accepted until the first hac_encoder_set_weight; afterwards, and with any other value, HAC_ERR_INVALID.  "bert" is the
 * reference's BERT class (src/models.py:66-110) over BertModel, base geometry: the tensors are "bert.embeddings.*" /
 * "bert.encoder.layer.N.*" (+ the same "embeddingHead.*", "norm.*"; "bert.pooler.*" and "classifier.*" are unused by forward:
 * do not pass them), and hac_encoder_finalize names the first tensor missing under the chosen model's names.  Position ids are
 * pos = t for every token, whatever its id ([PAD] = 0 inside a sequence is an ordinary token; pad_token_id is not read), so
 * the position table's max_pos rows serve L up to min(512, max_pos) -- "roberta" keeps HF's cumsum rule and its bound
 * min(512, max_pos - 2).  Row 0 of the token-type table (type_vocab = 2) is added, as the reference never passes
 * token_type_ids; ln_eps is the config's (1e-12).  The layer stack is the one kernel set in both models: every "gemm" family,
 * "precision", "pooling", "graph" (the model is part of a captured shape's key), "max_tokens" and hac_encoder_layer_state
 * work as described above.  hac_encoder_last_plan appends " model=bert" (nothing in "roberta"). */
int hac_encoder_set_option(hac_encoder *enc, const char *name, const char *value);
/* What the most recent forward ran: "gemm=gemm8|classic256|classic128 attn=stream|twopass sub_batches=N rows=R graph=off|eager-first|replay ksplit=S_out/S_down attn_form=woven|single|twopass"
 * (+ " precision=split", " pool=mean" and / or " model=bert" when the forward ran in those modes; tests and bench.py assert the kernel family they mean to check).  The GEMM family and, with the classic kernels, the tile
 * size are chosen once per call, from the rows of the whole batch: every sub-batch runs the same kernels. */
const char *hac_encoder_last_plan(hac_encoder *enc);

/* Profiling aid for bench.py: hipEvent pairs recorded on the launch stream (no host sync).  mask bit 0:
 * around the layer stack of each forward (sub-batch); bit 1+c: around every launch of kernel class c.
 * hac_encoder_profile_drain / _drain_class wait for the recorded pairs, write up to cap durations (ms, in
 * launch order) and clear the record. */
enum {
    /* kernels: large batches gemm8_kernel<EPI8_*> (gemm8.inc), small ones gemm_bf16_nt_kernel<EPI_*> */
    HAC_ENC_CLASS_QKV = 0,       /* <EPI8_QKV | EPI_QKV>:     [T,768] x [2304,768]^T (+ folded LayerNorm) + bias, Q scale, V regrouping */
    HAC_ENC_CLASS_ATTN = 1,      /* attention_stream_kernel<16|8> (both launches of a layer) */
    HAC_ENC_CLASS_OUTPROJ = 2,   /* <EPI8_RESID | EPI_RESID>: [T,768] x [768,768]^T + bias + residual (+ LayerNorm statistics) */
    HAC_ENC_CLASS_FFN_UP = 3,    /* <EPI8_GELU | EPI_GELU>:   [T,768] x [3072,768]^T (+ folded LayerNorm) + bias + erf GELU */
    HAC_ENC_CLASS_FFN_DOWN = 4,  /* <EPI8_RESID | EPI_RESID>: [T,3072] x [768,3072]^T + bias + residual (+ LayerNorm statistics) */
    HAC_ENC_CLASS_LN = 5,        /* LayerNorm passes that are their own kernel (ln_combine_kernel / ln_stats_rows_kernel; "pooling" = "mean": pool_mean_kernel too) */
    HAC_ENC_NCLASS = 6
};
int hac_encoder_set_profiling(hac_encoder *enc, int mask);
int hac_encoder_profile_drain(hac_encoder *enc, float *ms_out, int cap, int *n_out);
int hac_encoder_profile_drain_class(hac_encoder *enc, int cls, float *ms_out, int cap, int *n_out);
/* The shader clock the part sustained inside the most recent large-batch FFN-up launch made while class profiling was on:
 * workgroup 0 of gemm8_kernel<EPI8_GELU> reads the shader-clock counter (s_memtime) and the constant 100-MHz counter
 * (s_memrealtime) at its first and last instruction (same CU both times: the counters of different XCDs are not aligned).
 * out[0] = shader clocks, out[1] = 100-MHz ticks between the two readings (0, 0 if no such launch happened); waits for the
 * stream of that launch.  clock = out[0] / out[1] x 100 MHz -- the figure fractions of a peak are normalised by, because boxes
 * of one pool hold different clocks under the same load.  Costs the kernel nothing (two scalar reads, four stores). */
int hac_encoder_last_clock(hac_encoder *enc, uint64_t out[2]);
/* Test aid: how often the woven attention kernel (attn_pipe.inc) handed an item to the fix-up pass in the most recent forward
 * (last sub-batch) -- a wave counts its item when one of its rows left the window in which a row's softmax reference stays 0
 * (a score above 2^63 relative to 1, or a first key block wholly below 2^-64); several waves of one item may count it: an upper
 * bound of the items, 0 iff none.  Waits for the device.  The results do not depend on it: the fix-up pass is the one-block
 * kernel, whose outputs the woven kernel's equal bit for bit wherever it does not flag. */
int hac_encoder_attention_redo(hac_encoder *enc, long long *items_out);
/* Test entry point: the residual stream after encoder layer `layer` (-1: the embedding LayerNorm; at most n_layers - 2, the last
 * layer continues the <s> rows only -- except with "pooling" = "mean", where the last layer, n_layers - 1, is a layer like the
 * others and its state is what pool_mean_kernel reads).  Runs the launches of a forward of (ids, mask) -- same routing, options and workspaces,
 * never captured into a graph -- up to that layer, then unpacks every valid row t < len of sequence b to index b * L + t:
 *   rows_out  float32 [B][L][768]: the rows as stored, BEFORE that layer's output LayerNorm (the classic kernels keep them in
 *             fp32, the large-batch gemm8 path in bf16; layer -1: the normalized embedding rows);
 *   stats_out float32 [B][L][2]: their (mean, rstd) as the next layer reads them ((0, 1) for layer -1);
 *   norm_out  float32 [B][L][768] or NULL: (row - mean) * rstd * gamma + beta in fp32, the normalized rows the next layer's
 *             residual add forms (layer -1: the rows themselves).
 * Rows t >= len are zeros (statistics (0, 0)).  ids, mask: host int32 [B, L] as for hac_encoder_forward; B * roundup(L, 32) must
 * fit one pass ("max_tokens").  Synchronous; waits for the encoder's stream.  Not for the timed path. */
int hac_encoder_layer_state(hac_encoder *enc, const int32_t *ids, const int32_t *mask, int B, int L, int layer, float *rows_out,
                            float *stats_out, float *norm_out);

#ifdef __cplusplus
}
#endif
#endif /* HACONVDR_H */
