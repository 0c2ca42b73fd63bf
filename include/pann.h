/*
 * pann.h -- C-ABI of the MI355X-native graph-ANN hot path (beam search, robustPrune,
 * batched / all-pairs distances) that replaces, for this path only, ParlayANN's
 *
 *   algorithms/utils/beamSearch.h:22-214   filtered_beam_search           -> pann_batch_search*
 *   algorithms/utils/beamSearch.h:353-387  searchAll   (parallel_for seam) -> pann_batch_search*
 *   algorithms/utils/beamSearch.h:537-565  qsearchAll  (parallel_for seam) -> pann_batch_search*
 *   algorithms/utils/beamSearch.h:499-521  beam_search_rerank__ (build)    -> pann_batch_search* with
 *                                          query_ids != NULL and a visited-list output
 *   algorithms/utils/euclidian_point.h:54-90, mips_point.h:43-65           -> device distance functors
 *   algorithms/vamana/index.h:63-137       knn_index::robustPrune          -> pann_robust_prune_batch
 *   algorithms/vamana/index.h:247-266      batch_insert step 1 (search+prune per inserted point)
 *                                                                          -> pann_insert_batch
 *   algorithms/HCNNG/hcnng_index.h:145-181 MSTk all-pairs + per-row 10-NN  -> pann_leaf_knn
 *   data_tools/compute_groundtruth.cpp:22-59 brute-force kNN               -> pann_bruteforce_knn
 *   data_tools/compute_range_groundtruth.cpp:13-29 brute-force radius join -> pann_bruteforce_range
 *   algorithms/utils/beamSearch.h:567-614  RangeSearch (beam search + BFS)  -> pann_range_query
 *   algorithms/utils/beamSearch.h:390-454  beam_search_rerank (quantised)   -> pann_batch_search_rerank*
 *
 * The reference has no FFI of its own for this path (it is a header-only template library); these
 * entry points are what a cgo/ctypes/pybind binding placed at the parallel_for seams above would
 * bind.  INTEGRATION.md shows the reference-side stubs.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - every function returns an int status (PANN_OK == 0); pann_last_error() gives the text for the
 *     calling thread.  The reference prints and abort()s (beamSearch.h:38-41,368-372); host wrappers
 *     reproduce that on a non-zero status.
 *   - "host" entry points take host pointers and stage through the handle's device buffers;
 *     "_dev" entry points take device pointers (HIP) and a hipStream_t passed as void*, perform no
 *     allocation and no synchronisation, and are what bench.py times.
 *   - graph rows on the HOST side use the reference layout (graph.h:134-141,234-242):
 *     n x (max_deg+1) uint32, slot 0 = degree.  The device mirror is private to the handle.
 */
#ifndef PANN_H_
#define PANN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PANN_ABI_VERSION 3

/* status codes */
#define PANN_OK 0
#define PANN_ERR_BAD_ARG 1
#define PANN_ERR_HIP 2
#define PANN_ERR_NO_DEVICE 3
#define PANN_ERR_UNSUPPORTED 4
#define PANN_ERR_OVERFLOW 5 /* a per-query device buffer (visited list) was too small */

/* element type of the stored vectors (reference: Euclidian_Point<T>/Mips_Point<T>, T in
 * {uint8_t,int8_t,float}; PANN_F16 (IEEE binary16) and PANN_BF16 (bfloat16) are this build's two-byte
 * extensions: values are widened exactly to f32, arithmetic is f32).
 *
 * Four-bit types (DESIGN.md "Four-bit rows"): two coordinates per byte, packed as Quantized_Mips_Point<4>::assign packs them
 * (mips_point.h:399-406): a row is ceil(d / 2) bytes, coordinate j sits in byte j / 2, low nibble for even j; for odd d the
 * high nibble of the last byte must be zero (translate writes it so; rows and queries that are uploaded must keep it so).
 *   PANN_U4  unsigned nibbles 0..15, PANN_L2 only: the distance is sum (a - q)^2 on the nibble values -- the 4-bit analogue
 *            of Euclidian_Point<uint8_t>, this build's extension
 *   PANN_I4  two's-complement nibbles -8..7, PANN_MIPS only: Quantized_Mips_Point<4, trim>.  The distance is what distance_4
 *            (mips_point.h:342-354) returns as written -- its `<< 4` and `& 240` leave each factor scaled by 16 --, i.e.
 *            -256 * sum a * q, over ALL d coordinates (the reference's loops stop at dims / 2 bytes and so drop the last
 *            coordinate of an odd d)
 * Any other pairing is refused by pann_index_create* with PANN_ERR_UNSUPPORTED.  A 4-bit handle is searched
 * (pann_batch_search*, as `quant` of pann_batch_search_rerank*), measured (pann_pair_distances, pann_query_distances), and has
 * its points and graph moved (upload / download / set_graph / update_rows / get_graph); it gets its graph from
 * pann_index_create_quantized(copy_graph) or pann_index_set_graph.  Every entry point that builds, prunes, ranges, reranks ON
 * it, filters through a sketch or runs a dense all-pairs pass returns PANN_ERR_UNSUPPORTED before anything is launched,
 * allocated or written. */
typedef enum { PANN_U8 = 0, PANN_I8 = 1, PANN_F32 = 2, PANN_F16 = 3, PANN_BF16 = 4, PANN_U4 = 5, PANN_I4 = 6 } pann_dtype;

/* distance functor: euclidian_point.h:54-90 / mips_point.h:43-65 */
typedef enum { PANN_L2 = 0, PANN_MIPS = 1 } pann_metric;

/* field-for-field mirror of QueryParams (algorithms/utils/types.h:218-231) */
typedef struct pann_query_params {
  int64_t k;            /* QueryParams::k            (0 during build: no cut-prune) */
  int64_t beam;         /* QueryParams::beamSize */
  double cut;           /* QueryParams::cut */
  int64_t limit;        /* QueryParams::limit        (max number of visited vertices) */
  int64_t degree_limit; /* QueryParams::degree_limit */
  int32_t rerank_factor;/* QueryParams::rerank_factor (used by the rerank wrapper only) */
  float pad;            /* QueryParams::pad */
} pann_query_params;

/* Outputs of one batched search.  Any pointer may be NULL (that output is skipped).
 * ids/dists rows hold the first min(out_k, frontier size) entries of the final frontier, sorted
 * by (dist, id) (beamSearch.h:46-48,211); unused slots are 0xFFFFFFFF / +inf.
 * visited_ids/visited_dists hold the visited list (beamSearch.h:112-113) in VISIT order, at most
 * visited_cap entries per query (the reference keeps it sorted by (dist,id); callers that need
 * that order sort the row, robustPrune sorts its candidates anyway, vamana/index.h:83). */
typedef struct pann_search_out {
  uint32_t* ids;           /* nq x out_k */
  float* dists;            /* nq x out_k */
  uint32_t out_k;
  uint32_t* frontier_size; /* nq */
  uint32_t* visited_count; /* nq : visitedElts.size()  (stats.h:70-73 increment_visited) */
  uint32_t* dist_cmps;     /* nq : full_dist_cmps      (beamSearch.h:213) */
  uint32_t* degree_sum;    /* nq : sum over visited v of min(deg(v), degree_limit) -- roofline numerator */
  uint32_t* visited_ids;   /* nq x visited_cap */
  float* visited_dists;    /* nq x visited_cap */
  uint32_t visited_cap;
  uint32_t* status;        /* 1 word, optional: PANN_STATUS_* bits of this launch.  pann_batch_search_dev copies the
                              kernel's status word here on the launch stream (device pointer; read it after the stream
                              has been synchronised); the host entry points write it before returning. */
} pann_search_out;

/* bits of pann_search_out::status */
#define PANN_STATUS_VISITED_OVERFLOW 1u /* a visited list was longer than visited_cap: the lists are truncated */
#define PANN_STATUS_DROPPED_OVERFLOW 2u /* the per-query "dropped" scratch (equivalence 2) was too small:
                                           results of this launch are NOT valid.  The host entry points grow the scratch
                                           and run the batch again by themselves; after a _dev launch that reports it,
                                           call pann_index_reserve_dropped() with a larger capacity and launch again. */
#define PANN_STATUS_SHORT_FRONTIER 4u   /* pann_batch_search_rerank*: some query's frontier held fewer than k entries
                                           (beamSearch.h:416-419); its row is padded with 0xFFFFFFFF / +inf */
#define PANN_STATUS_BAD_GROUP 8u        /* pann_batch_search_grouped_labeled_dev: some query's table index was >= npreds; its row
                                           is padding and its result_count 0, the other queries' rows are valid */

typedef struct pann_index pann_index;

/* ---- library ------------------------------------------------------------------------------- */
int pann_abi_version(void);
const char* pann_last_error(void);
int pann_device_count(void);

/* ---- index handle: device mirror of PointRange (point_range.h:42-141) + Graph (graph.h:125-250) */

/* points: host slab, n rows of d elements, row stride row_stride_bytes (PointRange::aligned_bytes,
 * point_range.h:94).  graph: host n x (max_deg+1) uint32 in the reference layout, or NULL for an
 * empty graph (all degrees 0, as Graph(maxDeg,n) gives, graph.h:145-147). */
int pann_index_create(pann_index** out, const void* points, uint64_t n, uint32_t d, int dtype,
                      uint64_t row_stride_bytes, int metric, const uint32_t* graph,
                      uint32_t max_deg, int device);
/* Streaming form of the same (the reference's loaders read a whole file into host memory first --
 * point_range.h:74-117, graph.h:147-232; a shard of a 100M-point file need not exist on the host at once): an index of n zero
 * points and an empty graph, then any number of row ranges.  rows: nrows x d elements with row stride row_stride_bytes; the
 * range [first_row, first_row + nrows) must lie inside the index.  Graph rows stream through pann_index_update_rows. */
int pann_index_create_empty(pann_index** out, uint64_t n, uint32_t d, int dtype, int metric, uint32_t max_deg, int device);
int pann_index_upload_points(pann_index* idx, uint64_t first_row, const void* rows, uint64_t nrows, uint64_t row_stride_bytes);
void pann_index_destroy(pann_index* idx);

uint64_t pann_index_size(const pann_index* idx);
uint32_t pann_index_dims(const pann_index* idx);
uint32_t pann_index_max_degree(const pann_index* idx);
int pann_index_device(const pann_index* idx);

/* Validation mode for float element types (f32, f16): every distance is summed strictly left to right
 * with one rounding per subtract / multiply / add, as the reference's scalar loops do
 * (euclidian_point.h:83-90, mips_point.h:59-65), so results on REAL-valued data are bit-identical to
 * the CPU path (one lane per candidate: several times slower).  No effect on integer types. */
int pann_index_set_exact_float_order(pann_index* idx, int on);

/* Capacity (entries per query) of the scratch list that remembers visited vertices which the cut-prune
 * (beamSearch.h:190-195) dropped from a frontier that is not yet full; default 256.  Only searches with k > 0 on a
 * metric index that visit more than `cap` vertices before the frontier fills can exceed it (e.g. cut = 1.0 on a
 * path-like graph).  Never shrinks. */
int pann_index_reserve_dropped(pann_index* idx, uint32_t cap);
uint32_t pann_index_dropped_capacity(const pann_index* idx);

/* Replace the whole graph from a host n x (max_deg+1) slab.  Neighbour ids >= n are rejected with
 * PANN_ERR_BAD_ARG (the offending rows are left empty): the kernels gather points[id] unchecked. */
int pann_index_set_graph(pann_index* idx, const uint32_t* graph);
/* Replace m rows: rows is m x (max_deg+1) in the reference layout (edgeRange::update_neighbors,
 * graph.h:84-99).  Must not overlap a search on the same handle (vamana/index.h:247-270). */
int pann_index_update_rows(pann_index* idx, const uint32_t* row_ids, const uint32_t* rows,
                           uint64_t m);
/* Empty graph again (all degrees 0, as Graph(maxDeg, n) gives, graph.h:145-147) without a host slab: one fill on the handle's
 * stream.  A rebuild of the same points (bench.py's build modes) starts from it. */
int pann_index_clear_graph(pann_index* idx);
/* Copy the device graph back to a host n x (max_deg+1) slab. */
int pann_index_get_graph(pann_index* idx, uint32_t* graph_out);

/* ---- batched beam search (beamSearch.h:22-214 run for nq queries at once) -------------------- */

/* queries: nq rows of d elements of the index dtype, row stride q_stride_bytes; OR query_ids:
 * nq base-point ids (the query is Points[id] and neighbours equal to id are skipped, the
 * `Points[a].same_as(p)` test of beamSearch.h:133).  Exactly one of the two is non-NULL.
 * starts: nstarts start vertices shared by all queries (all in-scope drivers pass {0}:
 * vamana/index.h:148, check_nn_recall.h:178). */
int pann_batch_search(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                      uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts,
                      const pann_query_params* qp, const pann_search_out* out);

/* Same, all pointers are device pointers; launched on `stream` (hipStream_t); no sync, no alloc
 * except growth of the handle's private workspace on first use (call once to warm up). */
int pann_batch_search_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids,
                          uint64_t nq, uint64_t q_stride_bytes, const uint32_t* d_starts,
                          uint32_t nstarts, const pann_query_params* qp,
                          const pann_search_out* d_out, void* stream);

/* beamSearchRandom (beamSearch.h:309-351): like pann_batch_search, but every query has its OWN start
 * vertices: starts is nq x nstarts.  (The reference draws one random start per query from
 * parlay::random_generator; the caller supplies the draws here.)  Host pointers. */
int pann_batch_search_per_query_starts(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                                       uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts,
                                       const pann_query_params* qp, const pann_search_out* out);

/* ---- distances ------------------------------------------------------------------------------ */

/* out[i] = distance(Points[a_ids[i]], Points[b_ids[i]]), i < m  (Point::distance). host pointers */
int pann_pair_distances(pann_index* idx, const uint32_t* a_ids, const uint32_t* b_ids, uint64_t m,
                        float* out);
/* out[q*m + j] = distance(query q, Points[ids[j]])  for nq external queries. host pointers */
int pann_query_distances(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes,
                         const uint32_t* ids, uint64_t m, float* out);

/* Re-scoring of beam_search_rerank (beamSearch.h:426-452): for query i the first cand_counts[i]
 * (or c when cand_counts is NULL) ids of row i of cand_ids (nq x c) get their exact distance to
 * query i.  resort != 0: sort by (dist,id) and keep k (:437-442); resort == 0: keep the first k in
 * the given order (:447-452).  Unused output slots are 0xFFFFFFFF / +inf.  Host pointers. */
int pann_rerank(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes,
                const uint32_t* cand_ids, uint32_t c, const uint32_t* cand_counts, uint32_t k, int resort,
                uint32_t* out_ids, float* out_dists);

/* ---- robustPrune (vamana/index.h:63-137) ---------------------------------------------------- */

/* For each of m owners p_i: candidates = given list (ids, and dists to p_i; if cand_dists is NULL
 * they are computed as in the id-only overload :124-137) plus, when add_out_nbrs != 0, p_i's current
 * out-neighbours (:72-77); sort by (dist,id), unique by id, greedy alpha-prune to at most R.
 * cand_offsets has m+1 entries (CSR).  out_rows is m x (R+1) in the reference row layout
 * (slot 0 = count).  out_dist_cmps (optional) gets distance_comps per owner.  Host pointers. */
int pann_robust_prune_batch(pann_index* idx, const uint32_t* owners, uint64_t m,
                            const uint32_t* cand_ids, const float* cand_dists,
                            const uint64_t* cand_offsets, double alpha, uint32_t R,
                            int add_out_nbrs, uint32_t* out_rows, uint32_t* out_dist_cmps);

/* ---- Vamana batch_insert (vamana/index.h:188-316) ------------------------------------------- */

typedef struct pann_build_stats {
  double t_search_s, t_prune_s, t_bidirect_s, t_reprune_s; /* the reference's three phase timers, :217-222 */
  uint64_t search_dist_cmps, prune_dist_cmps, visited_total;
  /* optional host arrays of n entries each (NULL: skipped), ACCUMULATED like the reference's BuildStats
   * (stats.h:63-73): per inserted point its |visited| (vamana/index.h:262) and its beam-search + robustPrune
   * comparisons (:261,266); a re-pruned reverse-edge target gets that prune's comparisons (:298) */
  uint32_t* per_point_visited;
  uint32_t* per_point_dist_cmps;
} pann_build_stats;

/* One batch: for every id in batch_ids (m of them) beam-search from `start` with
 * QueryParams(0, L, 0.0, n, max_deg) (:250), robustPrune the visited list (:264), write the rows
 * (:268-270), then add the reverse edges: append-without-repeats when the row stays within R,
 * otherwise re-prune (:278-300).  The graph inside the handle is updated in place. */
int pann_vamana_insert_batch(pann_index* idx, const uint32_t* batch_ids, uint64_t m, uint32_t start,
                             uint32_t R, uint32_t L, double alpha, pann_build_stats* stats);

/* Whole build_index (vamana/index.h:150-186): num_passes passes of prefix-doubling batches over a
 * seeded random permutation (this build's own permutation), alpha = 1.0 on all but
 * the last pass, optional final neighbour sort by distance. */
int pann_vamana_build(pann_index* idx, uint32_t R, uint32_t L, double alpha, int num_passes,
                      uint64_t seed, int sort_neighbors, pann_build_stats* stats);

/* build_index with BP.single_batch = degree != 0 (vamana/index.h:156-170,236-240): every vertex first gets `degree` random
 * out-edges, then each pass inserts ALL points as one batch.  The reference draws the edges from parlay::random_generator over
 * [0, n] (n itself is out of range there); this build draws splitmix64(seed, i * degree + j) mod n. */
int pann_vamana_build_single_batch(pann_index* idx, uint32_t R, uint32_t L, double alpha, int num_passes, uint32_t degree,
                                   uint64_t seed, int sort_neighbors, pann_build_stats* stats);

/* The two phases of one batch on DEVICE pointers -- the seam of the multi-GPU build (SURVEY.md section 8e row 3;
 * parlayann_amd/distributed.py): with the points and the graph replicated, every rank runs phase A on its slice of the
 * batch, the slices' rows are all-gathered (ONE collective per batch, m x R x 4 bytes), and every rank applies the rows of
 * the whole batch with phase B, which is a deterministic function of (graph, batch ids, rows): all replicas stay identical
 * and equal to the single-GPU build.  Both calls run on the handle's stream and return after it has drained.
 *   A: beam search from `start` + robustPrune of the visited list (vamana/index.h:247-266) for the m ids given; reads the
 *      graph only.  d_rows_out: m x R uint32, unused slots 0xFFFFFFFF.
 *   B: write the rows (:268-270), reverse edges grouped by target, append-or-re-prune (:278-300).
 * Ids held in device memory are NOT validated (unlike pann_vamana_insert_batch, which checks its host ids, and unlike
 * pann_vamana_delete_batch_dev, which checks its ids on the device): every d_batch_ids[i], and every word of d_rows other than
 * 0xFFFFFFFF, must be < n -- the caller guarantees it; anything else indexes the points and the graph out of bounds.  The
 * scalar arguments are checked (PANN_ERR_BAD_ARG, nothing written): null pointers with m > 0, L outside [1, 65536], start >= n,
 * R outside [1, min(max_deg, 1024)].  m == 0 returns PANN_OK and touches nothing.  stats, when given, is accumulated into
 * (per-point arrays included): the calls of a split batch add up to what pann_vamana_insert_batch reports for the batch. */
int pann_vamana_search_prune_dev(pann_index* idx, const uint32_t* d_batch_ids, uint64_t m, uint32_t start, uint32_t R, uint32_t L,
                                 double alpha, uint32_t* d_rows_out, pann_build_stats* stats);
int pann_vamana_apply_rows_dev(pann_index* idx, const uint32_t* d_batch_ids, uint64_t m, const uint32_t* d_rows, uint32_t R,
                               double alpha, pann_build_stats* stats);
/* final neighbour sort of build_index (:180-185), ties by id */
int pann_vamana_sort_neighbors(pann_index* idx);
/* host-only helpers (no device needed), so that every rank derives the same schedule: the insertion order of this build
 * (Fisher-Yates driven by splitmix64(seed), DESIGN.md "Build determinism") and the prefix-doubling batch bounds of
 * batch_insert (:206-209, :223-234; base 2, max_fraction .02) for m inserts into a graph of n vertices: bounds gets
 * (floor, ceiling) pairs, at most cap of them; returns the number of batches. */
void pann_build_permutation(uint64_t n, uint64_t seed, uint32_t* out);
uint64_t pann_vamana_batch_schedule(uint64_t n, uint64_t m, uint64_t* bounds, uint64_t cap);

/* ---- deleting points: batched consolidation (DESIGN.md "Deleting points") -------------------- */

typedef struct pann_delete_stats {
  double t_expand_s, t_prune_s;           /* mark + count + fill ; keys + sort + greedy + row writes */
  uint64_t deleted, affected, candidates; /* |D| after de-duplication, |A|, total length of the candidate lists */
  uint64_t prune_dist_cmps;
  uint32_t* per_point_dist_cmps;          /* optional host array of n entries, ACCUMULATED like pann_build_stats */
} pann_delete_stats;

/* One batch of deletions.  The reference has none (knn_index::delete_set is never used); the rule is the delete consolidation
 * of FreshDiskANN (Singh et al. 2021, Algorithm 4) with the snapshot semantics of batch_insert.  With G the graph when the call
 * starts and D the ids given (duplicates mean nothing): every p not in D with an out-neighbour in D gets
 *   robustPrune(p, [N(p) \ D in row order] ++ [for v in N(p) & D in row order: N(v) \ D \ {p} in row order], alpha, R)
 * in the id-only form (distances computed and counted, add_out_nbrs = 0, (dist,id) ties: the rule and the distance_comps of
 * pann_robust_prune_batch(..., cand_dists = NULL, add_out_nbrs = 0)); all rows are read from G.  Then those rows are
 * replaced and the rows of D emptied; every other row and all points stay as they were (a freed slot keeps its vector until
 * pann_index_upload_points replaces it; pann_vamana_insert_batch then inserts it again).  Afterwards no row holds an id of D,
 * so a search cannot return one -- PROVIDED IT STARTS FROM A LIVE VERTEX: neither call takes or repairs a start vertex, the
 * caller must search (and insert) from a vertex it has not deleted.
 * An id >= n, R == 0 or R > max_deg: PANN_ERR_BAD_ARG, nothing written.  m == 0: PANN_OK, nothing changed.  All fields of
 * stats are added to.  The _dev form takes ids in device memory, checks them on the device, and runs on the handle's stream;
 * both return after the stream has drained. */
int pann_vamana_delete_batch(pann_index* idx, const uint32_t* del_ids, uint64_t m, uint32_t R, double alpha,
                             pann_delete_stats* stats);
int pann_vamana_delete_batch_dev(pann_index* idx, const uint32_t* d_del_ids, uint64_t m, uint32_t R, double alpha,
                                 pann_delete_stats* stats);

/* ---- dense all-pairs: HCNNG leaf (hcnng_index.h:145-181) and ground truth ------------------- */

/* For one leaf given by N ids: for each i the m smallest (dist,id) neighbours among the other
 * leaf members.  out_ids/out_dists are N x m (row i sorted ascending).  Host pointers. */
int pann_leaf_knn(pann_index* idx, const uint32_t* ids, uint32_t N, uint32_t m, uint32_t* out_ids,
                  float* out_dists);
/* Many leaves in one call: leaf_offsets has nleaves+1 entries into ids; outputs are
 * (total ids) x m. */
int pann_leaf_knn_batch(pann_index* idx, const uint32_t* ids, const uint64_t* leaf_offsets,
                        uint64_t nleaves, uint32_t m, uint32_t* out_ids, float* out_dists);

/* HCNNG cluster-tree split (clusterEdge.h:66-83): ids is the concatenation of nseg clusters
 * (seg_offsets, nseg+1 entries); cluster s has pivots pivot_a[s], pivot_b[s];
 * out_side[i] = 0 when d(ids[i], pivot_a) <= d(ids[i], pivot_b), else 1.  Host pointers. */
int pann_pivot_split(pann_index* idx, const uint32_t* ids, const uint64_t* seg_offsets, uint64_t nseg,
                     const uint32_t* pivot_a, const uint32_t* pivot_b, uint8_t* out_side);

/* BFS range search -- range_search (algorithms/utils/beamSearch.h:245-306; caller vamana/neighbors.h:88-101).
 * Per query: every start that is not the query's own vertex and lies within radius_2 seeds `result`
 * (:271-277); then result[position++] is expanded breadth first: neighbours not yet seen (an EXACT set,
 * :256) and not the query's own vertex are remembered, cost one distance comparison each and join `result`
 * iff dist <= radius_2 (:280-297).  Exactly one of queries / query_ids is given (a base-point query skips
 * its own vertex, Point::same_as).  starts is nstarts ids (shared) or nq x nstarts (starts_per_query != 0);
 * 0xFFFFFFFF entries are padding.  out_ids is nq x max_results in BFS order, out_counts[i] <= max_results (entries of a
 * row past its count are unspecified);
 * a query whose result would exceed max_results stops there and sets out_truncated[i] = 1.
 * out_dist_cmps / out_truncated may be NULL.  (The reference's first radius argument is unused, :250.) */
int pann_range_search(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                      uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, int starts_per_query,
                      float radius_2, uint32_t max_results, uint32_t* out_ids, uint32_t* out_counts,
                      uint32_t* out_dist_cmps, uint32_t* out_truncated);

/* Whole HCNNG build_index (hcnng_index.h:273-281) on the device: for each of num_clusters trees the
 * random two-pivot cluster tree (clusterEdge.h:99-144; level-synchronous: split kernel, prefix scan,
 * stable scatter), the all-pairs 10-NN of every leaf (hcnng_index.h:145-181), the per-leaf
 * de-duplicated, degree-bounded Kruskal (:183-228) and process_edges (:117-131).  Edges are appended to
 * the handle's graph (max_deg must be >= num_clusters * mst_deg, types.h:210-214).  Seeding rules as in
 * DESIGN.md "Build determinism".  times3 (optional): seconds spent in {tree, leaf kNN, MST}. */
int pann_hcnng_build(pann_index* idx, uint32_t num_clusters, uint32_t cluster_size, uint32_t mst_deg,
                     uint64_t seed, double* times3);
/* The stream the handle's calls run on (default: a private non-blocking stream).  A caller that produces the inputs of the
 * _dev phases on its own stream (torch's current stream: the all-gathered rows of the multi-GPU build) passes that stream here
 * once; work is then ordered by the stream and needs no synchronisation between the caller's kernels / collectives and the
 * library's.  use_private != 0: back to the private stream (stream is ignored); otherwise `stream` is used as given -- NULL is
 * the device's default stream, which is what torch's current stream usually is.  The stream must outlive its use by the handle. */
int pann_index_set_stream(pann_index* idx, void* stream, int use_private);

/* Per-handle tuning knobs; results never depend on them (0 = the library's own choice).  Unknown names: PANN_ERR_BAD_ARG.
 *   "forest_group": HCNNG -- the independent cluster trees (clusterEdge.h:146-153) are split level by level in groups of this
 *                   many trees (scratch: trees x n positions; default: as many as 2^31 positions allow)
 *   "gt_pieces"   : pann_bruteforce_knn, pann_bruteforce_range -- the base is cut into this many pieces per 64-query tile (default: the count that
 *                   fills whole rounds of the 256 CUs best)
 *   "locality_order": 1 (default) / 0 -- on tables beyond the Infinity Cache (> 1 GB of points) the Vamana builder launches the
 *                   searches of a batch ordered by the locality cell of the inserted point (nearest of 256 pivots, one pass per
 *                   handle); the graph does not depend on the launch order.  2: also on small tables and batches (tests)
 *   "filter_codes": 1 (default) / 0 -- the Vamana builder's L = 91..128 searches keep the lossy filter (beamSearch.h:52-59) as
 *                   12-bit class codes in LDS when every slot class has fewer than 4 095 members (n below ~16M), else as ids */
int pann_index_set_option(pann_index* idx, const char* name, int64_t value);
/* the current value; for "filter_codes": 1 while the class codes are in step with the graph (the next beam-91..128 search uses
 * them), 0 otherwise; -1: unknown name */
int64_t pann_index_get_option(const pann_index* idx, const char* name);

/* Sharded index: nlists result lists per query -- the output of ONE all-gather of every shard's
 * top-k -- laid out [nlists][nq][row_stride]: row (w, q) holds k_in ids at d_ids and k_in distances at d_dists (0xFFFFFFFF =
 * unused slot).  Two separate arrays: row_stride = k_in.  One packed array of [ids | distance bits] rows (what
 * parlayann_amd.distributed gathers): row_stride = 2 * k_in, d_dists = (float*)(d_ids + k_in).  d_list_base (optional, nlists
 * words): list w holds ids LOCAL to shard w and gets d_list_base[w] added; NULL: the ids are global.  out = per query the k_out
 * smallest under (dist, id) (beamSearch.h:46-48).  Device pointers, launched on `stream` of the current device, no
 * synchronisation. */
int pann_merge_topk_dev(const uint32_t* d_ids, const float* d_dists, uint32_t nlists, uint64_t nq, uint32_t k_in,
                        uint32_t row_stride, const uint32_t* d_list_base, uint32_t k_out, uint32_t* d_out_ids, float* d_out_dists,
                        void* stream);

/* HCNNG with the TREES split over GPUs (the cluster trees are independent,
 * clusterEdge.h:146-153): every rank holds all points; rank r builds trees r, r + W, r + 2W, ... of the forest that
 * pann_hcnng_build(seed) builds (same per-tree seeds) into a device slab, the slabs are all-gathered (ONE collective) and
 * every rank interleaves them in tree order: the graph of the single-GPU build, bit for bit.
 *   build_trees: trees first_tree, first_tree + tree_step, ... (ntrees of them); tree j of the call writes vertex v's edges
 *     (at most mst_deg, hcnng_index.h:213) into slots [j*mst_deg, (j+1)*mst_deg) of row v of d_slab (device, n rows of
 *     slab_stride uint32, 0xFFFFFFFF = empty; filled here).  The handle's own graph is not touched.
 *   assemble: d_slabs = nslabs slabs one after the other (the all-gather's output); slab w holds trees w, w + nslabs, ...;
 *     row v of the handle's graph gets, after its current neighbours, the edges of trees 0 .. ntrees-1 in tree order; a row
 *     takes edges while it has room and stops at max_deg (process_edges, hcnng_index.h:121-124).
 * The words of d_slabs are not validated either: every one other than 0xFFFFFFFF must be an id < n (what build_trees wrote).
 * Checked, PANN_ERR_BAD_ARG and nothing written: a null slab, mst_deg == 0, tree_step == 0; for assemble also nslabs == 0, slab
 * rows shorter than ceil(ntrees / nslabs) * mst_deg, and ntrees * mst_deg > max_deg.  build_trees refuses slab rows shorter
 * than ntrees * mst_deg and a cluster_size outside [2, 65535] too, but only after it has filled the slab with 0xFFFFFFFF. */
int pann_hcnng_build_trees_dev(pann_index* idx, uint32_t first_tree, uint32_t tree_step, uint32_t ntrees, uint32_t cluster_size,
                               uint32_t mst_deg, uint64_t seed, uint32_t* d_slab, uint32_t slab_stride, double* times3);
int pann_hcnng_assemble_dev(pann_index* idx, const uint32_t* d_slabs, uint32_t nslabs, uint32_t slab_stride, uint32_t ntrees,
                            uint32_t mst_deg);

/* Brute-force k nearest base points for nq external queries (compute_groundtruth.cpp:22-59):
 * out rows sorted by (dist,id). Host pointers. */
int pann_bruteforce_knn(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes,
                        uint32_t k, uint32_t* out_ids, float* out_dists);

/* compute_range_groundtruth (data_tools/compute_range_groundtruth.cpp:13-29): for each of nq external queries every base
 * point with distance <= radius (the handle's distance: PANN_L2, or PANN_MIPS = -q.x, where the radius may be negative; == is
 * inside), as CSR: ids of query i are out_ids[out_offsets[i] .. out_offsets[i + 1]), ascending, each once.  Host pointers.
 * out_offsets: nq + 1 entries, always written (out_offsets[nq] = number of matches).  out_ids == NULL: count only.  Otherwise
 * ids_capacity entries are available: fewer than out_offsets[nq] -> PANN_ERR_OVERFLOW, out_ids untouched, out_offsets valid.
 * Exact for the one-byte types and in exact-float-order mode; in default mode a float distance within its rounding bound of
 * the radius may fall on either side (DESIGN.md "Float summation order").  "gt_pieces" steers how the base is cut; results never
 * depend on it.  NaN radius, NULL queries / out_offsets, a stride shorter than a row -> PANN_ERR_BAD_ARG; nq == 0 -> PANN_OK. */
int pann_bruteforce_range(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, float radius,
                          uint64_t* out_offsets, uint32_t* out_ids, uint64_t ids_capacity);

/* RangeSearch (beamSearch.h:567-614) with its second round live: beam search with *qp from `starts` (shared), then the BFS of
 * range_search (:245-306) seeded PER QUERY with that query's final frontier (all of it, in frontier order), radius_2 =
 * radius.  Exactly one of queries / query_ids.  The queries go to the device once and the frontiers never leave it: results
 * equal pann_batch_search (out_k = beam) followed by pann_range_search (starts_per_query) on its ids.
 * out_ids: nq x max_results in BFS order; counts / truncated as pann_range_search; out_search_cmps / out_visited: the beam
 * search's dist_cmps / visited_count; out_range_cmps: the BFS's comparisons.  Any of the last four may be NULL. */
int pann_range_query(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                     uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                     float radius, uint32_t max_results, uint32_t* out_ids, uint32_t* out_counts,
                     uint32_t* out_search_cmps, uint32_t* out_visited, uint32_t* out_range_cmps,
                     uint32_t* out_truncated);

/* ---- scalar quantisation of a float index on the device --------------------------------------
 * The reference's translating PointRange constructor (point_range.h:54-72: generate_parameters + translate_point per row) and
 * Point::normalize, for the two one-byte quantisers the drivers use (-quantize_bits 8, -quantize_mode 1, python/graph_index.cpp):
 *   PANN_QUANT_EUCLID_U8  Euclidian_Point<uint8_t>      parameters euclidian_point.h:211-235, translate :182-209
 *   PANN_QUANT_MIPS_I8    Quantized_Mips_Point<8, trim> parameters mips_point.h:433-486,      translate :416-430
 * Results are bit-identical to those loops on finite inputs (std::round, products rounded before they are added, the norm
 * summed in double in index order).  Sources are f32 rows that are resident on the device: the callers in scope all hold the
 * full-precision slab there; a float file that is not resident is streamed through pann_quantize_rows by its owner.
 * Status: a source that is not f32 -> PANN_ERR_UNSUPPORTED; a kind that does not fit the metric (EUCLID_U8 <-> PANN_L2,
 * MIPS_I8 <-> PANN_MIPS), an unknown kind, n * d == 0, a stride smaller than a row or not a multiple of 4, NULL pointers
 * -> PANN_ERR_BAD_ARG.
 *
 * And their two four-bit forms, which give PANN_U4 / PANN_L2 and PANN_I4 / PANN_MIPS handles and packed rows of ceil(d / 2)
 * bytes (wherever "d bytes" is said of an output row below, read ceil(d / 2)):
 *   PANN_QUANT_EUCLID_U4  min / max as EUCLID_U8 finds them (running min / max that start at 0), WITHOUT the all-integers
 *                         substitution of euclidian_point.h:227-231 (a plain cast cannot fit 4 bits); slope = 15 / (max - min),
 *                         offset = (int32) round(min * slope); translate is :193-207 with range = 15:
 *                         r = (int64) round(x * slope) - offset, clamped to [0, 15] -- never the plain cast of :187-189.
 *                         Degenerate input (max == min, i.e. all zeros): as EUCLID_U8, slope = 15 / 0 = +inf and nothing is
 *                         special-cased; every translated value is then unspecified.
 *   PANN_QUANT_MIPS_I4    Quantized_Mips_Point<4, trim>: parameters exactly those of MIPS_I8 (mips_point.h:433-486, same trim
 *                         ranks); translate :416-430 with range = 15: scale = 7.0f / max_val, values below -max_val become -7,
 *                         above max_val +7, otherwise (int32) round(x * scale). */
enum { PANN_QUANT_EUCLID_U8 = 0, PANN_QUANT_MIPS_I8 = 1, PANN_QUANT_EUCLID_U4 = 2, PANN_QUANT_MIPS_I4 = 3 };
typedef struct pann_quant_params {
  int32_t kind;
  int32_t dims;
  float slope;            /* Euclidian_Point<uint8_t>::parameters (euclidian_point.h:100-110): 255 / (max - min) */
  int32_t offset;         /*   (int32) round(min * slope); slope == 1 && offset == 0: translate is a plain cast (:194) */
  float max_val;          /* Quantized_Mips_Point<8>::parameters (mips_point.h:395-403) */
  float min_seen, max_seen; /* the two values the reference prints ("scalar quantization: min value = ..., max value = ...") */
} pann_quant_params;

/* Point::normalize (mips_point.h:115-124, euclidian_point.h:150-158) for every row of an f32 handle, in place on the device. */
int pann_index_normalize(pann_index* idx);
/* generate_parameters over every coordinate of src (f32).  trim: Quantized_Mips_Point's template flag (the 1e-4 / 1 - 1e-4
 * order statistics instead of min / max; found exactly, by a radix select, without sorting); ignored for EUCLID_U8. */
int pann_quantize_params(pann_index* src, int kind, int trim, pann_quant_params* out);
/* The same over n rows of d floats at a device address (row stride stride_bytes), on `stream` of the current device.  Allocates
 * a few KB per device on first use and SYNCHRONISES the stream: a handful of words have to come back before the parameters can
 * be formed.  `out` is a host pointer. */
int pann_quantize_params_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride_bytes, int kind, int trim,
                             pann_quant_params* out, void* stream);
/* QPR Q_Points(Points) (vamana/neighbors.h:104-110, graph_index.cpp:90-99): a new handle of the same size, max_deg and device
 * whose points are src's rows translated on the device -- PANN_U8 / PANN_L2 or PANN_I8 / PANN_MIPS by p->kind.  copy_graph != 0:
 * src's graph is copied device to device; else the graph is empty.  Destroyed with pann_index_destroy like any handle. */
int pann_index_create_quantized(pann_index** out, pann_index* src, const pann_quant_params* p, int copy_graph);
/* QPR Q_Query_Points(Query_Points, Q_Points.params): n host rows of p->dims floats -> n rows of p->dims bytes at `out` (host).
 * normalize_first != 0: every row goes through Point::normalize first (the source is const: never in place).  Runs on device
 * `device`. */
int pann_quantize_rows(const pann_quant_params* p, const float* rows, uint64_t n, uint64_t stride_bytes, int normalize_first,
                       void* out, uint64_t out_stride_bytes, int device);
/* The same on device pointers, launched on `stream` of the current device; no allocation, no synchronisation.  Bytes
 * [p->dims, out_stride_bytes) of an output row are not written. */
int pann_quantize_rows_dev(const pann_quant_params* p, const float* d_rows, uint64_t n, uint64_t stride_bytes,
                           int normalize_first, void* d_out, uint64_t out_stride_bytes, void* stream);
/* Counterpart of pann_index_upload_points: rows [first_row, first_row + nrows) of the handle's points back to the host, d
 * elements of the handle's dtype per row, row stride out_stride_bytes. */
int pann_index_download_points(pann_index* idx, uint64_t first_row, uint64_t nrows, void* out, uint64_t out_stride_bytes);
/* host-only helper: the sorted positions generate_parameters reads for len = n * d values (mips_point.h:448-451):
 * a = (long)(.0001f * len) in float, b = (long)((1.0 - .0001f) * (len - 1)) in double; trim == 0: 0 and len - 1 */
void pann_quantize_select_ranks(uint64_t len, int trim, uint64_t* a, uint64_t* b);

/* ---- two-level search: bit sketches + filtered_beam_search(..., use_filtering = true) ---------
 * The reference's low-precision pre-filter (beamSearch.h:98-100,117-123,139-146): while the frontier is full, a neighbour that
 * passed the hash filter gets its full distance only if a cheap sketch distance to the query is below the running mean of the
 * sketch distance to the worst frontier entry.  Three of the reference's sketch point types, built on the device from a
 * resident f32 handle:
 *   PANN_SKETCH_EUCLID_BIT  Euclidean_Bit_Point (euclidian_point.h:332-420)  median = (long) sorted[n*d/2]; bit = x > (float) median
 *   PANN_SKETCH_MIPS_BIT    Mips_Bit_Point      (mips_point.h:625-702)       bit = x > 0
 *   PANN_SKETCH_MIPS_2BIT   Mips_2Bit_Point     (mips_point.h:495-623)       cut = max(sorted[b], -sorted[a]); per 64 dims a sign
 *                                                                            word and a non-zero-mask word
 * Host-visible sketch rows have the reference's num_bytes(): 8 * ceil(d / 64) bytes (one-bit kinds), 16 * ceil(d / 64) (2-bit:
 * word 2i = sign, word 2i + 1 = mask).  Bits the reference leaves uninitialised -- positions >= d, sign bits under a clear mask
 * bit, mask bits past the first position >= d -- are 0 here; distances never depend on them.
 * hamming_as_written (one-bit kinds; ignored for 2-bit): 0 = Hamming distance over all 64-bit blocks; 1 = the reference's loop
 * as written, which never advances its pointers (euclidian_point.h:360-361, mips_point.h:652-653): num_blocks * popcount of
 * block 0.  pann_sketch_params_generate sets 0.
 * Status: a source that is not f32, d > 2048 -> PANN_ERR_UNSUPPORTED; no sketch attached, n / d mismatch, a stride shorter than
 * a row (or not a multiple of 8 for sketch rows, 4 for float rows), NULL pointers, an unknown kind -> PANN_ERR_BAD_ARG. */
enum { PANN_SKETCH_EUCLID_BIT = 0, PANN_SKETCH_MIPS_BIT = 1, PANN_SKETCH_MIPS_2BIT = 2 };
#define PANN_SKETCH_MAX_DIMS 2048
typedef struct pann_sketch_params {
  int32_t kind;
  int32_t dims;
  int64_t median;              /* EUCLID_BIT */
  float cut;                   /* MIPS_2BIT */
  uint32_t hamming_as_written; /* one-bit kinds */
} pann_sketch_params;

/* generate_parameters over every coordinate of src (f32); the order statistics are found exactly by the radix select of
 * pann_quantize_params, nothing is sorted.  Synchronises src's stream. */
int pann_sketch_params_generate(pann_index* src, int kind, pann_sketch_params* out);
/* host-only helper: the sorted positions generate_parameters reads for len = n * d values.  EUCLID_BIT: a = b = len / 2;
 * MIPS_2BIT (mips_point.h:612-614): a = (long)(.3f * len) in float, b = (long)((1.0 - .3f) * (len - 1)) in double;
 * MIPS_BIT: none (a = b = 0). */
void pann_sketch_select_ranks(uint64_t len, int kind, uint64_t* a, uint64_t* b);
/* Sketch every row of src (f32, same n, d and device as idx; may be idx itself) with *p; the slab belongs to idx, is freed with
 * it, and replaces a sketch attached earlier.  idx is the handle that will be searched, of any element type. */
int pann_index_attach_sketch(pann_index* idx, pann_index* src, const pann_sketch_params* p);
/* The same from n host-layout sketch rows (row stride stride_bytes) that the caller already holds -- rows downloaded from
 * another handle, or a host PointRange of sketch points (parlayann_amd/host/sketch.h). */
int pann_index_upload_sketch(pann_index* idx, const pann_sketch_params* p, const void* rows, uint64_t stride_bytes);
int pann_index_drop_sketch(pann_index* idx);
int pann_index_sketch_kind(const pann_index* idx);      /* -1: no sketch attached */
/* rows [first_row, first_row + nrows) of the attached sketch, host layout, row stride out_stride_bytes */
int pann_index_download_sketch(pann_index* idx, uint64_t first_row, uint64_t nrows, void* out, uint64_t out_stride_bytes);
/* Sketches of n host rows of p->dims floats (the queries) -> n host-layout rows at `out`; runs on device `device`. */
int pann_sketch_rows(const pann_sketch_params* p, const float* rows, uint64_t n, uint64_t stride_bytes, void* out,
                     uint64_t out_stride_bytes, int device);
/* The same on device pointers (d_out and out_stride_bytes multiples of 8), on `stream` of the current device; no allocation, no
 * synchronisation. */
int pann_sketch_rows_dev(const pann_sketch_params* p, const float* d_rows, uint64_t n, uint64_t stride_bytes, void* d_out,
                         uint64_t out_stride_bytes, void* stream);

/* pann_batch_search with the sketch filter of the handle's attached sketch.  Exactly one of queries / query_ids is non-NULL.
 * With queries, sketch_queries is required: nq host-layout sketch rows (pann_sketch_rows), row stride sq_stride_bytes.  With
 * query_ids, sketch_queries must be NULL: the sketch query is the handle's own sketch row.
 * out->dist_cmps is the reference's full_dist_cmps (what it returns, beamSearch.h:213): starts + neighbours that got a full
 * distance.  out_pruned_cmps (optional, nq words) gets its local dist_cmps: starts + neighbours that passed the hash filter
 * (:83,137).  Every beam width runs the generic kernel.  The plain pann_batch_search* entries never look at the sketch. */
int pann_batch_search_filtered(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                               uint64_t q_stride_bytes, const void* sketch_queries, uint64_t sq_stride_bytes,
                               const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                               const pann_search_out* out, uint32_t* out_pruned_cmps);
/* Device pointers throughout, launched on `stream`; no sync, no alloc beyond the workspace growth of pann_batch_search_dev. */
int pann_batch_search_filtered_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                   uint64_t q_stride_bytes, const void* d_sketch_queries, uint64_t sq_stride_bytes,
                                   const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                   const pann_search_out* d_out, uint32_t* d_out_pruned_cmps, void* stream);

/* ---- quantised search + exact rerank in one call: beam_search_rerank (beamSearch.h:390-454) ----
 * full: the f32 handle; quant: its one-byte copy (pann_index_create_quantized(full, qparams, ...): same n, d, device and
 * metric).  Per batch of nq float query rows, all on the device and all on one stream:
 *   1. one kernel reads every query row once and writes its one-byte row (bit-identical to pann_quantize_rows_dev), with
 *      normalize_first the Point::normalize'd float row the rerank scores against, and with use_filter the sketch row
 *      (bit-identical to pann_sketch_rows_dev, parameters of the sketch attached to quant);
 *   2. the beam search of pann_batch_search_dev (use_filter: pann_batch_search_filtered_dev) on quant with *qp;
 *   3. the first num_check = min(qp->k * qp->rerank_factor, frontier size) (:428) frontier ids get their exact distance on
 *      `full` (the arithmetic of pann_rerank, exact-float-order flag included), are sorted by (dist, id), and k are kept.
 * Results equal pann_quantize_rows (+ pann_sketch_rows), pann_batch_search[_filtered] with out_k = beam and pann_rerank
 * (resort = 1) run one after the other, bit for bit.  A query whose frontier holds fewer than k entries writes what it has
 * and raises PANN_STATUS_SHORT_FRONTIER (the reference aborts there, :416-419; callers reproduce that).
 * Scratch (one-byte / sketch / normalised queries, frontiers) belongs to quant and grows on first use.
 * quant may also be a four-bit copy (PANN_U4 / PANN_I4, qparams of kind EUCLID_U4 / MIPS_I4): step 1 then writes packed nibble
 * rows, the contract is the same.  use_filter != 0 with a four-bit quant -> PANN_ERR_UNSUPPORTED. */
typedef struct pann_rerank_out {
  uint32_t* ids;            /* nq x k, sorted by (exact dist, id); unused slots 0xFFFFFFFF */
  float*    dists;          /* nq x k, exact distances on the full-precision handle; unused slots +inf */
  uint32_t* frontier_size;  /* nq, of the quantised search                      (optional) */
  uint32_t* visited_count;  /* nq                                               (optional) */
  uint32_t* dist_cmps;      /* nq, full_dist_cmps of the quantised search       (optional) */
  uint32_t* pruned_cmps;    /* nq, only with use_filter                         (optional) */
  uint32_t* status;         /* 1 word: PANN_STATUS_* bits of this call          (optional) */
} pann_rerank_out;

/* Device pointers throughout, launched on `stream`; no synchronisation, and no allocation once quant's scratch has reached
 * its size (call once to warm up).  d_out->status is written on the stream, as by pann_batch_search_dev.
 * Status: NULL handles / qparams / qp / out / ids / dists / queries / starts, k == 0, k > beam, nstarts == 0, handles that
 * differ in n, d, device or metric, a kind that does not fit quant's element type, use_filter without a sketch attached to
 * quant, a row stride shorter than a row or not a multiple of 4, beam > 4096 -> PANN_ERR_BAD_ARG; a `full` handle that is
 * not f32 -> PANN_ERR_UNSUPPORTED; nq == 0 -> PANN_OK.  Nothing is written on an error. */
int pann_batch_search_rerank_dev(pann_index* full, pann_index* quant, const pann_quant_params* qparams,
                                 const float* d_queries, uint64_t nq, uint64_t q_stride_bytes, int normalize_first,
                                 int use_filter, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                 const pann_rerank_out* d_out, void* stream);
/* Host pointers: queries and starts go up in one transfer, the outputs come back in one.  A launch that reports
 * PANN_STATUS_DROPPED_OVERFLOW is grown and run again as by pann_batch_search.  Runs on quant's stream. */
int pann_batch_search_rerank(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* queries,
                             uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter,
                             const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                             const pann_rerank_out* out);

/* ---- masked beam search: results restricted by an allow bitmap, traversal unchanged (DESIGN.md "Masked search") ----
 * allow: ceil(n / 32) uint32 words per row; point i is allowed iff bit (i & 31) of word (i >> 5) is set; bits at positions
 * >= n are ignored.  allow_stride_words == 0: one bitmap for the whole batch; >= ceil(n / 32): query q reads row q.
 * The search is pann_batch_search's, step for step: out->frontier_size, visited_count, dist_cmps, degree_sum and
 * visited_ids/dists are what pann_batch_search returns for the same arguments, whatever the bitmap holds.
 * out->ids/dists do NOT hold the head of the frontier: they hold, sorted by (dist, id), the min(out_k, count) best ALLOWED
 * points among all points whose full distance the search computed -- start points, neighbours at or beyond the cutoff and
 * candidates still unmerged at the end included, a point that was compared twice listed once.  Unused slots 0xFFFFFFFF / +inf.
 * out_result_count (optional, nq): entries of the query's list (<= out_k).  out_allowed_cmps (optional, nq): full distances
 * computed for allowed points, repeats counted -- a small value says that the mask starved the query.
 * Status: NULL bitmap, a stride between 1 and ceil(n / 32) - 1, out_k > beam -> PANN_ERR_BAD_ARG; out_k > 64 ->
 * PANN_ERR_UNSUPPORTED; everything else as pann_batch_search (a dropped-list overflow grows the list and repeats the batch).
 * Per-query rows are staged in one piece with the queries: nq * ceil(n / 32) * 4 bytes of pinned and of device memory (1.25 GB
 * for 10 000 queries at 1M points).  Callers with many per-query masks keep them on the device and use the _dev entry, or give
 * the points labels and send a predicate per query instead: 8 bytes each (pann_batch_search_labeled, below). */
int pann_batch_search_masked(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                             uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                             const uint32_t* allow, uint64_t allow_stride_words, const pann_search_out* out,
                             uint32_t* out_result_count, uint32_t* out_allowed_cmps);
/* Device pointers throughout, launched on `stream`; no sync, no alloc beyond the workspace growth of pann_batch_search_dev. */
int pann_batch_search_masked_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                 uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                 const uint32_t* d_allow, uint64_t allow_stride_words, const pann_search_out* d_out,
                                 uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, void* stream);

/* ---- masked search on the fused path: pann_batch_search_rerank with an allow bitmap (DESIGN.md "Masked search on the fused
 * path") ----  This project's own rule; the reference has no masks.  full: the f32 handle; quant: its one-byte or four-bit
 * copy; allow / allow_stride_words: the bitmap of pann_batch_search_masked (shared, or one row per query; bits at positions
 * >= n are ignored).
 *   1. The queries are quantised as by pann_batch_search_rerank (normalize_first: normalised first, and the normalised row is
 *      the one the rerank scores against).
 *   2. The masked search of pann_batch_search_masked_dev on quant with a result list of
 *      pool = min(qp->k * qp->rerank_factor, qp->beam, 64) entries (a rerank_factor below 1 counts as 1): per query the best
 *      min(pool, count) ALLOWED points by (quantised dist, id) among all points whose quantised distance the walk computed.  The
 *      walk is pann_batch_search's: out->frontier_size, visited_count and dist_cmps are what the plain quantised search (and
 *      pann_batch_search_rerank) returns for the same arguments, whatever the bitmap holds.
 *   3. num_check = result_count (<= pool): every list entry gets its exact distance on `full` (the arithmetic of pann_rerank,
 *      exact-float-order flag included), the entries are sorted by (exact dist, id), the first min(k, num_check) are written,
 *      the remaining slots hold 0xFFFFFFFF / +inf.
 * A short row is a legitimate answer under a mask: PANN_STATUS_SHORT_FRONTIER is NOT raised; read out_result_count.
 * out_result_count (optional, nq): length of the quantised list (<= pool).  out_allowed_cmps (optional, nq): as the masked search.
 * out->pruned_cmps is not written.  The result equals pann_quantize_rows, pann_batch_search_masked on quant with out_k = pool,
 * and pann_rerank on full with counts = result_count and resort = 1 run one after the other, bit for bit.
 * Device pointers throughout, launched on `stream`; no synchronisation, and no allocation once quant's scratch has reached
 * its size.
 * Status: k == 0, k > beam, a NULL bitmap, a stride between 1 and ceil(n / 32) - 1, and everything
 * pann_batch_search_rerank_dev rejects -> PANN_ERR_BAD_ARG; k > 64 (the list holds at most 64 keys), use_filter != 0 (there
 * is no sketch-filter x mask kernel), a `full` handle that is not f32 -> PANN_ERR_UNSUPPORTED; nq == 0 -> PANN_OK.  Nothing is
 * written on an error. */
int pann_batch_search_masked_rerank_dev(pann_index* full, pann_index* quant, const pann_quant_params* qparams,
                                        const float* d_queries, uint64_t nq, uint64_t q_stride_bytes, int normalize_first,
                                        int use_filter, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                        const uint32_t* d_allow, uint64_t allow_stride_words, const pann_rerank_out* d_out,
                                        uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, void* stream);
/* The same rule with host pointers: queries, starts and the bitmap rows (packed to ceil(n / 32) words each, as
 * pann_batch_search_masked stages them) go up in one transfer, all outputs come back in one.  A launch that reports
 * PANN_STATUS_DROPPED_OVERFLOW is grown and run again as by pann_batch_search.  Runs on quant's stream. */
int pann_batch_search_masked_rerank(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* queries,
                                    uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter,
                                    const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp, const uint32_t* allow,
                                    uint64_t allow_stride_words, const pann_rerank_out* out, uint32_t* out_result_count,
                                    uint32_t* out_allowed_cmps);

/* ---- exact kNN under an allow bitmap (DESIGN.md "Exact masked kNN") ----  This project's own; what a caller turns to when a mask
 * is so selective that the masked searches above see too few allowed points (out_allowed_cmps says so).  No graph is walked: the
 * allowed points are scored one by one.  allow / allow_stride_words: the bitmap of pann_batch_search_masked -- stride 0: one
 * bitmap for the whole batch; >= ceil(n / 32): query q reads row q; bits at positions >= n are ignored.
 * Row q of out_ids / out_dists holds the min(k, c_q) allowed points nearest to query q, sorted by (dist, id), c_q = the number of
 * allowed points; unused slots 0xFFFFFFFF / +inf.  out_counts (optional, nq): min(k, c_q).  A row with no allowed point is an
 * answer, not an error: all padding, count 0; an all-empty shared bitmap launches no distance kernel.
 * Exact wherever pann_bruteforce_knn is: the one-byte types, integer-valued floats, exact-float-order mode; in default float mode
 * the rounding caveat of DESIGN.md "Float summation order" applies.
 *   shared bitmap (stride 0), k <= 128: the bitmap is compacted on the device into the ascending list of allowed ids, and the
 *     dense kernels of pann_bruteforce_knn run over that list ("gt_pieces" is honoured).  The result equals pann_bruteforce_knn
 *     on an index made of the allowed rows in ascending id order, ids mapped back, bit for bit.
 *   per-query bitmaps, k <= 64: one wavefront per query walks its row.  Every returned distance equals, bit for bit and on any
 *     data, what pann_query_distances returns for the same (query, id) pair (the same arithmetic, exact-float-order flag included).
 * Status: NULL bitmap, queries or outputs, a stride between 1 and ceil(n / 32) - 1, a query stride shorter than a row, k == 0 ->
 * PANN_ERR_BAD_ARG; k > 64 with per-query bitmaps, k > 128 with a shared one, a four-bit handle -> PANN_ERR_UNSUPPORTED;
 * nq == 0 -> PANN_OK.  Nothing is written on an error.
 * Host pointers: the queries and the bitmap rows (packed to ceil(n / 32) words each) go up in one transfer, as
 * pann_batch_search_masked stages them -- the same memory note applies to per-query rows --, the outputs come back in one. */
int pann_bruteforce_knn_masked(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                               const uint32_t* allow, uint64_t allow_stride_words, uint32_t* out_ids, float* out_dists,
                               uint32_t* out_counts);
/* Device pointers throughout, launched on `stream`.  Per-query bitmaps: no synchronisation and no allocation.  Shared bitmap:
 * SYNCHRONISES the stream once -- the number of allowed points has to come back before the list can be allocated and the
 * distance launch sized -- and grows the handle's scratch to 4 bytes per allowed point on first use. */
int pann_bruteforce_knn_masked_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                   const uint32_t* d_allow, uint64_t allow_stride_words, uint32_t* d_out_ids, float* d_out_dists,
                                   uint32_t* d_out_counts, void* stream);
/* d_counts[r] = number of allowed points of bitmap row r, r < rows: rows x ceil(n / 32) words, allow_stride_words apart; bits at
 * positions >= n are ignored.  allow_stride_words == 0: one row (`rows` is not read).  Device pointers, on `stream` of the
 * current device; no synchronisation, no allocation.  n < 2^32.  NULL pointers, a stride between 1 and ceil(n / 32) - 1 ->
 * PANN_ERR_BAD_ARG. */
int pann_allow_count_dev(const uint32_t* d_allow, uint64_t n, uint64_t rows, uint64_t allow_stride_words, uint32_t* d_counts,
                         void* stream);

/* ---- label predicates: per-point labels in place of per-query bitmaps (DESIGN.md "Label predicates") ----  This project's own;
 * the reference has no filters.  A handle can own one uint32 label per point (n words on the device); a query's filter then is a
 * two-word predicate over the labels instead of a bitmap row of ceil(n / 32) words: 8 bytes per query, whatever n is.
 *   PANN_PRED_ANY    point i is allowed iff (label[i] & a) != 0          (b is ignored)   any of a category set
 *   PANN_PRED_MATCH  point i is allowed iff (label[i] & a) == b          all of a set (b == a), none of it (b == 0), equality of a
 *                                                                         bit field (a tenant id), a tombstone bit with any of these
 *   PANN_PRED_RANGE  point i is allowed iff a <= label[i] <= b, UNSIGNED, both ends inclusive (a > b allows nothing)
 * kind is one per call; npreds is 1 (preds[0] for the whole batch) or nq (query q uses preds[q]).
 * THE RULE: every labeled entry point returns, field for field and bit for bit, what its bitmap twin returns when query q's
 * bitmap row is { i < n : pred_q(label[i]) } -- pann_batch_search_labeled* <-> pann_batch_search_masked*,
 * pann_batch_search_labeled_rerank* <-> pann_batch_search_masked_rerank*, pann_bruteforce_knn_labeled* <->
 * pann_bruteforce_knn_masked* (one predicate <-> the shared bitmap, nq predicates <-> per-query rows).  Everything said at the
 * twins holds: the walk is not steered by the predicate and its counters do not depend on it, the result list holds at most 64
 * keys, empty rows are answers, no PANN_STATUS_SHORT_FRONTIER under a filter.
 * Status, beyond what the twin rejects with the twin's code (out_k > 64, k > 64, use_filter != 0, a four-bit handle on the exact
 * route -> PANN_ERR_UNSUPPORTED): a handle without labels, an unknown kind, NULL preds, a device preds pointer that is not 8-byte
 * aligned, npreds not in {1, nq} -> PANN_ERR_BAD_ARG; nq == 0 -> PANN_OK.  Nothing is written on an error. */
enum { PANN_PRED_ANY = 0, PANN_PRED_MATCH = 1, PANN_PRED_RANGE = 2 };
typedef struct pann_label_pred { uint32_t a, b; } pann_label_pred;

/* Labels on the handle.  A handle has none until the first set call, which allocates n words, zero filled.  set_labels: host
 * pointer; rows [first_row, first_row + nrows) get labels[0 .. nrows) -- the range form of pann_index_upload_points, so a refilled
 * slot of a dynamic index gets its label; waits for the handle's stream first and returns when the labels are in place.
 * set_labels_dev: device pointer, enqueued on the handle's stream, no synchronisation; allocates on the first call only.
 * get_labels: rows [first_row, first_row + nrows) to out (host).  drop_labels: frees them (waits for the stream).
 * has_labels: 1 / 0.  A range outside [0, n), a NULL pointer, get_labels on a handle without labels -> PANN_ERR_BAD_ARG, and
 * nothing is written (nor allocated).  pann_index_create_quantized copies no labels. */
int pann_index_set_labels(pann_index* idx, uint64_t first_row, const uint32_t* labels, uint64_t nrows);
int pann_index_set_labels_dev(pann_index* idx, uint64_t first_row, const uint32_t* d_labels, uint64_t nrows);
int pann_index_get_labels(pann_index* idx, uint64_t first_row, uint64_t nrows, uint32_t* out);
int pann_index_drop_labels(pann_index* idx);
int pann_index_has_labels(const pann_index* idx);

/* pann_batch_search_masked with (kind, preds, npreds) in place of the bitmap.  Host pointers: the predicates travel in the packed
 * transfer of the queries, 8 bytes per query. */
int pann_batch_search_labeled(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                              uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                              int kind, const pann_label_pred* preds, uint64_t npreds, const pann_search_out* out,
                              uint32_t* out_result_count, uint32_t* out_allowed_cmps);
/* Device pointers throughout, launched on `stream`; no sync, no alloc beyond the workspace growth of pann_batch_search_dev. */
int pann_batch_search_labeled_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                  uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                  int kind, const pann_label_pred* d_preds, uint64_t npreds, const pann_search_out* d_out,
                                  uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, void* stream);

/* ---- steered masked search: the walk spends its distances on allowed points only (DESIGN.md "Steered masked search") ----
 * This project's own rule.  pann_batch_search_masked / _labeled with ONE change: the neighbours of a visited vertex that passed
 * the hash filter and are NOT allowed get no distance; they are bridges.  After the vertex's own row, the bridges' rows are read in
 * order, each whole or not at all, until `fill` points wait for a distance; of a bridge's neighbours only the allowed ones are
 * looked at (and only they enter the hash filter), so there is no third hop.  fill: 1 .. deg_eff = min(degree_limit, max_degree);
 * 0 means deg_eff, a larger value is clamped.  Start points get a distance whether allowed or not; they are the only disallowed
 * points that do, so apart from them out->dist_cmps == out_allowed_cmps.  degree_sum counts the visited vertices' rows only.
 * The result rule, out_result_count and out_allowed_cmps are pann_batch_search_masked's.  With a bitmap that allows every point
 * every output equals pann_batch_search_masked's, whatever fill is.
 * out_steer (optional, nq x 2): per query the bridge rows expanded, and the entries the two-hop pass added.
 * Status: as the masked twin (out_k > 64 -> PANN_ERR_UNSUPPORTED, out_k > beam or k > beam -> PANN_ERR_BAD_ARG, ...).  There is no
 * form with the sketch filter, on the fused rerank path or for a sharded index. */
int pann_batch_search_steered(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                              uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                              const uint32_t* allow, uint64_t allow_stride_words, const pann_search_out* out,
                              uint32_t* out_result_count, uint32_t* out_allowed_cmps, uint32_t fill, uint32_t* out_steer);
/* Device pointers throughout, launched on `stream`; no sync, no alloc beyond the workspace growth of pann_batch_search_dev. */
int pann_batch_search_steered_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                  uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                  const uint32_t* d_allow, uint64_t allow_stride_words, const pann_search_out* d_out,
                                  uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, uint32_t fill, uint32_t* d_out_steer,
                                  void* stream);
/* The same with (kind, preds, npreds) in place of the bitmap, as pann_batch_search_labeled. */
int pann_batch_search_steered_labeled(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                                      uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                                      int kind, const pann_label_pred* preds, uint64_t npreds, const pann_search_out* out,
                                      uint32_t* out_result_count, uint32_t* out_allowed_cmps, uint32_t fill, uint32_t* out_steer);
int pann_batch_search_steered_labeled_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                          uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts,
                                          const pann_query_params* qp, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                                          const pann_search_out* d_out, uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps,
                                          uint32_t fill, uint32_t* d_out_steer, void* stream);

/* pann_batch_search_masked_rerank* with predicates.  The labels are read from `full`, the caller's primary handle; quant needs
 * none, and its own labels are not consulted. */
int pann_batch_search_labeled_rerank_dev(pann_index* full, pann_index* quant, const pann_quant_params* qparams,
                                         const float* d_queries, uint64_t nq, uint64_t q_stride_bytes, int normalize_first,
                                         int use_filter, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                         int kind, const pann_label_pred* d_preds, uint64_t npreds, const pann_rerank_out* d_out,
                                         uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, void* stream);
int pann_batch_search_labeled_rerank(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* queries,
                                     uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter,
                                     const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp, int kind,
                                     const pann_label_pred* preds, uint64_t npreds, const pann_rerank_out* out,
                                     uint32_t* out_result_count, uint32_t* out_allowed_cmps);

/* pann_bruteforce_knn_masked* with predicates.
 *   npreds == 1, k <= 128: the predicate is expanded on the device into one bitmap in the handle's scratch, and the shared-bitmap
 *     route of pann_bruteforce_knn_masked runs on it -- its one stream synchronisation included.
 *   npreds == nq, k <= 64: one wavefront per query scans the label array, 2 048 labels a step, no bitmap is materialised; no
 *     synchronisation and no allocation on the _dev entry. */
int pann_bruteforce_knn_labeled(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k, int kind,
                                const pann_label_pred* preds, uint64_t npreds, uint32_t* out_ids, float* out_dists,
                                uint32_t* out_counts);
int pann_bruteforce_knn_labeled_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                    int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t* d_out_ids,
                                    float* d_out_dists, uint32_t* d_out_counts, void* stream);

/* The bridge to every bitmap API: row r of d_allow (rows allow_stride_words >= ceil(n / 32) apart, npreds >= 1 rows) gets the
 * bitmap of d_preds[r] over the handle's labels, in the format of pann_batch_search_masked; bits at positions >= n of the last
 * word are written 0, words past ceil(n / 32) are not touched.  Device pointers, on `stream`; no synchronisation, no allocation.
 * A handle without labels, an unknown kind, NULL or misaligned pointers, a stride below ceil(n / 32) -> PANN_ERR_BAD_ARG. */
int pann_labels_to_allow_dev(pann_index* idx, int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t* d_allow,
                             uint64_t allow_stride_words, void* stream);
/* d_counts[r] = number of points d_preds[r] allows, r < npreds, without materialising rows: what a caller decides exact-or-walk
 * by.  Device pointers, on `stream`; no synchronisation, no allocation.  Status as pann_labels_to_allow_dev. */
int pann_label_count_dev(pann_index* idx, int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t* d_counts,
                         void* stream);

/* ---- exact kNN by predicate group: many queries, few distinct filters (DESIGN.md "Exact kNN by predicate group") ----
 * This project's own.  The call gives a TABLE of G >= 1 filters -- `npreds` predicates of one kind over the handle's labels, or
 * `nrows` bitmap rows allow_stride_words >= ceil(n / 32) apart (0 is allowed for one row) -- and one table index per query
 * (group_of_query / row_of_query, nq x uint32, each < G).
 * THE RULE: row q of the result is, field for field and bit for bit, what pann_bruteforce_knn_labeled with the ONE predicate
 * preds[group_of_query[q]] (pann_bruteforce_knn_masked with the ONE shared bitmap row row_of_query[q]) returns for query q: the
 * min(k, c) nearest allowed points sorted by (dist, id), c = the points the filter allows, then 0xFFFFFFFF / +inf;
 * out_counts[q] (optional) = min(k, c); a filter that allows nothing is an answer, not an error.  k <= 128 for any G.  Table
 * entries that no query names and entries that repeat a filter are allowed.  G == nq with all filters different is correct but
 * does the work of the per-query scan with more steps: the grouped call pays off when many queries share few filters.
 * How: the queries are sorted by table index on the device, every used entry is compacted into its ascending id list, the lists
 * of a chunk of entries lie one after the other, and ONE segmented launch of the dense kernels of pann_bruteforce_knn scores
 * every entry's queries against that entry's list ("gt_pieces" is honoured); the rows then go back to the caller's order.
 * max_list_ids bounds the ids materialised at once: table entries are processed in chunks of consecutive used entries whose
 * lists together hold at most max_list_ids ids (with predicates also: whose bitmap rows, expanded into scratch, hold at most
 * max_list_ids words); an entry whose own list is longer (<= n ids) is a chunk alone.  0 = the default, 16 Mi ids: 64 MB of ids
 * and, with predicates, as much of rows.  Results never depend on it.
 * Status: everything the twins refuse keeps its code (a four-bit handle, k > 128 -> PANN_ERR_UNSUPPORTED; k == 0, no labels, an
 * unknown kind, NULL or misaligned preds, NULL queries / outputs / bitmap, a short query stride -> PANN_ERR_BAD_ARG); an empty
 * table, a NULL index array, a bitmap stride below ceil(n / 32), a table index >= G -> PANN_ERR_BAD_ARG; nq == 0 -> PANN_OK.
 * Nothing is written on an error.
 * Host pointers: the table indices are checked on the host; index array, table and queries go up in one transfer, the outputs
 * come back in one (HostTrip, as the twins). */
int pann_bruteforce_knn_labeled_grouped(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                        int kind, const pann_label_pred* preds, uint64_t npreds, const uint32_t* group_of_query,
                                        uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts);
int pann_bruteforce_knn_masked_grouped(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                       const uint32_t* allow, uint64_t nrows, uint64_t allow_stride_words,
                                       const uint32_t* row_of_query, uint64_t max_list_ids, uint32_t* out_ids, float* out_dists,
                                       uint32_t* out_counts);
/* Device pointers throughout, launched on `stream`.  SYNCHRONISES the stream ONCE, as the shared route of
 * pann_bruteforce_knn_masked_dev does: the flag of the range check, the number of queries per table entry and the number of
 * allowed points per table entry come back in that one read, and the host plans the chunks, segments and tiles from them; the
 * plan goes up and everything after it is enqueued without another wait.  A table index >= G is detected by the grouping pass on
 * the device and reported as PANN_ERR_BAD_ARG after that synchronisation, with no output written.  Grows the handle's scratch
 * on first use (the sorted queries, a chunk's lists and rows, a chunk's queries and staged results); one call per handle at a
 * time. */
int pann_bruteforce_knn_labeled_grouped_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                            int kind, const pann_label_pred* d_preds, uint64_t npreds,
                                            const uint32_t* d_group_of_query, uint64_t max_list_ids, uint32_t* d_out_ids,
                                            float* d_out_dists, uint32_t* d_out_counts, void* stream);
int pann_bruteforce_knn_masked_grouped_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                           const uint32_t* d_allow, uint64_t nrows, uint64_t allow_stride_words,
                                           const uint32_t* d_row_of_query, uint64_t max_list_ids, uint32_t* d_out_ids,
                                           float* d_out_dists, uint32_t* d_out_counts, void* stream);

/* ---- entry points: the medoids of a table of filters, on the device (DESIGN.md "Entry points") ----  This project's own.
 * Where a filtered search starts: for every filter of a table the points nearest to the centroid of what it allows, so that a
 * tenant's queries begin in the tenant's region (the per-label entry points of FilteredDiskANN), and a dynamic index gets a live
 * start after pann_vamana_delete_batch without a host round trip.  The table formats are exactly those of
 * pann_bruteforce_knn_{labeled,masked}_grouped: G = npreds predicates of one kind over the handle's labels, or G = nrows bitmap
 * rows allow_stride_words >= ceil(n / 32) apart (0 is allowed for one row); there is no index array.  allow == NULL with
 * nrows == 1: every point -- the medoid of the index.
 * THE RULE, for table entry g with allowed set A_g, c_g = |A_g|:
 *   centroid[g][j] = (float)(S / (double)c_g), S = the sum over A_g of coordinate j widened exactly -- accumulated in 64-bit
 *     integers for PANN_U8 / PANN_I8, in double for the three float types -- ONE double division, ONE rounding to f32; c_g == 0:
 *     the row is all zeros.  out_centroids (optional): G x d floats.
 *   the query row = the centroid converted to the handle's element type: f32 as it is; f16 and bf16 round to nearest even (NaN
 *     -> 0x7FC0 in bf16); u8 / i8 rint (ties to even), clamped to the type's range.
 *   row g of out_ids / out_dists (G x per_filter) is, bit for bit, what pann_bruteforce_knn_*_grouped returns for that query row
 *     under filter g with k = per_filter: the min(per_filter, c_g) allowed points nearest to the centroid under the handle's
 *     distance, sorted by (dist, id); out_counts[g] (optional) = min(per_filter, c_g); unused slots hold fill_id / +inf.  A caller
 *     passes its ordinary start as fill_id and can use every row as a row of starts as it stands; 0xFFFFFFFF is plain padding.
 *   The sums are exact for the one-byte types and for float data whose double sums are exact (integer-valued data, dyadic
 *     grids).  On other float data the summation order is the implementation's -- a fixed one, without floating-point atomics:
 *     the same call on the same handle gives the same bits ("centroid_piece_ids" of pann_index_get_option, a compile-time
 *     constant that pann_index_set_option refuses, is the number of consecutive list ids one workgroup sums).
 * max_list_ids chunks the work as in the grouped route and never changes a result on exactly-summable data.
 * Status: per_filter in 1 .. 128 (0 -> PANN_ERR_BAD_ARG, above -> PANN_ERR_UNSUPPORTED); a four-bit handle ->
 * PANN_ERR_UNSUPPORTED; everything else the grouped twins refuse keeps its code (no labels, an unknown kind, NULL or misaligned
 * preds, a NULL bitmap with nrows != 1, NULL out_ids / out_dists, an empty table, a bitmap stride below ceil(n / 32) ->
 * PANN_ERR_BAD_ARG).  Nothing is written on an error.
 * Host pointers: the table goes up in one transfer, the outputs come back in one (HostTrip, as the twins). */
int pann_filter_medoids_labeled(pann_index* idx, int kind, const pann_label_pred* preds, uint64_t npreds, uint32_t per_filter,
                                uint32_t fill_id, uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts,
                                float* out_centroids);
int pann_filter_medoids_masked(pann_index* idx, const uint32_t* allow, uint64_t nrows, uint64_t allow_stride_words, uint32_t per_filter,
                               uint32_t fill_id, uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts,
                               float* out_centroids);
/* Device pointers throughout, launched on `stream`.  SYNCHRONISES the stream ONCE, as the grouped route does (the allowed points
 * per table entry come back and the host plans the chunks); scratch comes from the handle; one call per handle at a time. */
int pann_filter_medoids_labeled_dev(pann_index* idx, int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t per_filter,
                                    uint32_t fill_id, uint64_t max_list_ids, uint32_t* d_out_ids, float* d_out_dists,
                                    uint32_t* d_out_counts, float* d_out_centroids, void* stream);
int pann_filter_medoids_masked_dev(pann_index* idx, const uint32_t* d_allow, uint64_t nrows, uint64_t allow_stride_words,
                                   uint32_t per_filter, uint32_t fill_id, uint64_t max_list_ids, uint32_t* d_out_ids, float* d_out_dists,
                                   uint32_t* d_out_counts, float* d_out_centroids, void* stream);

/* Grouped labeled search: many queries, few distinct predicates, and a row of starts per predicate -- the rows that
 * pann_filter_medoids_labeled returns.  The table is `npreds` = G predicates of one kind, group_of_query (nq x uint32, each < G)
 * names every query's entry; starts holds start_rows x nstarts ids, start_rows == 1 (one row for the batch) or G.
 * THE RULE: row q of every output is what pann_batch_search_labeled returns for query q alone, with the ONE predicate
 * preds[group_of_query[q]] and the shared starts row starts[(start_rows == 1 ? 0 : group_of_query[q]) * nstarts ..]; with
 * steer != 0 the twin is pann_batch_search_steered_labeled with this `fill`, and out_steer (optional, nq x 2) its counters.  A
 * start that the filter disallows is treated as both twins treat it: it gets a distance and is no result.
 * How: one kernel gathers every query's predicate and start row into the handle's scratch; the search kernels then run with one
 * predicate and one start row per query.
 * Status: everything the twin refuses keeps its code; start_rows not in {1, G}, a NULL index array, an empty table ->
 * PANN_ERR_BAD_ARG.  Nothing is written on an error.  Host pointers: the table indices (each < G) and the starts (each < n) are
 * checked on the host. */
int pann_batch_search_grouped_labeled(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                                      uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, uint64_t start_rows,
                                      const pann_query_params* qp, int kind, const pann_label_pred* preds, uint64_t npreds,
                                      const uint32_t* group_of_query, const pann_search_out* out, uint32_t* out_result_count,
                                      uint32_t* out_allowed_cmps, int steer, uint32_t fill, uint32_t* out_steer);
/* Device pointers throughout, launched on `stream`; no sync, no alloc beyond the growth of the workspace and of the gather's
 * scratch.  Nothing is read back, so a bad table index cannot be refused: a query whose index is >= G reads no table entry -- it
 * gets a predicate that allows nothing and start row 0, its ids row is padding, its result_count 0, and PANN_STATUS_BAD_GROUP is
 * raised in d_out->status (when given); the other queries' rows are what they would have been.  The start ids are NOT validated
 * (the _dev convention): a start >= n is gathered unchecked. */
int pann_batch_search_grouped_labeled_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                          uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, uint64_t start_rows,
                                          const pann_query_params* qp, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                                          const uint32_t* d_group_of_query, const pann_search_out* d_out,
                                          uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, int steer, uint32_t fill,
                                          uint32_t* d_out_steer, void* stream);

/* ---- subset index: carve out, compact or grow a handle on the device (DESIGN.md "Subset index") ----  This project's own.
 * A new handle over the rows of src that a bitmap keeps, in ascending id order, with room for n_out rows; the graph is
 * renumbered, labels and sketch are carried over, nothing leaves the device.  Compaction after pann_vamana_delete_batch (the
 * bitmap without the deleted ids), a dedicated index over one tenant's or label's points (the bitmap of
 * pann_labels_to_allow_dev), growth (allow == NULL, n_out > n).
 * THE RULE.
 *   Bitmap: `allow` is ONE bitmap in the format of pann_batch_search_masked: ceil(n / 32) words, point i kept iff bit i & 31 of
 *     word i >> 5 is set; bits at positions >= n are ignored.  allow == NULL keeps every point: a clone, or a grown copy when
 *     n_out > n.
 *   Sizes: K = the kept ids in ascending order, m = |K|.  The new handle has n' = n_out ? n_out : m rows.
 *     new_to_old[r] = K[r] for r < m (entries past m are not written); old_to_new[i] = the rank of i in K, or 0xFFFFFFFF if i
 *     is dropped (n words); *kept_out = m.  All three outputs are optional (NULL).
 *   Fixed: the new handle has src's d, dtype, metric, max_deg and device.  Every element type is allowed, PANN_U4 / PANN_I4
 *     included: rows are moved as bytes.
 *   Points: row r < m is row K[r] of src, byte for byte, over the whole device row including its zero padding; rows [m, n')
 *     are zero.
 *   Graph: copy_graph != 0: row r < m holds the neighbours of src's row K[r] IN ROW ORDER, without those that are not in K, each
 *     mapped through old_to_new, packed at the front, the remaining slots empty; rows [m, n') are empty.  copy_graph == 0: every
 *     row is empty.
 *   Labels: if src has labels, row r < m gets label[K[r]] and rows [m, n') get 0; otherwise the new handle has none.
 *   Sketch: if src has a sketch attached its rows are gathered the same way, zero rows past m, and the new handle gets src's
 *     pann_sketch_params: pann_index_sketch_kind and the query sketching of the fused rerank behave as on src.
 *   Other state: the exact-float-order flag is carried.  NOT carried, left as on a fresh handle: filter-code tables, locality
 *     cells, options, dropped-list capacity, the stream -- the new handle has its own private stream.  src is not modified
 *     (its scratch is used).
 * Execution: the work runs on src's stream.  With a bitmap that stream is synchronised once for m, which must be known before
 * anything is allocated, and in every case once more before the call returns, as pann_index_create_quantized does.  The host form
 * moves the bitmap up and the maps down in packed transfers like every host-pointer entry point; the _dev form takes device
 * pointers (4-byte aligned) for the bitmap and the two maps -- out and kept_out are host pointers in both.
 * Status: NULL out or src, n_out != 0 && n_out < m, n' == 0, n' >= 2^31 - 1, a misaligned device pointer -> PANN_ERR_BAD_ARG;
 * new_to_old != NULL && new_to_old_cap < m -> PANN_ERR_OVERFLOW.  *kept_out is written whenever m was counted -- under
 * PANN_ERR_OVERFLOW and the n_out / n' errors it is valid, the ids_capacity convention of pann_bruteforce_range.  On every error
 * nothing is created, *out is left as it was and no output array is written. */
int pann_index_create_subset_dev(pann_index** out, pann_index* src, const uint32_t* d_allow, uint64_t n_out, int copy_graph,
                                 uint32_t* d_new_to_old, uint64_t new_to_old_cap, uint32_t* d_old_to_new, uint64_t* kept_out);
int pann_index_create_subset(pann_index** out, pann_index* src, const uint32_t* allow, uint64_t n_out, int copy_graph,
                             uint32_t* new_to_old, uint64_t new_to_old_cap, uint32_t* old_to_new, uint64_t* kept_out);

/* ---- graph reachability: BFS levels and degrees on the device (DESIGN.md "Graph reachability") ----  This project's own.
 * Which vertices can a search that starts at `starts` reach at all?  A level-synchronous breadth-first walk over the handle's
 * current rows.  Only the graph is read, never a point, so every element type is accepted, PANN_U4 / PANN_I4 included.  A
 * neighbour word >= n (the empty marker) is skipped.
 * THE RULE.
 *   level: level[v] = the length of a shortest directed path from any start to v; starts have level 0, duplicate starts mean
 *     nothing; 0xFFFFFFFF = no path.  n words, every one of them written.
 *   reached: the bitmap {v : level[v] != 0xFFFFFFFF} in the format of pann_batch_search_masked, ceil(n / 32) words, bits at
 *     positions >= n written 0: it goes as it is into pann_index_create_subset*, pann_allow_count_dev and every masked entry.
 *   consider: ONE bitmap in the same format, NULL = every vertex; bits at positions >= n are ignored.  It does NOT steer the walk
 *     (a masked search walks through disallowed points too); it only selects which vertices are counted and listed as unreached.
 *     The typical value is the live set after pann_vamana_delete_batch.
 *   unreached_ids: the considered vertices without a level, ascending, each once; entries past stats->unreached are not written.
 *     unreached_ids != NULL && unreached_cap < stats->unreached -> PANN_ERR_OVERFLOW: the list is untouched, stats, level and
 *     reached are valid (the ids_capacity convention of pann_bruteforce_range).
 *   max_rounds: 0 = expand until the frontier is empty.  r > 0 = at most r expansion rounds: levels 0 .. r are written, vertices
 *     beyond them are 0xFFFFFFFF and count as unreached, and stats->truncated = 1 iff the level-r frontier is not empty.
 *   stats (optional) is OVERWRITTEN, not added to.  Every output pointer is optional (NULL); without level no level array exists
 *     anywhere, the visited bitmap suffices.
 * Execution: as pann_vamana_delete_batch_dev -- the work runs on the handle's stream, scratch comes from the handle, and both
 * forms return after the stream has drained: the frontier lengths are read back once per group of rounds (not once per level),
 * and the unreached count before the list is written.  The host form moves starts and consider up and level, reached and the
 * ids down in packed transfers like every host-pointer entry point; the _dev form takes device pointers (4-byte aligned) for
 * them -- stats is a host pointer in both.
 * Status: NULL idx or starts, nstarts == 0, a start >= n, a misaligned device pointer -> PANN_ERR_BAD_ARG, nothing written (the
 * host form checks the starts on the host, the _dev form on the device before any output is written). */
typedef struct pann_reach_stats {
  uint64_t reached;       /* vertices that got a level, starts included */
  uint64_t unreached;     /* considered vertices without a level (no consider bitmap: n - reached) */
  uint64_t max_frontier;  /* population of the largest level */
  uint32_t levels;        /* 1 + the largest level written */
  uint32_t truncated;     /* 1: max_rounds stopped the walk with a non-empty frontier left unexpanded */
  double   t_s;           /* seconds on the device, events around the call's work */
} pann_reach_stats;

int pann_graph_reach_dev(pann_index* idx, const uint32_t* d_starts, uint32_t nstarts, const uint32_t* d_consider,
                         uint32_t max_rounds, uint32_t* d_level, uint32_t* d_reached, uint32_t* d_unreached_ids,
                         uint64_t unreached_cap, pann_reach_stats* stats);
int pann_graph_reach(pann_index* idx, const uint32_t* starts, uint32_t nstarts, const uint32_t* consider,
                     uint32_t max_rounds, uint32_t* level, uint32_t* reached, uint32_t* unreached_ids,
                     uint64_t unreached_cap, pann_reach_stats* stats);

/* out_deg[v] = the neighbour slots of row v that hold an id < n; in_deg[w] = the (row, slot) pairs that name w: a duplicate
 * in a row counts twice, a self loop counts.  n words each, either may be NULL.  The _dev form takes device pointers (4-byte
 * aligned) and runs on `stream` with no synchronisation and no allocation (it zero-fills d_in_deg itself, on that stream); the
 * host form goes through the handle's stream and returns when the arrays are home.  NULL idx, both outputs NULL, a misaligned
 * device pointer -> PANN_ERR_BAD_ARG. */
int pann_graph_degrees_dev(pann_index* idx, uint32_t* d_out_deg, uint32_t* d_in_deg, void* stream);
int pann_graph_degrees(pann_index* idx, uint32_t* out_deg, uint32_t* in_deg);

#ifdef __cplusplus
}
#endif
#endif /* PANN_H_ */
