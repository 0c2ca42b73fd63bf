// pann_internal.h -- private declarations shared by the HIP translation units of libpann.so.
// Target: gfx950 (MI355X, CDNA4) only.  64-lane wavefronts are assumed everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <string>

#include "../../include/pann.h"
#include "scratch_carve.h"
#include "search_plan.h"
#include "search_call.h"

namespace pann {

constexpr uint32_t SENTINEL = 0xFFFFFFFFu;  // empty adjacency slot on the device / empty filter slot

// Diagnostic A/B switches (environment variables that select kernel variants for same-box comparisons, tools/ab_*.sh) exist
// only in `make alt` builds (-DPANN_AB, lib/libpann_alt.so); the shipped libpann.so reads no environment variable.
#ifdef PANN_AB
inline const char* ab_env(const char* name) { return getenv(name); }
#else
inline const char* ab_env(const char*) { return nullptr; }
#endif

// ---- element types: bytes of one element (0 for the four-bit types: half a byte) and of one host-layout row of d elements.
// A four-bit row is the reference's num_bytes() = (dims * bits - 1) / 8 + 1 (mips_point.h:297), two coordinates per byte.
inline bool is_4bit_dtype(int dtype) { return dtype == PANN_U4 || dtype == PANN_I4; }
inline const char* dtype_name(int dtype) {
  switch (dtype) {
    case PANN_U8: return "PANN_U8"; case PANN_I8: return "PANN_I8"; case PANN_F32: return "PANN_F32"; case PANN_F16: return "PANN_F16";
    case PANN_BF16: return "PANN_BF16"; case PANN_U4: return "PANN_U4"; case PANN_I4: return "PANN_I4";
  }
  return "unknown dtype";
}
inline uint32_t esize_of(int dtype) {
  switch (dtype) { case PANN_U8: case PANN_I8: return 1; case PANN_F16: case PANN_BF16: return 2; case PANN_F32: return 4; }
  return 0;
}
inline bool dtype_known(int dtype) { return esize_of(dtype) != 0 || is_4bit_dtype(dtype); }
inline uint64_t row_bytes_of(int dtype, uint64_t d) { return is_4bit_dtype(dtype) ? (d + 1) / 2 : d * esize_of(dtype); }

// ---- device-side layout of one index (DESIGN.md "Data layout in HBM") ----
//  points: n rows, row stride pstride = nch * lpc * 16 bytes (>= row_bytes_of(dtype, d)), zero padded
//  graph : n rows of gstride uint32 (gstride = max_deg rounded up to 16), neighbours packed at the
//          front, unused slots = SENTINEL; the degree is not stored (it is the count of
//          non-sentinel slots), so a row of max_deg 64 is exactly one aligned 256-byte read.
struct DeviceIndex {
  uint8_t* points = nullptr;
  uint32_t* graph = nullptr;
  uint64_t n = 0;
  uint32_t d = 0;
  int dtype = 0, metric = 0;
  uint32_t esize = 0;    // bytes per element (0 for the four-bit types: sizes of rows come from dbytes)
  uint32_t dbytes = 0;   // row_bytes_of(dtype, d): bytes of one host-layout row
  uint32_t pstride = 0;  // device row stride in bytes
  uint32_t lpc = 0;      // lanes per candidate in the gather-distance loops (4,8,16,32)
  uint32_t nch = 0;      // 16-byte chunks per lane: pstride = nch*lpc*16
  uint32_t exact = 0;    // exact float order (validation mode): lane-per-candidate sequential sums; forces lpc=4
  uint32_t max_deg = 0;
  uint32_t gstride = 0;  // uint32 per graph row on the device
  uint32_t forest_group = 0;  // HCNNG: trees split level by level together (0 = as many as 2^31 positions allow)
  uint32_t b64_seen = 1;      // beam <= 64: search with the second-sighting table (0: without; search_plan.h make_plan)
  // filter-code table of the beam-91..128 searches (filter_codes.hip): the code of every id and, slot-aligned with the graph rows,
  // of every neighbour.  gcode is only read while codes_valid: every writer of graph rows either maintains it or clears the flag.
  const uint16_t* rank16 = nullptr;   // [n]
  uint16_t* gcode = nullptr;          // [n][gstride]
  uint32_t codes_valid = 0;
  // locality cell of every point (nearest of LOCALITY_PIVOTS pivots), for the order in which a batch's searches are launched
  // (vamana_build.hip: queries that run side by side then read rows of the same few regions); null = not computed
  const uint32_t* cell = nullptr;     // [n]
  uint32_t cell_min_batch = 4096;     // batches below this many searches keep the batch order
  // bit sketch of every point (sketch.hip), the second level of the filtered searches; null = none attached
  const uint8_t* sketch = nullptr;    // [n] rows of sk_stride bytes (host-layout row, zero padded to a multiple of 16)
  uint32_t sk_stride = 0;
  int sk_kind = -1;
  uint32_t sk_as_written = 0;         // one-bit kinds: the reference's distance loop as written (block 0 counted num_blocks times)
  // one label word per point (pann_index_set_labels), what the label predicates are evaluated on; null = none set
  const uint32_t* labels = nullptr;   // [n]
};

// query in registers or in LDS: the one definition is search_plan.h's
inline bool layout_query_in_registers(const DeviceIndex& ix) { return layout_query_in_registers(ix.lpc, ix.nch); }
inline size_t query_lds_bytes(const DeviceIndex& ix) { return query_lds_bytes(ix.lpc, ix.nch); }

inline bool pred_kind_known(int kind) { return kind == PANN_PRED_ANY || kind == PANN_PRED_MATCH || kind == PANN_PRED_RANGE; }

// SearchArgs (the launch arguments of one beam search), PointFilter and the request descriptors of the search family: search_call.h

// dense_topk_dev (dense.hip): for every A row the m nearest B rows.  A rows: external rows (a_ext, a_stride bytes apart) or the table's rows
// a_ids; B rows: the table's rows b_ids (null: 0 .. nb).  Segmented form: segment s pairs the A rows [a_off[s], a_off[s + 1]) with the B rows
// [b_off[s], b_off[s + 1]), tile t the 64 A rows from tile_a0[t] of segment tile_seg[t] (grouped_plan.h); all four null: one segment.  Device pointers.
struct DenseTopkCall {
  const uint8_t* a_ext = nullptr; uint64_t a_stride = 0;
  const uint32_t* a_ids = nullptr, *b_ids = nullptr, *tile_seg = nullptr, *tile_a0 = nullptr;
  const uint64_t* a_off = nullptr, *b_off = nullptr;
  uint32_t ntiles = 0, nsplit = 1, m = 0; uint64_t na = 0, nb = 0; int exclude_same = 0;      // nsplit: pieces B is cut into per tile
  uint32_t* out_ids = nullptr; float* out_dists = nullptr;      // na x m each
};

// the one growable device buffer: kernel scratch, staging regions, tables kept on a handle (grown on demand, never shrunk).
// A buffer of several arrays is laid out by ONE function that takes them from a Carve; carve_into(ws, tail_slack, layout) runs it
// dry to size the buffer, then on the buffer to set the pointers (scratch_carve.h).
struct Workspace {
  void* buf = nullptr; size_t bytes = 0;
  int ensure(size_t need);
  void release();
  template <typename T> T* as() const { return (T*)buf; }
};

void set_error(const std::string& s);
int hip_fail(hipError_t e, const char* what);
#define PANN_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return pann::hip_fail(e_, #call); } while (0)

// a device buffer owned by ONE call and freed on every return path: what is too large to stay on the handle, or as large as a
// count the device has just produced.  ensure() allocates exactly what is asked (16 bytes at least), carve_into() accepts it.
struct HBuf {
  void* buf = nullptr; size_t bytes = 0;
  HBuf() = default;
  HBuf(const HBuf&) = delete;
  HBuf& operator=(const HBuf&) = delete;
  ~HBuf() { if (buf) (void)hipFree(buf); }
  int ensure(size_t need) {
    if (buf && need <= bytes) return PANN_OK;
    if (buf) { PANN_HIP(hipFree(buf)); buf = nullptr; bytes = 0; }
    need = std::max<size_t>(need, 16);
    PANN_HIP(hipMalloc(&buf, need));
    bytes = need;
    return PANN_OK;
  }
  template <typename T> T* as() const { return (T*)buf; }
};

// the phase timers of the builders' statistics
using TimePoint = std::chrono::steady_clock::time_point;
inline TimePoint now() { return std::chrono::steady_clock::now(); }
inline double secs(TimePoint a, TimePoint b) { return std::chrono::duration<double>(b - a).count(); }

// beam_search.hip
size_t search_workspace_bytes(const DeviceIndex& ix, const SearchArgs& a);
int launch_beam_search(const DeviceIndex& ix, const SearchArgs& a, void* ws, size_t ws_bytes,
                       hipStream_t stream);
void choose_point_layout(uint32_t dbytes, uint32_t* lpc, uint32_t* nch);

// A launch carries its work-item count (blocks x threads) in 32 bits, and the runtime takes a larger count modulo 2^32 without
// an error: 2^26 + 4096 blocks of one wave run 4096 blocks.  A launch with a block or a wave per vertex therefore goes in slices
// of at most this many blocks, and its kernel adds the slice's first block to blockIdx.x.
inline uint32_t launch_slice_blocks(uint32_t threads) { return (1u << 31) / threads; }

// vamana_build.hip
int robust_prune_batch_host(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint32_t* owners,
                            uint64_t m, const uint32_t* cand_ids, const float* cand_dists,
                            const uint64_t* cand_offsets, double alpha, uint32_t R, int add_out_nbrs,
                            uint32_t* out_rows, uint32_t* out_dist_cmps);
int insert_batch_dev(const DeviceIndex& ix, Workspace& ws, Workspace& ws2, Workspace& search_ws, Workspace& rows_ws, hipStream_t st,
                     const uint32_t* d_batch, uint32_t m, uint32_t start, uint32_t R, uint32_t L, double alpha,
                     uint32_t* vcap_io, pann_build_stats* stats);
// the two phases of a batch (vamana_build.hip): A reads the graph and yields rows for the points given, B applies the
// rows of the whole batch; d_rows is m x R uint32, SENTINEL padded
int vamana_search_prune_dev(const DeviceIndex& ix, Workspace& ws, Workspace& search_ws, hipStream_t st, const uint32_t* d_batch,
                            uint32_t m, uint32_t start, uint32_t R, uint32_t L, double alpha, uint32_t* vcap_io,
                            uint32_t* d_rows, pann_build_stats* stats);
int vamana_apply_rows_dev(const DeviceIndex& ix, Workspace& ws, Workspace& ws2, hipStream_t st, const uint32_t* d_batch, uint32_t m,
                          const uint32_t* d_rows, uint32_t R, double alpha, pann_build_stats* stats);
int sort_neighbors_dev(const DeviceIndex& ix, hipStream_t st);
// robustPrune, id-only form without the owner's out-neighbours, over a device CSR slab of candidate ids (vamana_build.hip);
// d_rows: m x R uint32, SENTINEL padded; d_dc is accumulated.  Nothing reaches the graph.
int prune_csr_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint32_t* d_owners, uint32_t m,
                  const uint32_t* d_cand_ids, const uint64_t* d_cand_base, const uint32_t* d_cand_cnt,
                  const uint32_t* d_seg_begin, uint32_t total_keys, uint32_t max_seg_len, double alpha, uint32_t R,
                  uint32_t* d_rows, uint32_t* d_rcnt, uint32_t* d_dc);

// vamana_delete.hip: one batch of deletions consolidated on the device (DESIGN.md "Deleting points").  d_del: m ids on the
// device (checked there); ws / rows_ws: the call's own arrays and the new rows, prune_ws: the prune's key scratch.
// range_keys: most keys pruned at once (0 = what the 32-bit key index allows); synchronises st.
int vamana_delete_batch_dev(const DeviceIndex& ix, Workspace& ws, Workspace& prune_ws, Workspace& rows_ws, hipStream_t st,
                            const uint32_t* d_del, uint64_t m, uint32_t R, double alpha, uint64_t range_keys,
                            pann_delete_stats* stats);

// dense.hip
int dense_topk_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const DenseTopkCall& c);
int query_distances_dev(const DeviceIndex& ix, hipStream_t st, const uint8_t* d_q_ext, uint64_t q_stride,
                        const uint32_t* d_q_ids, uint64_t nq, const uint32_t* d_ids, uint64_t m, int paired,
                        float* d_out);

int pivot_split_dev(const DeviceIndex& ix, hipStream_t st, const uint32_t* d_ids, const uint32_t* d_tile_seg,
                    const uint64_t* d_tile_lo, const uint32_t* d_tile_cnt, uint32_t ntiles, const uint32_t* d_pa,
                    const uint32_t* d_pb, uint8_t* d_side);

int rerank_dev(const DeviceIndex& ix, hipStream_t st, const uint8_t* d_q, uint64_t q_stride, uint64_t nq,
               const uint32_t* d_cand, uint32_t c, const uint32_t* d_cnt, uint32_t k, int resort, uint32_t* d_out_ids,
               float* d_out_dists);

// masked_knn.hip: exact kNN under an allow bitmap (DESIGN.md "Exact masked kNN").  Bitmap rows as SearchArgs::allow.
// allow_count_dev: d_counts[r] = allowed points of row r (rows x stride words; bits at positions >= n ignored).
int allow_count_dev(const uint32_t* d_allow, uint64_t n, uint64_t rows, uint64_t stride, uint32_t* d_counts, hipStream_t st);
// Compaction of ONE bitmap in two calls that share d_scratch (allow_compact_scratch_bytes(n) bytes): count leaves the number of
// allowed points at *d_total (a word of the scratch; the caller reads it back), scatter writes their ids, ascending, to
// d_ids[0 .. count).
size_t allow_compact_scratch_bytes(uint64_t n);
int allow_compact_count_dev(const uint32_t* d_allow, uint64_t n, uint32_t* d_scratch, const uint32_t** d_total, hipStream_t st);
int allow_compact_scatter_dev(const uint32_t* d_allow, uint64_t n, const uint32_t* d_scratch, uint32_t* d_ids, uint32_t count,
                              hipStream_t st);
// pad != 0: nq x k ids / dists <- 0xFFFFFFFF / +inf; d_counts (optional): nq entries <- cnt
int knn_pad_dev(uint32_t* d_ids, float* d_dists, uint32_t* d_counts, uint64_t nq, uint32_t k, uint32_t cnt, int pad, hipStream_t st);
// one filter per query (device pointers), k <= 64: a bitmap row per query, F.stride words apart, or the bitmap words of query q
// built from F.labels and F.preds[q] as the scan goes.  nq x k ids and dists, rows sorted by (dist, id) and padded; counts (nq) optional
int filter_scan_dev(const DeviceIndex& ix, hipStream_t st, const uint8_t* d_q, uint64_t q_stride, uint64_t nq, const PointFilter& F,
                    uint32_t k, uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts);
// label predicates (DESIGN.md "Label predicates"): d_labels n words, d_preds npreds predicates of one kind
// row r of d_allow (stride words apart, >= ceil(n / 32)) <- the bitmap of d_preds[r]; dead bits of the last word 0
int labels_to_allow_dev(const uint32_t* d_labels, uint64_t n, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                        uint32_t* d_allow, uint64_t stride, hipStream_t st);
// d_counts[r] = points d_preds[r] allows
int label_count_dev(const uint32_t* d_labels, uint64_t n, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                    uint32_t* d_counts, hipStream_t st);

// grouped route (DESIGN.md "Exact kNN by predicate group"): a table of G filters, d_group[q] < G names the filter of query q.
// The queries sorted by table index, stably: d_hist[g] = queries of entry g, d_off[0 .. G] = the first slot of every entry (G + 1
// words), d_perm[slot] = query (nq words); an index >= G raises *d_flag, and that query gets no slot.  d_part: scratch of
// nblocks x G words, nblocks from group_sort_shape.  Nothing is synchronised.
void group_sort_shape(uint64_t nq, uint64_t G, uint32_t* nblocks, uint64_t* per_block);
int group_queries_dev(const uint32_t* d_group, uint64_t nq, uint64_t G, uint32_t* d_flag, uint32_t* d_hist, uint32_t* d_off,
                      uint32_t* d_part, uint32_t* d_perm, hipStream_t st);
// d_out[u] = d_preds[d_used[u]], u < m
int gather_preds_dev(const pann_label_pred* d_preds, const uint32_t* d_used, uint64_t m, pann_label_pred* d_out, hipStream_t st);
// Compaction of `rows` bitmaps in one go: row r is row d_rowidx[r] (null: r) of d_allow, rows `stride` words apart; the ascending id
// lists are written one after the other to d_ids[0 .. cap), cap = the sum of the rows' counts (< 2^32).  d_scratch:
// allow_rows_compact_scratch_bytes(n, rows) bytes.
size_t allow_rows_compact_scratch_bytes(uint64_t n, uint64_t rows);
int allow_rows_compact_dev(const uint32_t* d_allow, uint64_t n, const uint32_t* d_rowidx, uint64_t stride, uint32_t rows,
                           uint32_t* d_scratch, uint32_t* d_ids, uint32_t cap, hipStream_t st);
// row r of d_slab (slab_stride bytes apart, a multiple of 16, 16-byte aligned) <- the dbytes bytes of query d_perm[r], zero padded
int gather_query_rows_dev(const uint8_t* d_q, uint64_t q_stride, uint32_t dbytes, const uint32_t* d_perm, uint64_t rows, uint8_t* d_slab,
                          uint32_t slab_stride, hipStream_t st);
// row d_perm[r] of the outputs <- row r of the staged k-wide result; d_out_counts (optional): its entries that are not padding
int scatter_knn_rows_dev(const uint32_t* d_sids, const float* d_sdists, const uint32_t* d_perm, uint64_t rows, uint32_t k,
                         uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, hipStream_t st);

// entry_points.hip (DESIGN.md "Entry points"): the centroids of the S lists of a CSR (d_list, d_b_off: S + 1 offsets, as the grouped
// route makes them) as query rows.  Row s of d_slab (slab_stride bytes apart, a multiple of 16) <- the centroid of list s converted to
// the handle's element type, zero padded; d_centroids (optional): row d_entry[s] of d floats <- the centroid itself.  An empty list
// gives zeros.  `pieces`: centroid_chunk_pieces of the lists; d_scratch: CentroidScratch(S, pieces, centroid_row_sums(ix.dbytes, ix.esize)).bytes
// bytes, 256-byte aligned (grouped_plan.h).
int centroid_rows_dev(const DeviceIndex& ix, hipStream_t st, const uint32_t* d_list, const uint64_t* d_b_off, uint32_t S, uint64_t pieces,
                      void* d_scratch, const uint32_t* d_entry, uint8_t* d_slab, uint32_t slab_stride, float* d_centroids);
// grouped labeled search: d_out_preds[q] = d_table[d_group[q]] and d_out_starts[q * nstarts ..] = row d_group[q] (row 0 with
// start_rows == 1) of d_starts, q < nq.  A table index >= G reads no table: a predicate that allows nothing, start row 0, and
// *d_flag (zeroed here) is raised.  raise_status_dev: *d_status |= bit if *d_flag.
int group_rows_dev(const pann_label_pred* d_table, uint32_t G, int kind, const uint32_t* d_group, uint64_t nq, const uint32_t* d_starts,
                   uint32_t nstarts, uint32_t start_rows, pann_label_pred* d_out_preds, uint32_t* d_out_starts, uint32_t* d_flag, hipStream_t st);
int raise_status_dev(const uint32_t* d_flag, uint32_t bit, uint32_t* d_status, hipStream_t st);
// every id of d_ids[0 .. count) that is padding (0xFFFFFFFF) <- fill_id
int pad_fill_dev(uint32_t* d_ids, uint64_t count, uint32_t fill_id, hipStream_t st);

// subset.hip: the kernels of pann_index_create_subset* (DESIGN.md "Subset index").  d_new_to_old: the m kept ids, ascending
// (allow_compact_scatter_dev); every call is a no-op for m == 0 apart from the fill of subset_invert_dev.
// d_a[r] = d_b[r] = r, r < m (either may be null): the two maps when everything is kept
int subset_iota_dev(uint32_t* d_a, uint32_t* d_b, uint64_t m, hipStream_t st);
// d_old_to_new (n words) <- 0xFFFFFFFF, then d_old_to_new[d_new_to_old[r]] = r
int subset_invert_dev(const uint32_t* d_new_to_old, uint64_t m, uint32_t* d_old_to_new, uint64_t n, hipStream_t st);
// row r of d_dst <- row d_new_to_old[r] of d_src, r < m; rows of row_bytes bytes, dense: 4, or a multiple of 16 (16-byte aligned)
int subset_gather_rows_dev(const void* d_src, void* d_dst, uint32_t row_bytes, const uint32_t* d_new_to_old, uint64_t m, hipStream_t st);
// graph row r of d_dst_graph <- row d_new_to_old[r] of d_src_graph (n rows of gstride words) without the neighbours that
// d_old_to_new drops, the others mapped through it, in row order, packed at the front, SENTINEL behind them
int subset_renumber_graph_dev(const uint32_t* d_src_graph, uint32_t* d_dst_graph, uint32_t gstride, const uint32_t* d_new_to_old,
                              const uint32_t* d_old_to_new, uint64_t n, uint64_t m, hipStream_t st);

// graph_reach.hip: the kernels of pann_graph_reach* / pann_graph_degrees* (DESIGN.md "Graph reachability").  Only ix.graph,
// ix.gstride and ix.n are read.  d_visited: ceil(n / 32) words, zeroed by the caller; d_queue: n words; a counter is one word.
constexpr uint32_t REACH_GROUP = 8;      // rounds enqueued back to back between two read-backs of the frontier lengths
// every start below n that is not yet in d_visited enters it and d_queue (tail *d_qlen); a start >= n raises *d_flag instead
int reach_seed_dev(const uint32_t* d_starts, uint32_t nstarts, uint64_t n, uint32_t* d_visited, uint32_t* d_queue, uint32_t* d_qlen,
                   uint32_t* d_flag, hipStream_t st);
// d_level[d_queue[i]] = 0, i < *d_qlen: the level of the seeds, once the flag has come back clear
int reach_level0_dev(const uint32_t* d_queue, const uint32_t* d_qlen, uint64_t n, uint32_t* d_level, hipStream_t st);
// one round: every undiscovered neighbour of d_queue_in[0 .. *d_len_in) enters d_visited and d_queue_out (tail *d_len_out,
// zeroed by the caller) exactly once and, with d_level != null, gets level `next_level`.  *d_len_in == 0: a no-op.
int reach_expand_dev(const DeviceIndex& ix, const uint32_t* d_queue_in, const uint32_t* d_len_in, uint32_t* d_queue_out,
                     uint32_t* d_len_out, uint32_t* d_visited, uint32_t* d_level, uint32_t next_level, hipStream_t st);
// d_unreached[w] = ~d_visited[w] & d_consider[w] (null: all ones), bits at positions >= n cleared
int reach_finish_dev(const uint32_t* d_visited, const uint32_t* d_consider, uint64_t n, uint32_t* d_unreached, hipStream_t st);
// d_out_deg / d_in_deg (n words each, either may be null); d_in_deg is zero-filled here, on st
int graph_degrees_dev(const DeviceIndex& ix, uint32_t* d_out_deg, uint32_t* d_in_deg, hipStream_t st);

// leaf_knn.hip: lane-owns-row all-pairs top-m for one-byte element types (HCNNG leaves)
bool dense_gt_eligible(const DeviceIndex& ix, uint32_t m, bool b_ids, bool segmented, int exclude_same);
uint32_t dense_gt_slots(const DeviceIndex& ix, uint32_t m);
bool leaf_knn_rows_eligible(const DeviceIndex& ix, uint32_t m);
int leaf_knn_rows_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint32_t* d_ids, const uint64_t* d_off,
                      const uint64_t* h_off, uint64_t nseg, uint32_t m, int exclude_same, uint32_t* d_out_ids, float* d_out_dists);

// filter_codes.hip
int filter_codes_build_ranks(uint64_t n, uint32_t bits, Workspace& ws, hipStream_t st, uint16_t* rank16, uint32_t* max_rank_out);
int filter_codes_rebuild_rows(const DeviceIndex& ix, hipStream_t st);

// range_search.hip
int range_search_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint8_t* d_q, uint64_t q_stride,
                     const uint32_t* d_qids, uint64_t nq, const uint32_t* d_starts, uint32_t nstarts,
                     int starts_per_query, float radius_2, uint32_t cap, uint32_t* d_out_ids, uint32_t* d_out_counts,
                     uint32_t* d_out_cmps, uint32_t* d_out_trunc);

// range_gt.hip: dense radius join (every point within `radius` of every external query, CSR, ids ascending).  Two calls that
// share `ws`: count (pass 1 + scan -> d_offsets, nq + 1 entries) and fill (pass 2 -> d_out_ids); nothing else may use ws between.
uint32_t range_join_pieces(const DeviceIndex& ix, uint64_t nq, uint32_t wanted);
int range_join_count_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint8_t* d_q, uint64_t q_stride, uint64_t nq,
                         float radius, uint32_t nsplit, uint64_t* d_offsets);
int range_join_fill_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint8_t* d_q, uint64_t q_stride, uint64_t nq,
                        float radius, uint32_t nsplit, uint32_t* d_out_ids);

// quantize.hip: scalar quantisation of f32 rows (n rows of d floats, row stride in bytes, a multiple of 4)
size_t quant_scratch_bytes();                                     // device scratch quant_params_dev needs
void quant_select_ranks(uint64_t len, int trim, uint64_t* a, uint64_t* b);
int quant_params_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, int kind, int trim, pann_quant_params* out,
                     void* scratch, hipStream_t st);               // synchronises st (reads a few words back)
int quant_translate_dev(const pann_quant_params* p, const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, void* d_out,
                        uint64_t out_stride, hipStream_t st);
// p == nullptr: normalised f32 rows to d_out (may be d_rows: in place); else normalise and translate, bytes to d_out
int quant_normalize_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, const pann_quant_params* p, void* d_out,
                        uint64_t out_stride, hipStream_t st);

int quant_select_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, uint64_t rank_a, uint64_t rank_b, float* val_a,
                     float* val_b, void* scratch, hipStream_t st);  // values at two sorted positions; synchronises st

// sketch.hip: bit sketches of f32 rows
bool sketch_kind_ok(int kind);
uint32_t sketch_row_bytes(int kind, uint32_t d);                  // the reference's num_bytes()
uint32_t sketch_dev_stride(int kind, uint32_t d);                 // ... padded to a multiple of 16
void sketch_select_ranks(uint64_t len, int kind, uint64_t* a, uint64_t* b);
int sketch_params_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, int kind, pann_sketch_params* out, void* scratch,
                      hipStream_t st);                            // synchronises st
// out_row_bytes (a multiple of 8, >= sketch_row_bytes) are written per row: the row's words, then zeros
int sketch_translate_dev(const pann_sketch_params* p, const float* d_rows, uint64_t n, uint64_t stride, void* d_out, uint64_t out_stride,
                         uint32_t out_row_bytes, hipStream_t st);

float sketch_threshold(const pann_sketch_params* p);               // the value a coordinate is compared with (0 for MIPS_BIT)

// search_rerank.hip: beam_search_rerank on the device -- prepare the float queries (one-byte rows, sketch rows, normalised
// rows), beam search on the one-byte index, exact rerank of the frontier on the f32 index.  `scratch`: search_rerank_scratch_bytes
// bytes, 256-byte aligned; search_ws: the one-byte handle's search workspace (its status word gets the SHORT_FRONTIER bit).
// Masked form (r.filter given, with its two optional outputs of nq entries; DESIGN.md "Masked search on the fused path"):
// the search is the masked one with a result list of masked_rerank_pool(qp) ids per query, the rerank reads that list (result_count
// entries) instead of the frontier, raises no SHORT_FRONTIER, and the scratch is sized with the pool in place of the beam.
inline uint32_t masked_rerank_pool(const pann_query_params* qp) {   // min(k * rerank_factor, beam, 64), at least 1
  const int64_t want = std::max<int64_t>((int64_t)qp->k * qp->rerank_factor, 1);
  return (uint32_t)std::min<int64_t>(std::min<int64_t>(want, std::max<int64_t>(qp->beam, 1)), 64);
}
size_t search_rerank_scratch_bytes(const DeviceIndex& quant, uint64_t nq, uint32_t beam, int normalize_first, int use_filter);
// r: the request of the queries to launch (device pointers, r.dcap set); sparams: the parameters of quant's sketch (use_filter)
size_t search_rerank_ws_bytes(const DeviceIndex& quant, const RerankCall& r);      // of the search workspace, by the same request
int search_rerank_dev(const DeviceIndex& full, const DeviceIndex& quant, const Workspace& search_ws, void* scratch,
                      const pann_sketch_params* sparams, const RerankCall& r);

// hcnng_build.hip
int hcnng_build_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, uint32_t num_clusters, uint32_t cluster_size,
                    uint32_t mst_deg, uint64_t seed, double* times3, uint32_t first_tree = 0, uint32_t tree_step = 1,
                    uint32_t* slab = nullptr, uint32_t slab_stride = 0);
int hcnng_assemble_dev(const DeviceIndex& ix, hipStream_t st, const uint32_t* d_slabs, uint32_t W, uint32_t slab_stride,
                       uint32_t ntrees, uint32_t mst_deg);

}  // namespace pann
