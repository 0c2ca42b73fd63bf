// search_call.h -- what a call of the search family asks for, as data: the launch arguments of one beam search (SearchArgs), the point
// filter (PointFilter), the request of a beam-search entry point (SearchCall) and of a fused search + rerank entry point (RerankCall),
// and the ONE function that turns a request into launch arguments: slice().  Every entry point of api.hip fills a request by field
// name; the host path restates it on the staged copies and slices that per launch.  No HIP and nothing of pann_internal.h in here:
// tests/test_search_call_cpu.py builds it with a plain host compiler, under sanitizers, and checks the slice arithmetic there.
#pragma once
#include <stdint.h>
#include "../../include/pann.h"
#include "search_plan.h"

namespace pann {

struct SearchArgs {  // one batched beam search, everything device resident
  const uint8_t* queries; uint64_t qstride;  // external queries (or null)
  const uint32_t* query_ids;                 // base-point queries (or null)
  uint64_t nq;
  const uint32_t* starts; uint32_t nstarts;
  int starts_per_query = 0;                  // starts is nq x nstarts (beamSearchRandom)
  int64_t k, beam, limit, degree_limit; double cut;
  uint32_t dcap = 256;                       // dropped-list entries per query (pann_index_reserve_dropped)
  const uint32_t* order = nullptr;           // device, nq entries: launch slot -> query index (a permutation); null = identity
  pann_search_out out;
  // second level (filtered_beam_search with use_filtering): the handle's sketch decides which neighbours get a full distance
  int filter = 0;
  const uint8_t* sketch_queries = nullptr;   // nq host-layout sketch rows (external queries); base-point queries use their own row
  uint64_t sq_stride = 0;
  uint32_t* pruned_cmps = nullptr;           // nq, optional: the reference's local dist_cmps (starts + sum of pruned.size())
  // masked search (DESIGN.md "Masked search"): same traversal, out.ids/dists = the best allowed points that were compared
  int masked = 0;                            // MASK_NONE / MASK_BITMAP / MASK_LABELS
  const uint32_t* allow = nullptr;           // ceil(n / 32) words per row: point i allowed iff bit i & 31 of word i >> 5
  uint64_t allow_stride = 0;                 // words between the rows of two queries; 0: one bitmap for the batch
  uint32_t* result_count = nullptr;          // nq, optional: entries of the query's result list (<= out.out_k)
  uint32_t* allowed_cmps = nullptr;          // nq, optional: full distances computed for allowed points
  // MASK_LABELS (DESIGN.md "Label predicates"): point i allowed iff the query's predicate holds on labels[i]
  const uint32_t* labels = nullptr;          // n words; not necessarily the searched handle's own (the fused path reads `full`'s)
  const pann_label_pred* preds = nullptr;    // query q reads preds[q * pred_stride]
  uint32_t pred_stride = 0;                  // 0: one predicate for the batch, 1: one per query
  int pred_kind = 0;                         // PANN_PRED_*
  // steered form of a masked search (DESIGN.md "Steered masked search"): pruned = allowed neighbours + allowed neighbours of bridges
  int steer = 0; uint32_t fill = 0;          // fill: the two-hop pass stops at this many entries; 0 or above deg_eff: deg_eff
  uint32_t* steer_out = nullptr;             // nq x 2, optional: bridge_rows, hop2_cmps
};

// Which points a query may return: what every masked / labeled / grouped entry point builds once from its C arguments and
// everything behind it takes.  allow / preds / group are host or device pointers, as the entry point's other pointers (`dev`);
// labels is the device array of the handle whose labels are read.  Only the filter: the optional outputs of the masked
// searches (result_count, allowed_cmps) travel beside it, in the request.
struct PointFilter {
  enum { SHARED, PER_QUERY, TABLE };    // one filter for the batch | one per query | `count` table entries, query q uses entry group[q]
  int mode = MASK_NONE, layout = SHARED;      // MASK_BITMAP: rows of `allow`; MASK_LABELS: `preds` of one `kind` over `labels`
  uint64_t count = 1;                   // filters given, as the caller said it (the checks hold it against nq): 1, nq, or the table's entries
  const uint32_t* allow = nullptr; uint64_t stride = 0;      // bitmap rows, as SearchArgs::allow; words between two rows (0: one row)
  const uint32_t* labels = nullptr; int kind = 0; const pann_label_pred* preds = nullptr;
  const uint32_t* group = nullptr; bool dev = false;      // group: nq entries of a TABLE
  static PointFilter bitmap(const uint32_t* allow, uint64_t stride, uint64_t nq, bool dev) {      // a stride makes one row per query, even at nq == 1
    PointFilter f; f.mode = MASK_BITMAP; f.allow = allow; f.stride = stride; f.dev = dev;
    if (stride) { f.layout = PER_QUERY; f.count = nq; }
    return f;
  }
  PointFilter as_table(const uint32_t* group_of_query, uint64_t entries) const {
    PointFilter f = *this; f.layout = TABLE; f.count = entries; f.group = group_of_query; return f;
  }
  bool given() const { return mode != MASK_NONE; }
  bool shared() const { return layout == SHARED; }
  bool per_query() const { return layout == PER_QUERY; }
  bool is_table() const { return layout == TABLE; }
  static uint64_t row_words(uint64_t n) { return (n + 31) / 32; }
  PointFilter slice(uint64_t q0, uint64_t cnt) const {      // the filter of the queries [q0, q0 + cnt) (a shared one is its own slice)
    PointFilter f = *this;
    if (per_query()) { f.count = cnt; if (allow) f.allow += q0 * stride; if (preds) f.preds += q0; }
    return f;
  }
  void apply(SearchArgs& a) const {     // (a.result_count / a.allowed_cmps: slice() places them)
    a.masked = mode; a.allow = allow; a.allow_stride = stride;
    a.labels = labels; a.preds = preds; a.pred_stride = mode == MASK_LABELS && per_query() ? 1u : 0u; a.pred_kind = kind;
  }
};

// The request of a beam-search entry point, in the caller's words.  All pointers are host pointers or all are device pointers (`dev`;
// qp and the structs themselves are always the host's).  An optional part that was not asked for keeps its defaults.
struct SearchCall {
  enum { STARTS_SHARED, STARTS_PER_QUERY, STARTS_TABLE };      // one row of nstarts ids | nq rows | start_rows rows, query q starts from row group[q]
  const void* queries = nullptr; uint64_t qstride = 0;       // external query rows, qstride bytes apart, or ...
  const uint32_t* query_ids = nullptr; uint64_t nq = 0;      // ... base points as queries
  const uint32_t* starts = nullptr; uint32_t nstarts = 0; int starts_layout = STARTS_SHARED; uint64_t start_rows = 1;
  const pann_query_params* qp = nullptr;
  bool has_out = false; pann_search_out out{};               // set_out(): the caller's struct by value, and whether there was one
  bool sketch = false; const void* sketch_queries = nullptr; uint64_t sq_stride = 0; uint32_t* pruned_cmps = nullptr;      // second level
  PointFilter filter; uint32_t* result_count = nullptr, *allowed_cmps = nullptr;      // masked / labeled / grouped: filter.given()
  bool steer = false; uint32_t fill = 0; uint32_t* steer_out = nullptr;               // steered form of a masked call
  bool dev = false; void* stream = nullptr;                  // device pointers, and the hipStream_t the call is enqueued on
  void set_out(const pann_search_out* o) { has_out = o != nullptr; if (o) out = *o; }
  uint64_t start_count() const {      // ids behind `starts`
    return starts_layout == STARTS_TABLE ? start_rows * nstarts : starts_layout == STARTS_PER_QUERY ? nq * nstarts : (uint64_t)nstarts;
  }
};

inline void fill_search_params(SearchArgs& a, const pann_query_params* qp) {
  a.k = qp->k; a.beam = qp->beam; a.limit = qp->limit; a.degree_limit = qp->degree_limit; a.cut = qp->cut;
}

template <typename T> inline T* offset_or_null(T* p, uint64_t elements) { return p ? p + elements : nullptr; }      // an array that was not asked for stays null

// The launch arguments of the queries [q0, q0 + cnt) of a request whose pointers are device pointers, with a dropped list of dcap
// entries per query: a _dev entry is slice(c, 0, c.nq, dcap of the handle), the host path slices its staged request per launch.
// Shared starts, a shared filter and the status word do not move with q0; starts in a table have been gathered per query before.
inline SearchArgs slice(const SearchCall& c, uint64_t q0, uint64_t cnt, uint32_t dcap) {
  SearchArgs a;
  a.queries = offset_or_null((const uint8_t*)c.queries, q0 * c.qstride); a.qstride = c.qstride;
  a.query_ids = offset_or_null(c.query_ids, q0);
  a.nq = cnt;
  a.starts_per_query = c.starts_layout == SearchCall::STARTS_PER_QUERY;
  a.starts = a.starts_per_query ? offset_or_null(c.starts, q0 * c.nstarts) : c.starts; a.nstarts = c.nstarts;
  fill_search_params(a, c.qp);
  a.dcap = dcap;
  const uint64_t ok = c.out.out_k, vc = c.out.visited_cap;
  a.out = c.out;
  a.out.ids = offset_or_null(c.out.ids, q0 * ok); a.out.dists = offset_or_null(c.out.dists, q0 * ok);
  a.out.frontier_size = offset_or_null(c.out.frontier_size, q0); a.out.visited_count = offset_or_null(c.out.visited_count, q0);
  a.out.dist_cmps = offset_or_null(c.out.dist_cmps, q0); a.out.degree_sum = offset_or_null(c.out.degree_sum, q0);
  a.out.visited_ids = offset_or_null(c.out.visited_ids, q0 * vc); a.out.visited_dists = offset_or_null(c.out.visited_dists, q0 * vc);
  a.filter = c.sketch;
  a.sketch_queries = offset_or_null((const uint8_t*)c.sketch_queries, q0 * c.sq_stride); a.sq_stride = c.sq_stride;
  a.pruned_cmps = offset_or_null(c.pruned_cmps, q0);
  if (c.filter.given()) {
    c.filter.slice(q0, cnt).apply(a);
    a.result_count = offset_or_null(c.result_count, q0); a.allowed_cmps = offset_or_null(c.allowed_cmps, q0);
  }
  if (c.steer) { a.steer = 1; a.fill = c.fill; a.steer_out = offset_or_null(c.steer_out, 2 * q0); }
  return a;
}

// The request of a fused search + rerank entry point (search_rerank.hip): the float queries are quantised with qparams, searched on
// `quant` and the list is rescored on `full`.  slice() is the request of the queries [q0, q0 + cnt), as SearchCall's.
struct RerankCall {
  pann_index* full = nullptr, *quant = nullptr; const pann_quant_params* qparams = nullptr;
  const float* queries = nullptr; uint64_t nq = 0, qstride = 0;
  int normalize_first = 0, use_filter = 0;
  const uint32_t* starts = nullptr; uint32_t nstarts = 0;      // one row for the batch
  const pann_query_params* qp = nullptr;
  bool has_out = false; pann_rerank_out out{};
  PointFilter filter; uint32_t* result_count = nullptr, *allowed_cmps = nullptr;      // masked / labeled: filter.given()
  bool dev = false; void* stream = nullptr;
  const char* fn = "";                 // the entry point, for the messages
  uint32_t dcap = 0;                   // of a slice only: the dropped-list entries per query of the launch it was cut for (slice() sets it)
  void set_out(const pann_rerank_out* o) { has_out = o != nullptr; if (o) out = *o; }
  RerankCall slice(uint64_t q0, uint64_t cnt, uint32_t dropped_cap) const {
    RerankCall r = *this;
    const uint64_t k = (uint64_t)qp->k;
    r.queries = (const float*)offset_or_null((const uint8_t*)queries, q0 * qstride); r.nq = cnt; r.dcap = dropped_cap;
    r.out.ids = offset_or_null(out.ids, q0 * k); r.out.dists = offset_or_null(out.dists, q0 * k);
    r.out.frontier_size = offset_or_null(out.frontier_size, q0); r.out.visited_count = offset_or_null(out.visited_count, q0);
    r.out.dist_cmps = offset_or_null(out.dist_cmps, q0); r.out.pruned_cmps = offset_or_null(out.pruned_cmps, q0);
    if (filter.given()) r.filter = filter.slice(q0, cnt);
    r.result_count = offset_or_null(result_count, q0); r.allowed_cmps = offset_or_null(allowed_cmps, q0);
    return r;
  }
};

}  // namespace pann
