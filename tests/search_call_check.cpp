// search_call_check.cpp -- parlayann_amd/csrc/search_call.h on its own, built by a plain host compiler under sanitizers and run by
// tests/test_search_call_cpu.py: the launch arguments that slice() makes of a request, for every form of the search family and the
// query ranges (0, 11) and (5, 3).  A range that does not start at query 0 is launched only when a grown dropped list exceeds its
// budget for the whole batch, which no small GPU run reaches: this is the check of that arithmetic.  The requests are built from fake,
// distinct base addresses (nothing is dereferenced); the expectation is written out below in integers, from the formulae the entry
// points used before there was a request descriptor: rows move by q0 * stride bytes, per-query arrays by q0 (x out_k, x visited_cap,
// x nstarts, x 2 for the steer counters) elements, what is shared or was not asked for does not move.
#include <stdio.h>
#include <stdlib.h>

#include "../parlayann_amd/csrc/search_call.h"

using namespace pann;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, g_case); exit(1); } } while (0)
static const char* g_case = "";

constexpr uint64_t NQ = 11, NSTARTS = 2, OUT_K = 3, VCAP = 7, QSTRIDE = 112 /* a 96-byte row */, ALLOW_STRIDE = 5, SQ_STRIDE = 16, DCAP = 777;
// fake device addresses, 16 MiB apart
enum : uintptr_t { Q = 0x10000000, QID = 0x11000000, ST = 0x12000000, SK = 0x13000000, ALLOW = 0x14000000, PREDS = 0x15000000, LABELS = 0x16000000,
                   IDS = 0x20000000, DISTS = 0x21000000, FS = 0x22000000, VCNT = 0x23000000, CMPS = 0x24000000, DEG = 0x25000000,
                   VIDS = 0x26000000, VDISTS = 0x27000000, STATUS = 0x28000000, PRUNED = 0x29000000, RCNT = 0x2A000000, ACMPS = 0x2B000000,
                   STEER = 0x2C000000 };
template <typename T> static T* at(uintptr_t addr) { return reinterpret_cast<T*>(addr); }

enum { NO_MASK, BITMAP, LABELS_MASK };
struct Form {
  const char* name;
  bool ext;             // external queries (else query ids)
  bool per_query_starts, sketch;
  int mask; bool per_query_filter;
  bool steer;
  bool every_output;    // else: ids and the status word alone, every other output null
};
static const Form FORMS[] = {
  {"plain, external queries", true, false, false, NO_MASK, false, false, true},
  {"plain, query ids", false, false, false, NO_MASK, false, false, false},
  {"per-query starts", true, true, false, NO_MASK, false, false, true},
  {"filtered", true, false, true, NO_MASK, false, false, true},
  {"filtered, query ids, no pruned_cmps", false, false, true, NO_MASK, false, false, false},
  {"masked, shared bitmap", true, false, false, BITMAP, false, false, true},
  {"masked, per-query bitmap", true, false, false, BITMAP, true, false, false},
  {"labeled, shared predicate", false, false, false, LABELS_MASK, false, false, true},
  {"labeled, per-query predicates", true, false, false, LABELS_MASK, true, false, true},
  {"steered, per-query bitmap", true, false, false, BITMAP, true, true, true},
  {"steered labeled, shared, no counters", true, false, false, LABELS_MASK, false, true, false},
  {"grouped labeled after the gather", true, true, false, LABELS_MASK, true, true, true},      // a predicate and a start row per query
};

static const pann_query_params QP = {5, 16, 1.35, 40, 8, 2, 1.0f};

static SearchCall request(const Form& f) {
  SearchCall c;
  if (f.ext) { c.queries = at<void>(Q); } else c.query_ids = at<uint32_t>(QID);
  c.qstride = QSTRIDE; c.nq = NQ;
  c.starts = at<uint32_t>(ST); c.nstarts = NSTARTS;
  if (f.per_query_starts) c.starts_layout = SearchCall::STARTS_PER_QUERY;
  c.qp = &QP;
  pann_search_out o{};
  o.ids = at<uint32_t>(IDS); o.out_k = OUT_K; o.visited_cap = VCAP; o.status = at<uint32_t>(STATUS);
  if (f.every_output) {
    o.dists = at<float>(DISTS); o.frontier_size = at<uint32_t>(FS); o.visited_count = at<uint32_t>(VCNT); o.dist_cmps = at<uint32_t>(CMPS);
    o.degree_sum = at<uint32_t>(DEG); o.visited_ids = at<uint32_t>(VIDS); o.visited_dists = at<float>(VDISTS);
  }
  c.set_out(&o);
  if (f.sketch) {
    c.sketch = true; c.sq_stride = SQ_STRIDE;
    if (f.ext) c.sketch_queries = at<void>(SK);
    if (f.every_output) c.pruned_cmps = at<uint32_t>(PRUNED);
  }
  if (f.mask == BITMAP) c.filter = PointFilter::bitmap(at<uint32_t>(ALLOW), f.per_query_filter ? ALLOW_STRIDE : 0, NQ, true);
  if (f.mask == LABELS_MASK) {
    c.filter.mode = MASK_LABELS; c.filter.labels = at<uint32_t>(LABELS); c.filter.kind = PANN_PRED_RANGE; c.filter.preds = at<pann_label_pred>(PREDS);
    c.filter.dev = true;
    if (f.per_query_filter) { c.filter.layout = PointFilter::PER_QUERY; c.filter.count = NQ; }
  }
  if (f.mask != NO_MASK && f.every_output) { c.result_count = at<uint32_t>(RCNT); c.allowed_cmps = at<uint32_t>(ACMPS); }
  if (f.steer) { c.steer = true; c.fill = 3; if (f.every_output) c.steer_out = at<uint32_t>(STEER); }
  c.dev = true;
  return c;
}

// what the entry points computed by hand for the queries [q0, q0 + cnt)
static SearchArgs expected(const Form& f, uint64_t q0, uint64_t cnt) {
  SearchArgs e;
  e.queries = f.ext ? at<const uint8_t>(Q + q0 * QSTRIDE) : nullptr; e.qstride = QSTRIDE;
  e.query_ids = f.ext ? nullptr : at<const uint32_t>(QID + 4 * q0);
  e.nq = cnt;
  e.starts = at<const uint32_t>(f.per_query_starts ? ST + 4 * q0 * NSTARTS : ST); e.nstarts = NSTARTS; e.starts_per_query = f.per_query_starts ? 1 : 0;
  e.k = 5; e.beam = 16; e.cut = 1.35; e.limit = 40; e.degree_limit = 8;
  e.dcap = DCAP; e.order = nullptr;
  e.out = pann_search_out{};
  e.out.ids = at<uint32_t>(IDS + 4 * q0 * OUT_K); e.out.out_k = OUT_K; e.out.visited_cap = VCAP; e.out.status = at<uint32_t>(STATUS);
  if (f.every_output) {
    e.out.dists = at<float>(DISTS + 4 * q0 * OUT_K); e.out.frontier_size = at<uint32_t>(FS + 4 * q0); e.out.visited_count = at<uint32_t>(VCNT + 4 * q0);
    e.out.dist_cmps = at<uint32_t>(CMPS + 4 * q0); e.out.degree_sum = at<uint32_t>(DEG + 4 * q0);
    e.out.visited_ids = at<uint32_t>(VIDS + 4 * q0 * VCAP); e.out.visited_dists = at<float>(VDISTS + 4 * q0 * VCAP);
  }
  e.filter = f.sketch ? 1 : 0;
  if (f.sketch) {
    e.sketch_queries = f.ext ? at<const uint8_t>(SK + q0 * SQ_STRIDE) : nullptr; e.sq_stride = SQ_STRIDE;
    e.pruned_cmps = f.every_output ? at<uint32_t>(PRUNED + 4 * q0) : nullptr;
  }
  e.masked = f.mask == BITMAP ? MASK_BITMAP : f.mask == LABELS_MASK ? MASK_LABELS : MASK_NONE;
  if (f.mask == BITMAP) { e.allow = at<const uint32_t>(f.per_query_filter ? ALLOW + 4 * q0 * ALLOW_STRIDE : ALLOW); e.allow_stride = f.per_query_filter ? ALLOW_STRIDE : 0; }
  if (f.mask == LABELS_MASK) {
    e.labels = at<const uint32_t>(LABELS); e.pred_kind = PANN_PRED_RANGE;
    e.preds = at<const pann_label_pred>(f.per_query_filter ? PREDS + 8 * q0 : PREDS); e.pred_stride = f.per_query_filter ? 1 : 0;
  }
  if (f.mask != NO_MASK && f.every_output) { e.result_count = at<uint32_t>(RCNT + 4 * q0); e.allowed_cmps = at<uint32_t>(ACMPS + 4 * q0); }
  if (f.steer) { e.steer = 1; e.fill = 3; e.steer_out = f.every_output ? at<uint32_t>(STEER + 4 * 2 * q0) : nullptr; }
  return e;
}

static void check_equal(const SearchArgs& a, const SearchArgs& e) {
  CHECK(a.queries == e.queries); CHECK(a.qstride == e.qstride); CHECK(a.query_ids == e.query_ids); CHECK(a.nq == e.nq);
  CHECK(a.starts == e.starts); CHECK(a.nstarts == e.nstarts); CHECK(a.starts_per_query == e.starts_per_query);
  CHECK(a.k == e.k); CHECK(a.beam == e.beam); CHECK(a.limit == e.limit); CHECK(a.degree_limit == e.degree_limit); CHECK(a.cut == e.cut);
  CHECK(a.dcap == e.dcap); CHECK(a.order == e.order);
  CHECK(a.out.ids == e.out.ids); CHECK(a.out.dists == e.out.dists); CHECK(a.out.out_k == e.out.out_k);
  CHECK(a.out.frontier_size == e.out.frontier_size); CHECK(a.out.visited_count == e.out.visited_count); CHECK(a.out.dist_cmps == e.out.dist_cmps);
  CHECK(a.out.degree_sum == e.out.degree_sum); CHECK(a.out.visited_ids == e.out.visited_ids); CHECK(a.out.visited_dists == e.out.visited_dists);
  CHECK(a.out.visited_cap == e.out.visited_cap); CHECK(a.out.status == e.out.status);
  CHECK(a.filter == e.filter); CHECK(a.sketch_queries == e.sketch_queries); CHECK(a.sq_stride == e.sq_stride); CHECK(a.pruned_cmps == e.pruned_cmps);
  CHECK(a.masked == e.masked); CHECK(a.allow == e.allow); CHECK(a.allow_stride == e.allow_stride);
  CHECK(a.result_count == e.result_count); CHECK(a.allowed_cmps == e.allowed_cmps);
  CHECK(a.labels == e.labels); CHECK(a.preds == e.preds); CHECK(a.pred_stride == e.pred_stride); CHECK(a.pred_kind == e.pred_kind);
  CHECK(a.steer == e.steer); CHECK(a.fill == e.fill); CHECK(a.steer_out == e.steer_out);
}

// the fused call's request: the float rows, the k-wide results and the filter move with q0, the starts do not
static void check_rerank_slice() {
  g_case = "rerank request";
  RerankCall r;
  r.queries = at<float>(Q); r.nq = NQ; r.qstride = QSTRIDE; r.starts = at<uint32_t>(ST); r.nstarts = NSTARTS; r.qp = &QP; r.use_filter = 1;
  pann_rerank_out o{};
  o.ids = at<uint32_t>(IDS); o.dists = at<float>(DISTS); o.visited_count = at<uint32_t>(VCNT); o.status = at<uint32_t>(STATUS);
  r.set_out(&o);
  r.filter = PointFilter::bitmap(at<uint32_t>(ALLOW), ALLOW_STRIDE, NQ, true); r.allowed_cmps = at<uint32_t>(ACMPS);
  const RerankCall s = r.slice(5, 3, DCAP);
  CHECK(s.queries == at<float>(Q + 5 * QSTRIDE)); CHECK(s.nq == 3); CHECK(s.qstride == QSTRIDE); CHECK(s.dcap == DCAP);
  CHECK(s.starts == at<uint32_t>(ST)); CHECK(s.nstarts == NSTARTS); CHECK(s.qp == &QP); CHECK(s.use_filter == 1);
  CHECK(s.out.ids == at<uint32_t>(IDS + 4 * 5 * 5)); CHECK(s.out.dists == at<float>(DISTS + 4 * 5 * 5));      // k = 5
  CHECK(s.out.frontier_size == nullptr); CHECK(s.out.visited_count == at<uint32_t>(VCNT + 4 * 5)); CHECK(s.out.dist_cmps == nullptr);
  CHECK(s.out.pruned_cmps == nullptr); CHECK(s.out.status == at<uint32_t>(STATUS));
  CHECK(s.filter.allow == at<uint32_t>(ALLOW + 4 * 5 * ALLOW_STRIDE)); CHECK(s.filter.count == 3); CHECK(s.filter.stride == ALLOW_STRIDE);
  CHECK(s.result_count == nullptr); CHECK(s.allowed_cmps == at<uint32_t>(ACMPS + 4 * 5));
}

int main() {
  for (const Form& f : FORMS) {
    g_case = f.name;
    const SearchCall c = request(f);
    check_equal(slice(c, 0, NQ, DCAP), expected(f, 0, NQ));
    check_equal(slice(c, 5, 3, DCAP), expected(f, 5, 3));
  }
  // the ids behind `starts`: one row, a row per query, a row per table entry
  SearchCall c = request(FORMS[0]);
  CHECK(c.start_count() == NSTARTS);
  c.starts_layout = SearchCall::STARTS_PER_QUERY; CHECK(c.start_count() == NQ * NSTARTS);
  c.starts_layout = SearchCall::STARTS_TABLE; c.start_rows = 3; CHECK(c.start_count() == 3 * NSTARTS);
  SearchCall none; none.set_out(nullptr); CHECK(!none.has_out && !none.filter.given());
  check_rerank_slice();
  printf("search_call: ok\n");
  return 0;
}
