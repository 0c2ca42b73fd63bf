// check_range_recall.h -- host mirror of algorithms/utils/check_range_recall.h with the reference's argument lists:
//   RangeSearch(Query_Points, G, Base_Points, QueryStats, starting_point(s), RP)       beamSearch.h:567-614
//   checkRangeRecall(G, Base_Points, Query_Points, GT, RP, start_point)                 :17-63
//   range_search_wrapper(G, Base_Points, Query_Points, GT, rad, start_point)            :66-81
// RangeSearch is ONE pann_range_query: the beam search with QueryParams(initial_beam, initial_beam, 0.0, G.size(),
// G.max_degree()) (:587) and, as the second round the reference describes (:243-244, :594-605), the BFS of range_search
// seeded with each query's frontier.  Only the search is timed (:29-34).  Recall counts |reported ∩ truth| per query: the
// reference's ratio of counts (:44-50, "since distances are exact") whenever every reported id is a true match.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>

#include "beam_search.h"

namespace parlayANN {

struct range_result { long beam = 0; float pointwise_recall = 0, cumulative_recall = 0, QPS = 0; long avg_cmps = 0; bool rejected = false; };

template <typename Point, typename PointRange, typename indexType>
parlay::sequence<parlay::sequence<indexType>> RangeSearch(PointRange& Query_Points, Graph<indexType>& G, PointRange& Base_Points,
                                                          stats<indexType>& QueryStats, parlay::sequence<indexType> starting_points,
                                                          RangeParams& RP, long max_results = 0, int* status = nullptr) {
  auto L = device_mirror(G, Base_Points);
  const size_t nq = Query_Points.size();
  QueryParams QP(RP.initial_beam, RP.initial_beam, 0.0, (long)G.size(), G.max_degree());       // :587
  const pann_query_params q = to_pann(QP);
  // a ball holds at most every point; the default leaves room for a few thousand matches per query
  const uint32_t cap = (uint32_t)(max_results > 0 ? max_results : std::min<long>((long)G.size(), 4096));
  std::vector<uint32_t> ids(nq * (size_t)cap), cnt(nq), scmps(nq), vis(nq), rcmps(nq), trunc(nq);
  std::vector<uint32_t> st(starting_points.begin(), starting_points.end());
  const int rc = pann_range_query(L.h(), Query_Points.data(), nullptr, nq, Query_Points.get_aligned_bytes(), st.data(), (uint32_t)st.size(), &q,
                                  (float)RP.rad, cap, ids.data(), cnt.data(), scmps.data(), vis.data(), rcmps.data(), trunc.data());
  if (status) *status = rc;
  if (rc != PANN_OK) {
    if (!status) pann_check(rc);
    return parlay::sequence<parlay::sequence<indexType>>();
  }
  parlay::sequence<parlay::sequence<indexType>> all(nq);
  for (size_t i = 0; i < nq; i++) {
    all[i] = parlay::sequence<indexType>(ids.begin() + i * cap, ids.begin() + i * cap + cnt[i]);
    QueryStats.increment_visited((indexType)i, vis[i]);                                          // :607-608, plus the second round (:603-604)
    QueryStats.increment_dist((indexType)i, scmps[i] + rcmps[i]);
  }
  return all;
}

template <typename Point, typename PointRange, typename indexType>
parlay::sequence<parlay::sequence<indexType>> RangeSearch(PointRange& Query_Points, Graph<indexType>& G, PointRange& Base_Points,
                                                          stats<indexType>& QueryStats, indexType starting_point, RangeParams& RP) {
  parlay::sequence<indexType> start_points = {starting_point};                                   // :572
  return RangeSearch<Point, PointRange, indexType>(Query_Points, G, Base_Points, QueryStats, start_points, RP);
}

template <typename Point, typename PointRange, typename indexType>
range_result checkRangeRecall(Graph<indexType>& G, PointRange& Base_Points, PointRange& Query_Points, RangeGroundTruth<indexType> GT,
                              RangeParams RP, long start_point) {
  range_result res; res.beam = RP.initial_beam;
  stats<indexType> QueryStats(Query_Points.size());
  long widest = 1;                                              // room for the largest true ball: nothing is cut off
  for (size_t i = 0; i < GT.size(); i++) widest = std::max<long>(widest, (long)GT[(long)i].size());
  parlay::sequence<indexType> start_points = {(indexType)start_point};
  int rc = 0;
  const auto t0 = std::chrono::steady_clock::now();
  auto all_rr = RangeSearch<Point, PointRange, indexType>(Query_Points, G, Base_Points, QueryStats, start_points, RP, widest, &rc);
  const double query_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != PANN_OK) {                                          // a beam the library rejects is reported, not dropped
    res.rejected = true;
    std::cout << "For "; RP.print();
    std::cout << ", rejected: " << pann_last_error() << std::endl;
    return res;
  }
  float pointwise_recall = 0.0, reported_results = 0.0, total_results = 0.0, num_nonzero = 0.0;
  const size_t n = Query_Points.size();
  for (size_t i = 0; i < n; i++) {
    auto truth = GT[(long)i];
    std::vector<indexType> rep(all_rr[i].begin(), all_rr[i].end());
    std::sort(rep.begin(), rep.end());
    rep.erase(std::unique(rep.begin(), rep.end()), rep.end());
    float hits = 0;
    for (auto a : rep) if (std::binary_search(truth.begin(), truth.end(), a)) hits++;       // truth rows are ascending
    const float num_actual_results = (float)truth.size();
    reported_results += hits;
    total_results += num_actual_results;
    if (num_actual_results != 0) { pointwise_recall += hits / num_actual_results; num_nonzero++; }
  }
  pointwise_recall /= num_nonzero;
  res.pointwise_recall = pointwise_recall;
  res.cumulative_recall = reported_results / total_results;
  res.QPS = (float)(Query_Points.size() / query_time);
  res.avg_cmps = (long)QueryStats.dist_stats()[0];
  std::cout << "For "; RP.print();
  std::cout << ", Pointwise Recall = " << res.pointwise_recall << ", Cumulative Recall = " << res.cumulative_recall << ", QPS = " << res.QPS
            << ", comparisons = " << res.avg_cmps << std::endl;
  return res;
}

template <typename Point, typename PointRange, typename indexType>
std::vector<range_result> range_search_wrapper(Graph<indexType>& G, PointRange& Base_Points, PointRange& Query_Points,
                                               RangeGroundTruth<indexType> GT, double rad, indexType start_point = 0) {
  std::vector<long> beams = {10, 20, 30, 40, 50, 100, 1000, 2000, 3000};                        // :74
  std::vector<range_result> out;
  for (long b : beams) {
    RangeParams RP(rad, b);
    out.push_back(checkRangeRecall<Point, PointRange, indexType>(G, Base_Points, Query_Points, GT, RP, start_point));
  }
  return out;
}

}  // namespace parlayANN
