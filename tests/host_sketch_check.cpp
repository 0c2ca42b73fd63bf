// host_sketch_check.cpp -- a test TU that runs the two-level search of the C++ host mirror with the REFERENCE's argument lists
// (the three-range beam_search_rerank, beamSearch.h:390-454; the 10-argument qsearchAll, :537-565; filtered_beam_search with
// use_filtering, :22-33) on sketch ranges made by the translating PointRange constructor (point_range.h:54-72), and dumps what
// comes back as little-endian arrays in <outdir>/<name>.bin; tests/test_host_sketch_gpu.py compares every array with the Python
// composition.  usage: host_sketch_check <base.fbin> <query.fbin> <graph> <outdir> <l2|mips> <bit|2bit> <k> <beam> <rerank_factor>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../parlayann_amd/host/beam_search.h"
#include "../parlayann_amd/host/quantize.h"
#include "../parlayann_amd/host/sketch.h"

using namespace parlayANN;
using indexType = unsigned int;

static std::string g_out;
template <typename T>
static void dump(const std::string& name, const std::vector<T>& v) {
  FILE* f = std::fopen((g_out + "/" + name + ".bin").c_str(), "wb");
  if (!f) { std::printf("cannot write %s\n", name.c_str()); std::abort(); }
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
}
template <class R>
static std::vector<uint8_t> rows_of(const R& pr) {
  const size_t nb = (size_t)pr.params.num_bytes();
  std::vector<uint8_t> o(pr.size() * nb);
  for (size_t i = 0; i < pr.size(); i++) std::memcpy(o.data() + i * nb, pr.location((long)i), nb);
  return o;
}

template <class PR, class QPR, class QQPR>
static void run(PR& Points, PR& Query_Points, QPR& Q_Points, QPR& Q_Query_Points, Graph<indexType>& G, long k, long beam, int rf) {
  QQPR QQ_Points(Points);                                   // generate_parameters + translate_point
  QQPR QQ_Query_Points(Query_Points, QQ_Points.params);
  if (QQPR::Point::is_metric()) { std::printf("sketch points are not metric\n"); std::abort(); }
  dump("qq_median", std::vector<int64_t>{(int64_t)QQ_Points.params.median});
  dump("qq_cut", std::vector<float>{QQ_Points.params.cut});
  dump("qq_num_bytes", std::vector<int32_t>{QQ_Points.params.num_bytes()});
  dump("qq_base_rows", rows_of(QQ_Points));
  dump("qq_query_rows", rows_of(QQ_Query_Points));

  const long n = (long)Points.size();
  QueryParams QP(k, beam, 1.35, n, G.max_degree());
  QP.rerank_factor = rf;
  parlay::sequence<indexType> starts = {0};

  // ---- beam_search_rerank(p, qp, qqp, G, Base_Points, Q_Base_Points, QQ_Base_Points, QueryStats, starting_points, QP, stats) ----
  {
    stats<indexType> QS(Query_Points.size());
    std::vector<uint32_t> ids; std::vector<float> ds;
    for (size_t i = 0; i < Query_Points.size(); i++) {
      auto r = beam_search_rerank(Query_Points[(long)i], Q_Query_Points[(long)i], QQ_Query_Points[(long)i], G, Points, Q_Points, QQ_Points,
                                  QS, starts, QP, true);
      for (auto& p : r) { ids.push_back(p.first); ds.push_back(p.second); }
    }
    dump("rerank3_ids", ids); dump("rerank3_dists", ds); dump("rerank3_visited", QS.visited); dump("rerank3_cmps", QS.distances);
  }
  // ---- qsearchAll with a QQ range: ONE filtered launch for the batch ----
  {
    stats<indexType> QS(Query_Points.size());
    std::vector<float> dd;
    auto all = qsearchAll<PR, QPR, QQPR, indexType>(Query_Points, Q_Query_Points, QQ_Query_Points, G, Points, Q_Points, QQ_Points, QS,
                                                    (indexType)0, QP, &dd);
    std::vector<uint32_t> ids;
    for (auto& r : all) ids.insert(ids.end(), r.begin(), r.end());
    dump("qsearch3_ids", ids); dump("qsearch3_dists", dd); dump("qsearch3_visited", QS.visited); dump("qsearch3_cmps", QS.distances);
  }
  // ---- filtered_beam_search(G, p, Points, qp, Q_Points, starting_points, QP, use_filtering = true): external and base-point query ----
  for (int form = 0; form < 2; form++) {
    auto r = form == 0 ? filtered_beam_search(G, Q_Query_Points[2], Q_Points, QQ_Query_Points[2], QQ_Points, starts, QP, true)
                       : filtered_beam_search(G, Q_Points[77], Q_Points, QQ_Points[77], QQ_Points, starts, QP, true);
    const std::string name = form == 0 ? "fbs_ext" : "fbs_base";
    std::vector<uint32_t> fi, vi; std::vector<float> fd, vd;
    for (auto& p : r.first.first) { fi.push_back(p.first); fd.push_back(p.second); }
    for (auto& p : r.first.second) { vi.push_back(p.first); vd.push_back(p.second); }
    dump(name + "_frontier_ids", fi); dump(name + "_frontier_dists", fd); dump(name + "_visited_ids", vi); dump(name + "_visited_dists", vd);
    dump(name + "_cmps", std::vector<uint64_t>{(uint64_t)r.second});
  }
}

int main(int argc, char** argv) {
  if (argc < 10) { std::printf("usage: host_sketch_check base query graph outdir l2|mips bit|2bit k beam rerank_factor\n"); return 2; }
  g_out = argv[4];
  const std::string metric = argv[5], level = argv[6];
  const long k = std::atol(argv[7]), beam = std::atol(argv[8]);
  const int rf = std::atoi(argv[9]);
  Graph<indexType> G(argv[3]);
  if (metric == "l2") {
    using PR = PointRange<Euclidian_Point<float>>;
    using QPR = PointRange<Euclidian_Point<uint8_t>>;
    PR Points(argv[1]), Query_Points(argv[2]);
    const euclid_u8_parameters pm = generate_parameters_u8(Points);
    QPR Q_Points = quantize_u8(Points, pm), Q_Query_Points = quantize_u8(Query_Points, pm);
    run<PR, QPR, PointRange<Euclidean_Bit_Point>>(Points, Query_Points, Q_Points, Q_Query_Points, G, k, beam, rf);
  } else {
    using PR = PointRange<Mips_Point<float>>;
    using QPR = PointRange<Mips_Point<int8_t>>;
    PR Points(argv[1]), Query_Points(argv[2]);
    const float mv = generate_max_val_mips_i8(Points, true);
    QPR Q_Points = quantize_mips_i8(Points, mv), Q_Query_Points = quantize_mips_i8(Query_Points, mv);
    if (level == "2bit") run<PR, QPR, PointRange<Mips_2Bit_Point>>(Points, Query_Points, Q_Points, Q_Query_Points, G, k, beam, rf);
    else run<PR, QPR, PointRange<Mips_Bit_Point>>(Points, Query_Points, Q_Points, Q_Query_Points, G, k, beam, rf);
  }
  release_device_mirrors();
  std::printf("host_sketch_check done\n");
  return 0;
}
