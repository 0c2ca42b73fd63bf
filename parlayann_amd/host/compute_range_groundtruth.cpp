// compute_range_groundtruth.cpp -- the tool of data_tools/compute_range_groundtruth.cpp (flags :91-101) over the C-ABI: every
// base point within distance r of every query by brute force on the device (pann_bruteforce_range), written in the layout of
// write_rangeres (:64-88): [nq:i32][num_matches:i32][sizes nq x i32][ids num_matches x i32], the ids of a query ascending.
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "device_index.h"

using namespace parlayANN;

struct Args {
  std::map<std::string, std::string> kv;
  Args(int argc, char** argv) { for (int i = 1; i + 1 < argc; i += 2) kv[argv[i]] = argv[i + 1]; }
  const char* str(const char* k) const { auto it = kv.find(k); return it == kv.end() ? nullptr : it->second.c_str(); }
  long num(const char* k, long d) const { auto s = str(k); return s ? atol(s) : d; }
  double dbl(const char* k, double d) const { auto s = str(k); return s ? atof(s) : d; }
};

template <class Point>
int run(const Args& a, float r) {
  using PR = PointRange<Point>;
  PR Base(a.str("-base_path")), Queries(a.str("-query_path"));
  if (Base.dimension() != Queries.dimension()) { std::cout << "Error: base and query dimensions differ" << std::endl; abort(); }
  DeviceIndex<PR, unsigned int> DI(Base, nullptr, 1, (int)a.num("-device", 0));
  const size_t nq = Queries.size();
  std::vector<uint64_t> off(nq + 1, 0);
  pann_check(pann_bruteforce_range(DI.h, Queries.data(), nq, Queries.get_aligned_bytes(), r, off.data(), nullptr, 0));
  const uint64_t num_matches = off[nq];
  if (num_matches >= (1ull << 31) || nq >= (1ull << 31)) {      // the header is two 32-bit ints (:75)
    std::cout << "Error: " << num_matches << " matches do not fit the range ground-truth format (32-bit header)" << std::endl;
    abort();
  }
  std::vector<uint32_t> ids((size_t)num_matches);
  if (num_matches) pann_check(pann_bruteforce_range(DI.h, Queries.data(), nq, Queries.get_aligned_bytes(), r, off.data(), ids.data(), ids.size()));
  std::cout << "Done computing groundtruth" << std::endl;
  std::cout << "File contains range groundtruth for " << nq << " data points" << std::endl;
  std::cout << "Number of nonzero matches: " << num_matches << std::endl;
  std::ofstream w(a.str("-gt_path"), std::ios::binary | std::ios::out);
  if (!w.is_open()) { std::cout << "Error: cannot open " << a.str("-gt_path") << std::endl; abort(); }
  const int32_t hdr[2] = {(int32_t)nq, (int32_t)num_matches};
  std::vector<int32_t> sizes(nq);
  for (size_t i = 0; i < nq; i++) sizes[i] = (int32_t)(off[i + 1] - off[i]);
  w.write((const char*)hdr, 8);
  w.write((const char*)sizes.data(), (std::streamsize)(nq * 4));
  w.write((const char*)ids.data(), (std::streamsize)(ids.size() * 4));
  return 0;
}

int main(int argc, char** argv) {
  Args a(argc, argv);
  if (!a.str("-base_path") || !a.str("-query_path") || !a.str("-gt_path") || !a.str("-data_type") || !a.str("-dist_func")) {
    std::cout << "usage: compute_range_groundtruth -base_path <b> -query_path <q> -data_type <d> -r <r> -dist_func <d> -gt_path <outfile>" << std::endl;
    return 1;
  }
  const std::string df = a.str("-dist_func"), tp = a.str("-data_type");
  if (df != "Euclidian" && df != "mips") { std::cout << "Error: invalid distance type: specify Euclidian or mips" << std::endl; abort(); }
  if (tp != "uint8" && tp != "int8" && tp != "float") { std::cout << "Error: data type not specified correctly, specify int8, uint8, or float" << std::endl; abort(); }
  const float r = (float)a.dbl("-r", 0);
  std::cout << "Computing the groundtruth for radius " << r << std::endl;
  const bool mips = df == "mips";
  if (tp == "uint8") return mips ? run<Mips_Point<uint8_t>>(a, r) : run<Euclidian_Point<uint8_t>>(a, r);
  if (tp == "int8") return mips ? run<Mips_Point<int8_t>>(a, r) : run<Euclidian_Point<int8_t>>(a, r);
  return mips ? run<Mips_Point<float>>(a, r) : run<Euclidian_Point<float>>(a, r);
}
