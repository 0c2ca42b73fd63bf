// sketch.h -- host mirror of the reference's bit-sketch point types and of their translating PointRange constructor
// (algorithms/utils/point_range.h:54-72), the QQ ranges of the two-level search:
//   Euclidean_Bit_Point  euclidian_point.h:332-420      Mips_Bit_Point  mips_point.h:625-702
//   Mips_2Bit_Point      mips_point.h:495-623
// Same parameters, num_bytes() and is_metric() as upstream.  As everywhere in this mirror no distance is computed on the
// host: parameters and bits come from the device (pann_sketch_params_generate / pann_index_attach_sketch on a temporary f32
// handle for a base range, pann_sketch_rows for a query range), the range holds the host-layout rows, and a search hands them
// to the searched handle with pann_index_upload_sketch.  The mirror promises the reference's observable results, so the
// one-bit kinds run with hamming_as_written = 1 (the reference's distance loop counts block 0 num_blocks times).
#pragma once
#include <atomic>
#include <cstring>
#include <iostream>
#include <memory>

#include "device_mirror.h"
#include "point_range.h"

namespace parlayANN {

template <int KIND, int METRIC>
struct Sketch_Point_ {
  using T = uint8_t;
  using distanceType = float;
  using byte = uint8_t;
  static constexpr int sketch_kind = KIND;
  static constexpr int metric = METRIC;
  struct parameters {
    int dims = 0;
    long median = 0;      // Euclidean_Bit_Point
    float cut = .25f;     // Mips_2Bit_Point
    int num_bytes() const { return ((dims - 1) / 64 + 1) * 8 * (KIND == PANN_SKETCH_MIPS_2BIT ? 2 : 1); }
    parameters() {}
    explicit parameters(int dims) : dims(dims) {}
    pann_sketch_params to_pann() const {
      pann_sketch_params p;
      p.kind = KIND; p.dims = dims; p.median = median; p.cut = cut; p.hamming_as_written = 1;
      return p;
    }
  };
  static bool is_metric() { return false; }
  const byte* values = nullptr;
  long id_ = -1;
  parameters params;
  Sketch_Point_() {}
  Sketch_Point_(const byte* v, long id, parameters p) : values(v), id_(id), params(p) {}
  long id() const { return id_; }
  bool same_as(const Sketch_Point_& q) const { return values == q.values; }
  bool operator==(const Sketch_Point_& q) const { return std::memcmp(values, q.values, (size_t)params.num_bytes()) == 0; }
};
using Euclidean_Bit_Point = Sketch_Point_<PANN_SKETCH_EUCLID_BIT, PANN_L2>;
using Mips_Bit_Point = Sketch_Point_<PANN_SKETCH_MIPS_BIT, PANN_MIPS>;
using Mips_2Bit_Point = Sketch_Point_<PANN_SKETCH_MIPS_2BIT, PANN_MIPS>;

template <class P> struct is_sketch_point { static constexpr bool value = false; };
template <int K, int M> struct is_sketch_point<Sketch_Point_<K, M>> { static constexpr bool value = true; };

// PointRange of sketch points: rows of num_bytes() at a stride of aligned_bytes (64-byte multiples, point_range.h:94)
template <int KIND, int METRIC>
struct PointRange<Sketch_Point_<KIND, METRIC>> {
  using Point = Sketch_Point_<KIND, METRIC>;
  using parameters = typename Point::parameters;
  using byte = uint8_t;
  using T = uint8_t;

  long dimension() const { return dims; }
  size_t size() const { return n; }
  unsigned int get_aligned_bytes() const { return aligned_bytes; }
  const byte* data() const { return values.get(); }
  byte* data() { return values.get(); }
  PointRange() {}

  // QQPR QQ_Points(Points): generate_parameters over the float range, translate_point per row -- both on the device
  template <class FloatRange>
  explicit PointRange(const FloatRange& pr, int device = default_device()) : dims((unsigned int)pr.dimension()), n(pr.size()) {
    static_assert(std::is_same<typename FloatRange::T, float>::value, "sketches are made from float points");
    params = parameters((int)dims);
    allocate();
    if (n == 0) return;
    pann_index* h = nullptr;
    pann_check(pann_index_create(&h, pr.data(), n, dims, PANN_F32, pr.get_aligned_bytes(), METRIC, nullptr, 1, device));
    pann_sketch_params sp;
    pann_check(pann_sketch_params_generate(h, KIND, &sp));
    params.median = (long)sp.median; params.cut = sp.cut;
    if (KIND == PANN_SKETCH_EUCLID_BIT) std::cout << "single-bit quantization with median: " << params.median << std::endl;
    else if (KIND == PANN_SKETCH_MIPS_BIT) std::cout << "single-bit quantization" << std::endl;
    else std::cout << "3-value quantization with cut = " << params.cut << std::endl;
    pann_check(pann_index_attach_sketch(h, h, &sp));
    pann_check(pann_index_download_sketch(h, 0, n, values.get(), aligned_bytes));
    pann_index_destroy(h);
  }
  // QQPR QQ_Query_Points(Query_Points, QQ_Points.params)
  template <class FloatRange>
  PointRange(const FloatRange& pr, const parameters& p, int device = default_device()) : params(p), dims((unsigned int)pr.dimension()), n(pr.size()) {
    static_assert(std::is_same<typename FloatRange::T, float>::value, "sketches are made from float points");
    allocate();
    if (n == 0) return;
    const pann_sketch_params sp = params.to_pann();
    pann_check(pann_sketch_rows(&sp, (const float*)pr.data(), n, pr.get_aligned_bytes(), values.get(), aligned_bytes, device));
  }

  Point operator[](long i) const { return Point(values.get() + (size_t)i * aligned_bytes, i, params); }
  byte* location(long i) const { return values.get() + (size_t)i * aligned_bytes; }
  uint64_t version() const { return version_ ? version_->load(std::memory_order_relaxed) : 0; }
  void touch() const { if (version_) version_->fetch_add(1, std::memory_order_relaxed); }
  const std::shared_ptr<byte[]>& slab_handle() const { return values; }

  parameters params;

 private:
  void allocate() {
    const long nb = params.num_bytes();
    aligned_bytes = (unsigned int)(64 * ((nb - 1) / 64 + 1));
    const size_t total = std::max<size_t>(n * (size_t)aligned_bytes, 64);
    byte* ptr = (byte*)aligned_alloc(64, total);
    std::memset(ptr, 0, total);
    values = std::shared_ptr<byte[]>(ptr, std::free);
    version_ = std::make_shared<std::atomic<uint64_t>>(1);
  }
  std::shared_ptr<byte[]> values;
  std::shared_ptr<std::atomic<uint64_t>> version_;
  unsigned int dims = 0;
  unsigned int aligned_bytes = 0;
  size_t n = 0;
};

// the searched handle of lease L gets QQ's rows as its sketch, unless it already holds exactly these
template <class QQPointRange>
inline void ensure_sketch(MirrorLease& L, const QQPointRange& QQ) {
  if (L.m->sketch_src == (const void*)QQ.data() && L.m->sketch_version == QQ.version() &&
      pann_index_sketch_kind(L.h()) == QQPointRange::Point::sketch_kind) return;
  if (QQ.size() != pann_index_size(L.h())) { std::cout << "ERROR: sketch range and point range differ in size" << std::endl; abort(); }
  const pann_sketch_params sp = QQ.params.to_pann();
  pann_check(pann_index_upload_sketch(L.h(), &sp, QQ.data(), QQ.get_aligned_bytes()));
  L.m->sketch_src = QQ.data(); L.m->sketch_version = QQ.version();
}

}  // namespace parlayANN
