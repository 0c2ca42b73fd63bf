// api.hip -- the extern "C" boundary declared in include/pann.h: handle management (device
// mirrors of PointRange / Graph), host<->device staging, and dispatch into the gfx950 kernels.
// No CPU compute path exists here: without a HIP device every entry point fails loudly.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "grouped_plan.h"
#include "host_staging.h"
#include "pann_internal.h"
#include "quant_device.h"

namespace pann {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return PANN_ERR_HIP;
}

constexpr size_t kAllocSlack = 4096;      // a grown buffer gets a quarter more than was asked for, and this

int Workspace::ensure(size_t need) {
  if (need <= bytes) return PANN_OK;
  if (buf) { PANN_HIP(hipFree(buf)); buf = nullptr; bytes = 0; }
  size_t cap = need + need / 4 + kAllocSlack;
  PANN_HIP(hipMalloc(&buf, cap));
  bytes = cap;
  return PANN_OK;
}
void Workspace::release() { if (buf) (void)hipFree(buf); buf = nullptr; bytes = 0; }

// growable pinned host buffer: host-pointer calls pack their inputs / outputs here so that each direction is ONE
// DMA transfer (copies from or to pageable memory are staged and synchronised one by one by the runtime)
struct PinnedBuf {
  void* p = nullptr; size_t bytes = 0;
  int ensure(size_t need) {
    if (need <= bytes) return PANN_OK;
    if (p) { PANN_HIP(hipHostFree(p)); p = nullptr; bytes = 0; }
    size_t cap = need + need / 4 + kAllocSlack;
    PANN_HIP(hipHostMalloc(&p, cap, hipHostMallocDefault));
    bytes = cap;
    return PANN_OK;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};

}  // namespace pann

using namespace pann;

struct pann_index {
  DeviceIndex ix;
  int device = 0;
  hipStream_t stream = nullptr;      // the stream every call of this handle runs on: own_stream, or the caller's (pann_index_set_stream)
  hipStream_t own_stream = nullptr;
  Workspace ws, ws2, ws3, ws4;   // kernel scratch (builder: search / prune / re-prune / rows of a batch; exact kNN: ws2 partial lists, ws3 block counts, ws4 id lists)
  Workspace ws_rr;               // pann_batch_search_rerank*: prepared queries and frontiers (search_rerank.hip)
  uint32_t vcap = 0;        // visited-list capacity used by the builder (grows on overflow)
  uint32_t dcap = 256;      // dropped-list capacity of the searches (pann_index_reserve_dropped; grows on overflow)
  uint32_t delete_range_keys = 0;   // pann_index_set_option("delete_range_keys"): most keys one prune of a delete consolidation takes (0 = what the key index allows)
  uint32_t gt_pieces = 0;   // pann_index_set_option("gt_pieces"): pieces of the base per query tile in pann_bruteforce_knn (0 = auto)
  Workspace cell_buf;       // locality cell of every point (ensure_locality_cells)
  uint32_t locality_groups = 32;    // ... whose pivots are grouped by their nearest of this many top pivots (0 / 1: no grouping)
  uint32_t locality_pivots = 1024;   // cells of the locality order (pann_index_set_option("locality_pivots"): measurement knob)
  int cells_state = 0;      // 0 not tried, 1 computed, -1 not worth it (table small enough to be cache resident) or switched off
  Workspace code_rank, code_rows;   // filter-code table (filter_codes.hip): rank16[n], gcode[n][gstride]
  int codes_state = 0;      // 0 not tried, 1 available (rank16 built), -1 unavailable (a slot class has 4 095 or more members) or switched off
  PinnedBuf pin_in, pin_out;   // HostTrip: the packed inputs / outputs of a host-pointer call in pinned memory ...
  Workspace trip_in, trip_out; // ... and their device regions
  Workspace graph_slab, graph_row_ids, graph_bad;   // graph upload / download: a slice of host-layout rows, their row ids, the bad-neighbour flag
  Workspace batch_ids;         // the ids of a Vamana insert / delete batch, or the permutation of a whole build
  Workspace pivot_rows, pivot_dists;   // ensure_locality_cells: the pivots as a table; the top-1 distances (released after use)
  Workspace params_scratch;    // pann_quantize_params / pann_sketch_params_generate: each call is synchronised before it returns, so they share it
  Workspace sketch_buf;         // attached bit sketch (pann_index_attach_sketch): ix.sketch points into it
  pann_sketch_params sk_params{};   // ... and the parameters it was made with (the fused rerank sketches its queries with them)
  Workspace labels_buf;         // one label word per point (pann_index_set_labels): ix.labels points into it
  Workspace label_row;          // pann_bruteforce_knn_labeled*, one predicate: its bitmap row, expanded on the device
  // pann_bruteforce_knn_*_grouped* (grouped_knn_run): the sorted queries and counts; the plan; a chunk's bitmap rows and block
  // counts; a chunk's query slab and staged results; the read-back and the plan on the host
  Workspace grp_sort, grp_plan, grp_rows, grp_io;
  PinnedBuf grp_pin;
  Workspace grp_cen;            // pann_filter_medoids_*: a chunk's piece offsets and per-piece sums (entry_points.hip)
  Workspace grp_search;         // pann_batch_search_grouped_labeled*: every query's predicate and start row, gathered (entry_points.hip)
};

namespace {

struct DeviceGuard {
  int prev = -1; bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// reference layout n x (max_deg+1), slot 0 = degree  ->  device layout n x gstride, SENTINEL padded
// A neighbour id >= n would be gathered unchecked by every kernel (points + id * pstride): such a row is left empty
// and *bad is raised, the host then returns PANN_ERR_BAD_ARG (a graph file of another dataset, a truncated file).
__global__ void graph_to_device_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                       uint64_t nrows, uint32_t max_deg, uint32_t gstride,
                                       const uint32_t* __restrict__ row_ids, uint64_t n, uint32_t* __restrict__ bad) {
  const uint64_t r = blockIdx.x;
  if (r >= nrows) return;
  const uint32_t* s = src + r * (uint64_t)(max_deg + 1);
  const uint64_t target = row_ids ? row_ids[r] : r;
  uint32_t* d = dst + target * (uint64_t)gstride;
  const uint32_t deg = min(s[0], max_deg);
  bool ok = true;                                      // one wave per row
  for (uint32_t i0 = 0; i0 < deg; i0 += 64) {
    const uint32_t i = i0 + threadIdx.x;
    ok = ok && (__ballot(i < deg && (uint64_t)s[1 + i] >= n) == 0ull);
  }
  if (!ok && threadIdx.x == 0) atomicOr(bad, 1u);
  for (uint32_t i = threadIdx.x; i < gstride; i += blockDim.x) d[i] = (ok && i < deg) ? s[1 + i] : SENTINEL;
}

__global__ void graph_to_host_layout_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                            uint64_t nrows, uint32_t max_deg, uint32_t gstride) {
  const uint64_t r = blockIdx.x;
  if (r >= nrows) return;
  const uint32_t* s = src + r * (uint64_t)gstride;
  uint32_t* d = dst + r * (uint64_t)(max_deg + 1);
  // one wave per row: degree = number of non-sentinel slots (packed at the front)
  uint32_t deg = 0;
  for (uint32_t i0 = 0; i0 < gstride; i0 += 64) {
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t a = i < gstride ? s[i] : SENTINEL;
    deg += __popcll(__ballot(a != SENTINEL));
    if (i < max_deg) d[1 + i] = (a != SENTINEL) ? a : 0u;   // Graph slabs are zero filled (graph.h:138)
  }
  if (threadIdx.x == 0) d[0] = deg;
}

__global__ void fill_u32_kernel(uint32_t* p, uint64_t n, uint32_t v) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) p[i] = v;
}

int check_idx(const pann_index* idx, const char* fn) {
  if (!idx) { set_error(std::string(fn) + ": null index handle"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

// A four-bit handle is searched and measured; everything else refuses it (include/pann.h, pann_dtype) -- first thing after the
// null check, before anything is launched, allocated or written.  (PANN_TYPE_SWITCH has no four-bit branch.)
int refuse_4bit(const pann_index* idx, const char* fn) {
  if (!is_4bit_dtype(idx->ix.dtype)) return PANN_OK;
  set_error(std::string(fn) + ": not supported on a four-bit (" + dtype_name(idx->ix.dtype) + ") handle");
  return PANN_ERR_UNSUPPORTED;
}
int check_idx_no4(const pann_index* idx, const char* fn) {
  if (int rc = check_idx(idx, fn)) return rc;
  return refuse_4bit(idx, fn);
}

int k_beam_check(const pann_query_params* qp) {  // beamSearch.h:368-372, :549-553
  if (qp->k <= qp->beam) return PANN_OK;
  set_error("Error: beam search parameter Q = " + std::to_string(qp->beam) + " same size or smaller than k = " + std::to_string(qp->k));
  return PANN_ERR_BAD_ARG;
}

// a bitmap of n bits per row: rows lie allow_stride_words apart, 0 = `zero_means` in the caller's words
int allow_stride_check(const char* fn, const char* zero_means, uint64_t stride, uint64_t n) {
  const uint64_t words = (n + 31) / 32;
  if (stride == 0 || stride >= words) return PANN_OK;
  set_error(std::string(fn) + ": allow_stride_words must be 0 (" + zero_means + ") or at least ceil(n / 32) = " + std::to_string(words));
  return PANN_ERR_BAD_ARG;
}

// npreds predicates over the labels of `owner` (which the entry point's checks may yet find to be null)
PointFilter label_filter(const pann_index* owner, int kind, const pann_label_pred* preds, uint64_t npreds, bool dev) {
  PointFilter f;
  f.mode = MASK_LABELS; f.labels = owner ? owner->ix.labels : nullptr; f.kind = kind; f.preds = preds; f.count = npreds; f.dev = dev;
  if (npreds != 1) f.layout = PointFilter::PER_QUERY;
  return f;
}

// Every refusal that concerns the filter itself.  `owner`: the handle whose labels are read and whose size the bitmap rows have (not
// null); nq: what a per-query filter must count.  A table's rules are table_checks': the grouped entries test queries and k in between.
int filter_checks(const pann_index* owner, const char* fn, const PointFilter& F, uint64_t nq) {
  const std::string f = fn;
  if (F.mode == MASK_BITMAP) {
    if (!F.allow) { set_error(f + ": null allow bitmap"); return PANN_ERR_BAD_ARG; }
    return F.is_table() ? PANN_OK : allow_stride_check(fn, "one shared bitmap", F.stride, owner->ix.n);
  }
  if (!owner->ix.labels) { set_error(f + ": the handle has no labels (pann_index_set_labels)"); return PANN_ERR_BAD_ARG; }
  if (!pred_kind_known(F.kind)) { set_error(f + ": unknown predicate kind " + std::to_string(F.kind)); return PANN_ERR_BAD_ARG; }
  if (!F.preds) { set_error(f + ": null predicates"); return PANN_ERR_BAD_ARG; }
  if (F.dev && (uintptr_t)F.preds % 8 != 0) { set_error(f + ": device predicates must be 8-byte aligned"); return PANN_ERR_BAD_ARG; }
  if (!F.is_table() && F.count != 1 && F.count != nq) { set_error(f + ": npreds must be 1 (one predicate for the batch) or nq"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}
int table_checks(const pann_index* owner, const char* fn, const PointFilter& F, bool indexed = true) {      // indexed: by an array of the caller's
  const std::string f = fn;
  const uint64_t words = PointFilter::row_words(owner->ix.n);
  if (F.count == 0) { set_error(f + ": an empty filter table"); return PANN_ERR_BAD_ARG; }
  if (F.count > 0xFFFFFFFFull) { set_error(f + ": more than 2^32 - 1 table entries"); return PANN_ERR_BAD_ARG; }
  if (indexed && !F.group) { set_error(f + ": null index array"); return PANN_ERR_BAD_ARG; }
  if (F.mode == MASK_BITMAP && F.stride < words && !(F.stride == 0 && F.count == 1)) {
    set_error(f + ": allow_stride_words must be at least ceil(n / 32) = " + std::to_string(words));
    return PANN_ERR_BAD_ARG;
  }
  return PANN_OK;
}

int upload_graph_rows(pann_index* idx, const uint32_t* h_rows, uint64_t m, const uint32_t* h_row_ids) {
  DeviceIndex& ix = idx->ix;
  if (m == 0) return PANN_OK;
  ix.codes_valid = 0;                                   // rows change without their filter codes (filter_codes.hip)
  const size_t row_bytes = (size_t)(ix.max_deg + 1) * 4;
  // stream in slices so the staging buffer stays bounded (288 GB HBM, but host slabs can be huge)
  const uint64_t slice = std::max<uint64_t>(1, (256ull << 20) / row_bytes);
  if (int rc = idx->graph_bad.ensure(4)) return rc;
  PANN_HIP(hipMemsetAsync(idx->graph_bad.buf, 0, 4, idx->stream));
  for (uint64_t r0 = 0; r0 < m; r0 += slice) {
    const uint64_t cnt = std::min(slice, m - r0);
    int rc = idx->graph_slab.ensure(cnt * row_bytes); if (rc) return rc;
    PANN_HIP(hipMemcpyAsync(idx->graph_slab.buf, h_rows + r0 * (ix.max_deg + 1), cnt * row_bytes, hipMemcpyHostToDevice, idx->stream));
    const uint32_t* d_ids = nullptr;
    if (h_row_ids) {
      rc = idx->graph_row_ids.ensure(cnt * 4); if (rc) return rc;
      PANN_HIP(hipMemcpyAsync(idx->graph_row_ids.buf, h_row_ids + r0, cnt * 4, hipMemcpyHostToDevice, idx->stream));
      d_ids = idx->graph_row_ids.as<uint32_t>();
    }
    uint32_t* dst = h_row_ids ? ix.graph : ix.graph + r0 * (uint64_t)ix.gstride;
    hipLaunchKernelGGL(graph_to_device_kernel, dim3((uint32_t)cnt), dim3(64), 0, idx->stream,
                       idx->graph_slab.as<uint32_t>(), dst, cnt, ix.max_deg, ix.gstride, d_ids, ix.n, idx->graph_bad.as<uint32_t>());
    PANN_HIP(hipGetLastError());
    PANN_HIP(hipStreamSynchronize(idx->stream));
  }
  uint32_t bad = 0;
  PANN_HIP(hipMemcpy(&bad, idx->graph_bad.buf, 4, hipMemcpyDeviceToHost));
  if (bad) { set_error("graph upload: neighbour id out of range (>= number of points); those rows were left empty"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

// Locality cells: every point's nearest of 256 pivot points (evenly spaced ids), one dense top-1 pass per handle (~15 ms at
// 10M x 96 f32).  The Vamana builder launches the searches of a batch in cell order (vamana_build.hip): a 10M-point launch reads
// every row ~60 times, and queries that run side by side then read rows of the same few regions -- the 256 MiB Infinity Cache
// holds what a few cells need, not what 200 000 queries scattered over the whole table need (search phase -20 %; the graph does
// not depend on the launch order).  Only for tables beyond the cache.
__global__ void gather_rows_kernel(const uint8_t* points, uint32_t pstride, uint64_t n, uint32_t npiv, uint8_t* out) {
  const uint64_t src = (uint64_t)blockIdx.x * (n / npiv);
  for (uint32_t b = threadIdx.x * 16; b < pstride; b += blockDim.x * 16)
    *reinterpret_cast<uint4*>(out + (size_t)blockIdx.x * pstride + b) = *reinterpret_cast<const uint4*>(points + src * pstride + b);
}
// cell <- (group of the cell's pivot << 16) | cell: cells whose pivots share a nearest "top" pivot sort next to each other
__global__ void group_cells_kernel(uint32_t* cell, uint64_t n, const uint32_t* pivot_group) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i < n) { const uint32_t c = cell[i]; cell[i] = (pivot_group[c] << 16) | c; }
}
int ensure_locality_cells(pann_index* idx) {
  DeviceIndex& ix = idx->ix;
  const uint32_t NPIV = idx->locality_pivots;
  if (ix.cell || idx->cells_state != 0 || ix.exact) return PANN_OK;
  static const bool off = ab_env("PANN_NO_LOCALITY") != nullptr;          // diagnostic A/B switch
  const bool forced = ix.cell_min_batch < 4096;                           // pann_index_set_option("locality_order", 2): tests
  if (off || ix.n < 2 * NPIV || (!forced && ((uint64_t)ix.n * ix.pstride < (1ull << 30) || ix.n < 256ull * NPIV))) {
    idx->cells_state = -1; return PANN_OK;
  }
  hipStream_t st = idx->stream;
  if (int rc = idx->pivot_rows.ensure((size_t)NPIV * ix.pstride)) return rc;
  if (int rc = idx->pivot_dists.ensure((size_t)ix.n * 4)) return rc;                      // the distances (not kept)
  if (int rc = idx->cell_buf.ensure((size_t)ix.n * 4 + 256)) return rc;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(NPIV), dim3(64), 0, st, ix.points, ix.pstride, ix.n, NPIV,
                     idx->pivot_rows.as<uint8_t>());
  PANN_HIP(hipGetLastError());
  DeviceIndex pix = ix;                       // the pivots as a 256-point table; A rows = all base points, as external rows
  pix.points = idx->pivot_rows.as<uint8_t>(); pix.n = NPIV; pix.graph = nullptr; pix.gcode = nullptr; pix.rank16 = nullptr; pix.cell = nullptr;
  DenseTopkCall nearest;
  nearest.a_ext = ix.points; nearest.a_stride = ix.pstride; nearest.ntiles = (uint32_t)((ix.n + 63) / 64); nearest.na = ix.n; nearest.nb = NPIV;
  nearest.m = 1; nearest.out_ids = idx->cell_buf.as<uint32_t>(); nearest.out_dists = idx->pivot_dists.as<float>();
  if (int rc = dense_topk_dev(pix, idx->ws2, st, nearest)) return rc;
  if (idx->locality_groups > 1 && NPIV >= 4 * idx->locality_groups && NPIV <= 65536) {
    // the pivots themselves by their nearest of the first `groups` pivots (a prefix of the pivot slab is a table too)
    DeviceIndex gix = pix; gix.n = idx->locality_groups;
    uint32_t* d_pg = idx->pivot_dists.as<uint32_t>();                       // [NPIV] group of every pivot, then [NPIV] distances
    nearest.a_ext = pix.points; nearest.ntiles = (NPIV + 63) / 64; nearest.na = NPIV; nearest.nb = gix.n;
    nearest.out_ids = d_pg; nearest.out_dists = reinterpret_cast<float*>(d_pg + NPIV);
    if (int rc = dense_topk_dev(gix, idx->ws2, st, nearest)) return rc;
    hipLaunchKernelGGL(group_cells_kernel, dim3((uint32_t)((ix.n + 255) / 256)), dim3(256), 0, st, idx->cell_buf.as<uint32_t>(), ix.n, d_pg);
    PANN_HIP(hipGetLastError());
  }
  PANN_HIP(hipStreamSynchronize(st));
  idx->pivot_dists.release();
  ix.cell = idx->cell_buf.as<uint32_t>();
  idx->cells_state = 1;
  return PANN_OK;
}

// The builder's L = 91..128 searches use the 12-bit filter-code table (filter_codes.hip) when every slot class is small
// enough.  Called by the Vamana entry points before their searches: builds rank16 once per handle, and gcode from the
// current graph whenever something outside the builder's row writers has changed the graph since.
int ensure_filter_codes(pann_index* idx, uint32_t L) {
  DeviceIndex& ix = idx->ix;
  if (int rc = ensure_locality_cells(idx)) return rc;     // (every Vamana entry point comes through here before its searches)
  if (L <= 90 || L > 128 || idx->codes_state < 0) return PANN_OK;
  if (ix.codes_valid) return PANN_OK;
  if (idx->codes_state == 0) {
    static const bool off = ab_env("PANN_NO_FILTER_CODES") != nullptr;      // diagnostic A/B switch
    if (off) { idx->codes_state = -1; return PANN_OK; }
    if (int rc = idx->code_rank.ensure((size_t)ix.n * 2 + 256)) return rc;
    uint32_t max_rank = 0;
    if (int rc = filter_codes_build_ranks(ix.n, FILTER_CODE_BITS, idx->ws2, idx->stream, idx->code_rank.as<uint16_t>(), &max_rank)) return rc;
    if (max_rank >= 0xFFFu) { idx->codes_state = -1; idx->code_rank.release(); return PANN_OK; }      // a code would not fit 12 bits
    if (int rc = idx->code_rows.ensure((size_t)ix.n * ix.gstride * 2 + 256)) return rc;
    idx->codes_state = 1;
    ix.rank16 = idx->code_rank.as<uint16_t>(); ix.gcode = idx->code_rows.as<uint16_t>();
  }
  if (int rc = filter_codes_rebuild_rows(ix, idx->stream)) return rc;
  ix.codes_valid = 1;
  return PANN_OK;
}

}  // namespace

extern "C" {

int pann_abi_version(void) { return PANN_ABI_VERSION; }
const char* pann_last_error(void) { return g_err.c_str(); }

int pann_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static int index_create_impl(pann_index** out, const void* points, uint64_t n, uint32_t d, int dtype,
                             uint64_t row_stride_bytes, int metric, const uint32_t* graph,
                             uint32_t max_deg, int device);

int pann_index_create(pann_index** out, const void* points, uint64_t n, uint32_t d, int dtype,
                      uint64_t row_stride_bytes, int metric, const uint32_t* graph,
                      uint32_t max_deg, int device) {
  if (!points) { set_error("pann_index_create: null/empty argument"); return PANN_ERR_BAD_ARG; }
  return index_create_impl(out, points, n, d, dtype, row_stride_bytes, metric, graph, max_deg, device);
}

int pann_index_create_empty(pann_index** out, uint64_t n, uint32_t d, int dtype, int metric, uint32_t max_deg, int device) {
  return index_create_impl(out, nullptr, n, d, dtype, row_bytes_of(dtype, d), metric, nullptr, max_deg, device);
}

int pann_index_upload_points(pann_index* idx, uint64_t first_row, const void* rows, uint64_t nrows, uint64_t row_stride_bytes) {
  if (int rc = check_idx(idx, "pann_index_upload_points")) return rc;
  if (nrows == 0) return PANN_OK;
  const DeviceIndex& ix = idx->ix;
  if (!rows) { set_error("pann_index_upload_points: null argument"); return PANN_ERR_BAD_ARG; }
  if (first_row > ix.n || nrows > ix.n - first_row) { set_error("pann_index_upload_points: row range outside the index"); return PANN_ERR_BAD_ARG; }
  if (row_stride_bytes < ix.dbytes) { set_error("pann_index_upload_points: row stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));                  // no search may be reading the rows being replaced
  const uint64_t slice = std::max<uint64_t>(1, (1ull << 30) / std::max<uint64_t>(row_stride_bytes, 1));
  for (uint64_t r0 = 0; r0 < nrows; r0 += slice) {
    const uint64_t cnt = std::min(slice, nrows - r0);
    PANN_HIP(hipMemcpy2D(ix.points + (first_row + r0) * ix.pstride, ix.pstride, (const uint8_t*)rows + r0 * row_stride_bytes,
                         row_stride_bytes, ix.dbytes, cnt, hipMemcpyHostToDevice));
  }
  return PANN_OK;
}

// ---- labels (DESIGN.md "Label predicates"): one uint32 per point, owned by the handle ----

// the checks of the three range calls; nothing is allocated or written when one fails
static int label_range_checks(const pann_index* idx, const char* fn, uint64_t first_row, const void* p, uint64_t nrows) {
  if (int rc = check_idx(idx, fn)) return rc;
  if (!p) { set_error(std::string(fn) + ": null argument"); return PANN_ERR_BAD_ARG; }
  if (first_row > idx->ix.n || nrows > idx->ix.n - first_row) { set_error(std::string(fn) + ": row range outside the index"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

// the first set call: n words, zero filled on the handle's stream
static int ensure_labels(pann_index* idx) {
  if (idx->ix.labels) return PANN_OK;
  if (int rc = idx->labels_buf.ensure((size_t)idx->ix.n * 4)) return rc;
  PANN_HIP(hipMemsetAsync(idx->labels_buf.buf, 0, (size_t)idx->ix.n * 4, idx->stream));
  idx->ix.labels = idx->labels_buf.as<uint32_t>();
  return PANN_OK;
}

int pann_index_set_labels(pann_index* idx, uint64_t first_row, const uint32_t* labels, uint64_t nrows) {
  if (int rc = label_range_checks(idx, "pann_index_set_labels", first_row, labels, nrows)) return rc;
  DeviceGuard g(idx->device);
  if (int rc = ensure_labels(idx)) return rc;
  PANN_HIP(hipStreamSynchronize(idx->stream));                  // no search may be reading the labels being replaced
  if (nrows) PANN_HIP(hipMemcpy(idx->labels_buf.as<uint32_t>() + first_row, labels, (size_t)nrows * 4, hipMemcpyHostToDevice));
  return PANN_OK;
}

int pann_index_set_labels_dev(pann_index* idx, uint64_t first_row, const uint32_t* d_labels, uint64_t nrows) {
  if (int rc = label_range_checks(idx, "pann_index_set_labels_dev", first_row, d_labels, nrows)) return rc;
  DeviceGuard g(idx->device);
  if (int rc = ensure_labels(idx)) return rc;
  if (nrows) PANN_HIP(hipMemcpyAsync(idx->labels_buf.as<uint32_t>() + first_row, d_labels, (size_t)nrows * 4, hipMemcpyDeviceToDevice, idx->stream));
  return PANN_OK;
}

int pann_index_get_labels(pann_index* idx, uint64_t first_row, uint64_t nrows, uint32_t* out) {
  if (int rc = label_range_checks(idx, "pann_index_get_labels", first_row, out, nrows)) return rc;
  if (!idx->ix.labels) { set_error("pann_index_get_labels: the handle has no labels (pann_index_set_labels)"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));
  if (nrows) PANN_HIP(hipMemcpy(out, idx->ix.labels + first_row, (size_t)nrows * 4, hipMemcpyDeviceToHost));
  return PANN_OK;
}

int pann_index_drop_labels(pann_index* idx) {
  if (int rc = check_idx(idx, "pann_index_drop_labels")) return rc;
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));
  idx->ix.labels = nullptr;
  idx->labels_buf.release();
  return PANN_OK;
}

int pann_index_has_labels(const pann_index* idx) { return (idx && idx->ix.labels) ? 1 : 0; }

static int index_create_impl(pann_index** out, const void* points, uint64_t n, uint32_t d, int dtype,
                             uint64_t row_stride_bytes, int metric, const uint32_t* graph,
                             uint32_t max_deg, int device) {
  if (!out || n == 0 || d == 0) { set_error("pann_index_create: null/empty argument"); return PANN_ERR_BAD_ARG; }
  if (!dtype_known(dtype)) { set_error("pann_index_create: unknown dtype"); return PANN_ERR_BAD_ARG; }
  if (metric != PANN_L2 && metric != PANN_MIPS) { set_error("pann_index_create: unknown metric"); return PANN_ERR_BAD_ARG; }
  if ((dtype == PANN_U4 && metric != PANN_L2) || (dtype == PANN_I4 && metric != PANN_MIPS)) {
    set_error(std::string("pann_index_create: ") + dtype_name(dtype) + " goes with " + (dtype == PANN_U4 ? "PANN_L2" : "PANN_MIPS") + " only");
    return PANN_ERR_UNSUPPORTED;
  }
  if (row_stride_bytes < row_bytes_of(dtype, d)) { set_error("pann_index_create: row stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  if (n >= 0x7FFFFFFFull) { set_error("pann_index_create: n must be < 2^31 (robustPrune uses int ids, vamana/index.h:97)"); return PANN_ERR_BAD_ARG; }
  if (max_deg == 0 || max_deg > 4096) { set_error("pann_index_create: max_deg out of range [1,4096]"); return PANN_ERR_BAD_ARG; }
  int ndev = pann_device_count();
  if (ndev <= 0) { set_error("pann_index_create: no HIP device visible (this library has no CPU path)"); return PANN_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_error("pann_index_create: device ordinal out of range"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(device);
  if (!g.ok) { set_error("pann_index_create: hipSetDevice failed"); return PANN_ERR_HIP; }

  pann_index* idx = new pann_index();
  idx->device = device;
  DeviceIndex& ix = idx->ix;
  ix.n = n; ix.d = d; ix.dtype = dtype; ix.metric = metric; ix.esize = esize_of(dtype); ix.dbytes = (uint32_t)row_bytes_of(dtype, d);
  choose_point_layout(ix.dbytes, &ix.lpc, &ix.nch);
  ix.pstride = ix.lpc * ix.nch * 16;
  ix.max_deg = max_deg; ix.gstride = (max_deg + 15) / 16 * 16;
  auto fail = [&](int rc) { pann_index_destroy(idx); return rc; };
  if (hipStreamCreateWithFlags(&idx->own_stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return fail(PANN_ERR_HIP); }
  idx->stream = idx->own_stream;
  hipError_t e;
  if ((e = hipMalloc((void**)&ix.points, n * (size_t)ix.pstride)) != hipSuccess) return fail(hip_fail(e, "hipMalloc(points)"));
  if ((e = hipMalloc((void**)&ix.graph, n * (size_t)ix.gstride * 4)) != hipSuccess) return fail(hip_fail(e, "hipMalloc(graph)"));
  // points: strided copy into the zero-padded device rows
  if ((e = hipMemsetAsync(ix.points, 0, n * (size_t)ix.pstride, idx->stream)) != hipSuccess) return fail(hip_fail(e, "hipMemset(points)"));
  if ((e = hipStreamSynchronize(idx->stream)) != hipSuccess) return fail(hip_fail(e, "sync"));
  if (points) {
    const uint64_t slice = std::max<uint64_t>(1, (1ull << 30) / std::max<uint64_t>(row_stride_bytes, 1));
    for (uint64_t r0 = 0; r0 < n; r0 += slice) {
      const uint64_t cnt = std::min(slice, n - r0);
      e = hipMemcpy2D(ix.points + r0 * ix.pstride, ix.pstride, (const uint8_t*)points + r0 * row_stride_bytes,
                      row_stride_bytes, ix.dbytes, cnt, hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(hip_fail(e, "hipMemcpy2D(points)"));
    }
  }
  if (graph) {
    int rc = upload_graph_rows(idx, graph, n, nullptr);
    if (rc) return fail(rc);
  } else {
    hipLaunchKernelGGL(fill_u32_kernel, dim3(2048), dim3(256), 0, idx->stream, ix.graph, n * (uint64_t)ix.gstride, SENTINEL);
    if ((e = hipStreamSynchronize(idx->stream)) != hipSuccess) return fail(hip_fail(e, "fill graph"));
  }
  *out = idx;
  return PANN_OK;
}

void pann_index_destroy(pann_index* idx) {
  if (!idx) return;
  DeviceGuard g(idx->device);
  if (idx->stream) (void)hipStreamSynchronize(idx->stream);
  if (idx->ix.points) (void)hipFree(idx->ix.points);
  if (idx->ix.graph) (void)hipFree(idx->ix.graph);
  idx->ws.release(); idx->ws2.release(); idx->ws3.release(); idx->ws4.release(); idx->ws_rr.release();
  idx->pin_in.release(); idx->pin_out.release(); idx->trip_in.release(); idx->trip_out.release();
  idx->graph_slab.release(); idx->graph_row_ids.release(); idx->graph_bad.release(); idx->batch_ids.release();
  idx->pivot_rows.release(); idx->pivot_dists.release(); idx->params_scratch.release();
  idx->code_rank.release(); idx->code_rows.release(); idx->cell_buf.release();
  idx->sketch_buf.release(); idx->labels_buf.release(); idx->label_row.release();
  idx->grp_sort.release(); idx->grp_plan.release(); idx->grp_rows.release(); idx->grp_io.release(); idx->grp_pin.release();
  idx->grp_cen.release(); idx->grp_search.release();
  if (idx->own_stream) (void)hipStreamDestroy(idx->own_stream);
  delete idx;
}

uint64_t pann_index_size(const pann_index* idx) { return idx ? idx->ix.n : 0; }
uint32_t pann_index_dims(const pann_index* idx) { return idx ? idx->ix.d : 0; }
uint32_t pann_index_max_degree(const pann_index* idx) { return idx ? idx->ix.max_deg : 0; }
int pann_index_device(const pann_index* idx) { return idx ? idx->device : -1; }

int pann_index_set_exact_float_order(pann_index* idx, int on) {
  if (int rc = check_idx(idx, "pann_index_set_exact_float_order")) return rc;
  DeviceIndex& ix = idx->ix;
  const bool is_float = ix.dtype == PANN_F32 || ix.dtype == PANN_F16 || ix.dtype == PANN_BF16;
  if (on && is_float) { ix.exact = 1; ix.lpc = 4; ix.nch = ix.pstride / 64; }   // whole query in LDS, lane-per-candidate sums
  else { ix.exact = 0; choose_point_layout(ix.dbytes, &ix.lpc, &ix.nch); }
  return PANN_OK;
}

int pann_index_reserve_dropped(pann_index* idx, uint32_t cap) {
  if (int rc = check_idx(idx, "pann_index_reserve_dropped")) return rc;
  if (cap > (1u << 30)) { set_error("pann_index_reserve_dropped: capacity out of range"); return PANN_ERR_BAD_ARG; }
  if (cap > idx->dcap) idx->dcap = (cap + 63) / 64 * 64;
  return PANN_OK;
}
uint32_t pann_index_dropped_capacity(const pann_index* idx) { return idx ? idx->dcap : 0; }

int pann_index_set_graph(pann_index* idx, const uint32_t* graph) {
  if (int rc = check_idx(idx, "pann_index_set_graph")) return rc;
  if (!graph) { set_error("pann_index_set_graph: null graph"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  return upload_graph_rows(idx, graph, idx->ix.n, nullptr);
}

int pann_index_update_rows(pann_index* idx, const uint32_t* row_ids, const uint32_t* rows, uint64_t m) {
  if (int rc = check_idx(idx, "pann_index_update_rows")) return rc;
  if (m && (!row_ids || !rows)) { set_error("pann_index_update_rows: null argument"); return PANN_ERR_BAD_ARG; }
  for (uint64_t i = 0; i < m; i++)
    if (row_ids[i] >= idx->ix.n) { set_error("ERROR: graph index out of range"); return PANN_ERR_BAD_ARG; }  // graph.h:235-238
  DeviceGuard g(idx->device);
  return upload_graph_rows(idx, rows, m, row_ids);
}

int pann_index_clear_graph(pann_index* idx) {
  if (int rc = check_idx(idx, "pann_index_clear_graph")) return rc;
  DeviceGuard g(idx->device);
  PANN_HIP(hipMemsetAsync(idx->ix.graph, 0xFF, (size_t)idx->ix.n * idx->ix.gstride * 4, idx->stream));
  if (idx->ix.gcode) PANN_HIP(hipMemsetAsync(idx->ix.gcode, 0xFF, (size_t)idx->ix.n * idx->ix.gstride * 2, idx->stream));   // codes of an empty graph
  PANN_HIP(hipStreamSynchronize(idx->stream));
  return PANN_OK;
}

int64_t pann_index_get_option(const pann_index* idx, const char* name) {
  if (!idx || !name) return -1;
  const std::string nm = name;
  if (nm == "forest_group") return idx->ix.forest_group;
  if (nm == "gt_pieces") return idx->gt_pieces;
  if (nm == "delete_range_keys") return idx->delete_range_keys;
  if (nm == "b64_seen") return idx->ix.b64_seen;
  if (nm == "locality_order") return idx->ix.cell ? 1 : 0;
  if (nm == "filter_codes") return idx->ix.codes_valid ? 1 : 0;         // are the class codes in step with the graph right now?
  if (nm == "centroid_piece_ids") return CENTROID_PIECE_IDS;            // compile-time, not settable: list ids one workgroup of pann_filter_medoids_* sums
  if (nm == "pinned_bytes") return (int64_t)(idx->pin_in.bytes + idx->pin_out.bytes);   // pinned host memory the handle holds (HostTrip)
  return -1;
}

int pann_index_set_stream(pann_index* idx, void* stream, int use_private) {
  if (int rc = check_idx(idx, "pann_index_set_stream")) return rc;
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));                    // nothing of this handle is left on the stream it leaves
  idx->stream = use_private ? idx->own_stream : (hipStream_t)stream;
  return PANN_OK;
}

int pann_index_set_option(pann_index* idx, const char* name, int64_t value) {
  if (int rc = check_idx(idx, "pann_index_set_option")) return rc;
  const std::string nm = name ? name : "";
  if (value < 0 || value > 0x7FFFFFFF) { set_error("pann_index_set_option: value out of range"); return PANN_ERR_BAD_ARG; }
  if (nm == "forest_group") idx->ix.forest_group = (uint32_t)value;
  else if (nm == "gt_pieces") idx->gt_pieces = (uint32_t)value;
  else if (nm == "delete_range_keys") idx->delete_range_keys = (uint32_t)value;
  else if (nm == "b64_seen") idx->ix.b64_seen = value ? 1u : 0u;      // 0: the beam-64 search without the second-sighting table (tests, A/B)
  else if (nm == "locality_pivots") { idx->locality_pivots = std::max<uint32_t>(2, std::min<uint32_t>((uint32_t)value, 65536)); idx->ix.cell = nullptr; idx->cells_state = idx->cells_state < 0 ? idx->cells_state : 0; }
  else if (nm == "locality_groups") { idx->locality_groups = (uint32_t)std::min<int64_t>(value, 4096); idx->ix.cell = nullptr; idx->cells_state = idx->cells_state < 0 ? idx->cells_state : 0; }
  else if (nm == "locality_order") {        // 0: the builder launches a batch's searches in batch order
    idx->ix.cell = nullptr;
    idx->ix.cell_min_batch = value == 2 ? 64u : 4096u;       // 2: also on small tables and small batches (tests)
    idx->cells_state = value ? ((idx->cell_buf.buf && idx->cells_state == 1) ? 1 : 0) : -2;
    if (idx->cells_state == 1) idx->ix.cell = idx->cell_buf.as<uint32_t>();
  }
  else if (nm == "filter_codes") {          // 0: the beam-91..128 searches use the id table even where the class codes are available
    idx->ix.codes_valid = 0;
    idx->codes_state = value ? (idx->ix.rank16 ? 1 : 0) : -2;
  }
  else { set_error("pann_index_set_option: unknown option '" + nm + "'"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

int pann_index_get_graph(pann_index* idx, uint32_t* graph_out) {
  if (int rc = check_idx(idx, "pann_index_get_graph")) return rc;
  if (!graph_out) { set_error("pann_index_get_graph: null output"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  DeviceIndex& ix = idx->ix;
  const size_t row_bytes = (size_t)(ix.max_deg + 1) * 4;
  const uint64_t slice = std::max<uint64_t>(1, (256ull << 20) / row_bytes);
  for (uint64_t r0 = 0; r0 < ix.n; r0 += slice) {
    const uint64_t cnt = std::min(slice, ix.n - r0);
    if (int rc = idx->graph_slab.ensure(cnt * row_bytes)) return rc;
    hipLaunchKernelGGL(graph_to_host_layout_kernel, dim3((uint32_t)cnt), dim3(64), 0, idx->stream,
                       ix.graph + r0 * (uint64_t)ix.gstride, idx->graph_slab.as<uint32_t>(), cnt, ix.max_deg, ix.gstride);
    PANN_HIP(hipGetLastError());
    PANN_HIP(hipMemcpyAsync(graph_out + r0 * (ix.max_deg + 1), idx->graph_slab.buf, cnt * row_bytes, hipMemcpyDeviceToHost, idx->stream));
    PANN_HIP(hipStreamSynchronize(idx->stream));
  }
  return PANN_OK;
}

// ---------------------------------------------------------------------------------------------
// batched beam search
// ---------------------------------------------------------------------------------------------

// Every search entry point fills a SearchCall (search_call.h) by field name and goes through batch_search_host or batch_search_dev.

// the limits of a masked search with a result list of out_k entries (the fused path comes through here too, out_k = its list length).
// The bitmap's own checks lie between them; a labeled call has been through filter_checks ahead of the search's checks
static int masked_limits(const pann_index* idx, const PointFilter& F, uint64_t nq, const pann_query_params* qp, uint32_t out_k) {
  if ((int64_t)out_k > qp->beam) { set_error("pann_batch_search_masked: out_k larger than the beam"); return PANN_ERR_BAD_ARG; }
  if (F.mode == MASK_BITMAP) { if (int rc = filter_checks(idx, "pann_batch_search_masked", F, nq)) return rc; }
  if (out_k > 64) { set_error("pann_batch_search_masked: out_k > 64 is not supported"); return PANN_ERR_UNSUPPORTED; }
  return PANN_OK;
}

// What a search refuses before anything is staged or enqueued, in the order in which it is tested (tests/search_refusal_cases.py and
// tests/filter_refusal_cases.py pin the order and the texts).  `fn`: the entry point; only the label filter's and the four-bit refusals
// name it, everything else says pann_batch_search, pann_batch_search_masked or pann_batch_search_filtered (DESIGN.md lists these).
// The head is one chain; the tails of the host and the device path differ: a host call can read its arrays, and tests the queries'
// stride behind nq == 0 (batch_search_host); a device call leaves what it does not test here to the launcher (beam_search.hip).
static int search_refusals(const pann_index* idx, const SearchCall& c, const char* fn) {
  const PointFilter& F = c.filter;
  if (F.mode == MASK_LABELS) {      // the predicates, and a grouped call's table and start rows
    if (int rc = check_idx(idx, fn)) return rc;
    if (int rc = filter_checks(idx, fn, F, c.nq)) return rc;
    if (F.is_table()) {
      if (int rc = table_checks(idx, fn, F)) return rc;
      if (c.start_rows != 1 && c.start_rows != F.count) {
        set_error(std::string(fn) + ": start_rows must be 1 (one row of starts for the batch) or npreds (one per table entry)");
        return PANN_ERR_BAD_ARG;
      }
    }
  }
  if (int rc = check_idx(idx, "pann_batch_search")) return rc;
  if (!c.qp || !c.has_out) { set_error("pann_batch_search: null params/out"); return PANN_ERR_BAD_ARG; }
  if (int rc = k_beam_check(c.qp)) return rc;
  if (F.given()) { if (int rc = masked_limits(idx, F, c.nq, c.qp, c.out.out_k)) return rc; }
  if (c.sketch) { if (int rc = refuse_4bit(idx, fn)) return rc; }
  const uint64_t n = idx->ix.n;
  if (c.dev) {
    if (!c.starts) { set_error("beam search expects at least one start point"); return PANN_ERR_BAD_ARG; }
    if (c.queries && c.qstride < idx->ix.dbytes) { set_error("pann_batch_search: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
    return PANN_OK;
  }
  if (c.sketch) {
    if (!idx->ix.sketch) { set_error("pann_batch_search_filtered: no sketch attached to the index"); return PANN_ERR_BAD_ARG; }
    if ((c.queries != nullptr) != (c.sketch_queries != nullptr)) {
      set_error("pann_batch_search_filtered: sketch_queries go with queries, and only with them"); return PANN_ERR_BAD_ARG;
    }
    if (c.sketch_queries && c.sq_stride < sketch_row_bytes(idx->ix.sk_kind, idx->ix.d)) {
      set_error("pann_batch_search_filtered: sketch query stride smaller than a sketch row"); return PANN_ERR_BAD_ARG;
    }
  }
  if (!c.starts || c.nstarts == 0) { set_error("beam search expects at least one start point"); return PANN_ERR_BAD_ARG; }
  if ((c.queries == nullptr) == (c.query_ids == nullptr)) { set_error("pann_batch_search: exactly one of queries / query_ids must be given"); return PANN_ERR_BAD_ARG; }
  for (uint64_t i = 0, m = c.start_count(); i < m; i++)
    if (c.starts[i] >= n) { set_error("pann_batch_search: start point out of range"); return PANN_ERR_BAD_ARG; }
  for (uint64_t q = 0; F.is_table() && q < c.nq; q++)
    if (F.group[q] >= F.count) {
      set_error("pann_batch_search_grouped_labeled: table index " + std::to_string(F.group[q]) + " of query " + std::to_string(q) +
                " is out of range (>= " + std::to_string(F.count) + ")");
      return PANN_ERR_BAD_ARG;
    }
  for (uint64_t i = 0; c.query_ids && i < c.nq; i++)
    if (c.query_ids[i] >= n) { set_error("pann_batch_search: query id out of range"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

// The grouped labeled search (DESIGN.md "Entry points"): a table of G predicates, one table index per query and 1 or G rows of starts.
// d: the request on the device, its filter the table.  Every query's predicate and start row are gathered into the handle's scratch
// and d becomes a request with a predicate and a start row per query.  *flag (optional): the device word that is raised when a table
// index was >= G.
static int gather_group_rows(pann_index* idx, SearchCall& d, hipStream_t st, const uint32_t** flag) {
  const PointFilter T = d.filter;
  const size_t o_starts = (size_t)d.nq * sizeof(pann_label_pred), o_flag = (o_starts + (size_t)d.nq * d.nstarts * 4 + 7) & ~(size_t)7;
  if (int rc = idx->grp_search.ensure(o_flag + 8)) return rc;
  uint8_t* w = idx->grp_search.as<uint8_t>();
  pann_label_pred* d_preds = (pann_label_pred*)w;
  uint32_t* d_rows = (uint32_t*)(w + o_starts), *d_flag = (uint32_t*)(w + o_flag);
  if (int rc = group_rows_dev(T.preds, (uint32_t)T.count, T.kind, T.group, d.nq, d.starts, d.nstarts, (uint32_t)d.start_rows, d_preds, d_rows,
                              d_flag, st)) return rc;
  d.starts = d_rows; d.starts_layout = SearchCall::STARTS_PER_QUERY;
  d.filter = label_filter(idx, T.kind, d_preds, d.nq, true);
  if (flag) *flag = d_flag;
  return PANN_OK;
}

// a device-pointer search: the whole batch in one launch on the caller's stream, with the handle's dropped-list capacity
static int batch_search_dev(pann_index* idx, const SearchCall& c, const char* fn) {
  if (int rc = search_refusals(idx, c, fn)) return rc;
  DeviceGuard g(idx->device);
  hipStream_t st = (hipStream_t)c.stream;
  SearchCall d = c;
  const uint32_t* bad_group = nullptr;
  if (c.filter.is_table()) { if (int rc = gather_group_rows(idx, d, st, &bad_group)) return rc; }
  const SearchArgs a = slice(d, 0, d.nq, idx->dcap);
  if (int rc = idx->ws.ensure(search_workspace_bytes(idx->ix, a))) return rc;
  if (int rc = launch_beam_search(idx->ix, a, idx->ws.buf, idx->ws.bytes, st)) return rc;
  return bad_group && d.out.status ? raise_status_dev(bad_group, PANN_STATUS_BAD_GROUP, d.out.status, st) : PANN_OK;
}

int pann_batch_search_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids,
                          uint64_t nq, uint64_t q_stride_bytes, const uint32_t* d_starts,
                          uint32_t nstarts, const pann_query_params* qp,
                          const pann_search_out* d_out, void* stream) {
  SearchCall c;
  c.queries = d_queries; c.qstride = q_stride_bytes; c.query_ids = d_query_ids; c.nq = nq; c.starts = d_starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(d_out); c.dev = true; c.stream = stream;
  return batch_search_dev(idx, c, "pann_batch_search_dev");
}

int pann_batch_search_filtered_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                   uint64_t q_stride_bytes, const void* d_sketch_queries, uint64_t sq_stride_bytes,
                                   const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                   const pann_search_out* d_out, uint32_t* d_out_pruned_cmps, void* stream) {
  SearchCall c;
  c.queries = d_queries; c.qstride = q_stride_bytes; c.query_ids = d_query_ids; c.nq = nq; c.starts = d_starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(d_out); c.dev = true; c.stream = stream;
  c.sketch = true; c.sketch_queries = d_sketch_queries; c.sq_stride = sq_stride_bytes; c.pruned_cmps = d_out_pruned_cmps;
  return batch_search_dev(idx, c, "pann_batch_search_filtered_dev");
}

int pann_batch_search_masked_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                 uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                 const uint32_t* d_allow, uint64_t allow_stride_words, const pann_search_out* d_out,
                                 uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, void* stream) {
  SearchCall c;
  c.queries = d_queries; c.qstride = q_stride_bytes; c.query_ids = d_query_ids; c.nq = nq; c.starts = d_starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(d_out); c.dev = true; c.stream = stream;
  c.filter = PointFilter::bitmap(d_allow, allow_stride_words, nq, true); c.result_count = d_out_result_count; c.allowed_cmps = d_out_allowed_cmps;
  return batch_search_dev(idx, c, "pann_batch_search_masked_dev");
}

int pann_batch_search_labeled_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                  uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                  int kind, const pann_label_pred* d_preds, uint64_t npreds, const pann_search_out* d_out,
                                  uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, void* stream) {
  SearchCall c;
  c.queries = d_queries; c.qstride = q_stride_bytes; c.query_ids = d_query_ids; c.nq = nq; c.starts = d_starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(d_out); c.dev = true; c.stream = stream;
  c.filter = label_filter(idx, kind, d_preds, npreds, true); c.result_count = d_out_result_count; c.allowed_cmps = d_out_allowed_cmps;
  return batch_search_dev(idx, c, "pann_batch_search_labeled_dev");
}

int pann_batch_search_steered_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                  uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                  const uint32_t* d_allow, uint64_t allow_stride_words, const pann_search_out* d_out,
                                  uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, uint32_t fill, uint32_t* d_out_steer,
                                  void* stream) {
  SearchCall c;
  c.queries = d_queries; c.qstride = q_stride_bytes; c.query_ids = d_query_ids; c.nq = nq; c.starts = d_starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(d_out); c.dev = true; c.stream = stream;
  c.filter = PointFilter::bitmap(d_allow, allow_stride_words, nq, true); c.result_count = d_out_result_count; c.allowed_cmps = d_out_allowed_cmps;
  c.steer = true; c.fill = fill; c.steer_out = d_out_steer;
  return batch_search_dev(idx, c, "pann_batch_search_steered_dev");
}

int pann_batch_search_steered_labeled_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                          uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts,
                                          const pann_query_params* qp, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                                          const pann_search_out* d_out, uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps,
                                          uint32_t fill, uint32_t* d_out_steer, void* stream) {
  SearchCall c;
  c.queries = d_queries; c.qstride = q_stride_bytes; c.query_ids = d_query_ids; c.nq = nq; c.starts = d_starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(d_out); c.dev = true; c.stream = stream;
  c.filter = label_filter(idx, kind, d_preds, npreds, true); c.result_count = d_out_result_count; c.allowed_cmps = d_out_allowed_cmps;
  c.steer = true; c.fill = fill; c.steer_out = d_out_steer;
  return batch_search_dev(idx, c, "pann_batch_search_steered_labeled_dev");
}

int pann_batch_search_grouped_labeled_dev(pann_index* idx, const void* d_queries, const uint32_t* d_query_ids, uint64_t nq,
                                          uint64_t q_stride_bytes, const uint32_t* d_starts, uint32_t nstarts, uint64_t start_rows,
                                          const pann_query_params* qp, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                                          const uint32_t* d_group_of_query, const pann_search_out* d_out, uint32_t* d_out_result_count,
                                          uint32_t* d_out_allowed_cmps, int steer, uint32_t fill, uint32_t* d_out_steer, void* stream) {
  SearchCall c;
  c.queries = d_queries; c.qstride = q_stride_bytes; c.query_ids = d_query_ids; c.nq = nq;
  c.starts = d_starts; c.nstarts = nstarts; c.starts_layout = SearchCall::STARTS_TABLE; c.start_rows = start_rows;
  c.qp = qp; c.set_out(d_out); c.dev = true; c.stream = stream;
  c.filter = label_filter(idx, kind, d_preds, npreds, true).as_table(d_group_of_query, npreds);
  c.result_count = d_out_result_count; c.allowed_cmps = d_out_allowed_cmps;
  if (steer) { c.steer = true; c.fill = fill; c.steer_out = d_out_steer; }
  return batch_search_dev(idx, c, "pann_batch_search_grouped_labeled_dev");
}

}  // extern "C"

constexpr size_t kQuerySlack = 16;      // kept free behind external query rows: the kernels read a row in 16-byte chunks

// The host round trip of a host-pointer call.  The caller adds its arrays to `in` and `out`, then: begin() packs the inputs into
// pin_in and sends them up into trip_in in ONE transfer, and makes room for the outputs in trip_out / pin_out (with room for a
// status word behind them); after the launches finish() brings the outputs down into pin_out in ONE transfer, waits, and hands
// them to their arrays.  Scratch pieces (PackedLayout::add_scratch) lie in the same regions and are never copied; added last,
// they take no pinned room either.  Outside the search family an array of kDirectBytes or more is a direct piece: it goes
// between the caller's memory and its place in the region in a transfer of its own, as every array did before there was a trip.
// Every array added behind it is direct too (PackedLayout), so the packed pieces are a prefix of the region and only that prefix
// has pinned room and a packed transfer: the callers add their small arrays first.
// Unpacking runs at about 15 GB/s on the host (80 MB of pann_leaf_knn_batch results: +5.5 ms; 8 MB of pann_bruteforce_knn: +0.48 ms;
// the two 400 KB outputs of a 10K-query pann_rerank: +0.06 ms over the 0.51 ms of their own two transfers), so a transfer of its
// own is the cheaper way from somewhere below 400 KB on; at the bound the copy costs 17 us.  (tools/host_trip_time.py)
constexpr size_t kDirectBytes = 256u << 10;

struct HostTrip {
  pann_index* h;
  hipStream_t st;
  PackedLayout in, out;
  int home = 0;          // leading output pieces that fetch_head() has brought down already
  // packed_only: the search family, whose results are a few hundred KB and come down with the status word in one transfer
  explicit HostTrip(pann_index* handle, bool packed_only = false) : h(handle), st(handle->stream) {
    if (!packed_only) in.direct_from = out.direct_from = kDirectBytes;
  }
  int move_direct(const PackedLayout& l, void* region, bool up, int first, int last) {
    for (int i = first; i < std::min(last, l.count); i++) {
      if (!l.pc[i].direct) continue;
      if (up) PANN_HIP(hipMemcpyAsync(l.at(region, i), l.pc[i].host, l.pc[i].bytes, hipMemcpyHostToDevice, st));
      else PANN_HIP(hipMemcpyAsync(l.pc[i].host, l.at(region, i), l.pc[i].bytes, hipMemcpyDeviceToHost, st));
    }
    return PANN_OK;
  }

  int begin() {
    if (int rc = h->pin_in.ensure(in.host_end)) return rc;
    if (int rc = h->trip_in.ensure(in.total)) return rc;
    if (int rc = h->trip_out.ensure(out.total + 256)) return rc;
    if (int rc = h->pin_out.ensure(out.host_end + 256)) return rc;
    in.copy(h->pin_in.p, true);
    if (in.host_end) PANN_HIP(hipMemcpyAsync(h->trip_in.buf, h->pin_in.p, in.host_end, hipMemcpyHostToDevice, st));
    return move_direct(in, h->trip_in.buf, true, 0, in.count);
  }
  template <typename T> const T* din(int piece) const { return (const T*)in.at(h->trip_in.buf, piece); }
  template <typename T> T* dout(int piece) const { return (T*)out.at(h->trip_out.buf, piece); }      // an output (null if not asked for)
  uint32_t* status_slot() const { return (uint32_t*)((uint8_t*)h->trip_out.buf + out.total); }

  // the first npieces outputs ahead of the rest, waited for: the host decides something by them (how many ids to fetch)
  int fetch_head(int npieces) {
    const size_t head = std::min(out.end_of(npieces), out.host_end);
    if (head) PANN_HIP(hipMemcpyAsync(h->pin_out.p, h->trip_out.buf, head, hipMemcpyDeviceToHost, st));
    if (int rc = move_direct(out, h->trip_out.buf, false, 0, npieces)) return rc;
    PANN_HIP(hipStreamSynchronize(st));
    out.copy(h->pin_out.p, false, 0, npieces);
    home = npieces;
    return PANN_OK;
  }

  int finish(bool results_home = false) {          // results_home: the packed outputs already sit in pin_out
    if (!results_home) {
      const size_t from = out.end_of(home);
      if (out.host_end > from)
        PANN_HIP(hipMemcpyAsync((uint8_t*)h->pin_out.p + from, (uint8_t*)h->trip_out.buf + from, out.host_end - from, hipMemcpyDeviceToHost, st));
      if (int rc = move_direct(out, h->trip_out.buf, false, home, out.count)) return rc;
      PANN_HIP(hipStreamSynchronize(st));
    }
    out.copy(h->pin_out.p, false, home);
    return PANN_OK;
  }

  // The launches under the dropped-list growth policy of host_staging.h, then finish().  launch(q0, cnt, dcap, &d_word): enqueue queries
  // [q0, q0 + cnt) and say where on the device the launch's status word lies.
  template <class Launch>
  int run_grown(uint64_t nq, const pann_query_params* qp, const char* fn, uint32_t* status, Launch&& launch) {
    assert(out.host_end == out.total);      // the status word lies behind the outputs and comes down with them: no scratch, no direct piece
    bool results_home = false;
    if (int rc = run_with_dropped_growth(h->dcap, h->ix.n, nq, qp->limit, fn, status, &results_home, &g_err,
        [&](uint64_t q0, uint64_t cnt, uint32_t dcap, uint32_t* st_word) -> int {
        const uint32_t* d_word = nullptr;
        if (int rc = launch(q0, cnt, dcap, &d_word)) return rc;
        if (cnt == nq) {           // the whole batch in one launch (the normal case): the word travels with the results, ONE transfer
          if (d_word != status_slot()) PANN_HIP(hipMemcpyAsync(status_slot(), d_word, 4, hipMemcpyDeviceToDevice, st));
          PANN_HIP(hipMemcpyAsync(h->pin_out.p, h->trip_out.buf, out.total + 4, hipMemcpyDeviceToHost, st));
          PANN_HIP(hipStreamSynchronize(st));
          std::memcpy(st_word, (uint8_t*)h->pin_out.p + out.total, 4);
        } else {
          PANN_HIP(hipMemcpyAsync(st_word, d_word, 4, hipMemcpyDeviceToHost, st));
          PANN_HIP(hipStreamSynchronize(st));
        }
        return PANN_OK;
      })) return rc;
    if (h->ws.bytes > (2ull << 30)) h->ws.release();          // a one-off worst-case scratch is not kept on the handle
    return finish(results_home);
  }
};

// A point filter on a host trip.  The constructor adds the filter's host arrays to t.in where it is called (the packed layout and the
// small-before-large rule of direct pieces depend on the place): the table index of every query, then the predicates or the bitmap rows
// packed to ceil(n / 32) words each.  After t.begin(), on_device() is the same filter on the staged copies.  `host` null: no filter.
struct StagedFilter {
  PointFilter f;
  int i_group = -1, i_rows = -1; uint64_t words;
  StagedFilter(HostTrip& t, const PointFilter* host, uint64_t n, uint64_t nq) : words(PointFilter::row_words(n)) {
    if (!host) return;
    f = *host;
    if (f.is_table()) i_group = t.in.add(f.group, (size_t)nq * 4);
    // (a stride of 0 goes with one row -- the shared bitmap, or a table with G == 1 -- where the stride is never applied)
    i_rows = f.mode == MASK_LABELS ? t.in.add(f.preds, (size_t)f.count * sizeof(pann_label_pred))
                                   : t.in.add_rows(f.allow, (size_t)f.count, words * 4, (size_t)(f.stride ? f.stride : words) * 4);
  }
  PointFilter on_device(const HostTrip& t) const {
    PointFilter d = f; d.dev = true;
    if (i_group >= 0) d.group = t.din<uint32_t>(i_group);
    if (f.mode == MASK_LABELS) d.preds = t.din<pann_label_pred>(i_rows);
    else if (f.mode == MASK_BITMAP) { d.allow = t.din<uint32_t>(i_rows); d.stride = f.shared() ? 0 : words; }
    return d;
  }
};

// A host-pointer search: one round trip.  The request is restated once on the staged copies (t.din / t.dout) and sliced per launch.
static int batch_search_host(pann_index* idx, const SearchCall& c, const char* fn) {
  if (int rc = search_refusals(idx, c, fn)) return rc;
  const uint64_t nq = c.nq;
  if (nq == 0) return PANN_OK;
  DeviceGuard g(idx->device);
  const DeviceIndex& ix = idx->ix;
  // ---- inputs: packed into pinned memory, one H2D transfer ----
  if (c.queries && c.qstride < ix.dbytes) { set_error("pann_batch_search: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  const uint32_t sk_row = c.sketch ? sketch_row_bytes(ix.sk_kind, ix.d) : 0;
  HostTrip t(idx, true);
  const int i_q = c.queries ? t.in.add(c.queries, (nq - 1) * c.qstride + ix.dbytes, kQuerySlack) : t.in.add(c.query_ids, nq * 4);
  const int i_st = t.in.add(c.starts, (size_t)c.start_count() * 4);
  const StagedFilter staged(t, c.filter.given() ? &c.filter : nullptr, ix.n, nq);      // masked / labeled: the bitmap rows or the predicates travel with them
  const int i_sk = c.sketch ? t.in.add_rows(c.sketch_queries, nq, sk_row, c.sq_stride) : -1;      // filtered: the sketch rows, dense
  // ---- outputs: one packed device region, one D2H transfer into pinned memory, then host copies ----
  const pann_search_out& out = c.out;
  const size_t ok = out.out_k, vc = out.visited_cap;
  const int o_ids = t.out.add(out.ids, nq * ok * 4), o_dists = t.out.add(out.dists, nq * ok * 4);
  const int o_fs = t.out.add(out.frontier_size, nq * 4), o_vcnt = t.out.add(out.visited_count, nq * 4);
  const int o_cmps = t.out.add(out.dist_cmps, nq * 4), o_deg = t.out.add(out.degree_sum, nq * 4);
  const int o_vids = t.out.add(out.visited_ids, nq * vc * 4), o_vdists = t.out.add(out.visited_dists, nq * vc * 4);
  const int o_pruned = t.out.add(c.pruned_cmps, nq * 4);
  const int o_rcnt = t.out.add(c.result_count, nq * 4), o_acmps = t.out.add(c.allowed_cmps, nq * 4);
  const int o_steer = t.out.add(c.steer_out, nq * 8);
  if (int rc = t.begin()) return rc;
  // ---- the request on the device.  Where it differs from what a _dev caller would have passed, it says so ----
  SearchCall d = c;
  d.dev = true; d.stream = t.st;
  d.queries = c.queries ? t.din<uint8_t>(i_q) : nullptr; d.query_ids = c.queries ? nullptr : t.din<uint32_t>(i_q);
  d.starts = t.din<uint32_t>(i_st);
  d.filter = staged.on_device(t);
  d.sketch_queries = c.sketch ? t.din<uint8_t>(i_sk) : nullptr; d.sq_stride = sk_row;      // the staged sketch rows are dense
  d.out.ids = t.dout<uint32_t>(o_ids); d.out.dists = t.dout<float>(o_dists);
  d.out.frontier_size = t.dout<uint32_t>(o_fs); d.out.visited_count = t.dout<uint32_t>(o_vcnt);
  d.out.dist_cmps = t.dout<uint32_t>(o_cmps); d.out.degree_sum = t.dout<uint32_t>(o_deg);
  d.out.visited_ids = t.dout<uint32_t>(o_vids); d.out.visited_dists = t.dout<float>(o_vdists);
  if (!d.out.visited_ids && !d.out.visited_dists) d.out.visited_cap = 0;      // HOST ONLY: no visited array, no visited list (a _dev call keeps its visited_cap)
  d.out.status = nullptr;      // HOST ONLY: the status word is read from the workspace (a _dev call gets it copied to its own word)
  d.pruned_cmps = t.dout<uint32_t>(o_pruned);
  d.result_count = t.dout<uint32_t>(o_rcnt); d.allowed_cmps = t.dout<uint32_t>(o_acmps);
  d.steer_out = t.dout<uint32_t>(o_steer);
  if (d.filter.is_table()) { if (int rc = gather_group_rows(idx, d, t.st, nullptr)) return rc; }      // (the indices were checked above: no flag to read)
  uint32_t status = 0;
  if (int rc = t.run_grown(nq, c.qp, "pann_batch_search", &status,
      [&](uint64_t q0, uint64_t cnt, uint32_t dcap, const uint32_t** d_word) -> int {
      const SearchArgs a = slice(d, q0, cnt, dcap);
      if (int rc = idx->ws.ensure(search_workspace_bytes(ix, a))) return rc;
      *d_word = (const uint32_t*)((uint8_t*)idx->ws.buf + 64);
      return launch_beam_search(ix, a, idx->ws.buf, idx->ws.bytes, t.st);
    })) return rc;
  if (out.status) *out.status = status;
  if (status & PANN_STATUS_VISITED_OVERFLOW) { set_error("pann_batch_search: visited list longer than visited_cap"); return PANN_ERR_OVERFLOW; }
  return PANN_OK;
}

extern "C" {

int pann_batch_search(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                      uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts,
                      const pann_query_params* qp, const pann_search_out* out) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq; c.starts = starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(out);
  return batch_search_host(idx, c, "pann_batch_search");
}

int pann_batch_search_filtered(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                               uint64_t q_stride_bytes, const void* sketch_queries, uint64_t sq_stride_bytes,
                               const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                               const pann_search_out* out, uint32_t* out_pruned_cmps) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq; c.starts = starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(out);
  c.sketch = true; c.sketch_queries = sketch_queries; c.sq_stride = sq_stride_bytes; c.pruned_cmps = out_pruned_cmps;
  return batch_search_host(idx, c, "pann_batch_search_filtered");
}

int pann_batch_search_masked(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                             uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                             const uint32_t* allow, uint64_t allow_stride_words, const pann_search_out* out,
                             uint32_t* out_result_count, uint32_t* out_allowed_cmps) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq; c.starts = starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(out);
  c.filter = PointFilter::bitmap(allow, allow_stride_words, nq, false); c.result_count = out_result_count; c.allowed_cmps = out_allowed_cmps;
  return batch_search_host(idx, c, "pann_batch_search_masked");
}

int pann_batch_search_labeled(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                              uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                              int kind, const pann_label_pred* preds, uint64_t npreds, const pann_search_out* out,
                              uint32_t* out_result_count, uint32_t* out_allowed_cmps) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq; c.starts = starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(out);
  c.filter = label_filter(idx, kind, preds, npreds, false); c.result_count = out_result_count; c.allowed_cmps = out_allowed_cmps;
  return batch_search_host(idx, c, "pann_batch_search_labeled");
}

int pann_batch_search_steered(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                              uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                              const uint32_t* allow, uint64_t allow_stride_words, const pann_search_out* out,
                              uint32_t* out_result_count, uint32_t* out_allowed_cmps, uint32_t fill, uint32_t* out_steer) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq; c.starts = starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(out);
  c.filter = PointFilter::bitmap(allow, allow_stride_words, nq, false); c.result_count = out_result_count; c.allowed_cmps = out_allowed_cmps;
  c.steer = true; c.fill = fill; c.steer_out = out_steer;
  return batch_search_host(idx, c, "pann_batch_search_steered");
}

int pann_batch_search_steered_labeled(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                                      uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                                      int kind, const pann_label_pred* preds, uint64_t npreds, const pann_search_out* out,
                                      uint32_t* out_result_count, uint32_t* out_allowed_cmps, uint32_t fill, uint32_t* out_steer) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq; c.starts = starts; c.nstarts = nstarts;
  c.qp = qp; c.set_out(out);
  c.filter = label_filter(idx, kind, preds, npreds, false); c.result_count = out_result_count; c.allowed_cmps = out_allowed_cmps;
  c.steer = true; c.fill = fill; c.steer_out = out_steer;
  return batch_search_host(idx, c, "pann_batch_search_steered_labeled");
}

int pann_batch_search_grouped_labeled(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq, uint64_t q_stride_bytes,
                                      const uint32_t* starts, uint32_t nstarts, uint64_t start_rows, const pann_query_params* qp, int kind,
                                      const pann_label_pred* preds, uint64_t npreds, const uint32_t* group_of_query, const pann_search_out* out,
                                      uint32_t* out_result_count, uint32_t* out_allowed_cmps, int steer, uint32_t fill, uint32_t* out_steer) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq;
  c.starts = starts; c.nstarts = nstarts; c.starts_layout = SearchCall::STARTS_TABLE; c.start_rows = start_rows;
  c.qp = qp; c.set_out(out);
  c.filter = label_filter(idx, kind, preds, npreds, false).as_table(group_of_query, npreds);
  c.result_count = out_result_count; c.allowed_cmps = out_allowed_cmps;
  if (steer) { c.steer = true; c.fill = fill; c.steer_out = out_steer; }
  return batch_search_host(idx, c, "pann_batch_search_grouped_labeled");
}

int pann_batch_search_per_query_starts(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                                       uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts,
                                       const pann_query_params* qp, const pann_search_out* out) {
  SearchCall c;
  c.queries = queries; c.qstride = q_stride_bytes; c.query_ids = query_ids; c.nq = nq;
  c.starts = starts; c.nstarts = nstarts; c.starts_layout = SearchCall::STARTS_PER_QUERY;
  c.qp = qp; c.set_out(out);
  return batch_search_host(idx, c, "pann_batch_search_per_query_starts");
}


// ---------------------------------------------------------------------------------------------
// robustPrune / Vamana build
// ---------------------------------------------------------------------------------------------

int pann_robust_prune_batch(pann_index* idx, const uint32_t* owners, uint64_t m, const uint32_t* cand_ids,
                            const float* cand_dists, const uint64_t* cand_offsets, double alpha, uint32_t R,
                            int add_out_nbrs, uint32_t* out_rows, uint32_t* out_dist_cmps) {
  if (int rc = check_idx_no4(idx, "pann_robust_prune_batch")) return rc;
  if (m && (!owners || !cand_offsets || !out_rows)) { set_error("pann_robust_prune_batch: null argument"); return PANN_ERR_BAD_ARG; }
  if (m && cand_offsets[m] && !cand_ids) { set_error("pann_robust_prune_batch: null candidate ids"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  return robust_prune_batch_host(idx->ix, idx->ws2, idx->stream, owners, m, cand_ids, cand_dists, cand_offsets,
                                 alpha, R, add_out_nbrs, out_rows, out_dist_cmps);
}

static uint32_t default_vcap(uint32_t L) { return std::max<uint32_t>(2 * L, 128); }

int pann_vamana_insert_batch(pann_index* idx, const uint32_t* batch_ids, uint64_t m, uint32_t start, uint32_t R,
                             uint32_t L, double alpha, pann_build_stats* stats) {
  if (int rc = check_idx_no4(idx, "pann_vamana_insert_batch")) return rc;
  if (m == 0) return PANN_OK;
  if (!batch_ids) { set_error("pann_vamana_insert_batch: null batch"); return PANN_ERR_BAD_ARG; }
  if (L == 0 || L > 65536) { set_error("pann_vamana_insert_batch: L out of range"); return PANN_ERR_BAD_ARG; }
  if (start >= idx->ix.n) { set_error("pann_vamana_insert_batch: start out of range"); return PANN_ERR_BAD_ARG; }
  for (uint64_t i = 0; i < m; i++)
    if (batch_ids[i] >= idx->ix.n) {  // vamana/index.h:193-198
      set_error("ERROR: invalid point " + std::to_string(batch_ids[i]) + " given to batch_insert"); return PANN_ERR_BAD_ARG;
    }
  DeviceGuard g(idx->device);
  if (int rc = ensure_filter_codes(idx, L)) return rc;
  if (int rc = idx->batch_ids.ensure(m * 4)) return rc;
  PANN_HIP(hipMemcpyAsync(idx->batch_ids.buf, batch_ids, m * 4, hipMemcpyHostToDevice, idx->stream));
  if (idx->vcap < default_vcap(L)) idx->vcap = default_vcap(L);
  return insert_batch_dev(idx->ix, idx->ws2, idx->ws3, idx->ws, idx->ws4, idx->stream, idx->batch_ids.as<uint32_t>(), (uint32_t)m,
                          start, R, L, alpha, &idx->vcap, stats);
}

// ---- the two phases of a batch on device pointers: the seam of the multi-GPU build (parlayann_amd/distributed.py) ----

int pann_vamana_search_prune_dev(pann_index* idx, const uint32_t* d_batch_ids, uint64_t m, uint32_t start, uint32_t R, uint32_t L,
                                 double alpha, uint32_t* d_rows_out, pann_build_stats* stats) {
  if (int rc = check_idx_no4(idx, "pann_vamana_search_prune_dev")) return rc;
  if (m == 0) return PANN_OK;
  if (!d_batch_ids || !d_rows_out) { set_error("pann_vamana_search_prune_dev: null argument"); return PANN_ERR_BAD_ARG; }
  if (L == 0 || L > 65536) { set_error("pann_vamana_search_prune_dev: L out of range"); return PANN_ERR_BAD_ARG; }
  if (start >= idx->ix.n || m > 0xFFFFFFF0ull) { set_error("pann_vamana_search_prune_dev: start / batch size out of range"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  if (int rc = ensure_filter_codes(idx, L)) return rc;
  if (idx->vcap < default_vcap(L)) idx->vcap = default_vcap(L);
  return vamana_search_prune_dev(idx->ix, idx->ws2, idx->ws, idx->stream, d_batch_ids, (uint32_t)m, start, R, L, alpha, &idx->vcap,
                                 d_rows_out, stats);
}

int pann_vamana_apply_rows_dev(pann_index* idx, const uint32_t* d_batch_ids, uint64_t m, const uint32_t* d_rows, uint32_t R,
                               double alpha, pann_build_stats* stats) {
  if (int rc = check_idx_no4(idx, "pann_vamana_apply_rows_dev")) return rc;
  if (m == 0) return PANN_OK;
  if (!d_batch_ids || !d_rows) { set_error("pann_vamana_apply_rows_dev: null argument"); return PANN_ERR_BAD_ARG; }
  if (m > 0xFFFFFFF0ull) { set_error("pann_vamana_apply_rows_dev: batch too large"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  return vamana_apply_rows_dev(idx->ix, idx->ws2, idx->ws3, idx->stream, d_batch_ids, (uint32_t)m, d_rows, R, alpha, stats);
}

// ---- deleting points (vamana_delete.hip) ----

static int delete_batch_checks(const pann_index* idx, const char* fn, const uint32_t* ids, uint64_t m, uint32_t R) {
  if (!idx && pann_device_count() <= 0) { set_error(std::string(fn) + ": no HIP device visible (this library has no CPU path)"); return PANN_ERR_NO_DEVICE; }
  if (int rc = check_idx_no4(idx, fn)) return rc;
  if (R == 0 || R > idx->ix.max_deg || R > 1024) { set_error(std::string(fn) + ": R must be in [1, min(max_deg,1024)]"); return PANN_ERR_BAD_ARG; }
  if (m > 0xFFFFFFF0ull) { set_error(std::string(fn) + ": batch too large"); return PANN_ERR_BAD_ARG; }
  if (m && !ids) { set_error(std::string(fn) + ": null ids"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

int pann_vamana_delete_batch(pann_index* idx, const uint32_t* del_ids, uint64_t m, uint32_t R, double alpha,
                             pann_delete_stats* stats) {
  if (int rc = delete_batch_checks(idx, "pann_vamana_delete_batch", del_ids, m, R)) return rc;
  if (m == 0) return PANN_OK;
  for (uint64_t i = 0; i < m; i++)
    if (del_ids[i] >= idx->ix.n) {
      set_error("pann_vamana_delete_batch: id " + std::to_string(del_ids[i]) + " out of range; nothing was changed"); return PANN_ERR_BAD_ARG;
    }
  DeviceGuard g(idx->device);
  if (int rc = idx->batch_ids.ensure(m * 4)) return rc;
  PANN_HIP(hipMemcpyAsync(idx->batch_ids.buf, del_ids, m * 4, hipMemcpyHostToDevice, idx->stream));
  return vamana_delete_batch_dev(idx->ix, idx->ws3, idx->ws2, idx->ws4, idx->stream, idx->batch_ids.as<uint32_t>(), m, R, alpha,
                                 idx->delete_range_keys, stats);
}

int pann_vamana_delete_batch_dev(pann_index* idx, const uint32_t* d_del_ids, uint64_t m, uint32_t R, double alpha,
                                 pann_delete_stats* stats) {
  if (int rc = delete_batch_checks(idx, "pann_vamana_delete_batch_dev", d_del_ids, m, R)) return rc;
  if (m == 0) return PANN_OK;
  DeviceGuard g(idx->device);
  return vamana_delete_batch_dev(idx->ix, idx->ws3, idx->ws2, idx->ws4, idx->stream, d_del_ids, m, R, alpha, idx->delete_range_keys, stats);
}

int pann_vamana_sort_neighbors(pann_index* idx) {
  if (int rc = check_idx_no4(idx, "pann_vamana_sort_neighbors")) return rc;
  DeviceGuard g(idx->device);
  idx->ix.codes_valid = 0;                              // the rows are permuted without their filter codes
  return sort_neighbors_dev(idx->ix, idx->stream);
}

// the insertion order of this build: Fisher-Yates driven by splitmix64(seed) (DESIGN.md "Build
// determinism"; parlay::random_permutation, vamana/index.h:212, is not reproducible offline)
static void build_permutation(uint64_t m, uint64_t seed, uint32_t* out) {
  for (uint64_t i = 0; i < m; i++) out[i] = (uint32_t)i;
  uint64_t s = seed;
  auto next = [&]() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  };
  // The swap partners do not depend on the array, so they are drawn a block ahead and their cache lines requested before the
  // swaps are made in order: the same permutation, without a cache miss per step (10M ids: 0.32 -> 0.1 s of every build).
  constexpr uint64_t BLK = 64;
  uint64_t part[BLK];
  for (uint64_t hi = m; hi > 1;) {
    const uint64_t cnt = std::min<uint64_t>(BLK, hi - 1);
    for (uint64_t k = 0; k < cnt; k++) { part[k] = next() % (hi - k); __builtin_prefetch(&out[part[k]], 1); }
    for (uint64_t k = 0; k < cnt; k++) std::swap(out[hi - k - 1], out[part[k]]);
    hi -= cnt;
  }
}

void pann_build_permutation(uint64_t n, uint64_t seed, uint32_t* out) {
  if (!out) return;
  build_permutation(n, seed, out);
}

uint64_t pann_vamana_batch_schedule(uint64_t n, uint64_t m, uint64_t* bounds, uint64_t cap) {
  // vamana/index.h:206-209, :223-234 with base 2 and max_fraction .02 (the values build_index passes, :174-177)
  size_t max_batch = std::min<size_t>((size_t)(0.02 * (double)(float)n), 1000000ul);
  if (max_batch == 0) max_batch = n;
  uint64_t nb = 0;
  size_t count = 0, inc = 0;
  while (count < m) {
    size_t floor, ceiling;
    if (std::pow(2.0, (double)inc) <= (double)max_batch) {
      floor = (size_t)std::pow(2.0, (double)inc) - 1;
      ceiling = std::min((size_t)std::pow(2.0, (double)(inc + 1)) - 1, (size_t)m);
      count = ceiling;
    } else {
      floor = count;
      ceiling = std::min(count + max_batch, (size_t)m);
      count += max_batch;
    }
    if (bounds && nb < cap) { bounds[2 * nb] = floor; bounds[2 * nb + 1] = ceiling; }
    nb++;
    inc++;
  }
  return nb;
}

namespace {
// vamana/index.h:156-170 with this build's own generator: edge j of vertex i = splitmix64(seed + golden * (i*degree + j + 1)) mod n
__global__ void random_edges_kernel(uint32_t* graph, uint32_t gstride, uint64_t n, uint32_t degree, uint64_t seed) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * gstride) return;
  const uint64_t i = t / gstride, j = t % gstride;
  uint32_t v = SENTINEL;
  if (j < degree) {
    uint64_t z = seed + 0x9e3779b97f4a7c15ull * (i * degree + j + 1);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    v = (uint32_t)(z % n);
  }
  graph[t] = v;
}
}  // namespace

int pann_vamana_build_single_batch(pann_index* idx, uint32_t R, uint32_t L, double alpha, int num_passes, uint32_t degree,
                                   uint64_t seed, int sort_neighbors, pann_build_stats* stats) {
  if (int rc = check_idx_no4(idx, "pann_vamana_build_single_batch")) return rc;
  if (L == 0 || L > 65536 || num_passes < 1) { set_error("pann_vamana_build_single_batch: bad L / num_passes"); return PANN_ERR_BAD_ARG; }
  if (degree == 0 || degree > idx->ix.max_deg) { set_error("pann_vamana_build_single_batch: degree must be in [1, max_deg]"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  const uint64_t n = idx->ix.n;
  if (n >= 0xFFFFFFFFull / 2) { set_error("pann_vamana_build_single_batch: n too large for one batch"); return PANN_ERR_BAD_ARG; }
  // (generated into the handle's pinned staging: no first-touch page faults per build -- they cost more than the shuffle -- and a
  // DMA transfer without a bounce buffer)
  if (int rc = idx->pin_in.ensure(n * 4)) return rc;
  uint32_t* perm = static_cast<uint32_t*>(idx->pin_in.p);
  build_permutation(n, seed, perm);
  if (int rc = idx->batch_ids.ensure(n * 4)) return rc;
  PANN_HIP(hipMemcpyAsync(idx->batch_ids.buf, perm, n * 4, hipMemcpyHostToDevice, idx->stream));
  {
    const uint64_t tot = n * idx->ix.gstride;
    hipLaunchKernelGGL(random_edges_kernel, dim3((uint32_t)((tot + 255) / 256)), dim3(256), 0, idx->stream, idx->ix.graph,
                       idx->ix.gstride, n, degree, seed);
    PANN_HIP(hipGetLastError());
  }
  PANN_HIP(hipStreamSynchronize(idx->stream));
  idx->ix.codes_valid = 0;                              // random_edges_kernel wrote rows
  if (int rc = ensure_filter_codes(idx, L)) return rc;
  if (idx->vcap < default_vcap(L)) idx->vcap = default_vcap(L);
  for (int pass = 0; pass < num_passes; pass++) {
    const double a = (pass == num_passes - 1) ? alpha : 1.0;   // :173-178
    if (int rc = insert_batch_dev(idx->ix, idx->ws2, idx->ws3, idx->ws, idx->ws4, idx->stream, idx->batch_ids.as<uint32_t>(),
                                  (uint32_t)n, 0u, R, L, a, &idx->vcap, stats))      // floor = 0, ceiling = m (:236-240)
      return rc;
  }
  if (sort_neighbors) { idx->ix.codes_valid = 0; return sort_neighbors_dev(idx->ix, idx->stream); }
  return PANN_OK;
}

int pann_vamana_build(pann_index* idx, uint32_t R, uint32_t L, double alpha, int num_passes, uint64_t seed,
                      int sort_neighbors, pann_build_stats* stats) {
  if (int rc = check_idx_no4(idx, "pann_vamana_build")) return rc;
  if (L == 0 || L > 65536 || num_passes < 1) { set_error("pann_vamana_build: bad L / num_passes"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  const uint64_t n = idx->ix.n;
  // (generated into the handle's pinned staging: no first-touch page faults per build -- they cost more than the shuffle -- and a
  // DMA transfer without a bounce buffer)
  if (int rc = idx->pin_in.ensure(n * 4)) return rc;
  uint32_t* perm = static_cast<uint32_t*>(idx->pin_in.p);
  build_permutation(n, seed, perm);
  if (int rc = idx->batch_ids.ensure(n * 4)) return rc;
  PANN_HIP(hipMemcpyAsync(idx->batch_ids.buf, perm, n * 4, hipMemcpyHostToDevice, idx->stream));
  PANN_HIP(hipStreamSynchronize(idx->stream));
  const uint32_t* d_perm = idx->batch_ids.as<uint32_t>();
  if (int rc = ensure_filter_codes(idx, L)) return rc;
  if (idx->vcap < default_vcap(L)) idx->vcap = default_vcap(L);
  // vamana/index.h:206-209
  size_t max_batch = std::min<size_t>((size_t)(0.02 * (double)(float)n), 1000000ul);
  if (max_batch == 0) max_batch = n;
  for (int pass = 0; pass < num_passes; pass++) {
    const double a = (pass == num_passes - 1) ? alpha : 1.0;   // :173-178
    size_t count = 0, inc = 0;
    while (count < n) {                                         // :223-234
      size_t floor, ceiling;
      if (std::pow(2.0, (double)inc) <= (double)max_batch) {
        floor = (size_t)std::pow(2.0, (double)inc) - 1;
        ceiling = std::min((size_t)std::pow(2.0, (double)(inc + 1)) - 1, (size_t)n);
        count = ceiling;
      } else {
        floor = count;
        ceiling = std::min(count + max_batch, (size_t)n);
        count += max_batch;
      }
      if (int rc = insert_batch_dev(idx->ix, idx->ws2, idx->ws3, idx->ws, idx->ws4, idx->stream, d_perm + floor,
                                    (uint32_t)(ceiling - floor), 0u /* set_start(): vertex 0, :148 */, R, L, a,
                                    &idx->vcap, stats))
        return rc;
      inc++;
    }
  }
  if (sort_neighbors) { idx->ix.codes_valid = 0; return sort_neighbors_dev(idx->ix, idx->stream); }   // :180-185
  return PANN_OK;
}


// ---------------------------------------------------------------------------------------------
// distances, HCNNG leaf kNN, brute-force ground truth
// ---------------------------------------------------------------------------------------------

int pann_pair_distances(pann_index* idx, const uint32_t* a_ids, const uint32_t* b_ids, uint64_t m, float* out) {
  if (int rc = check_idx(idx, "pann_pair_distances")) return rc;
  if (m == 0) return PANN_OK;
  if (!a_ids || !b_ids || !out) { set_error("pann_pair_distances: null argument"); return PANN_ERR_BAD_ARG; }
  for (uint64_t i = 0; i < m; i++)
    if (a_ids[i] >= idx->ix.n || b_ids[i] >= idx->ix.n) { set_error("pann_pair_distances: id out of range"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  HostTrip t(idx);
  const int i_a = t.in.add(a_ids, m * 4), i_b = t.in.add(b_ids, m * 4), o_d = t.out.add(out, m * 4);
  if (int rc = t.begin()) return rc;
  if (int rc = query_distances_dev(idx->ix, t.st, nullptr, 0, t.din<uint32_t>(i_a), m, t.din<uint32_t>(i_b), m, 1, t.dout<float>(o_d))) return rc;
  return t.finish();
}

int pann_query_distances(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes,
                         const uint32_t* ids, uint64_t m, float* out) {
  if (int rc = check_idx(idx, "pann_query_distances")) return rc;
  if (nq == 0 || m == 0) return PANN_OK;
  if (!queries || !ids || !out) { set_error("pann_query_distances: null argument"); return PANN_ERR_BAD_ARG; }
  if (q_stride_bytes < idx->ix.dbytes) { set_error("pann_query_distances: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  for (uint64_t i = 0; i < m; i++)
    if (ids[i] >= idx->ix.n) { set_error("pann_query_distances: id out of range"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  HostTrip t(idx);
  const int i_ids = t.in.add(ids, m * 4), i_q = t.in.add(queries, (nq - 1) * q_stride_bytes + idx->ix.dbytes, kQuerySlack);
  const int o_d = t.out.add(out, nq * m * 4);
  if (int rc = t.begin()) return rc;
  if (int rc = query_distances_dev(idx->ix, t.st, t.din<uint8_t>(i_q), q_stride_bytes, nullptr, nq, t.din<uint32_t>(i_ids), m, 0,
                                   t.dout<float>(o_d))) return rc;
  return t.finish();
}

int pann_leaf_knn_batch(pann_index* idx, const uint32_t* ids, const uint64_t* leaf_offsets, uint64_t nleaves,
                        uint32_t m, uint32_t* out_ids, float* out_dists) {
  if (int rc = check_idx_no4(idx, "pann_leaf_knn_batch")) return rc;
  if (nleaves == 0) return PANN_OK;
  if (!ids || !leaf_offsets || !out_ids || !out_dists) { set_error("pann_leaf_knn: null argument"); return PANN_ERR_BAD_ARG; }
  const uint64_t total = leaf_offsets[nleaves];
  if (total == 0) return PANN_OK;
  for (uint64_t i = 0; i < total; i++)
    if (ids[i] >= idx->ix.n) { set_error("pann_leaf_knn: id out of range"); return PANN_ERR_BAD_ARG; }
  for (uint64_t s = 0; s < nleaves; s++)
    if (leaf_offsets[s + 1] < leaf_offsets[s]) { set_error("pann_leaf_knn: offsets not monotone"); return PANN_ERR_BAD_ARG; }
  std::vector<uint32_t> tseg, ta0;
  append_tiles(leaf_offsets, nleaves, std::back_inserter(tseg), std::back_inserter(ta0));
  DeviceGuard g(idx->device);
  const size_t nt = tseg.size();
  HostTrip t(idx);
  const int i_off = t.in.add(leaf_offsets, (nleaves + 1) * 8), i_tseg = t.in.add(tseg.data(), nt * 4), i_ta0 = t.in.add(ta0.data(), nt * 4);
  const int i_ids = t.in.add(ids, total * 4);
  const int o_ids = t.out.add(out_ids, total * m * 4), o_dists = t.out.add(out_dists, total * m * 4);
  if (int rc = t.begin()) return rc;
  const uint32_t* d_ids = t.din<uint32_t>(i_ids);
  const uint64_t* d_off = t.din<uint64_t>(i_off);
  if (leaf_knn_rows_eligible(idx->ix, m)) {     // one-byte element types: lane-owns-row kernel (leaf_knn.hip)
    if (int rc = leaf_knn_rows_dev(idx->ix, idx->ws2, t.st, d_ids, d_off, leaf_offsets, nleaves, m, 1, t.dout<uint32_t>(o_ids),
                                   t.dout<float>(o_dists))) return rc;
  } else {
    DenseTopkCall c;
    c.a_ids = c.b_ids = d_ids; c.a_off = c.b_off = d_off; c.tile_seg = t.din<uint32_t>(i_tseg); c.tile_a0 = t.din<uint32_t>(i_ta0);
    c.ntiles = (uint32_t)nt; c.na = c.nb = total; c.m = m; c.exclude_same = 1;
    c.out_ids = t.dout<uint32_t>(o_ids); c.out_dists = t.dout<float>(o_dists);
    if (int rc = dense_topk_dev(idx->ix, idx->ws2, t.st, c)) return rc;
  }
  return t.finish();
}

int pann_leaf_knn(pann_index* idx, const uint32_t* ids, uint32_t N, uint32_t m, uint32_t* out_ids, float* out_dists) {
  const uint64_t off[2] = {0, N};
  return pann_leaf_knn_batch(idx, ids, off, 1, m, out_ids, out_dists);
}

// B is cut into nsplit pieces per A tile.  Every piece warms up its own top-k lists (about k * ln(piece / k) + k list inserts per
// query: 10K x 1M, k = 100 spent 7.5 G instructions there at 14 pieces), and at k = 100 the lists leave room for ONE workgroup
// per CU, so what matters is how evenly ntiles * nsplit workgroups fill whole rounds of the 256 CUs: the smallest count (<= 8,
// or enough to reach every CU when there are few queries) with the best fill wins (10K queries: 157 tiles x 3 = 1.84 rounds,
// 43 ms; x 1: 53 ms; x 14: 68 ms).  slots: 256 x the workgroups a CU holds (1 for the LDS-list kernels); nb: B rows.
static uint32_t choose_gt_pieces(const pann_index* idx, uint32_t ntiles, double slots, uint64_t nb) {
  uint32_t want = 1;
  double best = -1.0;
  const uint32_t smax = std::max<uint32_t>(8, ((uint32_t)slots + ntiles - 1) / ntiles);
  for (uint32_t sp = 1; sp <= smax; sp++) {
    const double wgs = (double)ntiles * sp;
    const double fill = wgs / (slots * std::ceil(wgs / slots)) - 0.02 * std::min<uint32_t>(sp, 8);
    if (fill > best + 1e-9) { best = fill; want = sp; }
  }
  const uint32_t env_split = idx->gt_pieces;      // pann_index_set_option("gt_pieces")
  const uint32_t nsplit = std::max<uint32_t>(1, std::min<uint32_t>(env_split ? env_split : want, (uint32_t)((nb + 4095) / 4096)));
  return std::min<uint32_t>(nsplit, 64);
}

int pann_bruteforce_knn(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                        uint32_t* out_ids, float* out_dists) {
  if (int rc = check_idx_no4(idx, "pann_bruteforce_knn")) return rc;
  if (nq == 0) return PANN_OK;
  if (!queries || !out_ids || !out_dists) { set_error("pann_bruteforce_knn: null argument"); return PANN_ERR_BAD_ARG; }
  if (q_stride_bytes < idx->ix.dbytes) { set_error("pann_bruteforce_knn: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  HostTrip t(idx);
  const int i_q = t.in.add(queries, (nq - 1) * q_stride_bytes + idx->ix.dbytes, kQuerySlack);
  const int o_ids = t.out.add(out_ids, nq * k * 4), o_dists = t.out.add(out_dists, nq * k * 4);
  if (int rc = t.begin()) return rc;
  DenseTopkCall c;
  c.a_ext = t.din<uint8_t>(i_q); c.a_stride = q_stride_bytes; c.ntiles = (uint32_t)((nq + 63) / 64); c.na = nq; c.nb = idx->ix.n;
  c.nsplit = choose_gt_pieces(idx, c.ntiles, (double)dense_gt_slots(idx->ix, k), idx->ix.n); c.m = k;
  c.out_ids = t.dout<uint32_t>(o_ids); c.out_dists = t.dout<float>(o_dists);
  if (int rc = dense_topk_dev(idx->ix, idx->ws2, t.st, c)) return rc;
  return t.finish();
}

// ---- exact kNN under a point filter (masked_knn.hip; DESIGN.md "Exact masked kNN", "Label predicates") ----

int pann_allow_count_dev(const uint32_t* d_allow, uint64_t n, uint64_t rows, uint64_t allow_stride_words, uint32_t* d_counts,
                         void* stream) {
  if (!d_allow || !d_counts) { set_error("pann_allow_count_dev: null argument"); return PANN_ERR_BAD_ARG; }
  if (n > 0xFFFFFFFFull) { set_error("pann_allow_count_dev: n must be < 2^32"); return PANN_ERR_BAD_ARG; }
  if (int rc = allow_stride_check("pann_allow_count_dev", "one row", allow_stride_words, n)) return rc;
  return allow_count_dev(d_allow, n, allow_stride_words ? rows : 1, allow_stride_words, d_counts, (hipStream_t)stream);
}

// everything that is refused, behind the handle's own checks, before anything is launched, allocated or written: the arguments, the filter,
// the queries and k -- one filter or a table is the dense route, k <= 128; one per query the scan, k <= 64 -- and, behind those, a table's rules
static int filtered_knn_checks(const pann_index* idx, const char* fn, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                               const PointFilter& F, const uint32_t* out_ids, const float* out_dists) {
  if (!queries || !out_ids || !out_dists) { set_error(std::string(fn) + ": null argument"); return PANN_ERR_BAD_ARG; }
  if (int rc = filter_checks(idx, fn, F, nq)) return rc;
  if (q_stride_bytes < idx->ix.dbytes) { set_error(std::string(fn) + ": query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  if (k == 0) { set_error(std::string(fn) + ": k == 0"); return PANN_ERR_BAD_ARG; }
  if (k > (F.per_query() ? 64u : 128u)) {
    set_error(std::string(fn) + (F.per_query() ? ": k > 64 with per-query bitmaps or predicates is not supported" : ": k > 128 is not supported"));
    return PANN_ERR_UNSUPPORTED;
  }
  return F.is_table() ? table_checks(idx, fn, F) : PANN_OK;
}

// The routes, on device pointers.  One bitmap: its id list, then the dense kernels on the list.  SYNCHRONISES st (the count sizes the launch).
static int masked_knn_run(pann_index* idx, const uint8_t* d_q, uint64_t nq, uint64_t q_stride_bytes, uint32_t k, const uint32_t* d_allow,
                          uint32_t* d_ids, float* d_dists, uint32_t* d_counts, hipStream_t st) {
  const DeviceIndex& ix = idx->ix;
  if (int rc = idx->ws3.ensure(allow_compact_scratch_bytes(ix.n))) return rc;
  const uint32_t* d_total = nullptr;
  if (int rc = allow_compact_count_dev(d_allow, ix.n, (uint32_t*)idx->ws3.buf, &d_total, st)) return rc;
  uint32_t count = 0;
  PANN_HIP(hipMemcpyAsync(&count, d_total, 4, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipStreamSynchronize(st));
  if (count == 0) return knn_pad_dev(d_ids, d_dists, d_counts, nq, k, 0, 1, st);       // an empty mask: no distance kernel
  if (int rc = idx->ws4.ensure((size_t)count * 4)) return rc;
  uint32_t* d_list = (uint32_t*)idx->ws4.buf;
  if (int rc = allow_compact_scatter_dev(d_allow, ix.n, (const uint32_t*)idx->ws3.buf, d_list, count, st)) return rc;
  // the list as B rows makes the launch one of the LDS-list kernels: one workgroup per CU
  DenseTopkCall c;
  c.a_ext = d_q; c.a_stride = q_stride_bytes; c.b_ids = d_list; c.ntiles = (uint32_t)((nq + 63) / 64); c.na = nq; c.nb = count;
  c.nsplit = choose_gt_pieces(idx, c.ntiles, 256.0, count); c.m = k; c.out_ids = d_ids; c.out_dists = d_dists;
  if (int rc = dense_topk_dev(ix, idx->ws2, st, c)) return rc;
  return knn_pad_dev(nullptr, nullptr, d_counts, nq, k, std::min(count, k), 0, st);
}

// One predicate for the batch: its bitmap row is expanded into the handle's scratch and the route above runs on it
static int labeled_knn_run(pann_index* idx, const uint8_t* d_q, uint64_t nq, uint64_t q_stride_bytes, uint32_t k, const PointFilter& F,
                           uint32_t* d_ids, float* d_dists, uint32_t* d_counts, hipStream_t st) {
  const DeviceIndex& ix = idx->ix;
  const uint64_t words = PointFilter::row_words(ix.n);
  if (int rc = idx->label_row.ensure((size_t)words * 4)) return rc;
  if (int rc = labels_to_allow_dev(F.labels, ix.n, F.kind, F.preds, 1, idx->label_row.as<uint32_t>(), words, st)) return rc;
  return masked_knn_run(idx, d_q, nq, q_stride_bytes, k, idx->label_row.as<uint32_t>(), d_ids, d_dists, d_counts, st);
}

// ---- exact kNN by predicate group (masked_knn.hip, DESIGN.md "Exact kNN by predicate group") ----

// the medoid form of the grouped route (pann_filter_medoids_*): ONE query per table entry, the entry's centroid, made on the device from
// the entry's id list instead of gathered from the caller's queries; d_centroids (optional): G x d floats
struct CentroidReq { float* d_centroids; };

// A table of filters.  SYNCHRONISES st once: the flag of the range check, the queries per table entry and the allowed points per
// table entry come back in one read, and the chunks, segments and tiles are planned from them (grouped_plan.h).
// cen != null: nq == T.count, d_q and T.group are not read -- query g belongs to entry g and is that entry's centroid.
static int grouped_knn_run(pann_index* idx, const char* fn, const uint8_t* d_q, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                           const PointFilter& T, uint64_t max_list_ids, uint32_t* d_ids, float* d_dists, uint32_t* d_counts, hipStream_t st,
                           const CentroidReq* cen = nullptr) {
  const DeviceIndex& ix = idx->ix;
  const uint64_t G = T.count, words = PointFilter::row_words(ix.n), stride = T.stride ? T.stride : words;
  const bool lab = T.mode == MASK_LABELS;
  // ---- before the read-back: sort the queries by table index, count what every entry allows ----
  uint32_t nblocks; uint64_t per_block;
  group_sort_shape(nq, G, &nblocks, &per_block);
  const size_t head_words = 1 + 2 * (size_t)G;       // flag | queries per entry | allowed points per entry
  uint32_t *d_head, *d_off, *d_part, *d_perm;      // the head is read back as one block; d_perm: the slots, then (cen) the iota table indices
  if (int rc = carve_into(idx->grp_sort, 0, [&](Carve& c) {
    d_head = c.take<uint32_t>(head_words); d_off = c.take<uint32_t>(G + 1); d_part = c.take<uint32_t>((size_t)nblocks * G);
    d_perm = c.take<uint32_t>((size_t)nq + (cen ? (size_t)nq : 0));
  })) return rc;
  uint32_t* d_hist = d_head + 1, *d_allowed = d_hist + G;
  const uint32_t* d_group = T.group;
  if (cen) { if (int rc = subset_iota_dev(d_perm + nq, nullptr, nq, st)) return rc; d_group = d_perm + nq; }
  if (int rc = group_queries_dev(d_group, nq, G, d_head, d_hist, d_off, d_part, d_perm, st)) return rc;
  if (lab) { if (int rc = label_count_dev(T.labels, ix.n, T.kind, T.preds, G, d_allowed, st)) return rc; }
  else if (int rc = allow_count_dev(T.allow, ix.n, G, stride, d_allowed, st)) return rc;
  if (int rc = idx->grp_pin.ensure(head_words * 4)) return rc;
  PANN_HIP(hipMemcpyAsync(idx->grp_pin.p, d_head, head_words * 4, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipStreamSynchronize(st));
  const std::vector<uint32_t> head((const uint32_t*)idx->grp_pin.p, (const uint32_t*)idx->grp_pin.p + head_words);
  if (head[0]) { set_error(std::string(fn) + ": a query's table index is out of range (>= " + std::to_string(G) + ")"); return PANN_ERR_BAD_ARG; }
  const uint32_t* hist = head.data() + 1, *allowed = hist + G;
  // ---- the plan, written into pinned memory (the read-back has been copied out of it) ----
  const uint64_t budget = grouped_budget(max_list_ids);
  const GroupedPlan plan(hist, allowed, G, budget, grouped_row_cap(budget, words, lab));
  const size_t U = plan.used.size();
  if (int rc = idx->grp_pin.ensure(plan.plan_bytes)) return rc;
  uint8_t* hp = (uint8_t*)idx->grp_pin.p;
  plan.write(allowed, hp);
  // ---- device room for the largest chunk, then the plan goes up in one transfer ----
  const uint32_t a_stride = (ix.dbytes + 15) / 16 * 16;
  uint8_t* dp; pann_label_pred* d_upreds;      // the plan goes up as one block; the predicates of the used entries (label form)
  if (int rc = carve_into(idx->grp_plan, 0, [&](Carve& c) {
    dp = c.take<uint8_t>(plan.plan_bytes); d_upreds = c.take<pann_label_pred>(lab ? U : 0);
  })) return rc;
  uint32_t *d_rows, *d_bc;      // a chunk's bitmap rows (label form) and the block counts of their compaction
  if (int rc = carve_into(idx->grp_rows, 0, [&](Carve& c) {
    d_rows = c.take<uint32_t>(lab ? plan.max_rows * words : 0);
    d_bc = (uint32_t*)c.take<uint8_t>(allow_rows_compact_scratch_bytes(ix.n, plan.max_rows));
  })) return rc;
  if (int rc = idx->ws4.ensure(std::max<size_t>(plan.max_ids, 1) * 4)) return rc;
  if (cen) {      // the pieces of every chunk's lists and the room for their sums (grouped_plan.h)
    size_t need = 0;
    for (const GroupedChunk& c : plan.chunks)
      need = std::max(need, CentroidScratch(c.u1 - c.u0, centroid_chunk_pieces(plan, c, allowed), centroid_row_sums(ix.dbytes, ix.esize)).bytes);
    if (int rc = idx->grp_cen.ensure(need)) return rc;
  }
  uint8_t* d_slab; uint32_t* d_sids; float* d_sdists;      // a chunk's query rows and its staged results
  if (int rc = carve_into(idx->grp_io, 0, [&](Carve& c) {
    d_slab = c.take<uint8_t>(plan.max_na * a_stride, kQuerySlack);
    d_sids = c.take<uint32_t>(plan.max_na * k); d_sdists = c.take<float>(plan.max_na * k);
  })) return rc;
  PANN_HIP(hipMemcpyAsync(dp, hp, plan.plan_bytes, hipMemcpyHostToDevice, st));
  const uint32_t* d_used = (const uint32_t*)dp;
  if (lab) { if (int rc = gather_preds_dev(T.preds, d_used, U, d_upreds, st)) return rc; }
  uint32_t* d_list = idx->ws4.as<uint32_t>();
  // ---- per chunk: id lists (CSR), query slab, ONE segmented dense launch, rows back to the caller's order ----
  for (const GroupedChunk& c : plan.chunks) {
    const uint32_t S = (uint32_t)(c.u1 - c.u0);
    if (c.ids) {
      if (lab) {
        if (int rc = labels_to_allow_dev(T.labels, ix.n, T.kind, d_upreds + c.u0, S, d_rows, words, st)) return rc;
        if (int rc = allow_rows_compact_dev(d_rows, ix.n, nullptr, words, S, d_bc, d_list, (uint32_t)c.ids, st)) return rc;
      } else if (int rc = allow_rows_compact_dev(T.allow, ix.n, d_used + c.u0, stride, S, d_bc, d_list, (uint32_t)c.ids, st)) return rc;
    }
    if (cen) {      // one query per entry: slab row s is the centroid of list s
      if (int rc = centroid_rows_dev(ix, st, d_list, (const uint64_t*)(dp + c.o_boff), S, centroid_chunk_pieces(plan, c, allowed), idx->grp_cen.buf, d_perm + c.a_base, d_slab,
                                     a_stride, cen->d_centroids)) return rc;
    } else if (int rc = gather_query_rows_dev(d_q, q_stride_bytes, ix.dbytes, d_perm + c.a_base, c.na, d_slab, a_stride, st)) return rc;
    // the lists as B rows: the LDS-list kernels, one workgroup per CU (as masked_knn_run); the pieces cut every segment's list
    DenseTopkCall call;
    call.a_ext = d_slab; call.a_stride = a_stride; call.b_ids = d_list;
    call.a_off = (const uint64_t*)(dp + c.o_aoff); call.b_off = (const uint64_t*)(dp + c.o_boff);
    call.tile_seg = (const uint32_t*)(dp + c.o_tseg); call.tile_a0 = (const uint32_t*)(dp + c.o_ta0);
    call.ntiles = c.ntiles; call.na = c.na; call.nb = c.ids; call.nsplit = choose_gt_pieces(idx, c.ntiles, 256.0, c.max_ids); call.m = k;
    call.out_ids = d_sids; call.out_dists = d_sdists;
    if (int rc = dense_topk_dev(ix, idx->ws2, st, call)) return rc;
    if (int rc = scatter_knn_rows_dev(d_sids, d_sdists, d_perm + c.a_base, c.na, k, d_ids, d_dists, d_counts, st)) return rc;
  }
  return PANN_OK;
}

// the route of a filter: a table -> grouped; one per query -> the scan, which synchronises nothing; one predicate -> its row, then
// as one bitmap; one bitmap -> compaction and the dense kernels
static int filtered_knn_run(pann_index* idx, const char* fn, const uint8_t* d_q, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                            const PointFilter& F, uint64_t max_list_ids, uint32_t* d_ids, float* d_dists, uint32_t* d_counts, hipStream_t st) {
  if (F.is_table()) return grouped_knn_run(idx, fn, d_q, nq, q_stride_bytes, k, F, max_list_ids, d_ids, d_dists, d_counts, st);
  if (F.per_query()) return filter_scan_dev(idx->ix, st, d_q, q_stride_bytes, nq, F, k, d_ids, d_dists, d_counts);
  if (F.mode == MASK_LABELS) return labeled_knn_run(idx, d_q, nq, q_stride_bytes, k, F, d_ids, d_dists, d_counts, st);
  return masked_knn_run(idx, d_q, nq, q_stride_bytes, k, F.allow, d_ids, d_dists, d_counts, st);
}

static int filtered_knn_dev(pann_index* idx, const char* fn, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                            const PointFilter& F, uint64_t max_list_ids, uint32_t* d_ids, float* d_dists, uint32_t* d_counts, void* stream) {
  if (int rc = check_idx_no4(idx, fn)) return rc;
  if (nq == 0) return PANN_OK;
  if (int rc = filtered_knn_checks(idx, fn, d_queries, nq, q_stride_bytes, k, F, d_ids, d_dists)) return rc;
  DeviceGuard g(idx->device);
  return filtered_knn_run(idx, fn, (const uint8_t*)d_queries, nq, q_stride_bytes, k, F, max_list_ids, d_ids, d_dists, d_counts, (hipStream_t)stream);
}

static int filtered_knn_host(pann_index* idx, const char* fn, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                             const PointFilter& F, uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts) {
  if (int rc = check_idx_no4(idx, fn)) return rc;
  if (nq == 0) return PANN_OK;
  if (int rc = filtered_knn_checks(idx, fn, queries, nq, q_stride_bytes, k, F, out_ids, out_dists)) return rc;
  for (uint64_t q = 0; F.is_table() && q < nq; q++)      // the index array is checked on the host: nothing is staged for a call that will be refused
    if (F.group[q] >= F.count) {
      set_error(std::string(fn) + ": table index " + std::to_string(F.group[q]) + " of query " + std::to_string(q) + " is out of range (>= " + std::to_string(F.count) + ")");
      return PANN_ERR_BAD_ARG;
    }
  DeviceGuard g(idx->device);
  // in: the filter and the queries; out: counts, ids and dists (the small one first: ids and dists can be large enough to travel on their own)
  HostTrip t(idx);
  const StagedFilter staged(t, &F, idx->ix.n, nq);
  const int i_q = t.in.add(queries, (nq - 1) * q_stride_bytes + idx->ix.dbytes, kQuerySlack);
  const size_t row_bytes = (size_t)nq * k * 4;
  const int o_counts = t.out.add(out_counts, nq * 4), o_ids = t.out.add(out_ids, row_bytes), o_dists = t.out.add(out_dists, row_bytes);
  if (int rc = t.begin()) return rc;
  if (int rc = filtered_knn_run(idx, fn, t.din<uint8_t>(i_q), nq, q_stride_bytes, k, staged.on_device(t), max_list_ids, t.dout<uint32_t>(o_ids),
                                t.dout<float>(o_dists), t.dout<uint32_t>(o_counts), t.st)) return rc;
  return t.finish();
}

int pann_bruteforce_knn_masked_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                   const uint32_t* d_allow, uint64_t allow_stride_words, uint32_t* d_out_ids, float* d_out_dists,
                                   uint32_t* d_out_counts, void* stream) {
  return filtered_knn_dev(idx, "pann_bruteforce_knn_masked_dev", d_queries, nq, q_stride_bytes, k,
                          PointFilter::bitmap(d_allow, allow_stride_words, nq, true), 0, d_out_ids, d_out_dists, d_out_counts, stream);
}

int pann_bruteforce_knn_masked(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                               const uint32_t* allow, uint64_t allow_stride_words, uint32_t* out_ids, float* out_dists,
                               uint32_t* out_counts) {
  return filtered_knn_host(idx, "pann_bruteforce_knn_masked", queries, nq, q_stride_bytes, k,
                           PointFilter::bitmap(allow, allow_stride_words, nq, false), 0, out_ids, out_dists, out_counts);
}

int pann_bruteforce_knn_labeled_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                    int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t* d_out_ids,
                                    float* d_out_dists, uint32_t* d_out_counts, void* stream) {
  return filtered_knn_dev(idx, "pann_bruteforce_knn_labeled_dev", d_queries, nq, q_stride_bytes, k, label_filter(idx, kind, d_preds, npreds, true), 0,
                          d_out_ids, d_out_dists, d_out_counts, stream);
}

int pann_bruteforce_knn_labeled(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k, int kind,
                                const pann_label_pred* preds, uint64_t npreds, uint32_t* out_ids, float* out_dists,
                                uint32_t* out_counts) {
  return filtered_knn_host(idx, "pann_bruteforce_knn_labeled", queries, nq, q_stride_bytes, k, label_filter(idx, kind, preds, npreds, false), 0,
                           out_ids, out_dists, out_counts);
}

// the two helpers: a device output that is there and aligned, then the predicates' checks -- one row or count each, so any number is "one per query"
static int label_helper_checks(const pann_index* idx, const char* fn, const PointFilter& F, const uint32_t* d_out) {
  if (int rc = check_idx(idx, fn)) return rc;
  if (!d_out) { set_error(std::string(fn) + ": null output"); return PANN_ERR_BAD_ARG; }
  if ((uintptr_t)d_out % 4 != 0) { set_error(std::string(fn) + ": the output must be 4-byte aligned"); return PANN_ERR_BAD_ARG; }
  return filter_checks(idx, fn, F, F.count);
}

int pann_labels_to_allow_dev(pann_index* idx, int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t* d_allow,
                             uint64_t allow_stride_words, void* stream) {
  const PointFilter F = label_filter(idx, kind, d_preds, npreds, true);
  if (int rc = label_helper_checks(idx, "pann_labels_to_allow_dev", F, d_allow)) return rc;
  if (allow_stride_words < PointFilter::row_words(idx->ix.n)) {
    set_error("pann_labels_to_allow_dev: allow_stride_words must be at least ceil(n / 32) = " + std::to_string(PointFilter::row_words(idx->ix.n)));
    return PANN_ERR_BAD_ARG;
  }
  DeviceGuard g(idx->device);
  return labels_to_allow_dev(F.labels, idx->ix.n, kind, d_preds, npreds, d_allow, allow_stride_words, (hipStream_t)stream);
}

int pann_label_count_dev(pann_index* idx, int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t* d_counts,
                         void* stream) {
  const PointFilter F = label_filter(idx, kind, d_preds, npreds, true);
  if (int rc = label_helper_checks(idx, "pann_label_count_dev", F, d_counts)) return rc;
  DeviceGuard g(idx->device);
  return label_count_dev(F.labels, idx->ix.n, kind, d_preds, npreds, d_counts, (hipStream_t)stream);
}

int pann_bruteforce_knn_labeled_grouped_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                            int kind, const pann_label_pred* d_preds, uint64_t npreds, const uint32_t* d_group_of_query,
                                            uint64_t max_list_ids, uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                            void* stream) {
  return filtered_knn_dev(idx, "pann_bruteforce_knn_labeled_grouped_dev", d_queries, nq, q_stride_bytes, k,
                          label_filter(idx, kind, d_preds, npreds, true).as_table(d_group_of_query, npreds), max_list_ids, d_out_ids, d_out_dists,
                          d_out_counts, stream);
}

int pann_bruteforce_knn_masked_grouped_dev(pann_index* idx, const void* d_queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                           const uint32_t* d_allow, uint64_t nrows, uint64_t allow_stride_words,
                                           const uint32_t* d_row_of_query, uint64_t max_list_ids, uint32_t* d_out_ids, float* d_out_dists,
                                           uint32_t* d_out_counts, void* stream) {
  return filtered_knn_dev(idx, "pann_bruteforce_knn_masked_grouped_dev", d_queries, nq, q_stride_bytes, k,
                          PointFilter::bitmap(d_allow, allow_stride_words, nq, true).as_table(d_row_of_query, nrows), max_list_ids, d_out_ids,
                          d_out_dists, d_out_counts, stream);
}

int pann_bruteforce_knn_labeled_grouped(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k, int kind,
                                        const pann_label_pred* preds, uint64_t npreds, const uint32_t* group_of_query,
                                        uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts) {
  return filtered_knn_host(idx, "pann_bruteforce_knn_labeled_grouped", queries, nq, q_stride_bytes, k,
                           label_filter(idx, kind, preds, npreds, false).as_table(group_of_query, npreds), max_list_ids, out_ids, out_dists,
                           out_counts);
}

int pann_bruteforce_knn_masked_grouped(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, uint32_t k,
                                       const uint32_t* allow, uint64_t nrows, uint64_t allow_stride_words, const uint32_t* row_of_query,
                                       uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts) {
  return filtered_knn_host(idx, "pann_bruteforce_knn_masked_grouped", queries, nq, q_stride_bytes, k,
                           PointFilter::bitmap(allow, allow_stride_words, nq, false).as_table(row_of_query, nrows), max_list_ids, out_ids, out_dists,
                           out_counts);
}

}  // extern "C"

// ---- entry points: the medoids of a table of filters (entry_points.hip, DESIGN.md "Entry points") ----

// the table of a medoid call: the G filters themselves, no index array; a NULL bitmap with one row is "every point"
static bool medoid_all_points(const PointFilter& F) { return F.mode == MASK_BITMAP && !F.allow && F.count == 1; }
static PointFilter medoid_bitmap_table(const uint32_t* allow, uint64_t nrows, uint64_t stride, bool dev) {
  PointFilter f = PointFilter::bitmap(allow, stride, nrows, dev);
  f.count = nrows;
  return f;
}

// what the grouped twins refuse, in their order: the handle, the outputs, the filter, per_filter as their k, the table
static int filter_medoids_checks(const pann_index* idx, const char* fn, const PointFilter& F, uint32_t per_filter, const uint32_t* out_ids,
                                 const float* out_dists) {
  if (int rc = check_idx_no4(idx, fn)) return rc;
  if (!out_ids || !out_dists) { set_error(std::string(fn) + ": null argument"); return PANN_ERR_BAD_ARG; }
  if (!medoid_all_points(F)) { if (int rc = filter_checks(idx, fn, F, F.count)) return rc; }
  if (per_filter == 0) { set_error(std::string(fn) + ": per_filter == 0"); return PANN_ERR_BAD_ARG; }
  if (per_filter > 128) { set_error(std::string(fn) + ": per_filter > 128 is not supported"); return PANN_ERR_UNSUPPORTED; }
  return table_checks(idx, fn, F, false);
}

// T: the table on the device.  The grouped route with one query per entry, made there; then the padding takes the caller's id.
static int filter_medoids_run(pann_index* idx, const char* fn, PointFilter T, uint32_t per_filter, uint32_t fill_id, uint64_t max_list_ids,
                              uint32_t* d_ids, float* d_dists, uint32_t* d_counts, float* d_centroids, hipStream_t st) {
  if (medoid_all_points(T)) {      // one row of all ones (bits at positions >= n are ignored)
    const size_t row = (size_t)PointFilter::row_words(idx->ix.n) * 4;
    if (int rc = idx->label_row.ensure(row)) return rc;
    PANN_HIP(hipMemsetAsync(idx->label_row.buf, 0xFF, row, st));
    T.allow = idx->label_row.as<uint32_t>(); T.stride = 0;
  }
  const CentroidReq cen{d_centroids};
  if (int rc = grouped_knn_run(idx, fn, nullptr, T.count, 0, per_filter, T.as_table(nullptr, T.count), max_list_ids, d_ids, d_dists, d_counts, st,
                               &cen)) return rc;
  return pad_fill_dev(d_ids, T.count * per_filter, fill_id, st);
}

static int filter_medoids_dev(pann_index* idx, const char* fn, const PointFilter& F, uint32_t per_filter, uint32_t fill_id, uint64_t max_list_ids,
                              uint32_t* d_ids, float* d_dists, uint32_t* d_counts, float* d_centroids, void* stream) {
  if (int rc = filter_medoids_checks(idx, fn, F, per_filter, d_ids, d_dists)) return rc;
  DeviceGuard g(idx->device);
  return filter_medoids_run(idx, fn, F, per_filter, fill_id, max_list_ids, d_ids, d_dists, d_counts, d_centroids, (hipStream_t)stream);
}

static int filter_medoids_host(pann_index* idx, const char* fn, const PointFilter& F, uint32_t per_filter, uint32_t fill_id, uint64_t max_list_ids,
                               uint32_t* out_ids, float* out_dists, uint32_t* out_counts, float* out_centroids) {
  if (int rc = filter_medoids_checks(idx, fn, F, per_filter, out_ids, out_dists)) return rc;
  DeviceGuard g(idx->device);
  const uint64_t G = F.count;
  HostTrip t(idx);
  const bool all = medoid_all_points(F);
  const StagedFilter staged(t, all ? nullptr : &F, idx->ix.n, G);
  const size_t row_bytes = (size_t)G * per_filter * 4;
  const int o_counts = t.out.add(out_counts, G * 4), o_ids = t.out.add(out_ids, row_bytes), o_dists = t.out.add(out_dists, row_bytes);
  const int o_cen = t.out.add(out_centroids, (size_t)G * idx->ix.d * 4);
  if (int rc = t.begin()) return rc;
  PointFilter T = all ? F : staged.on_device(t);
  T.dev = true; T.count = G;
  if (int rc = filter_medoids_run(idx, fn, T, per_filter, fill_id, max_list_ids, t.dout<uint32_t>(o_ids), t.dout<float>(o_dists),
                                  t.dout<uint32_t>(o_counts), t.dout<float>(o_cen), t.st)) return rc;
  return t.finish();
}

extern "C" {

int pann_filter_medoids_labeled_dev(pann_index* idx, int kind, const pann_label_pred* d_preds, uint64_t npreds, uint32_t per_filter,
                                    uint32_t fill_id, uint64_t max_list_ids, uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                    float* d_out_centroids, void* stream) {
  PointFilter F = label_filter(idx, kind, d_preds, npreds, true);
  F.count = npreds;
  return filter_medoids_dev(idx, "pann_filter_medoids_labeled_dev", F, per_filter, fill_id, max_list_ids, d_out_ids, d_out_dists, d_out_counts,
                            d_out_centroids, stream);
}

int pann_filter_medoids_masked_dev(pann_index* idx, const uint32_t* d_allow, uint64_t nrows, uint64_t allow_stride_words, uint32_t per_filter,
                                   uint32_t fill_id, uint64_t max_list_ids, uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                   float* d_out_centroids, void* stream) {
  return filter_medoids_dev(idx, "pann_filter_medoids_masked_dev", medoid_bitmap_table(d_allow, nrows, allow_stride_words, true), per_filter,
                            fill_id, max_list_ids, d_out_ids, d_out_dists, d_out_counts, d_out_centroids, stream);
}

int pann_filter_medoids_labeled(pann_index* idx, int kind, const pann_label_pred* preds, uint64_t npreds, uint32_t per_filter, uint32_t fill_id,
                                uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts, float* out_centroids) {
  PointFilter F = label_filter(idx, kind, preds, npreds, false);
  F.count = npreds;
  return filter_medoids_host(idx, "pann_filter_medoids_labeled", F, per_filter, fill_id, max_list_ids, out_ids, out_dists, out_counts,
                             out_centroids);
}

int pann_filter_medoids_masked(pann_index* idx, const uint32_t* allow, uint64_t nrows, uint64_t allow_stride_words, uint32_t per_filter,
                               uint32_t fill_id, uint64_t max_list_ids, uint32_t* out_ids, float* out_dists, uint32_t* out_counts,
                               float* out_centroids) {
  return filter_medoids_host(idx, "pann_filter_medoids_masked", medoid_bitmap_table(allow, nrows, allow_stride_words, false), per_filter, fill_id,
                             max_list_ids, out_ids, out_dists, out_counts, out_centroids);
}

int pann_pivot_split(pann_index* idx, const uint32_t* ids, const uint64_t* seg_offsets, uint64_t nseg,
                     const uint32_t* pivot_a, const uint32_t* pivot_b, uint8_t* out_side) {
  if (int rc = check_idx_no4(idx, "pann_pivot_split")) return rc;
  if (nseg == 0) return PANN_OK;
  if (!ids || !seg_offsets || !pivot_a || !pivot_b || !out_side) { set_error("pann_pivot_split: null argument"); return PANN_ERR_BAD_ARG; }
  const uint64_t total = seg_offsets[nseg];
  if (total == 0) return PANN_OK;
  for (uint64_t i = 0; i < total; i++)
    if (ids[i] >= idx->ix.n) { set_error("pann_pivot_split: id out of range"); return PANN_ERR_BAD_ARG; }
  std::vector<uint32_t> tseg, tcnt; std::vector<uint64_t> tlo;
  for (uint64_t s = 0; s < nseg; s++) {
    if (pivot_a[s] >= idx->ix.n || pivot_b[s] >= idx->ix.n) { set_error("pann_pivot_split: pivot out of range"); return PANN_ERR_BAD_ARG; }
    for (uint64_t a = seg_offsets[s]; a < seg_offsets[s + 1]; a += 64) {
      tseg.push_back((uint32_t)s); tlo.push_back(a); tcnt.push_back((uint32_t)std::min<uint64_t>(64, seg_offsets[s + 1] - a));
    }
  }
  DeviceGuard g(idx->device);
  const size_t nt = tseg.size();
  HostTrip t(idx);
  const int i_pa = t.in.add(pivot_a, nseg * 4), i_pb = t.in.add(pivot_b, nseg * 4);
  const int i_tseg = t.in.add(tseg.data(), nt * 4), i_tcnt = t.in.add(tcnt.data(), nt * 4), i_tlo = t.in.add(tlo.data(), nt * 8);
  const int i_ids = t.in.add(ids, total * 4);
  const int o_side = t.out.add(out_side, total);
  if (int rc = t.begin()) return rc;
  if (int rc = pivot_split_dev(idx->ix, t.st, t.din<uint32_t>(i_ids), t.din<uint32_t>(i_tseg), t.din<uint64_t>(i_tlo),
                               t.din<uint32_t>(i_tcnt), (uint32_t)nt, t.din<uint32_t>(i_pa), t.din<uint32_t>(i_pb),
                               t.dout<uint8_t>(o_side))) return rc;
  return t.finish();
}


int pann_rerank(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, const uint32_t* cand_ids,
                uint32_t c, const uint32_t* cand_counts, uint32_t k, int resort, uint32_t* out_ids, float* out_dists) {
  if (int rc = check_idx_no4(idx, "pann_rerank")) return rc;
  if (nq == 0) return PANN_OK;
  if (!queries || !cand_ids || !out_ids || !out_dists || k == 0) { set_error("pann_rerank: null argument"); return PANN_ERR_BAD_ARG; }
  if (q_stride_bytes < idx->ix.dbytes) { set_error("pann_rerank: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  for (uint64_t i = 0; i < nq; i++) {
    const uint32_t cn = cand_counts ? std::min(cand_counts[i], c) : c;
    for (uint32_t j = 0; j < cn; j++)
      if (cand_ids[i * c + j] >= idx->ix.n) { set_error("pann_rerank: candidate id out of range"); return PANN_ERR_BAD_ARG; }
  }
  DeviceGuard g(idx->device);
  HostTrip t(idx);
  const int i_cnt = t.in.add(cand_counts, nq * 4), i_q = t.in.add(queries, (nq - 1) * q_stride_bytes + idx->ix.dbytes, kQuerySlack);
  const int i_cand = t.in.add(cand_ids, nq * c * 4);
  const int o_ids = t.out.add(out_ids, nq * k * 4), o_dists = t.out.add(out_dists, nq * k * 4);
  if (int rc = t.begin()) return rc;
  if (int rc = rerank_dev(idx->ix, t.st, t.din<uint8_t>(i_q), q_stride_bytes, nq, t.din<uint32_t>(i_cand), c, t.din<uint32_t>(i_cnt), k,
                          resort, t.dout<uint32_t>(o_ids), t.dout<float>(o_dists))) return rc;
  return t.finish();
}


// The tail of a range call, whose first output piece is the counts and whose id rows are the scratch piece o_ids.  The counts
// come down and are waited for; of the id rows only the columns any query filled come back, straight into the caller's rows
// (max_results is a cap, the rows are mostly empty; entries past a row's count are unspecified: include/pann.h); then the
// other outputs in one transfer.
static int download_range_results(HostTrip& t, int o_ids, uint64_t nq, uint32_t max_results, uint32_t* out_ids, const uint32_t* out_counts) {
  if (int rc = t.fetch_head(1)) return rc;
  uint32_t widest = 0;
  for (uint64_t i = 0; i < nq; i++) widest = std::max(widest, out_counts[i]);
  widest = std::min(widest, max_results);
  if (widest)
    PANN_HIP(hipMemcpy2DAsync(out_ids, (size_t)max_results * 4, t.dout<uint32_t>(o_ids), (size_t)max_results * 4, (size_t)widest * 4, nq,
                              hipMemcpyDeviceToHost, t.st));
  return t.finish();
}

int pann_range_search(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                      uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, int starts_per_query,
                      float radius_2, uint32_t max_results, uint32_t* out_ids, uint32_t* out_counts,
                      uint32_t* out_dist_cmps, uint32_t* out_truncated) {
  if (int rc = check_idx_no4(idx, "pann_range_search")) return rc;
  if (nq == 0) return PANN_OK;
  const DeviceIndex& ix = idx->ix;
  if ((queries == nullptr) == (query_ids == nullptr)) { set_error("pann_range_search: exactly one of queries / query_ids must be given"); return PANN_ERR_BAD_ARG; }
  if (!starts || nstarts == 0 || !out_ids || !out_counts || max_results == 0) { set_error("pann_range_search: null or empty argument"); return PANN_ERR_BAD_ARG; }
  if (queries && q_stride_bytes < ix.dbytes) { set_error("pann_range_search: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  if (query_ids)
    for (uint64_t i = 0; i < nq; i++)
      if (query_ids[i] >= ix.n) { set_error("pann_range_search: query id out of range"); return PANN_ERR_BAD_ARG; }
  const uint64_t ns_total = (starts_per_query ? nq : 1) * (uint64_t)nstarts;
  for (uint64_t i = 0; i < ns_total; i++)
    if (starts[i] != SENTINEL && starts[i] >= ix.n) { set_error("pann_range_search: start id out of range"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  HostTrip t(idx);
  const int i_st = t.in.add(starts, ns_total * 4);
  const int i_q = queries ? t.in.add(queries, (nq - 1) * q_stride_bytes + ix.dbytes, kQuerySlack) : t.in.add(query_ids, nq * 4);
  const int o_counts = t.out.add(out_counts, nq * 4);
  const int o_cmps = t.out.add_or_scratch(out_dist_cmps, nq * 4), o_trunc = t.out.add_or_scratch(out_truncated, nq * 4);
  const int o_ids = t.out.add_scratch(nq * (size_t)max_results * 4);
  if (int rc = t.begin()) return rc;
  if (int rc = range_search_dev(ix, idx->ws, t.st, queries ? t.din<uint8_t>(i_q) : nullptr, q_stride_bytes,
                                queries ? nullptr : t.din<uint32_t>(i_q), nq, t.din<uint32_t>(i_st), nstarts, starts_per_query, radius_2,
                                max_results, t.dout<uint32_t>(o_ids), t.dout<uint32_t>(o_counts), t.dout<uint32_t>(o_cmps),
                                t.dout<uint32_t>(o_trunc))) return rc;
  return download_range_results(t, o_ids, nq, max_results, out_ids, out_counts);
}


// a NULL handle where no device exists is the missing device, not a caller's mistake: the two entry points below say so
static int check_idx_or_device(const pann_index* idx, const char* fn) {
  if (!idx && pann_device_count() <= 0) { set_error(std::string(fn) + ": no HIP device visible (this library has no CPU path)"); return PANN_ERR_NO_DEVICE; }
  return check_idx(idx, fn);
}

int pann_bruteforce_range(pann_index* idx, const void* queries, uint64_t nq, uint64_t q_stride_bytes, float radius,
                          uint64_t* out_offsets, uint32_t* out_ids, uint64_t ids_capacity) {
  if (int rc = check_idx_or_device(idx, "pann_bruteforce_range")) return rc;
  if (int rc = refuse_4bit(idx, "pann_bruteforce_range")) return rc;
  if (std::isnan(radius)) { set_error("pann_bruteforce_range: radius is NaN"); return PANN_ERR_BAD_ARG; }
  if (!out_offsets) { set_error("pann_bruteforce_range: null out_offsets"); return PANN_ERR_BAD_ARG; }
  if (nq == 0) { out_offsets[0] = 0; return PANN_OK; }
  if (!queries) { set_error("pann_bruteforce_range: null queries"); return PANN_ERR_BAD_ARG; }
  if (q_stride_bytes < idx->ix.dbytes) { set_error("pann_bruteforce_range: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  const DeviceIndex& ix = idx->ix;
  HostTrip t(idx);
  const int i_q = t.in.add(queries, (nq - 1) * q_stride_bytes + ix.dbytes, kQuerySlack);
  const int o_off = t.out.add(out_offsets, (nq + 1) * 8);
  if (int rc = t.begin()) return rc;
  const uint8_t* d_q = t.din<uint8_t>(i_q);
  const uint32_t nsplit = range_join_pieces(ix, nq, idx->gt_pieces);       // pann_index_set_option("gt_pieces")
  if (int rc = range_join_count_dev(ix, idx->ws2, t.st, d_q, q_stride_bytes, nq, radius, nsplit, t.dout<uint64_t>(o_off))) return rc;
  if (int rc = t.finish()) return rc;
  const uint64_t total = out_offsets[nq];
  if (!out_ids) return PANN_OK;                                            // count only
  if (ids_capacity < total) {
    set_error("pann_bruteforce_range: " + std::to_string(total) + " matches, room for " + std::to_string(ids_capacity));
    return PANN_ERR_OVERFLOW;
  }
  if (total == 0) return PANN_OK;
  HostTrip fill(idx);       // a second trip for the ids, now that their number is known: no inputs, so the queries stay where they are
  const int o_ids = fill.out.add(out_ids, total * 4);
  if (int rc = fill.begin()) return rc;
  if (int rc = range_join_fill_dev(ix, idx->ws2, fill.st, d_q, q_stride_bytes, nq, radius, nsplit, fill.dout<uint32_t>(o_ids))) return rc;
  return fill.finish();
}

int pann_range_query(pann_index* idx, const void* queries, const uint32_t* query_ids, uint64_t nq,
                     uint64_t q_stride_bytes, const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp,
                     float radius, uint32_t max_results, uint32_t* out_ids, uint32_t* out_counts,
                     uint32_t* out_search_cmps, uint32_t* out_visited, uint32_t* out_range_cmps,
                     uint32_t* out_truncated) {
  if (int rc = check_idx_or_device(idx, "pann_range_query")) return rc;
  if (int rc = refuse_4bit(idx, "pann_range_query")) return rc;
  const DeviceIndex& ix = idx->ix;
  if (!qp) { set_error("pann_range_query: null params"); return PANN_ERR_BAD_ARG; }
  if (int rc = k_beam_check(qp)) return rc;
  if (qp->beam < 1 || qp->beam > 0x7FFFFFFF) { set_error("pann_range_query: beam out of range"); return PANN_ERR_BAD_ARG; }
  if ((queries == nullptr) == (query_ids == nullptr)) { set_error("pann_range_query: exactly one of queries / query_ids must be given"); return PANN_ERR_BAD_ARG; }
  if (!starts || nstarts == 0) { set_error("beam search expects at least one start point"); return PANN_ERR_BAD_ARG; }
  if (std::isnan(radius) || !out_ids || !out_counts || max_results == 0) { set_error("pann_range_query: null, empty or NaN argument"); return PANN_ERR_BAD_ARG; }
  if (queries && q_stride_bytes < ix.dbytes) { set_error("pann_range_query: query stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  for (uint32_t i = 0; i < nstarts; i++)
    if (starts[i] >= ix.n) { set_error("pann_range_query: start point out of range"); return PANN_ERR_BAD_ARG; }
  if (query_ids)
    for (uint64_t i = 0; i < nq; i++)
      if (query_ids[i] >= ix.n) { set_error("pann_range_query: query id out of range"); return PANN_ERR_BAD_ARG; }
  if (nq == 0) return PANN_OK;
  DeviceGuard g(idx->device);
  const uint32_t beam = (uint32_t)qp->beam;
  HostTrip t(idx);
  hipStream_t st = t.st;
  // ---- inputs go up once: the queries (or their ids) and the shared starts ----
  const int i_st = t.in.add(starts, (size_t)nstarts * 4);
  const int i_q = queries ? t.in.add(queries, (nq - 1) * q_stride_bytes + ix.dbytes, kQuerySlack) : t.in.add(query_ids, nq * 4);
  // ---- outputs: the counts first (download_range_results); the frontiers never leave the device ----
  const int o_counts = t.out.add(out_counts, nq * 4);
  const int o_rcmps = t.out.add_or_scratch(out_range_cmps, nq * 4), o_trunc = t.out.add_or_scratch(out_truncated, nq * 4);
  const int o_scmps = t.out.add_or_scratch(out_search_cmps, nq * 4), o_vis = t.out.add_or_scratch(out_visited, nq * 4);
  const int o_ids = t.out.add_scratch(nq * (size_t)max_results * 4), o_front = t.out.add_scratch(nq * (size_t)beam * 4);
  if (int rc = t.begin()) return rc;
  const uint8_t* d_q = queries ? t.din<uint8_t>(i_q) : nullptr;
  const uint32_t* d_qid = queries ? nullptr : t.din<uint32_t>(i_q);
  // ---- round 1: the beam search; a launch that reports a full dropped list is grown and repeated (as batch_search_host) ----
  SearchCall round1;      // on the staged copies: the frontiers (beam ids per query) and the two counters
  round1.queries = d_q; round1.qstride = q_stride_bytes; round1.query_ids = d_qid; round1.nq = nq;
  round1.starts = t.din<uint32_t>(i_st); round1.nstarts = nstarts; round1.qp = qp; round1.dev = true; round1.stream = st;
  round1.out.ids = t.dout<uint32_t>(o_front); round1.out.out_k = beam;
  round1.out.dist_cmps = t.dout<uint32_t>(o_scmps); round1.out.visited_count = t.dout<uint32_t>(o_vis);
  uint32_t status = 0;
  bool whole = false;
  if (int rc = run_with_dropped_growth(idx->dcap, ix.n, nq, qp->limit, "pann_range_query", &status, &whole, &g_err,
      [&](uint64_t q0, uint64_t cnt, uint32_t dcap, uint32_t* st_word) -> int {
      const SearchArgs a = slice(round1, q0, cnt, dcap);
      if (int rc = idx->ws.ensure(search_workspace_bytes(ix, a))) return rc;
      if (int rc = launch_beam_search(ix, a, idx->ws.buf, idx->ws.bytes, st)) return rc;
      PANN_HIP(hipMemcpyAsync(st_word, (uint8_t*)idx->ws.buf + 64, 4, hipMemcpyDeviceToHost, st));
      PANN_HIP(hipStreamSynchronize(st));
      return PANN_OK;
    })) return rc;
  // ---- round 2: the BFS, seeded per query with its frontier as it lies on the device (SENTINEL padding is skipped) ----
  if (int rc = range_search_dev(ix, idx->ws, st, d_q, q_stride_bytes, d_qid, nq, t.dout<uint32_t>(o_front), beam, 1, radius, max_results,
                                t.dout<uint32_t>(o_ids), t.dout<uint32_t>(o_counts), t.dout<uint32_t>(o_rcmps),
                                t.dout<uint32_t>(o_trunc))) return rc;
  if (int rc = download_range_results(t, o_ids, nq, max_results, out_ids, out_counts)) return rc;
  if (idx->ws.bytes > (2ull << 30)) idx->ws.release();          // a one-off worst-case scratch is not kept on the handle
  return PANN_OK;
}

int pann_hcnng_build_trees_dev(pann_index* idx, uint32_t first_tree, uint32_t tree_step, uint32_t ntrees, uint32_t cluster_size,
                               uint32_t mst_deg, uint64_t seed, uint32_t* d_slab, uint32_t slab_stride, double* times3) {
  if (int rc = check_idx_no4(idx, "pann_hcnng_build_trees_dev")) return rc;
  if (mst_deg == 0 || tree_step == 0 || !d_slab) { set_error("pann_hcnng_build_trees_dev: null / zero argument"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  hipLaunchKernelGGL(fill_u32_kernel, dim3(2048), dim3(256), 0, idx->stream, d_slab, idx->ix.n * (uint64_t)slab_stride, SENTINEL);
  PANN_HIP(hipGetLastError());
  if (ntrees == 0) { PANN_HIP(hipStreamSynchronize(idx->stream)); return PANN_OK; }
  return hcnng_build_dev(idx->ix, idx->ws2, idx->stream, ntrees, cluster_size, mst_deg, seed, times3, first_tree, tree_step, d_slab, slab_stride);
}

int pann_hcnng_assemble_dev(pann_index* idx, const uint32_t* d_slabs, uint32_t nslabs, uint32_t slab_stride, uint32_t ntrees,
                            uint32_t mst_deg) {
  if (int rc = check_idx_no4(idx, "pann_hcnng_assemble_dev")) return rc;
  if (!d_slabs || mst_deg == 0) { set_error("pann_hcnng_assemble_dev: null / zero argument"); return PANN_ERR_BAD_ARG; }
  if ((uint64_t)ntrees * mst_deg > idx->ix.max_deg) { set_error("pann_hcnng_assemble_dev: max_deg < ntrees * mst_deg"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  idx->ix.codes_valid = 0;
  return hcnng_assemble_dev(idx->ix, idx->stream, d_slabs, nslabs, slab_stride, ntrees, mst_deg);
}

int pann_hcnng_build(pann_index* idx, uint32_t num_clusters, uint32_t cluster_size, uint32_t mst_deg, uint64_t seed,
                     double* times3) {
  if (int rc = check_idx_no4(idx, "pann_hcnng_build")) return rc;
  if (num_clusters == 0 || mst_deg == 0) { set_error("pann_hcnng_build: num_clusters and mst_deg must be positive"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  idx->ix.codes_valid = 0;
  return hcnng_build_dev(idx->ix, idx->ws2, idx->stream, num_clusters, cluster_size, mst_deg, seed, times3);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// scalar quantisation on the device (quantize.hip)
// ---------------------------------------------------------------------------------------------

namespace {

int check_quant_kind(int kind, const char* fn) {
  if (kind != PANN_QUANT_EUCLID_U8 && kind != PANN_QUANT_MIPS_I8 && kind != PANN_QUANT_EUCLID_U4 && kind != PANN_QUANT_MIPS_I4) { set_error(std::string(fn) + ": unknown quantisation kind"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}
int check_quant_rows(const float* rows, uint64_t n, uint32_t d, uint64_t stride, const char* fn) {
  if (!rows || n == 0 || d == 0) { set_error(std::string(fn) + ": null/empty rows (n * d == 0)"); return PANN_ERR_BAD_ARG; }
  if (stride < 4ull * d || stride % 4 != 0) { set_error(std::string(fn) + ": row stride smaller than a row or not a multiple of 4"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}
int check_quant_params(const pann_quant_params* p, const char* fn) {
  if (!p) { set_error(std::string(fn) + ": null parameters"); return PANN_ERR_BAD_ARG; }
  if (int rc = check_quant_kind(p->kind, fn)) return rc;
  if (p->dims <= 0) { set_error(std::string(fn) + ": parameters without dimensions"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}
int check_quant_source(const pann_index* src, int kind, const char* fn) {
  if (int rc = check_idx(src, fn)) return rc;
  if (src->ix.dtype != PANN_F32) { set_error(std::string(fn) + ": the source index must hold float (PANN_F32) points"); return PANN_ERR_UNSUPPORTED; }
  if (int rc = check_quant_kind(kind, fn)) return rc;
  if (quant_kind_is_euclid(kind) != (src->ix.metric == PANN_L2)) {
    set_error(std::string(fn) + ": kind does not fit the index's metric (EUCLID_U8 / EUCLID_U4 <-> L2, MIPS_I8 / MIPS_I4 <-> MIPS)"); return PANN_ERR_BAD_ARG;
  }
  return PANN_OK;
}

// scratch of the handle-less _dev form: one small buffer per device, allocated on first use; the lock is held for the call
// (pann_quantize_params_dev synchronises anyway)
std::mutex g_qscratch_mu;
Workspace g_qscratch[64];

// The handle-free host forms (pann_quantize_rows, pann_sketch_rows): n host rows of floats go through the current device a slice of
// 256 MiB at a time (query sets are small; a base that is not resident streams through here) -- dense copy up, per_slice(d_in, cnt,
// d_out) on the null stream, dense copy of the out_row_bytes results down.  The two slice buffers are freed on every way out.
template <class PerSlice>
int rows_through_device(const float* rows, uint64_t n, uint64_t stride_bytes, size_t in_row_bytes, void* out, uint64_t out_stride_bytes,
                        size_t out_row_bytes, PerSlice&& per_slice) {
  const uint64_t slice = std::max<uint64_t>(1, (256ull << 20) / in_row_bytes);
  Workspace in, ob;
  auto done = [&](int rc) { in.release(); ob.release(); return rc; };
  const uint64_t cap = std::min(slice, n);
  if (int rc = in.ensure(cap * in_row_bytes)) return done(rc);
  if (int rc = ob.ensure(cap * out_row_bytes)) return done(rc);
  for (uint64_t r0 = 0; r0 < n; r0 += slice) {
    const uint64_t cnt = std::min(slice, n - r0);
    hipError_t e = hipMemcpy2D(in.buf, in_row_bytes, (const uint8_t*)rows + r0 * stride_bytes, stride_bytes, in_row_bytes, cnt, hipMemcpyHostToDevice);
    if (e != hipSuccess) return done(hip_fail(e, "hipMemcpy2D(rows)"));
    if (int rc = per_slice(in.as<float>(), cnt, ob.buf)) return done(rc);
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return done(hip_fail(e, "hipStreamSynchronize"));
    e = hipMemcpy2D((uint8_t*)out + r0 * out_stride_bytes, out_stride_bytes, ob.buf, out_row_bytes, out_row_bytes, cnt, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(hip_fail(e, "hipMemcpy2D(out)"));
  }
  return done(PANN_OK);
}

}  // namespace

extern "C" {

void pann_quantize_select_ranks(uint64_t len, int trim, uint64_t* a, uint64_t* b) {
  if (!a || !b || len == 0) return;
  quant_select_ranks(len, trim, a, b);
}

int pann_index_normalize(pann_index* idx) {
  if (int rc = check_idx_no4(idx, "pann_index_normalize")) return rc;
  DeviceIndex& ix = idx->ix;
  if (ix.dtype != PANN_F32) { set_error("pann_index_normalize: float (PANN_F32) handles only"); return PANN_ERR_UNSUPPORTED; }
  DeviceGuard g(idx->device);
  if (int rc = quant_normalize_dev(reinterpret_cast<const float*>(ix.points), ix.n, ix.d, ix.pstride, nullptr, ix.points, ix.pstride, idx->stream)) return rc;
  PANN_HIP(hipStreamSynchronize(idx->stream));
  return PANN_OK;
}

int pann_quantize_params(pann_index* src, int kind, int trim, pann_quant_params* out) {
  if (int rc = check_quant_source(src, kind, "pann_quantize_params")) return rc;
  if (!out) { set_error("pann_quantize_params: null output"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(src->device);
  if (int rc = src->params_scratch.ensure(quant_scratch_bytes())) return rc;
  const DeviceIndex& ix = src->ix;
  return quant_params_dev(reinterpret_cast<const float*>(ix.points), ix.n, ix.d, ix.pstride, kind, trim, out, src->params_scratch.buf, src->stream);
}

int pann_quantize_params_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride_bytes, int kind, int trim,
                             pann_quant_params* out, void* stream) {
  if (int rc = check_quant_kind(kind, "pann_quantize_params_dev")) return rc;
  if (int rc = check_quant_rows(d_rows, n, d, stride_bytes, "pann_quantize_params_dev")) return rc;
  if (!out) { set_error("pann_quantize_params_dev: null output"); return PANN_ERR_BAD_ARG; }
  int dev = 0;
  PANN_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) { set_error("pann_quantize_params_dev: device ordinal out of range"); return PANN_ERR_BAD_ARG; }
  std::lock_guard<std::mutex> lk(g_qscratch_mu);
  if (int rc = g_qscratch[dev].ensure(quant_scratch_bytes())) return rc;
  return quant_params_dev(d_rows, n, d, stride_bytes, kind, trim, out, g_qscratch[dev].buf, (hipStream_t)stream);
}

int pann_index_create_quantized(pann_index** out, pann_index* src, const pann_quant_params* p, int copy_graph) {
  if (!out) { set_error("pann_index_create_quantized: null output"); return PANN_ERR_BAD_ARG; }
  if (int rc = check_quant_params(p, "pann_index_create_quantized")) return rc;
  if (int rc = check_quant_source(src, p->kind, "pann_index_create_quantized")) return rc;
  const DeviceIndex& sx = src->ix;
  if ((uint32_t)p->dims != sx.d) { set_error("pann_index_create_quantized: parameters made for another dimension"); return PANN_ERR_BAD_ARG; }
  const int qdt = quant_kind_dtype(p->kind);
  pann_index* q = nullptr;
  if (int rc = index_create_impl(&q, nullptr, sx.n, sx.d, qdt, row_bytes_of(qdt, sx.d), quant_kind_is_euclid(p->kind) ? PANN_L2 : PANN_MIPS, nullptr,
                                 sx.max_deg, src->device)) return rc;
  DeviceGuard g(src->device);
  auto fail = [&](int rc) { pann_index_destroy(q); return rc; };
  // the new handle's rows are zero (pad bytes included) and its stream is idle; src's stream orders the reads of src
  if (int rc = quant_translate_dev(p, reinterpret_cast<const float*>(sx.points), sx.n, sx.d, sx.pstride, q->ix.points, q->ix.pstride, src->stream)) return fail(rc);
  hipError_t e;
  if (copy_graph && (e = hipMemcpyAsync(q->ix.graph, sx.graph, (size_t)sx.n * sx.gstride * 4, hipMemcpyDeviceToDevice, src->stream)) != hipSuccess)
    return fail(hip_fail(e, "hipMemcpyAsync(graph)"));
  if ((e = hipStreamSynchronize(src->stream)) != hipSuccess) return fail(hip_fail(e, "hipStreamSynchronize"));
  *out = q;
  return PANN_OK;
}

// ---- subset index (subset.hip, DESIGN.md "Subset index"): a new handle over the rows of src that a bitmap keeps ----

static int subset_checks(pann_index* const* out, const pann_index* src, const char* fn) {
  if (!out) { set_error(std::string(fn) + ": null output"); return PANN_ERR_BAD_ARG; }
  return check_idx(src, fn);
}

// The first half: m = the points d_allow keeps (null: all of them), counted on st and waited for -- the ONE synchronisation
// before anything is allocated -- and every check that needs m.  The block offsets of the count stay in src->ws3 for the
// scatter of subset_build.  *kept_out is written as soon as m is known, whatever the checks behind it say.
static int subset_count(pann_index* src, const char* fn, const uint32_t* d_allow, uint64_t n_out, bool want_new_to_old,
                        uint64_t new_to_old_cap, uint64_t* kept_out, uint64_t* m_out, uint64_t* rows_out, hipStream_t st) {
  const std::string f = fn;
  const uint64_t n = src->ix.n;
  if (n_out >= 0x7FFFFFFFull) { set_error(f + ": n_out must be < 2^31 - 1 (as n of pann_index_create)"); return PANN_ERR_BAD_ARG; }
  uint64_t m = n;
  if (d_allow) {
    if (int rc = src->ws3.ensure(allow_compact_scratch_bytes(n))) return rc;
    const uint32_t* d_total = nullptr;
    if (int rc = allow_compact_count_dev(d_allow, n, src->ws3.as<uint32_t>(), &d_total, st)) return rc;
    uint32_t count = 0;
    PANN_HIP(hipMemcpyAsync(&count, d_total, 4, hipMemcpyDeviceToHost, st));
    PANN_HIP(hipStreamSynchronize(st));
    m = count;
  }
  if (kept_out) *kept_out = m;
  if (n_out && n_out < m) {
    set_error(f + ": the bitmap keeps " + std::to_string(m) + " points, n_out has room for " + std::to_string(n_out)); return PANN_ERR_BAD_ARG;
  }
  if (m == 0 && n_out == 0) { set_error(f + ": the bitmap keeps no point and n_out is 0: the new handle would have no rows"); return PANN_ERR_BAD_ARG; }
  if (want_new_to_old && new_to_old_cap < m) {
    set_error(f + ": " + std::to_string(m) + " kept points, new_to_old has room for " + std::to_string(new_to_old_cap)); return PANN_ERR_OVERFLOW;
  }
  *m_out = m; *rows_out = n_out ? n_out : m;
  return PANN_OK;
}

// everything that is enqueued on st once the new handle q exists (zero rows, empty graph, idle stream: index_create_impl)
static int subset_fill(pann_index* q, pann_index* src, const uint32_t* d_allow, uint64_t m, int copy_graph, uint32_t* d_new_to_old,
                       uint32_t* d_old_to_new, hipStream_t st) {
  const DeviceIndex& sx = src->ix;
  DeviceIndex& qx = q->ix;
  const uint64_t n = sx.n, rows = qx.n;
  qx.exact = sx.exact; qx.lpc = sx.lpc; qx.nch = sx.nch;        // the exact-float-order flag (same dbytes: same pstride)
  if (sx.labels) {
    if (int rc = q->labels_buf.ensure((size_t)rows * 4)) return rc;
    if (rows > m) PANN_HIP(hipMemsetAsync(q->labels_buf.as<uint32_t>() + m, 0, (size_t)(rows - m) * 4, st));
    qx.labels = q->labels_buf.as<uint32_t>();
  }
  if (sx.sketch) {
    if (int rc = q->sketch_buf.ensure((size_t)rows * sx.sk_stride)) return rc;
    if (rows > m) PANN_HIP(hipMemsetAsync(q->sketch_buf.as<uint8_t>() + (size_t)m * sx.sk_stride, 0, (size_t)(rows - m) * sx.sk_stride, st));
    qx.sketch = q->sketch_buf.as<uint8_t>(); qx.sk_stride = sx.sk_stride; qx.sk_kind = sx.sk_kind; qx.sk_as_written = sx.sk_as_written;
    q->sk_params = src->sk_params;
  }
  if (!d_allow) {      // everything is kept (m == n): the rows as they are, and the identity for the maps
    PANN_HIP(hipMemcpyAsync(qx.points, sx.points, (size_t)n * sx.pstride, hipMemcpyDeviceToDevice, st));
    if (copy_graph) PANN_HIP(hipMemcpyAsync(qx.graph, sx.graph, (size_t)n * sx.gstride * 4, hipMemcpyDeviceToDevice, st));
    if (sx.labels) PANN_HIP(hipMemcpyAsync(q->labels_buf.buf, sx.labels, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    if (sx.sketch) PANN_HIP(hipMemcpyAsync(q->sketch_buf.buf, sx.sketch, (size_t)n * sx.sk_stride, hipMemcpyDeviceToDevice, st));
    return subset_iota_dev(d_new_to_old, d_old_to_new, n, st);
  }
  if (m) { if (int rc = allow_compact_scatter_dev(d_allow, n, src->ws3.as<uint32_t>(), d_new_to_old, (uint32_t)m, st)) return rc; }
  if (d_old_to_new) { if (int rc = subset_invert_dev(d_new_to_old, m, d_old_to_new, n, st)) return rc; }
  if (int rc = subset_gather_rows_dev(sx.points, qx.points, sx.pstride, d_new_to_old, m, st)) return rc;
  if (sx.labels) { if (int rc = subset_gather_rows_dev(sx.labels, q->labels_buf.buf, 4, d_new_to_old, m, st)) return rc; }
  if (sx.sketch) { if (int rc = subset_gather_rows_dev(sx.sketch, q->sketch_buf.buf, sx.sk_stride, d_new_to_old, m, st)) return rc; }
  if (copy_graph) return subset_renumber_graph_dev(sx.graph, qx.graph, sx.gstride, d_new_to_old, d_old_to_new, n, m, st);
  return PANN_OK;
}

// The second half, on device pointers: allocate (scratch on src for a map the caller did not ask for, then the new handle), enqueue
// on st.  NOT synchronised: the caller waits for st before it hands *q_out on.  Nothing is enqueued before everything is allocated
// but the labels and the sketch of the new handle itself.
static int subset_build(pann_index** q_out, pann_index* src, const uint32_t* d_allow, uint64_t m, uint64_t rows, int copy_graph,
                        uint32_t* d_new_to_old, uint32_t* d_old_to_new, hipStream_t st) {
  const DeviceIndex& sx = src->ix;
  if (d_allow && m && !d_new_to_old) {
    if (int rc = src->ws4.ensure((size_t)m * 4)) return rc;
    d_new_to_old = src->ws4.as<uint32_t>();
  }
  if (d_allow && m && copy_graph && !d_old_to_new) {
    if (int rc = src->ws2.ensure((size_t)sx.n * 4)) return rc;
    d_old_to_new = src->ws2.as<uint32_t>();
  }
  pann_index* q = nullptr;
  if (int rc = index_create_impl(&q, nullptr, rows, sx.d, sx.dtype, row_bytes_of(sx.dtype, sx.d), sx.metric, nullptr, sx.max_deg, src->device)) return rc;
  if (int rc = subset_fill(q, src, d_allow, m, copy_graph, d_new_to_old, d_old_to_new, st)) {
    (void)hipStreamSynchronize(st);      // nothing of q may still be written when it goes
    pann_index_destroy(q);
    return rc;
  }
  *q_out = q;
  return PANN_OK;
}

int pann_index_create_subset_dev(pann_index** out, pann_index* src, const uint32_t* d_allow, uint64_t n_out, int copy_graph,
                                 uint32_t* d_new_to_old, uint64_t new_to_old_cap, uint32_t* d_old_to_new, uint64_t* kept_out) {
  const char* fn = "pann_index_create_subset_dev";
  if (int rc = subset_checks(out, src, fn)) return rc;
  if ((uintptr_t)d_allow % 4 != 0 || (uintptr_t)d_new_to_old % 4 != 0 || (uintptr_t)d_old_to_new % 4 != 0) {
    set_error(std::string(fn) + ": device pointers must be 4-byte aligned"); return PANN_ERR_BAD_ARG;
  }
  DeviceGuard g(src->device);
  hipStream_t st = src->stream;
  uint64_t m = 0, rows = 0;
  if (int rc = subset_count(src, fn, d_allow, n_out, d_new_to_old != nullptr, new_to_old_cap, kept_out, &m, &rows, st)) return rc;
  pann_index* q = nullptr;
  if (int rc = subset_build(&q, src, d_allow, m, rows, copy_graph, d_new_to_old, d_old_to_new, st)) return rc;
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) { pann_index_destroy(q); return hip_fail(e, "hipStreamSynchronize"); }
  *out = q;
  return PANN_OK;
}

int pann_index_create_subset(pann_index** out, pann_index* src, const uint32_t* allow, uint64_t n_out, int copy_graph,
                             uint32_t* new_to_old, uint64_t new_to_old_cap, uint32_t* old_to_new, uint64_t* kept_out) {
  const char* fn = "pann_index_create_subset";
  if (int rc = subset_checks(out, src, fn)) return rc;
  DeviceGuard g(src->device);
  const uint64_t n = src->ix.n;
  // up: the bitmap, ceil(n / 32) words; the count decides what comes down, so the maps travel in a trip of their own
  HostTrip up(src);
  const int i_allow = up.in.add(allow, (size_t)((n + 31) / 32) * 4);
  if (allow) { if (int rc = up.begin()) return rc; }
  const uint32_t* d_allow = allow ? up.din<uint32_t>(i_allow) : nullptr;
  uint64_t m = 0, rows = 0;
  if (int rc = subset_count(src, fn, d_allow, n_out, new_to_old != nullptr, new_to_old_cap, kept_out, &m, &rows, up.st)) return rc;
  HostTrip down(src);       // no inputs: the bitmap stays where it is
  const int o_n2o = down.out.add(new_to_old, (size_t)m * 4), o_o2n = down.out.add(old_to_new, (size_t)n * 4);
  if (int rc = down.begin()) return rc;
  pann_index* q = nullptr;
  if (int rc = subset_build(&q, src, d_allow, m, rows, copy_graph, down.dout<uint32_t>(o_n2o), down.dout<uint32_t>(o_o2n), down.st)) return rc;
  if (int rc = down.finish()) { pann_index_destroy(q); return rc; }      // waits for the stream: the new handle is complete
  *out = q;
  return PANN_OK;
}

// ---- graph reachability (graph_reach.hip, DESIGN.md "Graph reachability"): BFS levels from a set of starts, degrees ----

namespace {

// the scratch of one walk, all of it in idx->ws3: the counter block (the bad-start flag, then the frontier lengths of one group
// of rounds), the visited and the unreached bitmap, the block offsets of the compaction, the two frontier queues
struct ReachScratch {
  uint32_t *flag, *lens, *visited, *unreached, *compact, *queue[2];
  int place(pann_index* idx) {
    const uint64_t n = idx->ix.n;
    const size_t words = (size_t)((n + 31) / 32);
    if (int rc = carve_into(idx->ws3, 0, [&](Carve& c) {
      flag = c.take<uint32_t>(64);      // the counter block: 256 bytes cleared as one, the lengths behind the flag
      visited = c.take<uint32_t>(words); unreached = c.take<uint32_t>(words);
      compact = (uint32_t*)c.take<uint8_t>(allow_compact_scratch_bytes(n));
      queue[0] = c.take<uint32_t>(n); queue[1] = c.take<uint32_t>(n);
    })) return rc;
    lens = flag + 1;
    return PANN_OK;
  }
};
static_assert((2 + REACH_GROUP) * 4 <= 256, "the counter block holds the flag and REACH_GROUP + 1 frontier lengths");

struct EventPair {      // t_s of pann_reach_stats: two events around the call's work on the stream
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  int start(hipStream_t st) { PANN_HIP(hipEventCreate(&a)); PANN_HIP(hipEventCreate(&b)); PANN_HIP(hipEventRecord(a, st)); return PANN_OK; }
  int stop(hipStream_t st) { PANN_HIP(hipEventRecord(b, st)); return PANN_OK; }
  int seconds(double* out) { float ms = 0; PANN_HIP(hipEventElapsedTime(&ms, a, b)); *out = (double)ms * 1e-3; return PANN_OK; }      // after b has completed
};

int reach_checks(const pann_index* idx, const char* fn, const uint32_t* starts, uint32_t nstarts) {
  if (int rc = check_idx(idx, fn)) return rc;
  if (!starts || nstarts == 0) { set_error(std::string(fn) + ": no start vertex"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

// The walk and the count, on device pointers.  The seeds go into the scratch alone; d_level (optional, n words) is first written
// once the flag has come back clear.  Rounds are enqueued in groups of REACH_GROUP with one read-back of their frontier lengths
// per group.  Everything of *rs but t_s; st has drained when it returns.
int reach_walk(pann_index* idx, const char* fn, const uint32_t* d_starts, uint32_t nstarts, const uint32_t* d_consider,
               uint32_t max_rounds, uint32_t* d_level, ReachScratch& s, pann_reach_stats* rs, hipStream_t st) {
  const DeviceIndex& ix = idx->ix;
  const uint64_t n = ix.n, words = (n + 31) / 32;
  if (int rc = s.place(idx)) return rc;
  PANN_HIP(hipMemsetAsync(s.flag, 0, 256, st));
  PANN_HIP(hipMemsetAsync(s.visited, 0, (size_t)words * 4, st));
  if (int rc = reach_seed_dev(d_starts, nstarts, n, s.visited, s.queue[0], s.lens, s.flag, st)) return rc;
  uint32_t h[2 + REACH_GROUP] = {0};
  PANN_HIP(hipMemcpyAsync(h, s.flag, 8, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipStreamSynchronize(st));
  if (h[0]) { set_error(std::string(fn) + ": a start vertex is out of range (>= number of points); nothing was written"); return PANN_ERR_BAD_ARG; }
  if (d_level) {
    PANN_HIP(hipMemsetAsync(d_level, 0xFF, (size_t)n * 4, st));
    if (int rc = reach_level0_dev(s.queue[0], s.lens, n, d_level, st)) return rc;
  }
  uint64_t frontier = h[1], reached = h[1], max_frontier = h[1];
  uint32_t levels = 1, rounds = 0, cur = 0, truncated = 0;
  while (frontier) {
    if (max_rounds && rounds == max_rounds) { truncated = 1; break; }
    const uint32_t g = max_rounds ? std::min(REACH_GROUP, max_rounds - rounds) : REACH_GROUP;
    PANN_HIP(hipMemsetAsync(s.lens + 1, 0, (size_t)g * 4, st));
    for (uint32_t j = 0; j < g; j++)
      if (int rc = reach_expand_dev(ix, s.queue[(cur + j) & 1], s.lens + j, s.queue[(cur + j + 1) & 1], s.lens + j + 1, s.visited,
                                    d_level, rounds + j + 1, st)) return rc;
    PANN_HIP(hipMemcpyAsync(h + 1, s.lens + 1, (size_t)g * 4, hipMemcpyDeviceToHost, st));
    PANN_HIP(hipMemcpyAsync(s.lens, s.lens + g, 4, hipMemcpyDeviceToDevice, st));      // the last frontier opens the next group
    PANN_HIP(hipStreamSynchronize(st));
    for (uint32_t j = 1; j <= g && frontier; j++) {
      frontier = h[j];
      if (!frontier) break;
      reached += frontier; max_frontier = std::max(max_frontier, frontier); levels++;
    }
    rounds += g; cur = (cur + g) & 1;
  }
  if (int rc = reach_finish_dev(s.visited, d_consider, n, s.unreached, st)) return rc;
  const uint32_t* d_total = nullptr;
  if (int rc = allow_compact_count_dev(s.unreached, n, s.compact, &d_total, st)) return rc;
  uint32_t count = 0;
  PANN_HIP(hipMemcpyAsync(&count, d_total, 4, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipStreamSynchronize(st));
  rs->reached = reached; rs->unreached = count; rs->max_frontier = max_frontier; rs->levels = levels; rs->truncated = truncated;
  rs->t_s = 0;
  return PANN_OK;
}

// what leaves the scratch after the walk: the reached bitmap (the visited bitmap as it is: no bit at or past n was ever set) and
// the ascending list of the rs.unreached ids; either may be null
int reach_emit(pann_index* idx, const ReachScratch& s, const pann_reach_stats& rs, uint32_t* d_reached, uint32_t* d_ids, hipStream_t st) {
  const uint64_t n = idx->ix.n;
  if (d_reached) PANN_HIP(hipMemcpyAsync(d_reached, s.visited, (size_t)((n + 31) / 32) * 4, hipMemcpyDeviceToDevice, st));
  if (d_ids && rs.unreached) return allow_compact_scatter_dev(s.unreached, n, s.compact, d_ids, (uint32_t)rs.unreached, st);
  return PANN_OK;
}

int reach_overflow(const char* fn, const pann_reach_stats& rs, uint64_t cap) {
  set_error(std::string(fn) + ": " + std::to_string(rs.unreached) + " unreached vertices, unreached_ids has room for " + std::to_string(cap));
  return PANN_ERR_OVERFLOW;
}

}  // namespace

int pann_graph_reach_dev(pann_index* idx, const uint32_t* d_starts, uint32_t nstarts, const uint32_t* d_consider,
                         uint32_t max_rounds, uint32_t* d_level, uint32_t* d_reached, uint32_t* d_unreached_ids,
                         uint64_t unreached_cap, pann_reach_stats* stats) {
  const char* fn = "pann_graph_reach_dev";
  if (int rc = reach_checks(idx, fn, d_starts, nstarts)) return rc;
  if ((uintptr_t)d_starts % 4 != 0 || (uintptr_t)d_consider % 4 != 0 || (uintptr_t)d_level % 4 != 0 || (uintptr_t)d_reached % 4 != 0 ||
      (uintptr_t)d_unreached_ids % 4 != 0) {
    set_error(std::string(fn) + ": device pointers must be 4-byte aligned"); return PANN_ERR_BAD_ARG;
  }
  DeviceGuard g(idx->device);
  hipStream_t st = idx->stream;
  EventPair ev;
  if (int rc = ev.start(st)) return rc;
  ReachScratch s;
  pann_reach_stats rs{};
  if (int rc = reach_walk(idx, fn, d_starts, nstarts, d_consider, max_rounds, d_level, s, &rs, st)) return rc;
  const bool overflow = d_unreached_ids && unreached_cap < rs.unreached;
  if (int rc = reach_emit(idx, s, rs, d_reached, overflow ? nullptr : d_unreached_ids, st)) return rc;
  if (int rc = ev.stop(st)) return rc;
  PANN_HIP(hipStreamSynchronize(st));
  if (int rc = ev.seconds(&rs.t_s)) return rc;
  if (stats) *stats = rs;
  return overflow ? reach_overflow(fn, rs, unreached_cap) : PANN_OK;
}

int pann_graph_reach(pann_index* idx, const uint32_t* starts, uint32_t nstarts, const uint32_t* consider,
                     uint32_t max_rounds, uint32_t* level, uint32_t* reached, uint32_t* unreached_ids,
                     uint64_t unreached_cap, pann_reach_stats* stats) {
  const char* fn = "pann_graph_reach";
  if (int rc = reach_checks(idx, fn, starts, nstarts)) return rc;
  const uint64_t n = idx->ix.n, words = (n + 31) / 32;
  for (uint32_t i = 0; i < nstarts; i++)
    if (starts[i] >= n) { set_error(std::string(fn) + ": start " + std::to_string(starts[i]) + " out of range; nothing was written"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  // up: the starts and the bitmap; the unreached count decides what comes down, so the outputs travel in a trip of their own
  // (as pann_index_create_subset) and the levels are walked in the handle's scratch
  HostTrip up(idx);
  const int i_starts = up.in.add(starts, (size_t)nstarts * 4), i_consider = up.in.add(consider, (size_t)words * 4);
  if (int rc = up.begin()) return rc;
  EventPair ev;
  if (int rc = ev.start(up.st)) return rc;
  uint32_t* d_level = nullptr;
  if (level) { if (int rc = idx->ws4.ensure((size_t)n * 4)) return rc; d_level = idx->ws4.as<uint32_t>(); }
  ReachScratch s;
  pann_reach_stats rs{};
  if (int rc = reach_walk(idx, fn, up.din<uint32_t>(i_starts), nstarts, up.din<uint32_t>(i_consider), max_rounds, d_level, s, &rs, up.st)) return rc;
  const bool overflow = unreached_ids && unreached_cap < rs.unreached;
  HostTrip down(idx);       // no inputs; the small pieces first
  const int o_reached = down.out.add(reached, (size_t)words * 4);
  const int o_ids = down.out.add(overflow ? nullptr : unreached_ids, (size_t)rs.unreached * 4);
  const int o_level = down.out.add(level, (size_t)n * 4);
  if (int rc = down.begin()) return rc;
  if (int rc = reach_emit(idx, s, rs, down.dout<uint32_t>(o_reached), down.dout<uint32_t>(o_ids), down.st)) return rc;
  if (level) PANN_HIP(hipMemcpyAsync(down.dout<uint32_t>(o_level), d_level, (size_t)n * 4, hipMemcpyDeviceToDevice, down.st));
  if (int rc = ev.stop(down.st)) return rc;
  if (int rc = down.finish()) return rc;
  if (int rc = ev.seconds(&rs.t_s)) return rc;
  if (stats) *stats = rs;
  return overflow ? reach_overflow(fn, rs, unreached_cap) : PANN_OK;
}

static int degrees_checks(const pann_index* idx, const char* fn, const uint32_t* out_deg, const uint32_t* in_deg) {
  if (int rc = check_idx(idx, fn)) return rc;
  if (!out_deg && !in_deg) { set_error(std::string(fn) + ": both outputs are null"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

int pann_graph_degrees_dev(pann_index* idx, uint32_t* d_out_deg, uint32_t* d_in_deg, void* stream) {
  const char* fn = "pann_graph_degrees_dev";
  if (int rc = degrees_checks(idx, fn, d_out_deg, d_in_deg)) return rc;
  if ((uintptr_t)d_out_deg % 4 != 0 || (uintptr_t)d_in_deg % 4 != 0) { set_error(std::string(fn) + ": device pointers must be 4-byte aligned"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  return graph_degrees_dev(idx->ix, d_out_deg, d_in_deg, (hipStream_t)stream);
}

int pann_graph_degrees(pann_index* idx, uint32_t* out_deg, uint32_t* in_deg) {
  if (int rc = degrees_checks(idx, "pann_graph_degrees", out_deg, in_deg)) return rc;
  DeviceGuard g(idx->device);
  HostTrip t(idx);
  const size_t bytes = (size_t)idx->ix.n * 4;
  const int o_out = t.out.add(out_deg, bytes), o_in = t.out.add(in_deg, bytes);
  if (int rc = t.begin()) return rc;
  if (int rc = graph_degrees_dev(idx->ix, t.dout<uint32_t>(o_out), t.dout<uint32_t>(o_in), t.st)) return rc;
  return t.finish();
}

int pann_quantize_rows_dev(const pann_quant_params* p, const float* d_rows, uint64_t n, uint64_t stride_bytes,
                           int normalize_first, void* d_out, uint64_t out_stride_bytes, void* stream) {
  if (int rc = check_quant_params(p, "pann_quantize_rows_dev")) return rc;
  if (int rc = check_quant_rows(d_rows, n, (uint32_t)p->dims, stride_bytes, "pann_quantize_rows_dev")) return rc;
  if (!d_out) { set_error("pann_quantize_rows_dev: null output"); return PANN_ERR_BAD_ARG; }
  if (out_stride_bytes < row_bytes_of(quant_kind_dtype(p->kind), (uint64_t)p->dims)) { set_error("pann_quantize_rows_dev: output stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  if (normalize_first) return quant_normalize_dev(d_rows, n, (uint32_t)p->dims, stride_bytes, p, d_out, out_stride_bytes, (hipStream_t)stream);
  return quant_translate_dev(p, d_rows, n, (uint32_t)p->dims, stride_bytes, d_out, out_stride_bytes, (hipStream_t)stream);
}

int pann_quantize_rows(const pann_quant_params* p, const float* rows, uint64_t n, uint64_t stride_bytes, int normalize_first,
                       void* out, uint64_t out_stride_bytes, int device) {
  if (int rc = check_quant_params(p, "pann_quantize_rows")) return rc;
  const uint32_t d = (uint32_t)p->dims;
  if (int rc = check_quant_rows(rows, n, d, stride_bytes, "pann_quantize_rows")) return rc;
  if (!out) { set_error("pann_quantize_rows: null output"); return PANN_ERR_BAD_ARG; }
  const uint64_t ob_row = row_bytes_of(quant_kind_dtype(p->kind), d);     // bytes of one output row: d, or ceil(d / 2) packed
  if (out_stride_bytes < ob_row) { set_error("pann_quantize_rows: output stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  const int ndev = pann_device_count();
  if (ndev <= 0) { set_error("pann_quantize_rows: no HIP device visible (this library has no CPU path)"); return PANN_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_error("pann_quantize_rows: device ordinal out of range"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(device);
  if (!g.ok) { set_error("pann_quantize_rows: hipSetDevice failed"); return PANN_ERR_HIP; }
  return rows_through_device(rows, n, stride_bytes, (size_t)d * 4, out, out_stride_bytes, ob_row,
      [&](const float* d_in, uint64_t cnt, void* d_ob) { return pann_quantize_rows_dev(p, d_in, cnt, (uint64_t)d * 4, normalize_first, d_ob, ob_row, nullptr); });
}

int pann_index_download_points(pann_index* idx, uint64_t first_row, uint64_t nrows, void* out, uint64_t out_stride_bytes) {
  if (int rc = check_idx(idx, "pann_index_download_points")) return rc;
  if (nrows == 0) return PANN_OK;
  const DeviceIndex& ix = idx->ix;
  if (!out) { set_error("pann_index_download_points: null output"); return PANN_ERR_BAD_ARG; }
  if (first_row > ix.n || nrows > ix.n - first_row) { set_error("pann_index_download_points: row range outside the index"); return PANN_ERR_BAD_ARG; }
  if (out_stride_bytes < ix.dbytes) { set_error("pann_index_download_points: row stride smaller than a row"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));
  const uint64_t slice = std::max<uint64_t>(1, (1ull << 30) / std::max<uint64_t>(out_stride_bytes, 1));
  for (uint64_t r0 = 0; r0 < nrows; r0 += slice) {
    const uint64_t cnt = std::min(slice, nrows - r0);
    PANN_HIP(hipMemcpy2D((uint8_t*)out + r0 * out_stride_bytes, out_stride_bytes, ix.points + (first_row + r0) * ix.pstride, ix.pstride,
                         ix.dbytes, cnt, hipMemcpyDeviceToHost));
  }
  return PANN_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// bit sketches (sketch.hip): the second level of the filtered searches
// ---------------------------------------------------------------------------------------------

namespace {

int check_sketch_params(const pann_sketch_params* p, const char* fn) {
  if (!p) { set_error(std::string(fn) + ": null parameters"); return PANN_ERR_BAD_ARG; }
  if (!sketch_kind_ok(p->kind)) { set_error(std::string(fn) + ": unknown sketch kind"); return PANN_ERR_BAD_ARG; }
  if (p->dims <= 0) { set_error(std::string(fn) + ": parameters without dimensions"); return PANN_ERR_BAD_ARG; }
  if (p->dims > PANN_SKETCH_MAX_DIMS) { set_error(std::string(fn) + ": sketches of more than 2048 dimensions are not supported"); return PANN_ERR_UNSUPPORTED; }
  return PANN_OK;
}
int check_sketch_source(const pann_index* src, const char* fn) {
  if (int rc = check_idx(src, fn)) return rc;
  if (src->ix.dtype != PANN_F32) { set_error(std::string(fn) + ": the source index must hold float (PANN_F32) points"); return PANN_ERR_UNSUPPORTED; }
  if (src->ix.d > PANN_SKETCH_MAX_DIMS) { set_error(std::string(fn) + ": sketches of more than 2048 dimensions are not supported"); return PANN_ERR_UNSUPPORTED; }
  return PANN_OK;
}
int check_sketch_rows_args(const pann_sketch_params* p, const float* rows, uint64_t stride, const void* out, uint64_t out_stride, const char* fn) {
  if (int rc = check_sketch_params(p, fn)) return rc;
  if (!rows || !out) { set_error(std::string(fn) + ": null rows / output"); return PANN_ERR_BAD_ARG; }
  if (stride < 4ull * (uint32_t)p->dims || stride % 4 != 0) { set_error(std::string(fn) + ": row stride smaller than a row or not a multiple of 4"); return PANN_ERR_BAD_ARG; }
  if (out_stride < sketch_row_bytes(p->kind, (uint32_t)p->dims)) { set_error(std::string(fn) + ": output stride smaller than a sketch row"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

}  // namespace

extern "C" {

void pann_sketch_select_ranks(uint64_t len, int kind, uint64_t* a, uint64_t* b) {
  if (!a || !b || len == 0) return;
  sketch_select_ranks(len, kind, a, b);
}

int pann_sketch_params_generate(pann_index* src, int kind, pann_sketch_params* out) {
  if (!sketch_kind_ok(kind)) { set_error("pann_sketch_params_generate: unknown sketch kind"); return PANN_ERR_BAD_ARG; }
  if (!out) { set_error("pann_sketch_params_generate: null output"); return PANN_ERR_BAD_ARG; }
  if (int rc = check_sketch_source(src, "pann_sketch_params_generate")) return rc;
  const DeviceIndex& ix = src->ix;
  if (ix.n == 0 || ix.d == 0) { set_error("pann_sketch_params_generate: empty index"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(src->device);
  if (int rc = src->params_scratch.ensure(quant_scratch_bytes())) return rc;
  return sketch_params_dev(reinterpret_cast<const float*>(ix.points), ix.n, ix.d, ix.pstride, kind, out, src->params_scratch.buf, src->stream);
}

int pann_index_attach_sketch(pann_index* idx, pann_index* src, const pann_sketch_params* p) {
  if (int rc = check_idx_no4(idx, "pann_index_attach_sketch")) return rc;
  if (int rc = check_idx(src, "pann_index_attach_sketch")) return rc;
  if (int rc = check_sketch_params(p, "pann_index_attach_sketch")) return rc;
  if (int rc = check_sketch_source(src, "pann_index_attach_sketch")) return rc;
  const DeviceIndex& sx = src->ix;
  if (sx.n != idx->ix.n || sx.d != idx->ix.d || (uint32_t)p->dims != sx.d || src->device != idx->device) {
    set_error("pann_index_attach_sketch: source, parameters and index must agree in size, dimension and device"); return PANN_ERR_BAD_ARG;
  }
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));           // no search of idx may still read the old slab
  const uint32_t stride = sketch_dev_stride(p->kind, sx.d);
  idx->ix.sketch = nullptr; idx->ix.sk_kind = -1;
  if (int rc = idx->sketch_buf.ensure((size_t)sx.n * stride)) return rc;
  if (int rc = sketch_translate_dev(p, reinterpret_cast<const float*>(sx.points), sx.n, sx.pstride, idx->sketch_buf.buf, stride, stride, src->stream)) return rc;
  PANN_HIP(hipStreamSynchronize(src->stream));
  idx->ix.sketch = idx->sketch_buf.as<uint8_t>(); idx->ix.sk_stride = stride; idx->ix.sk_kind = p->kind;
  idx->sk_params = *p;
  idx->ix.sk_as_written = (p->kind != PANN_SKETCH_MIPS_2BIT && p->hamming_as_written) ? 1u : 0u;
  return PANN_OK;
}

int pann_index_upload_sketch(pann_index* idx, const pann_sketch_params* p, const void* rows, uint64_t stride_bytes) {
  if (int rc = check_idx_no4(idx, "pann_index_upload_sketch")) return rc;
  if (int rc = check_sketch_params(p, "pann_index_upload_sketch")) return rc;
  const DeviceIndex& ix = idx->ix;
  if (!rows) { set_error("pann_index_upload_sketch: null rows"); return PANN_ERR_BAD_ARG; }
  if ((uint32_t)p->dims != ix.d) { set_error("pann_index_upload_sketch: parameters made for another dimension"); return PANN_ERR_BAD_ARG; }
  const uint32_t row = sketch_row_bytes(p->kind, ix.d), stride = sketch_dev_stride(p->kind, ix.d);
  if (stride_bytes < row) { set_error("pann_index_upload_sketch: row stride smaller than a sketch row"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));           // no search of idx may still read the old slab
  idx->ix.sketch = nullptr; idx->ix.sk_kind = -1;
  if (ix.n == 0) { set_error("pann_index_upload_sketch: empty index"); return PANN_ERR_BAD_ARG; }
  if (int rc = idx->sketch_buf.ensure((size_t)ix.n * stride)) return rc;
  if (stride != row) PANN_HIP(hipMemset(idx->sketch_buf.buf, 0, (size_t)ix.n * stride));      // the pad bytes of a device row are zero
  PANN_HIP(hipMemcpy2D(idx->sketch_buf.buf, stride, rows, stride_bytes, row, ix.n, hipMemcpyHostToDevice));
  idx->ix.sketch = idx->sketch_buf.as<uint8_t>(); idx->ix.sk_stride = stride; idx->ix.sk_kind = p->kind;
  idx->sk_params = *p;
  idx->ix.sk_as_written = (p->kind != PANN_SKETCH_MIPS_2BIT && p->hamming_as_written) ? 1u : 0u;
  return PANN_OK;
}

int pann_index_drop_sketch(pann_index* idx) {
  if (int rc = check_idx(idx, "pann_index_drop_sketch")) return rc;
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));
  idx->ix.sketch = nullptr; idx->ix.sk_kind = -1; idx->ix.sk_stride = 0; idx->ix.sk_as_written = 0;
  idx->sketch_buf.release();
  return PANN_OK;
}

int pann_index_sketch_kind(const pann_index* idx) { return (idx && idx->ix.sketch) ? idx->ix.sk_kind : -1; }

int pann_index_download_sketch(pann_index* idx, uint64_t first_row, uint64_t nrows, void* out, uint64_t out_stride_bytes) {
  if (int rc = check_idx(idx, "pann_index_download_sketch")) return rc;
  const DeviceIndex& ix = idx->ix;
  if (!ix.sketch) { set_error("pann_index_download_sketch: no sketch attached to the index"); return PANN_ERR_BAD_ARG; }
  if (nrows == 0) return PANN_OK;
  if (!out) { set_error("pann_index_download_sketch: null output"); return PANN_ERR_BAD_ARG; }
  if (first_row > ix.n || nrows > ix.n - first_row) { set_error("pann_index_download_sketch: row range outside the index"); return PANN_ERR_BAD_ARG; }
  const uint32_t row = sketch_row_bytes(ix.sk_kind, ix.d);
  if (out_stride_bytes < row) { set_error("pann_index_download_sketch: row stride smaller than a sketch row"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(idx->device);
  PANN_HIP(hipStreamSynchronize(idx->stream));
  PANN_HIP(hipMemcpy2D(out, out_stride_bytes, ix.sketch + first_row * ix.sk_stride, ix.sk_stride, row, nrows, hipMemcpyDeviceToHost));
  return PANN_OK;
}

int pann_sketch_rows_dev(const pann_sketch_params* p, const float* d_rows, uint64_t n, uint64_t stride_bytes, void* d_out,
                         uint64_t out_stride_bytes, void* stream) {
  if (int rc = check_sketch_rows_args(p, d_rows, stride_bytes, d_out, out_stride_bytes, "pann_sketch_rows_dev")) return rc;
  if (out_stride_bytes % 8 != 0 || (uintptr_t)d_out % 8 != 0) { set_error("pann_sketch_rows_dev: output rows must be 8-byte aligned"); return PANN_ERR_BAD_ARG; }
  if (n == 0) return PANN_OK;
  return sketch_translate_dev(p, d_rows, n, stride_bytes, d_out, out_stride_bytes, sketch_row_bytes(p->kind, (uint32_t)p->dims), (hipStream_t)stream);
}

int pann_sketch_rows(const pann_sketch_params* p, const float* rows, uint64_t n, uint64_t stride_bytes, void* out,
                     uint64_t out_stride_bytes, int device) {
  if (int rc = check_sketch_rows_args(p, rows, stride_bytes, out, out_stride_bytes, "pann_sketch_rows")) return rc;
  const int ndev = pann_device_count();
  if (ndev <= 0) { set_error("pann_sketch_rows: no HIP device visible (this library has no CPU path)"); return PANN_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_error("pann_sketch_rows: device ordinal out of range"); return PANN_ERR_BAD_ARG; }
  if (n == 0) return PANN_OK;
  DeviceGuard g(device);
  if (!g.ok) { set_error("pann_sketch_rows: hipSetDevice failed"); return PANN_ERR_HIP; }
  const uint32_t d = (uint32_t)p->dims, row = sketch_row_bytes(p->kind, d);
  return rows_through_device(rows, n, stride_bytes, (size_t)d * 4, out, out_stride_bytes, row,
      [&](const float* d_in, uint64_t cnt, void* d_ob) { return pann_sketch_rows_dev(p, d_in, cnt, (uint64_t)d * 4, d_ob, row, nullptr); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// quantised search + exact rerank in one call (search_rerank.hip)
// ---------------------------------------------------------------------------------------------

namespace {

// Every fused entry point fills a RerankCall (search_call.h) by field name and goes through search_rerank.

// everything that can be refused before anything is enqueued; r.fn names the entry point in the messages.  use_filter: the
// caller's, or 0 where a masked call tests it itself
int search_rerank_checks(const RerankCall& r, int use_filter) {
  const std::string f = r.fn;
  const pann_query_params* qp = r.qp;
  if (!r.full || !r.quant) { set_error(f + ": null index handle"); return PANN_ERR_BAD_ARG; }
  if (!r.qparams || !qp || !r.has_out || !r.out.ids || !r.out.dists) { set_error(f + ": null parameters / outputs"); return PANN_ERR_BAD_ARG; }
  if (qp->k <= 0) { set_error(f + ": k must be at least 1"); return PANN_ERR_BAD_ARG; }
  if (int rc = k_beam_check(qp)) return rc;
  const DeviceIndex& fx = r.full->ix;
  const DeviceIndex& qx = r.quant->ix;
  if (fx.dtype != PANN_F32) { set_error(f + ": the full-precision index must hold float (PANN_F32) points"); return PANN_ERR_UNSUPPORTED; }
  if (fx.n != qx.n || fx.d != qx.d || r.full->device != r.quant->device || fx.metric != qx.metric) {
    set_error(f + ": the two indices must agree in size, dimension, device and metric"); return PANN_ERR_BAD_ARG;
  }
  if (int rc = check_quant_kind(r.qparams->kind, r.fn)) return rc;
  const bool eu = quant_kind_is_euclid(r.qparams->kind);
  if (qx.dtype != quant_kind_dtype(r.qparams->kind) || qx.metric != (eu ? PANN_L2 : PANN_MIPS) || (uint32_t)r.qparams->dims != qx.d) {
    set_error(f + ": the quantisation parameters do not fit the one-byte index (EUCLID_U8 <-> u8 / L2, MIPS_I8 <-> i8 / MIPS, EUCLID_U4 <-> "
                  "u4 / L2, MIPS_I4 <-> i4 / MIPS, same dimension)");
    return PANN_ERR_BAD_ARG;
  }
  if (use_filter && is_4bit_dtype(qx.dtype)) {
    set_error(f + ": use_filter is not supported with a four-bit (" + dtype_name(qx.dtype) + ") quantised index"); return PANN_ERR_UNSUPPORTED;
  }
  if (use_filter && !qx.sketch) { set_error(f + ": use_filter needs a sketch attached to the one-byte index"); return PANN_ERR_BAD_ARG; }
  if (r.qstride < 4ull * fx.d || r.qstride % 4 != 0) { set_error(f + ": query stride smaller than a row or not a multiple of 4"); return PANN_ERR_BAD_ARG; }
  if (!r.starts || r.nstarts == 0) { set_error("beam search expects at least one start point"); return PANN_ERR_BAD_ARG; }
  if (qp->beam > 4096) { set_error("pann_rerank: candidates per query must be in [1,4096]"); return PANN_ERR_BAD_ARG; }
  if (r.nq && !r.queries) { set_error(f + ": null queries"); return PANN_ERR_BAD_ARG; }
  return PANN_OK;
}

// pann_batch_search_{masked,labeled}_rerank*: the rerank checks, then the filter's -- predicates over the labels of `full`, ahead
// of the masked search's own limits on `quant` (out_k = the list length), which hold the bitmap's
int masked_rerank_checks(const RerankCall& r) {
  if (int rc = search_rerank_checks(r, 0)) return rc;
  const std::string f = r.fn;
  if (r.use_filter) { set_error(f + ": a mask together with the sketch filter is not supported (use_filter must be 0)"); return PANN_ERR_UNSUPPORTED; }
  if (r.filter.mode == MASK_LABELS) { if (int rc = filter_checks(r.full, r.fn, r.filter, r.nq)) return rc; }
  if (int rc = masked_limits(r.quant, r.filter, r.nq, r.qp, masked_rerank_pool(r.qp))) return rc;
  if (r.qp->k > 64) { set_error(f + ": k > 64 is not supported (the result list holds at most 64 keys)"); return PANN_ERR_UNSUPPORTED; }
  return PANN_OK;
}

// one launch sequence for the queries of r (device pointers, r.dcap set); grows quant's workspaces on first use
int search_rerank_launch(const RerankCall& r) {
  pann_index* quant = r.quant;
  const uint32_t list = r.filter.given() ? masked_rerank_pool(r.qp) : (uint32_t)r.qp->beam;     // ids kept per query between search and rerank
  if (int rc = quant->ws.ensure(search_rerank_ws_bytes(quant->ix, r))) return rc;
  if (int rc = quant->ws_rr.ensure(search_rerank_scratch_bytes(quant->ix, r.nq, list, r.normalize_first, r.use_filter))) return rc;
  return search_rerank_dev(r.full->ix, quant->ix, quant->ws, quant->ws_rr.buf, &quant->sk_params, r);
}

// a host-pointer fused call after its checks: one host round trip, with the bitmap rows -- or the predicates -- and the two masked
// outputs when there is a filter.  The request is restated once on the staged copies and sliced per launch.
int search_rerank_host(const RerankCall& c) {
  pann_index* quant = c.quant;
  const uint64_t nq = c.nq;
  for (uint32_t i = 0; i < c.nstarts; i++)
    if (c.starts[i] >= quant->ix.n) { set_error(std::string(c.fn) + ": start point out of range"); return PANN_ERR_BAD_ARG; }
  if (nq == 0) return PANN_OK;
  DeviceGuard g(quant->device);
  const DeviceIndex& qx = quant->ix;
  const uint32_t k = (uint32_t)c.qp->k;
  HostTrip t(quant, true);
  // ---- inputs: the float rows, the starts and the filter's arrays, one transfer up ----
  const int i_q = t.in.add(c.queries, (nq - 1) * c.qstride + 4ull * qx.d);
  const int i_st = t.in.add(c.starts, (size_t)c.nstarts * 4);
  const StagedFilter staged(t, c.filter.given() ? &c.filter : nullptr, qx.n, nq);
  // ---- outputs: one packed device region (the status word last), one transfer down ----
  const pann_rerank_out& out = c.out;
  const int o_ids = t.out.add(out.ids, nq * k * 4), o_dists = t.out.add(out.dists, nq * k * 4);
  const int o_fs = t.out.add(out.frontier_size, nq * 4), o_vcnt = t.out.add(out.visited_count, nq * 4);
  const int o_cmps = t.out.add(out.dist_cmps, nq * 4);
  const int o_pruned = t.out.add(c.use_filter ? out.pruned_cmps : nullptr, nq * 4);       // (no room where it is not asked for)
  const int o_rcnt = t.out.add(c.result_count, nq * 4), o_acmps = t.out.add(c.allowed_cmps, nq * 4);
  if (int rc = t.begin()) return rc;
  RerankCall d = c;
  d.dev = true; d.stream = t.st;
  d.queries = (const float*)t.din<uint8_t>(i_q); d.starts = t.din<uint32_t>(i_st); d.filter = staged.on_device(t);
  d.out.ids = t.dout<uint32_t>(o_ids); d.out.dists = t.dout<float>(o_dists);
  d.out.frontier_size = t.dout<uint32_t>(o_fs); d.out.visited_count = t.dout<uint32_t>(o_vcnt);
  d.out.dist_cmps = t.dout<uint32_t>(o_cmps); d.out.pruned_cmps = t.dout<uint32_t>(o_pruned);
  d.out.status = t.status_slot();      // the status word comes down with the results
  d.result_count = t.dout<uint32_t>(o_rcnt); d.allowed_cmps = t.dout<uint32_t>(o_acmps);
  uint32_t status = 0;
  if (int rc = t.run_grown(nq, c.qp, c.fn, &status,
      [&](uint64_t q0, uint64_t cnt, uint32_t dcap, const uint32_t** d_word) -> int {
      *d_word = t.status_slot();
      return search_rerank_launch(d.slice(q0, cnt, dcap));
    })) return rc;
  if (out.status) *out.status = status;
  return PANN_OK;
}

// every fused entry behind its request: the checks, then the host round trip or (r.dev) the launch on the caller's stream
int search_rerank(const RerankCall& r) {
  if (int rc = r.filter.given() ? masked_rerank_checks(r) : search_rerank_checks(r, r.use_filter)) return rc;
  if (!r.dev) return search_rerank_host(r);
  if (r.nq == 0) return PANN_OK;
  if ((uintptr_t)r.queries % 4 != 0) { set_error(std::string(r.fn) + ": query rows must be 4-byte aligned"); return PANN_ERR_BAD_ARG; }
  DeviceGuard g(r.quant->device);
  return search_rerank_launch(r.slice(0, r.nq, r.quant->dcap));
}

}  // namespace

extern "C" {

int pann_batch_search_rerank_dev(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* d_queries,
                                 uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter, const uint32_t* d_starts,
                                 uint32_t nstarts, const pann_query_params* qp, const pann_rerank_out* d_out, void* stream) {
  RerankCall r;
  r.full = full; r.quant = quant; r.qparams = qparams; r.queries = d_queries; r.nq = nq; r.qstride = q_stride_bytes;
  r.normalize_first = normalize_first; r.use_filter = use_filter; r.starts = d_starts; r.nstarts = nstarts; r.qp = qp; r.set_out(d_out);
  r.dev = true; r.stream = stream; r.fn = "pann_batch_search_rerank_dev";
  return search_rerank(r);
}

int pann_batch_search_rerank(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* queries,
                             uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter, const uint32_t* starts,
                             uint32_t nstarts, const pann_query_params* qp, const pann_rerank_out* out) {
  RerankCall r;
  r.full = full; r.quant = quant; r.qparams = qparams; r.queries = queries; r.nq = nq; r.qstride = q_stride_bytes;
  r.normalize_first = normalize_first; r.use_filter = use_filter; r.starts = starts; r.nstarts = nstarts; r.qp = qp; r.set_out(out);
  r.fn = "pann_batch_search_rerank";
  return search_rerank(r);
}

int pann_batch_search_masked_rerank_dev(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* d_queries,
                                        uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter,
                                        const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp, const uint32_t* d_allow,
                                        uint64_t allow_stride_words, const pann_rerank_out* d_out, uint32_t* d_out_result_count,
                                        uint32_t* d_out_allowed_cmps, void* stream) {
  RerankCall r;
  r.full = full; r.quant = quant; r.qparams = qparams; r.queries = d_queries; r.nq = nq; r.qstride = q_stride_bytes;
  r.normalize_first = normalize_first; r.use_filter = use_filter; r.starts = d_starts; r.nstarts = nstarts; r.qp = qp; r.set_out(d_out);
  r.filter = PointFilter::bitmap(d_allow, allow_stride_words, nq, true); r.result_count = d_out_result_count; r.allowed_cmps = d_out_allowed_cmps;
  r.dev = true; r.stream = stream; r.fn = "pann_batch_search_masked_rerank_dev";
  return search_rerank(r);
}

int pann_batch_search_masked_rerank(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* queries,
                                    uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter, const uint32_t* starts,
                                    uint32_t nstarts, const pann_query_params* qp, const uint32_t* allow, uint64_t allow_stride_words,
                                    const pann_rerank_out* out, uint32_t* out_result_count, uint32_t* out_allowed_cmps) {
  RerankCall r;
  r.full = full; r.quant = quant; r.qparams = qparams; r.queries = queries; r.nq = nq; r.qstride = q_stride_bytes;
  r.normalize_first = normalize_first; r.use_filter = use_filter; r.starts = starts; r.nstarts = nstarts; r.qp = qp; r.set_out(out);
  r.filter = PointFilter::bitmap(allow, allow_stride_words, nq, false); r.result_count = out_result_count; r.allowed_cmps = out_allowed_cmps;
  r.fn = "pann_batch_search_masked_rerank";
  return search_rerank(r);
}

int pann_batch_search_labeled_rerank_dev(pann_index* full, pann_index* quant, const pann_quant_params* qparams,
                                         const float* d_queries, uint64_t nq, uint64_t q_stride_bytes, int normalize_first,
                                         int use_filter, const uint32_t* d_starts, uint32_t nstarts, const pann_query_params* qp,
                                         int kind, const pann_label_pred* d_preds, uint64_t npreds, const pann_rerank_out* d_out,
                                         uint32_t* d_out_result_count, uint32_t* d_out_allowed_cmps, void* stream) {
  RerankCall r;
  r.full = full; r.quant = quant; r.qparams = qparams; r.queries = d_queries; r.nq = nq; r.qstride = q_stride_bytes;
  r.normalize_first = normalize_first; r.use_filter = use_filter; r.starts = d_starts; r.nstarts = nstarts; r.qp = qp; r.set_out(d_out);
  r.filter = label_filter(full, kind, d_preds, npreds, true); r.result_count = d_out_result_count; r.allowed_cmps = d_out_allowed_cmps;
  r.dev = true; r.stream = stream; r.fn = "pann_batch_search_labeled_rerank_dev";
  return search_rerank(r);
}

int pann_batch_search_labeled_rerank(pann_index* full, pann_index* quant, const pann_quant_params* qparams, const float* queries,
                                     uint64_t nq, uint64_t q_stride_bytes, int normalize_first, int use_filter,
                                     const uint32_t* starts, uint32_t nstarts, const pann_query_params* qp, int kind,
                                     const pann_label_pred* preds, uint64_t npreds, const pann_rerank_out* out,
                                     uint32_t* out_result_count, uint32_t* out_allowed_cmps) {
  RerankCall r;
  r.full = full; r.quant = quant; r.qparams = qparams; r.queries = queries; r.nq = nq; r.qstride = q_stride_bytes;
  r.normalize_first = normalize_first; r.use_filter = use_filter; r.starts = starts; r.nstarts = nstarts; r.qp = qp; r.set_out(out);
  r.filter = label_filter(full, kind, preds, npreds, false); r.result_count = out_result_count; r.allowed_cmps = out_allowed_cmps;
  r.fn = "pann_batch_search_labeled_rerank";
  return search_rerank(r);
}

}  // extern "C"
