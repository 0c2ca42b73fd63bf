// subset.hip -- the device half of pann_index_create_subset* (DESIGN.md "Subset index"): a new handle over the rows of another
// that a bitmap keeps, in ascending id order.  masked_knn.hip turns the bitmap into new_to_old (the ascending list of kept ids);
// here are the inverse map, the row gathers and the graph renumbering.  All of it is bandwidth work on plain vector loads and
// stores: every output word has exactly one writer, so nothing needs an atomic or LDS.
//
//   subset_iota_kernel       the maps of "keep everything": new_to_old[r] = old_to_new[r] = r
//   subset_invert_kernel     old_to_new[new_to_old[r]] = r over a table the host filled with 0xFFFFFFFF (4n bytes)
//   subset_gather_rows_kernel  dst row r <- src row new_to_old[r], rows of a multiple of 16 bytes (points: pstride, sketch:
//                            sk_stride), 16 bytes per lane, consecutive lanes on consecutive chunks of a row
//   subset_gather_u32_kernel   the same for 4-byte rows (labels)
//   subset_renumber_kernel   one wavefront per new row: the old row in passes of 64 slots, every live neighbour through
//                            old_to_new, the kept ones packed at the front in row order (ballot + popcount of the lower lanes +
//                            a running base), the tail filled with the empty marker
#include "pann_device.h"

namespace pann {
namespace {

constexpr uint32_t SS_BLOCK = 256;
constexpr uint32_t SS_MAX_GRID = 2048;      // blocks of a grid-stride launch: 8 waves per SIMD on 256 CUs

inline uint32_t stride_grid(uint64_t work) { return (uint32_t)std::min<uint64_t>((work + SS_BLOCK - 1) / SS_BLOCK, SS_MAX_GRID); }

__global__ void __launch_bounds__(SS_BLOCK) subset_iota_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, uint64_t m) {
  const uint64_t step = (uint64_t)gridDim.x * SS_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * SS_BLOCK + threadIdx.x; r < m; r += step) {
    if (a) a[r] = (uint32_t)r;
    if (b) b[r] = (uint32_t)r;
  }
}

// new_to_old is ascending and below n (allow_scatter_kernel), so every write lands inside the table and on a word of its own
__global__ void __launch_bounds__(SS_BLOCK) subset_invert_kernel(const uint32_t* __restrict__ new_to_old, uint64_t m,
                                                                 uint32_t* __restrict__ old_to_new, uint64_t n) {
  const uint64_t step = (uint64_t)gridDim.x * SS_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * SS_BLOCK + threadIdx.x; r < m; r += step) {
    const uint32_t o = new_to_old[r];
    if (o < n) old_to_new[o] = (uint32_t)r;
  }
}

// cpr: 16-byte chunks of a row; lanes = min(cpr, SS_BLOCK) threads share a row, SS_BLOCK / lanes rows per block and step
__global__ void __launch_bounds__(SS_BLOCK) subset_gather_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                      uint32_t cpr, uint32_t lanes,
                                                                      const uint32_t* __restrict__ new_to_old, uint64_t m) {
  const uint32_t rpb = SS_BLOCK / lanes, lr = threadIdx.x / lanes, ch0 = threadIdx.x - lr * lanes;
  if (lr >= rpb) return;
  const uint64_t step = (uint64_t)gridDim.x * rpb;
  for (uint64_t r = (uint64_t)blockIdx.x * rpb + lr; r < m; r += step) {
    const uint4* s = src + (uint64_t)new_to_old[r] * cpr;
    uint4* d = dst + r * cpr;
    for (uint32_t c = ch0; c < cpr; c += lanes) d[c] = s[c];
  }
}

__global__ void __launch_bounds__(SS_BLOCK) subset_gather_u32_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                     const uint32_t* __restrict__ new_to_old, uint64_t m) {
  const uint64_t step = (uint64_t)gridDim.x * SS_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * SS_BLOCK + threadIdx.x; r < m; r += step) dst[r] = src[new_to_old[r]];
}

// One wave per new row (SS_BLOCK / 64 rows per block).  gstride <= 64 is the single-pass shape, anything wider takes
// gstride / 64 passes (rounded up) with `base` carrying the slots written so far.  A neighbour id that is not below n -- the
// empty marker, or what no checked upload lets in -- is dropped like one that the bitmap drops.
__global__ void __launch_bounds__(SS_BLOCK) subset_renumber_kernel(const uint32_t* __restrict__ src_graph, uint32_t* __restrict__ dst_graph,
                                                                   uint32_t gstride, const uint32_t* __restrict__ new_to_old,
                                                                   const uint32_t* __restrict__ old_to_new, uint64_t n, uint64_t m) {
  const uint32_t lane = threadIdx.x & (PANN_WAVE - 1);
  const uint64_t r = (uint64_t)blockIdx.x * (SS_BLOCK / PANN_WAVE) + threadIdx.x / PANN_WAVE;
  if (r >= m) return;                                     // wave uniform
  const uint32_t* s = src_graph + (uint64_t)new_to_old[r] * gstride;
  uint32_t* d = dst_graph + r * gstride;
  uint32_t base = 0;
  for (uint32_t p0 = 0; p0 < gstride; p0 += PANN_WAVE) {
    const uint32_t slot = p0 + lane;
    const uint32_t id = slot < gstride ? s[slot] : SENTINEL;
    const uint32_t nid = id < n ? old_to_new[id] : SENTINEL;
    const bool kept = nid != SENTINEL;
    const uint64_t b = __ballot(kept);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (kept) d[base + below] = nid;                      // base + below <= slot < gstride
    base += (uint32_t)__popcll(b);
  }
  for (uint32_t i = base + lane; i < gstride; i += PANN_WAVE) d[i] = SENTINEL;
}

}  // namespace

int subset_iota_dev(uint32_t* d_a, uint32_t* d_b, uint64_t m, hipStream_t st) {
  if (m == 0 || (!d_a && !d_b)) return PANN_OK;
  hipLaunchKernelGGL(subset_iota_kernel, dim3(stride_grid(m)), dim3(SS_BLOCK), 0, st, d_a, d_b, m);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int subset_invert_dev(const uint32_t* d_new_to_old, uint64_t m, uint32_t* d_old_to_new, uint64_t n, hipStream_t st) {
  if (n == 0) return PANN_OK;
  PANN_HIP(hipMemsetAsync(d_old_to_new, 0xFF, (size_t)n * 4, st));
  if (m == 0) return PANN_OK;
  hipLaunchKernelGGL(subset_invert_kernel, dim3(stride_grid(m)), dim3(SS_BLOCK), 0, st, d_new_to_old, m, d_old_to_new, n);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int subset_gather_rows_dev(const void* d_src, void* d_dst, uint32_t row_bytes, const uint32_t* d_new_to_old, uint64_t m, hipStream_t st) {
  if (m == 0 || row_bytes == 0) return PANN_OK;
  if (row_bytes == 4) {
    hipLaunchKernelGGL(subset_gather_u32_kernel, dim3(stride_grid(m)), dim3(SS_BLOCK), 0, st, (const uint32_t*)d_src, (uint32_t*)d_dst,
                       d_new_to_old, m);
    PANN_HIP(hipGetLastError());
    return PANN_OK;
  }
  if (row_bytes % 16 != 0 || (uintptr_t)d_src % 16 != 0 || (uintptr_t)d_dst % 16 != 0) {
    set_error("subset_gather_rows_dev: rows must be 4 bytes or an aligned multiple of 16 bytes"); return PANN_ERR_BAD_ARG;
  }
  const uint32_t cpr = row_bytes / 16, lanes = std::min(cpr, SS_BLOCK), rpb = SS_BLOCK / lanes;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((m + rpb - 1) / rpb, SS_MAX_GRID);
  hipLaunchKernelGGL(subset_gather_rows_kernel, dim3(grid), dim3(SS_BLOCK), 0, st, (const uint4*)d_src, (uint4*)d_dst, cpr, lanes,
                     d_new_to_old, m);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int subset_renumber_graph_dev(const uint32_t* d_src_graph, uint32_t* d_dst_graph, uint32_t gstride, const uint32_t* d_new_to_old,
                              const uint32_t* d_old_to_new, uint64_t n, uint64_t m, hipStream_t st) {
  if (m == 0) return PANN_OK;
  constexpr uint32_t rows_per_block = SS_BLOCK / PANN_WAVE;
  hipLaunchKernelGGL(subset_renumber_kernel, dim3((uint32_t)((m + rows_per_block - 1) / rows_per_block)), dim3(SS_BLOCK), 0, st,
                     d_src_graph, d_dst_graph, gstride, d_new_to_old, d_old_to_new, n, m);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

}  // namespace pann
