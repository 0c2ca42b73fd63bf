// entry_points.hip -- where a filtered search starts (DESIGN.md "Entry points"): the centroid of every filter of a table, made
// on the device from the ascending id lists of the grouped exact route (masked_knn.hip, CSR), as that route's query slab.
//
//   piece_scan_kernel     piece_off[s] = pieces of the lists before segment s, a piece = CENTROID_PIECE_IDS consecutive list ids
//   list_sum_kernel       one workgroup per (segment, piece): the rows of the piece's ids are read once, in 16-byte chunks, and
//                         summed per coordinate -- 32-bit integers inside a piece for the one-byte types (exact), double for the
//                         float types -- in a fixed order: a thread adds its rows in list order, then the threads of one chunk
//                         are added in thread order.  The piece's sums go to scratch as int64 / double.  No atomics.
//   centroid_rows_kernel  per (segment, coordinate): the pieces added in ascending piece order, ONE double division by the
//                         list's length, ONE rounding to f32 (the centroid); the centroid converted to the handle's element
//                         type is the segment's row of the query slab, zero padded to the slab stride.
//   pad_fill_kernel       ids that are padding (0xFFFFFFFF) <- the caller's fill id
#include "grouped_plan.h"
#include "pann_device.h"
#include "pann_internal.h"

namespace pann {
namespace {

constexpr uint32_t EP_BLOCK = 256;
constexpr uint32_t P = CENTROID_PIECE_IDS;
static_assert((uint64_t)P * 255 < (1ull << 31), "a piece of one-byte values is summed in 32 bits");

template <int DT> struct Chunk;      // the 16 bytes of a row as NE coordinates, widened exactly to the type a thread sums in
template <> struct Chunk<PANN_U8> { static constexpr int NE = 16; using acc_t = int; using wide_t = long long; };
template <> struct Chunk<PANN_I8> { static constexpr int NE = 16; using acc_t = int; using wide_t = long long; };
template <> struct Chunk<PANN_F16> { static constexpr int NE = 8; using acc_t = double; using wide_t = double; };
template <> struct Chunk<PANN_BF16> { static constexpr int NE = 8; using acc_t = double; using wide_t = double; };
template <> struct Chunk<PANN_F32> { static constexpr int NE = 4; using acc_t = double; using wide_t = double; };

template <int DT>
__device__ __forceinline__ void chunk_add(typename Chunk<DT>::acc_t (&acc)[Chunk<DT>::NE], const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if constexpr (DT == PANN_U8) {
#pragma unroll
      for (int b = 0; b < 4; b++) acc[4 * i + b] += (int)((w[i] >> (8 * b)) & 0xFFu);
    } else if constexpr (DT == PANN_I8) {
#pragma unroll
      for (int b = 0; b < 4; b++) acc[4 * i + b] += (int)(int8_t)((w[i] >> (8 * b)) & 0xFFu);
    } else if constexpr (DT == PANN_F16) {
      acc[2 * i] += (double)__builtin_bit_cast(_Float16, (uint16_t)(w[i] & 0xFFFFu));
      acc[2 * i + 1] += (double)__builtin_bit_cast(_Float16, (uint16_t)(w[i] >> 16));
    } else if constexpr (DT == PANN_BF16) {
      acc[2 * i] += (double)bf16_lo(w[i]);
      acc[2 * i + 1] += (double)bf16_hi(w[i]);
    } else {
      acc[i] += (double)__uint_as_float(w[i]);
    }
  }
}

// the centroid as one element of the handle's type (include/pann.h, pann_filter_medoids_*: the conversion rule)
template <int DT> __device__ __forceinline__ void store_converted(uint8_t* p, float c) {
  if constexpr (DT == PANN_U8) *p = (uint8_t)fminf(fmaxf(rintf(c), 0.f), 255.f);
  else if constexpr (DT == PANN_I8) *reinterpret_cast<int8_t*>(p) = (int8_t)fminf(fmaxf(rintf(c), -128.f), 127.f);
  else if constexpr (DT == PANN_F16) *reinterpret_cast<_Float16*>(p) = (_Float16)c;      // round to nearest even
  else if constexpr (DT == PANN_BF16) {
    const uint32_t u = __float_as_uint(c);
    *reinterpret_cast<uint16_t*>(p) = c != c ? (uint16_t)0x7FC0u : (uint16_t)((u + ((u >> 16) & 1u) + 0x7FFFu) >> 16);
  } else *reinterpret_cast<float*>(p) = c;
}

// one workgroup; piece_off has S + 1 entries
__global__ void __launch_bounds__(EP_BLOCK) piece_scan_kernel(const uint64_t* __restrict__ b_off, uint32_t S, uint32_t* __restrict__ piece_off) {
  __shared__ uint32_t sh[EP_BLOCK];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < S; base += EP_BLOCK) {
    const uint32_t s = base + threadIdx.x;
    const uint32_t v = s < S ? (uint32_t)centroid_pieces_of(b_off[s + 1] - b_off[s]) : 0u;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = 1; o < EP_BLOCK; o <<= 1) {
      const uint32_t t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (s < S) piece_off[s] = carry + sh[threadIdx.x] - v;
    carry += sh[EP_BLOCK - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) piece_off[S] = carry;
}

// Workgroup block0 + blockIdx.x sums one piece.  cpr: the 16-byte chunks of a row that hold coordinates (the device rows are zero
// padded behind them); partial: cpr * NE sums per piece.  A workgroup covers min(cpr, 256) chunks of 256 / that many rows at a time.
template <int DT>
__global__ void __launch_bounds__(EP_BLOCK) list_sum_kernel(const uint8_t* __restrict__ points, uint32_t pstride, uint32_t cpr,
                                                            const uint32_t* __restrict__ list, const uint64_t* __restrict__ b_off,
                                                            const uint32_t* __restrict__ piece_off, uint32_t S, uint32_t block0,
                                                            typename Chunk<DT>::wide_t* __restrict__ partial) {
  constexpr int NE = Chunk<DT>::NE;
  using acc_t = typename Chunk<DT>::acc_t;
  using wide_t = typename Chunk<DT>::wide_t;
  __shared__ acc_t red[EP_BLOCK * NE];
  const uint32_t piece = block0 + blockIdx.x;
  uint32_t lo = 0, hi = S;                         // piece_off[lo] <= piece < piece_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (piece_off[mid] <= piece) lo = mid; else hi = mid;
  }
  const uint64_t first = b_off[lo] + (uint64_t)(piece - piece_off[lo]) * P;
  const uint32_t cnt = (uint32_t)(min(b_off[lo + 1], first + P) - first);
  const uint32_t* ids = list + first;
  wide_t* out = partial + (uint64_t)piece * cpr * NE;
  for (uint32_t c0 = 0; c0 < cpr; c0 += EP_BLOCK) {
    const uint32_t w = min(EP_BLOCK, cpr - c0), rpp = EP_BLOCK / w;
    const uint32_t r = threadIdx.x / w;
    const size_t off = (size_t)(c0 + threadIdx.x % w) * 16;
    if (r < rpp) {
      acc_t acc[NE];
#pragma unroll
      for (int e = 0; e < NE; e++) acc[e] = 0;
      uint32_t i = r;
      for (; i + 3 * rpp < cnt; i += 4 * rpp) {    // four rows in flight; added in list order
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = row_load16(points + (uint64_t)ids[i + u * rpp] * pstride + off);
#pragma unroll
        for (int u = 0; u < 4; u++) chunk_add<DT>(acc, v[u]);
      }
      for (; i < cnt; i += rpp) chunk_add<DT>(acc, row_load16(points + (uint64_t)ids[i] * pstride + off));
#pragma unroll
      for (int e = 0; e < NE; e++) red[threadIdx.x * NE + e] = acc[e];
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < w * NE; o += EP_BLOCK) {
      wide_t sum = 0;
      for (uint32_t rr = 0; rr < rpp; rr++) sum += (wide_t)red[rr * w * NE + o];
      out[(size_t)c0 * NE + o] = sum;
    }
    __syncthreads();
  }
}

// slab row s, coordinate j (j < slab_stride / element size; zeros from d on); entry[s]: the row of `centroids` (optional)
template <int DT>
__global__ void __launch_bounds__(EP_BLOCK) centroid_rows_kernel(const typename Chunk<DT>::wide_t* __restrict__ partial,
                                                                 const uint32_t* __restrict__ piece_off, const uint64_t* __restrict__ b_off,
                                                                 uint32_t S, uint32_t d, uint32_t row_sums, const uint32_t* __restrict__ entry,
                                                                 uint8_t* __restrict__ slab, uint32_t slab_stride, float* __restrict__ centroids) {
  constexpr uint32_t ES = 16 / Chunk<DT>::NE;
  const uint32_t per_row = slab_stride / ES;
  const uint64_t total = (uint64_t)S * per_row, step = (uint64_t)gridDim.x * EP_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * EP_BLOCK + threadIdx.x; i < total; i += step) {
    const uint32_t s = (uint32_t)(i / per_row), j = (uint32_t)(i % per_row);
    float c = 0.f;
    if (j < d) {
      const uint64_t len = b_off[s + 1] - b_off[s];
      if (len) {
        typename Chunk<DT>::wide_t sum = 0;
        for (uint32_t p = piece_off[s]; p < piece_off[s + 1]; p++) sum += partial[(uint64_t)p * row_sums + j];
        c = (float)((double)sum / (double)len);
      }
      if (centroids) centroids[(uint64_t)entry[s] * d + j] = c;
    }
    store_converted<DT>(slab + (uint64_t)s * slab_stride + (size_t)j * ES, c);
  }
}

__global__ void __launch_bounds__(EP_BLOCK) pad_fill_kernel(uint32_t* __restrict__ ids, uint64_t count, uint32_t fill_id) {
  const uint64_t step = (uint64_t)gridDim.x * EP_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * EP_BLOCK + threadIdx.x; i < count; i += step)
    if (ids[i] == SENTINEL) ids[i] = fill_id;
}

// Grouped labeled search: query q gets the predicate table[group[q]] and the start row group[q] (row 0 with one row) as its own.
// A table index >= G never indexes the table: that query gets a predicate that allows nothing and start row 0, and *flag is raised.
__global__ void __launch_bounds__(EP_BLOCK) group_rows_kernel(const pann_label_pred* __restrict__ table, uint32_t G, uint32_t kind,
                                                              const uint32_t* __restrict__ group, uint64_t nq,
                                                              const uint32_t* __restrict__ starts, uint32_t nstarts, uint32_t start_rows,
                                                              pann_label_pred* __restrict__ out_preds, uint32_t* __restrict__ out_starts,
                                                              uint32_t* __restrict__ flag) {
  const uint64_t step = (uint64_t)gridDim.x * EP_BLOCK;
  for (uint64_t q = (uint64_t)blockIdx.x * EP_BLOCK + threadIdx.x; q < nq; q += step) {
    const uint32_t g = group[q];
    const bool bad = g >= G;
    pann_label_pred p;
    if (bad) { p.a = kind == PANN_PRED_RANGE ? 1u : 0u; p.b = kind == PANN_PRED_MATCH ? 1u : 0u; atomicOr(flag, 1u); }
    else p = table[g];
    out_preds[q] = p;
    const uint32_t* row = starts + (size_t)((bad || start_rows == 1) ? 0u : g) * nstarts;
    for (uint32_t i = 0; i < nstarts; i++) out_starts[q * nstarts + i] = row[i];
  }
}

__global__ void raise_status_kernel(const uint32_t* __restrict__ flag, uint32_t bit, uint32_t* __restrict__ status) {
  if (*flag) atomicOr(status, bit);
}

inline uint32_t data_chunks(const DeviceIndex& ix) { return (ix.dbytes + 15) / 16; }

template <int DT>
int centroid_rows_run(const DeviceIndex& ix, hipStream_t st, const uint32_t* d_list, const uint64_t* d_b_off, uint32_t S, uint64_t pieces,
                      void* d_scratch, const uint32_t* d_entry, uint8_t* d_slab, uint32_t slab_stride, float* d_centroids) {
  using wide_t = typename Chunk<DT>::wide_t;
  uint32_t* d_piece_off = (uint32_t*)d_scratch;
  const uint32_t cpr = data_chunks(ix);
  static_assert(centroid_row_sums(16, 16 / Chunk<DT>::NE) == Chunk<DT>::NE, "the plan counts a chunk's sums as the kernels do");
  wide_t* d_partial = (wide_t*)((uint8_t*)d_scratch + CentroidScratch(S, pieces, cpr * Chunk<DT>::NE).o_partial);
  hipLaunchKernelGGL(piece_scan_kernel, dim3(1), dim3(EP_BLOCK), 0, st, d_b_off, S, d_piece_off);
  PANN_HIP(hipGetLastError());
  const uint64_t slice = launch_slice_blocks(EP_BLOCK);
  for (uint64_t b0 = 0; b0 < pieces; b0 += slice) {
    hipLaunchKernelGGL(list_sum_kernel<DT>, dim3((uint32_t)std::min(slice, pieces - b0)), dim3(EP_BLOCK), 0, st, ix.points, ix.pstride, cpr,
                       d_list, d_b_off, (const uint32_t*)d_piece_off, S, (uint32_t)b0, d_partial);
    PANN_HIP(hipGetLastError());
  }
  const uint64_t work = (uint64_t)S * (slab_stride / (16 / Chunk<DT>::NE));
  hipLaunchKernelGGL(centroid_rows_kernel<DT>, dim3((uint32_t)std::min<uint64_t>((work + EP_BLOCK - 1) / EP_BLOCK, 65536)), dim3(EP_BLOCK), 0, st,
                     (const wide_t*)d_partial, (const uint32_t*)d_piece_off, d_b_off, S, ix.d, cpr * Chunk<DT>::NE, d_entry, d_slab, slab_stride,
                     d_centroids);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

}  // namespace

int centroid_rows_dev(const DeviceIndex& ix, hipStream_t st, const uint32_t* d_list, const uint64_t* d_b_off, uint32_t S, uint64_t pieces,
                      void* d_scratch, const uint32_t* d_entry, uint8_t* d_slab, uint32_t slab_stride, float* d_centroids) {
  if (S == 0) return PANN_OK;
  switch (ix.dtype) {
    case PANN_U8: return centroid_rows_run<PANN_U8>(ix, st, d_list, d_b_off, S, pieces, d_scratch, d_entry, d_slab, slab_stride, d_centroids);
    case PANN_I8: return centroid_rows_run<PANN_I8>(ix, st, d_list, d_b_off, S, pieces, d_scratch, d_entry, d_slab, slab_stride, d_centroids);
    case PANN_F16: return centroid_rows_run<PANN_F16>(ix, st, d_list, d_b_off, S, pieces, d_scratch, d_entry, d_slab, slab_stride, d_centroids);
    case PANN_BF16: return centroid_rows_run<PANN_BF16>(ix, st, d_list, d_b_off, S, pieces, d_scratch, d_entry, d_slab, slab_stride, d_centroids);
    case PANN_F32: return centroid_rows_run<PANN_F32>(ix, st, d_list, d_b_off, S, pieces, d_scratch, d_entry, d_slab, slab_stride, d_centroids);
  }
  set_error(std::string("centroid_rows_dev: not supported on a ") + dtype_name(ix.dtype) + " handle");
  return PANN_ERR_UNSUPPORTED;
}

int group_rows_dev(const pann_label_pred* d_table, uint32_t G, int kind, const uint32_t* d_group, uint64_t nq, const uint32_t* d_starts,
                   uint32_t nstarts, uint32_t start_rows, pann_label_pred* d_out_preds, uint32_t* d_out_starts, uint32_t* d_flag, hipStream_t st) {
  PANN_HIP(hipMemsetAsync(d_flag, 0, 4, st));
  if (nq == 0) return PANN_OK;
  hipLaunchKernelGGL(group_rows_kernel, dim3((uint32_t)std::min<uint64_t>((nq + EP_BLOCK - 1) / EP_BLOCK, 4096)), dim3(EP_BLOCK), 0, st, d_table, G,
                     (uint32_t)kind, d_group, nq, d_starts, nstarts, start_rows, d_out_preds, d_out_starts, d_flag);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int raise_status_dev(const uint32_t* d_flag, uint32_t bit, uint32_t* d_status, hipStream_t st) {
  hipLaunchKernelGGL(raise_status_kernel, dim3(1), dim3(1), 0, st, d_flag, bit, d_status);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int pad_fill_dev(uint32_t* d_ids, uint64_t count, uint32_t fill_id, hipStream_t st) {
  if (count == 0 || fill_id == SENTINEL) return PANN_OK;
  hipLaunchKernelGGL(pad_fill_kernel, dim3((uint32_t)std::min<uint64_t>((count + EP_BLOCK - 1) / EP_BLOCK, 4096)), dim3(EP_BLOCK), 0, st, d_ids,
                     count, fill_id);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

}  // namespace pann
