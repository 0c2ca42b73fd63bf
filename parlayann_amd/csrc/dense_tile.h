// dense_tile.h -- what the 64-row tile kernels of dense.hip and range_gt.hip share: the tile geometry, the row loader and
// row norms of the staging code, the matrix-core contraction step, the LDS-only barrier, and the host-side walk over
// (element type, metric) that picks and launches an instantiation.
#pragma once
#include <type_traits>

#include "pann_device.h"

namespace pann {

constexpr int DT_A = 64;        // A rows per workgroup
constexpr int DT_AW = 16;       // A rows per wave
constexpr int DT_B = 64;        // B rows per lane group (one per lane)
constexpr int DT_SEG = 256;     // bytes of the dimension staged per step
constexpr int DT_BSTRIDE = DT_SEG + 16;

// A workgroup's share of the work: A rows [a0, a0 + na_tile) against B rows [bs, be) -- piece blockIdx.y of the B range
// [b_lo, b_hi), which is cut into pieces of `per` rows (a whole number of tiles).
struct TileGeom { uint64_t a0; uint32_t na_tile; uint64_t bs, be; };
__device__ __forceinline__ uint64_t piece_rows(uint64_t nb, uint32_t nsplit, uint32_t tile) {
  return ((nb + nsplit - 1) / nsplit + tile - 1) / tile * tile;
}
// segmented form: the tile starts at A row a0 of a segment that ends at a_hi
__device__ __forceinline__ TileGeom tile_geom(uint64_t a0, uint64_t a_hi, uint64_t b_lo, uint64_t b_hi, uint64_t per) {
  const uint64_t nb = b_hi - b_lo;
  return {a0, (uint32_t)min((uint64_t)DT_A, a_hi - a0), b_lo + min(nb, (uint64_t)blockIdx.y * per), b_lo + min(nb, (uint64_t)(blockIdx.y + 1) * per)};
}
// contiguous form: A rows 0 .. na in tiles of 64 (blockIdx.x), B rows 0 .. nb
__device__ __forceinline__ TileGeom tile_geom(uint64_t na, uint64_t nb, uint64_t per) {
  return tile_geom((uint64_t)blockIdx.x * DT_A, na, 0ull, nb, per);
}

// 16 bytes at `off` of a row that may be unaligned (an external query row) and ends after `valid` bytes
__device__ __forceinline__ uint4 load16_unaligned(const uint8_t* rp, uint32_t off, uint32_t valid) {
  if ((reinterpret_cast<uintptr_t>(rp) & 15) == 0) return load16_guarded(rp, off, valid);
  uint8_t tmp[16];
#pragma unroll
  for (int i = 0; i < 16; i++) tmp[i] = (off + i < valid) ? rp[off + i] : (uint8_t)0;
  uint4 v;
  __builtin_memcpy(&v, tmp, 16);
  return v;
}

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains the vector memory counter, which would wait
// for the tile requested two iterations ahead at every tile (measured: 2.6 us per tile, the loaded HBM latency)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

typedef _Float16 mf_half8 __attribute__((ext_vector_type(8)));
typedef __bf16 mf_bf8 __attribute__((ext_vector_type(8)));
typedef float mf_float4 __attribute__((ext_vector_type(4)));

// sum of squares of 16 bytes of a two-byte float type, one f32 fma chain
template <bool BF>
__device__ __forceinline__ float sumsq16(uint4 v) {
  float ss = 0.f;
  if constexpr (BF) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++) { const float lo = bf16_lo(w[i]), hi = bf16_hi(w[i]); ss = fmaf(lo, lo, ss); ss = fmaf(hi, hi, ss); }
  } else {
    mf_half8 h; __builtin_memcpy(&h, &v, 16);
#pragma unroll
    for (int i = 0; i < 8; i++) { const float f = (float)h[i]; ss = fmaf(f, f, ss); }
  }
  return ss;
}
// sum of squares of 16 bytes of a one-byte type (exact)
template <int DT>
__device__ __forceinline__ int sumsq16_i8(uint4 v) {
  if constexpr (DT == PANN_U8) {
    uint32_t x = __builtin_amdgcn_udot4(v.x, v.x, 0u, false); x = __builtin_amdgcn_udot4(v.y, v.y, x, false);
    x = __builtin_amdgcn_udot4(v.z, v.z, x, false); x = __builtin_amdgcn_udot4(v.w, v.w, x, false);
    return (int)x;
  } else {
    int x = __builtin_amdgcn_sdot4((int)v.x, (int)v.x, 0, false); x = __builtin_amdgcn_sdot4((int)v.y, (int)v.y, x, false);
    x = __builtin_amdgcn_sdot4((int)v.z, (int)v.z, x, false); x = __builtin_amdgcn_sdot4((int)v.w, (int)v.w, x, false);
    return x;
  }
}

// One contraction step on the matrix cores: acc (16 x 16) += 32 two-byte elements of 16 A rows (araw: row lane & 15, elements
// 8 (lane >> 4) ..) times the same elements of 16 B rows (braw, same layout).
// BF == false: IEEE binary16 operands (v_mfma_f32_16x16x32_f16); BF == true: bfloat16 (v_mfma_f32_16x16x32_bf16).
// Both accumulate in f32; products of two-byte values are exact in f32, so integer-valued data gives exact sums.
template <bool BF>
__device__ __forceinline__ mf_float4 mfma_step(const uint4& araw, const uint4& braw, mf_float4 acc) {
  std::conditional_t<BF, mf_bf8, mf_half8> a8, b8;
  __builtin_memcpy(&a8, &araw, 16);
  __builtin_memcpy(&b8, &braw, 16);
  if constexpr (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8, b8, acc, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, b8, acc, 0, 0, 0);
}
// The four steps of a 64-row B tile (braw[t]: B rows t*16 + (lane & 15)), for the kernels of dense.hip.  Written out, not
// built on the one above: through one more level of inlining two dense_gt_mfma_kernel instances (MIPS, k <= 16) went from 0
// to 9 spilled SGPRs, and range_join_mfma_kernel through this form from 24-28 to 16 AGPRs (its FILL L2 instances + 20 VGPRs).
template <bool BF>
__device__ __forceinline__ void mfma_step(const uint4& araw, const uint4 (&braw)[4], mf_float4 (&acc)[4]) {
  std::conditional_t<BF, mf_bf8, mf_half8> a8, b8;
  __builtin_memcpy(&a8, &araw, 16);
#pragma unroll
  for (int t = 0; t < 4; t++) {
    __builtin_memcpy(&b8, &braw[t], 16);
    if constexpr (BF) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8, b8, acc[t], 0, 0, 0);
    else acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, b8, acc[t], 0, 0, 0);
  }
}

// ---- host side ----
// f(element type tag, metric tag) for a handle's type and metric; the tags convert to the PANN_* constants at compile time
template <int V> using Tag = std::integral_constant<int, V>;
template <typename F>
static auto dispatch_type_metric(int dtype, int metric, F&& f) {
  auto with_metric = [&](auto dt) { return metric == PANN_L2 ? f(dt, Tag<PANN_L2>{}) : f(dt, Tag<PANN_MIPS>{}); };
  switch (dtype) {
    case PANN_U8: return with_metric(Tag<PANN_U8>{});
    case PANN_I8: return with_metric(Tag<PANN_I8>{});
    case PANN_F16: return with_metric(Tag<PANN_F16>{});
    case PANN_BF16: return with_metric(Tag<PANN_BF16>{});
    default: return with_metric(Tag<PANN_F32>{});
  }
}
constexpr bool is_two_byte(int dt) { return dt == PANN_F16 || dt == PANN_BF16; }

// launch with `lds` bytes of dynamic LDS (beyond 48 KB a kernel has to be told)
template <typename K, typename... Args>
static void launch_lds(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
}

}  // namespace pann
