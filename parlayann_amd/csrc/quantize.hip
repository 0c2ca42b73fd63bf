// quantize.hip -- scalar quantisation of an f32 slab on the device: the reference's translating PointRange constructor
// (point_range.h:54-72) and Point::normalize, which the host mirror and quantize.py restate on the CPU.
//
//   euclid_params_kernel   Euclidian_Point<uint8_t>::generate_parameters   euclidian_point.h:211-235  (min, max, all-integers flag)
//   select_hist_kernel     Quantized_Mips_Point<8,trim>::generate_parameters mips_point.h:433-486     (exact order statistics without
//   select_scan_kernel                                                                                  a sort: 11 + 11 + 10 bit radix select)
//   normalize_rows_kernel  Mips_Point::normalize                           mips_point.h:115-124       (double sum in index order)
//   translate_kernel       translate_point                                 euclidian_point.h:182-209, mips_point.h:416-430
//   translate4_kernel      the same with range = 15, two coordinates per output byte (Quantized_Mips_Point<4>::assign, :399-406)
//
// Results are bit-identical to the sequential C++ restatement (oracle/) on finite inputs.  Two things that takes:
//   * products are rounded before anything is added to them -- the pragma below (hipcc contracts a * b + c by default);
//   * rounding is roundf (halves away from zero), not floor(v + 0.5f): 0.49999997f rounds to 0.
// Sources are rows of f32 with any row stride (a multiple of 4 bytes); nothing outside [row, row + d) is read.  Rows that start
// on 16-byte boundaries are read with 16-byte loads, others one float at a time; a dense slab (stride == 4 * d) is re-cut into
// rows of 1024 floats so that its alignment does not depend on d.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pann_internal.h"
#include "quant_device.h"

namespace pann {
namespace {

constexpr uint32_t QBINS = 2048;          // bins of one select pass (passes 1, 2: 11 bits; pass 3: 10 bits)
constexpr uint32_t FLAT_LEN = 1024;       // floats per row of a re-cut dense slab
constexpr uint32_t MAX_BLOCKS = 2048;     // 256 CUs x 8 blocks of 4 waves

// order-preserving 32-bit key of a float (-0.0 sorts just below +0.0; the callers compare zeros with ==)
__device__ __forceinline__ uint32_t fkey(float v) {
  const uint32_t u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
inline float key_to_float(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  float f; std::memcpy(&f, &u, 4);
  return f;
}

// state of the select, device resident between the passes
struct SelectState {
  uint32_t prefix[2];               // digits found so far of the key at rank a / b
  uint32_t pad[2];
  unsigned long long rank[2];       // rank of the wanted key among the keys that share the prefix
};
// scratch layout (quant_scratch_bytes): [0, 64) SelectState or the three words of the Euclid pass; [256, ...) 2 x QBINS 64-bit counts
constexpr size_t SCRATCH_HIST_OFF = 256;

// ---- walking a view: nrows rows of len floats, row r at base + r * stride bytes ----------------------------------------------
// A wave takes 64 >> logL rows at a time, 1 << logL lanes per row (the smallest power of two that covers a row's units, so that
// no lane divides).  V = 4: every row starts on a 16-byte boundary -- units are float4, the last 1..3 floats are read one by one.
template <int V, class F4, class F1>
__device__ __forceinline__ void walk_view(const uint8_t* __restrict__ base, uint64_t nrows, uint32_t len, uint64_t stride,
                                          uint32_t logL, F4 f4, F1 f1) {
  const uint32_t lane = threadIdx.x & 63, L = 1u << logL, rpw = 64u >> logL;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t sub = lane >> logL, col = lane & (L - 1);
  for (uint64_t r = wave * rpw + sub; r < nrows; r += nwaves * rpw) {
    const float* __restrict__ row = reinterpret_cast<const float*>(base + r * stride);
    if (V == 4) {
      const uint32_t full = len >> 2;
      for (uint32_t c = col; c < full; c += L) f4(*reinterpret_cast<const float4*>(row + 4 * c));
      for (uint32_t t = (full << 2) + col; t < len; t += L) f1(row[t]);
    } else {
      for (uint32_t c = col; c < len; c += L) f1(row[c]);
    }
  }
}

// ---- Euclid parameters: min (from 0), max (from 0), "some value is negative or not an integer" --------------------------------
// out[0] = key of the minimum, out[1] = key of the maximum, out[2] = flag; initialised by quant_init_kernel
template <int V>
__global__ __launch_bounds__(256) void euclid_params_kernel(const uint8_t* __restrict__ base, uint64_t nrows, uint32_t len,
                                                            uint64_t stride, uint32_t logL, uint32_t* __restrict__ out) {
  uint32_t kmin = 0x80000000u, kmax = 0x80000000u, bad = 0;           // key(0.0f)
  auto f1 = [&](float v) {
    const uint32_t k = fkey(v);
    kmin = min(kmin, k); kmax = max(kmax, k);
    bad |= (v >= 0.0f && v == truncf(v)) ? 0u : 1u;                   // (v - (long)v) == 0, euclidian_point.h:222
  };
  auto f4 = [&](float4 x) { f1(x.x); f1(x.y); f1(x.z); f1(x.w); };
  walk_view<V>(base, nrows, len, stride, logL, f4, f1);
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o));
    kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
    bad |= (uint32_t)__shfl_xor((int)bad, o);
  }
  __shared__ uint32_t red[3][4];
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = kmin; red[1][w] = kmax; red[2][w] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t i = 1; i < (blockDim.x >> 6); i++) { kmin = min(kmin, red[0][i]); kmax = max(kmax, red[1][i]); bad |= red[2][i]; }
    // integer keys: no float atomics on values of mixed sign.  The three words settle after a few blocks; a block that cannot
    // change one (a plain load says so) leaves it alone instead of queueing one more atomic on the same cache line.
    if (kmin < __hip_atomic_load(out + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(out + 0, kmin);
    if (kmax > __hip_atomic_load(out + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out + 1, kmax);
    if (bad && !__hip_atomic_load(out + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(out + 2, 1u);
  }
}

// ---- radix select -------------------------------------------------------------------------------------------------------------
__global__ void quant_init_kernel(uint8_t* scratch, int kind, unsigned long long rank_a, unsigned long long rank_b) {
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(scratch + SCRATCH_HIST_OFF);
  for (uint32_t i = threadIdx.x; i < 2 * QBINS; i += blockDim.x) hist[i] = 0;
  if (threadIdx.x == 0) {
    if (quant_kind_is_euclid(kind)) {
      uint32_t* w = reinterpret_cast<uint32_t*>(scratch);
      w[0] = 0x80000000u; w[1] = 0x80000000u; w[2] = 0;
    } else {
      SelectState* st = reinterpret_cast<SelectState*>(scratch);
      st->prefix[0] = st->prefix[1] = 0; st->pad[0] = st->pad[1] = 0;
      st->rank[0] = rank_a; st->rank[1] = rank_b;
    }
  }
}

// One pass over the data.  PASS 1: counts of the top 11 key bits (one histogram serves both ranks).  PASS 2 / 3: per rank, counts
// of the next 11 / last 10 bits among the keys whose leading 11 / 22 bits equal that rank's prefix.  Counts are private to the
// block in LDS (32-bit: a block sees far fewer than 2^32 values) and merged into the 64-bit global histogram with vector atomics.
template <int V, int PASS>
__global__ __launch_bounds__(256) void select_hist_kernel(const uint8_t* __restrict__ base, uint64_t nrows, uint32_t len,
                                                          uint64_t stride, uint32_t logL, const SelectState* __restrict__ st,
                                                          unsigned long long* __restrict__ ghist) {
  __shared__ uint32_t h[2 * QBINS];
  constexpr uint32_t USED = PASS == 1 ? QBINS : 2 * QBINS;
  for (uint32_t i = threadIdx.x; i < USED; i += blockDim.x) h[i] = 0;
  __syncthreads();
  const uint32_t p0 = st->prefix[0], p1 = st->prefix[1];
  auto f1 = [&](float v) {
    const uint32_t k = fkey(v);
    if (PASS == 1) atomicAdd(&h[k >> 21], 1u);
    else if (PASS == 2) {
      if ((k >> 21) == p0) atomicAdd(&h[(k >> 10) & 2047u], 1u);
      if ((k >> 21) == p1) atomicAdd(&h[QBINS + ((k >> 10) & 2047u)], 1u);
    } else {
      if ((k >> 10) == p0) atomicAdd(&h[k & 1023u], 1u);
      if ((k >> 10) == p1) atomicAdd(&h[QBINS + (k & 1023u)], 1u);
    }
  };
  auto f4 = [&](float4 x) {
    if (PASS == 1) {       // neighbouring coordinates often share sign and exponent: one LDS add per run of equal bins
      const uint32_t b0 = fkey(x.x) >> 21, b1 = fkey(x.y) >> 21, b2 = fkey(x.z) >> 21, b3 = fkey(x.w) >> 21;
      uint32_t cur = b0, cnt = 1;
      if (b1 == cur) cnt++; else { atomicAdd(&h[cur], cnt); cur = b1; cnt = 1; }
      if (b2 == cur) cnt++; else { atomicAdd(&h[cur], cnt); cur = b2; cnt = 1; }
      if (b3 == cur) cnt++; else { atomicAdd(&h[cur], cnt); cur = b3; cnt = 1; }
      atomicAdd(&h[cur], cnt);
    } else { f1(x.x); f1(x.y); f1(x.z); f1(x.w); }
  };
  walk_view<V>(base, nrows, len, stride, logL, f4, f1);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < USED; i += blockDim.x)
    if (h[i]) atomicAdd(&ghist[i], (unsigned long long)h[i]);
}

// After a pass: per rank the bin that holds it and the rank inside that bin; then the histogram is cleared for the next pass.
__global__ __launch_bounds__(256) void select_scan_kernel(SelectState* st, unsigned long long* ghist, int pass) {
  __shared__ unsigned long long part[256];
  const uint32_t nb = pass == 3 ? 1024u : QBINS, per = nb / 256;
  for (int j = 0; j < 2; j++) {
    const unsigned long long* h = ghist + (pass == 1 ? 0 : j * QBINS);
    unsigned long long s = 0;
    for (uint32_t i = 0; i < per; i++) s += h[threadIdx.x * per + i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long rank = st->rank[j];
      uint32_t t = 0;
      while (t < 255 && rank >= part[t]) { rank -= part[t]; t++; }
      uint32_t b = t * per;
      const uint32_t last = b + per - 1;
      while (b < last && rank >= h[b]) { rank -= h[b]; b++; }
      st->rank[j] = rank;
      st->prefix[j] = pass == 1 ? b : ((st->prefix[j] << (pass == 2 ? 11 : 10)) | b);
    }
    __syncthreads();
  }
  for (uint32_t i = threadIdx.x; i < 2 * QBINS; i += blockDim.x) ghist[i] = 0;
}

// ---- translate_point (QParams, quantize_one / quantize_four: quant_device.h) -----------------------------------------------
// CH floats in, CH bytes out per lane and step: 16 (four 16-byte loads, one 16-byte store), 4 or 1, by the alignment of both
// sides.  A row's last, partial chunk goes float by float, byte by byte.  Only [0, len) of a destination row is written.
template <int CH>
__global__ __launch_bounds__(256) void translate_kernel(const uint8_t* __restrict__ src, uint64_t sstride, uint64_t nrows,
                                                        uint32_t len, uint32_t logL, QParams q, uint8_t* __restrict__ dst,
                                                        uint64_t dstride) {
  const uint32_t lane = threadIdx.x & 63, L = 1u << logL, rpw = 64u >> logL;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t sub = lane >> logL, col = lane & (L - 1);
  const uint32_t full = len / CH, units = (len + CH - 1) / CH;
  for (uint64_t r = wave * rpw + sub; r < nrows; r += nwaves * rpw) {
    const float* __restrict__ row = reinterpret_cast<const float*>(src + r * sstride);
    uint8_t* __restrict__ o = dst + r * dstride;
    for (uint32_t c = col; c < units; c += L) {
      if (c < full) {
        if (CH == 16) {
          const float4* p = reinterpret_cast<const float4*>(row + 16 * c);
          const float4 x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
          uint4 w;
          w.x = quantize_four(x0, q); w.y = quantize_four(x1, q); w.z = quantize_four(x2, q); w.w = quantize_four(x3, q);
          *reinterpret_cast<uint4*>(o + 16 * c) = w;
        } else if (CH == 4) {
          *reinterpret_cast<uint32_t*>(o + 4 * c) = quantize_four(*reinterpret_cast<const float4*>(row + 4 * c), q);
        } else {
          o[c] = (uint8_t)quantize_one(row[c], q);
        }
      } else {
        for (uint32_t t = c * CH; t < len; t++) o[t] = (uint8_t)quantize_one(row[t], q);
      }
    }
  }
}

// Four-bit kinds: one thread produces one whole output byte from two coordinates (the last byte of an odd row from one, its high
// nibble zero), so no two threads share a byte and every store is a plain byte store.  Thread t -> byte t % rb of row t / rb.
__global__ __launch_bounds__(256) void translate4_kernel(const uint8_t* __restrict__ src, uint64_t sstride, uint64_t nrows,
                                                         uint32_t len, QParams q, uint8_t* __restrict__ dst, uint64_t dstride) {
  const uint32_t rb = (len + 1) / 2;
  const uint64_t total = nrows * rb;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = t / rb;
    const uint32_t c = (uint32_t)(t - r * rb);
    const float* __restrict__ row = reinterpret_cast<const float*>(src + r * sstride);
    const bool hi = 2 * c + 1 < len;
    dst[r * dstride + c] = (uint8_t)quantize_pair4(row[2 * c], hi ? row[2 * c + 1] : 0.0f, hi, q);
  }
}

// ---- normalize (and, for const sources, normalize + translate in one go) ------------------------------------------------------
// One wave per block.  A tile of R rows is staged in LDS with coalesced loads (row stride ld floats, odd: lanes that walk
// different rows hit different banks); lane r then walks row r in index order -- float product, double sum, as the reference's
// loop does; the order is part of the result -- and the tile is written back scaled, coalesced again.
// mode 0: f32 rows to dst (dst == src: in place; a tile is read completely before any of it is written);
// mode 1: the scaled values go through translate_point, bytes to dst (a four-bit kind: one lane per output byte, two values).
template <int V>
__global__ __launch_bounds__(64) void normalize_rows_kernel(const uint8_t* src, uint64_t sstride, uint64_t n, uint32_t d,
                                                            uint32_t R, uint32_t ld, int mode, QParams q, uint8_t* dst,
                                                            uint64_t dstride, int dst_al4) {
  extern __shared__ float tile[];                 // R * ld floats, then R inverse norms
  float* invs = tile + (size_t)R * ld;
  const uint32_t lane = threadIdx.x;
  for (uint64_t r0 = (uint64_t)blockIdx.x * R; r0 < n; r0 += (uint64_t)gridDim.x * R) {
    const uint32_t rows = (uint32_t)min((uint64_t)R, n - r0);
    for (uint32_t r = 0; r < rows; r++) {
      const float* row = reinterpret_cast<const float*>(src + (r0 + r) * sstride);
      float* t = tile + (size_t)r * ld;
      if (V == 4) {
        const uint32_t full = d >> 2;
        for (uint32_t c = lane; c < full; c += 64) {
          const float4 x = *reinterpret_cast<const float4*>(row + 4 * c);
          t[4 * c] = x.x; t[4 * c + 1] = x.y; t[4 * c + 2] = x.z; t[4 * c + 3] = x.w;
        }
        for (uint32_t c = (full << 2) + lane; c < d; c += 64) t[c] = row[c];
      } else {
        for (uint32_t c = lane; c < d; c += 64) t[c] = row[c];
      }
    }
    __syncthreads();
    if (lane < rows) {
      const float* t = tile + (size_t)lane * ld;
      double norm = 0.0;
      for (uint32_t j = 0; j < d; j++) { const float p = t[j] * t[j]; norm += (double)p; }     // mips_point.h:117-118
      norm = __dsqrt_rn(norm);
      if (norm == 0) norm = 1.0;
      invs[lane] = (float)__ddiv_rn(1.0, norm);                                                // float inv_norm = 1.0 / norm
    }
    __syncthreads();
    for (uint32_t r = 0; r < rows; r++) {
      const float* t = tile + (size_t)r * ld;
      const float inv = invs[r];
      uint8_t* orow = dst + (r0 + r) * dstride;
      if (mode == 0) {
        float* o = reinterpret_cast<float*>(orow);
        if (V == 4) {
          const uint32_t full = d >> 2;
          for (uint32_t c = lane; c < full; c += 64) {
            float4 x;
            x.x = t[4 * c] * inv; x.y = t[4 * c + 1] * inv; x.z = t[4 * c + 2] * inv; x.w = t[4 * c + 3] * inv;
            *reinterpret_cast<float4*>(o + 4 * c) = x;
          }
          for (uint32_t c = (full << 2) + lane; c < d; c += 64) o[c] = t[c] * inv;
        } else {
          for (uint32_t c = lane; c < d; c += 64) o[c] = t[c] * inv;
        }
      } else if (q.bits4) {
        for (uint32_t c = lane; c < (d + 1) / 2; c += 64) {
          const bool hi = 2 * c + 1 < d;
          orow[c] = (uint8_t)quantize_pair4(t[2 * c] * inv, hi ? t[2 * c + 1] * inv : 0.0f, hi, q);
        }
      } else {
        const uint32_t full = dst_al4 ? (d >> 2) : 0;
        for (uint32_t c = lane; c < full; c += 64) {
          float4 x;
          x.x = t[4 * c] * inv; x.y = t[4 * c + 1] * inv; x.z = t[4 * c + 2] * inv; x.w = t[4 * c + 3] * inv;
          *reinterpret_cast<uint32_t*>(orow + 4 * c) = quantize_four(x, q);
        }
        for (uint32_t c = (full << 2) + lane; c < d; c += 64) orow[c] = (uint8_t)quantize_one(t[c] * inv, q);
      }
    }
    __syncthreads();
  }
}

// ---- host side: views, launch geometry ----------------------------------------------------------------------------------------
struct View { const uint8_t* src; uint8_t* dst; uint64_t nrows; uint32_t len; uint64_t sstride, dstride; };

// a dense source (and, where there is one, a dense destination) is one long array: rows of FLAT_LEN floats and one remainder row
int make_views(const float* rows, uint64_t n, uint32_t d, uint64_t sstride, uint8_t* dst, uint64_t dstride, View v[2]) {
  const uint8_t* s = reinterpret_cast<const uint8_t*>(rows);
  if (sstride == 4ull * d && (!dst || dstride == d) && n > 1) {
    const uint64_t total = n * d, R = total / FLAT_LEN;
    const uint32_t rem = (uint32_t)(total % FLAT_LEN);
    int c = 0;
    if (R) v[c++] = View{s, dst, R, FLAT_LEN, 4ull * FLAT_LEN, FLAT_LEN};
    if (rem) v[c++] = View{s + R * 4ull * FLAT_LEN, dst ? dst + R * FLAT_LEN : nullptr, 1, rem, 4ull * rem, rem};
    return c;
  }
  v[0] = View{s, dst, n, d, sstride, dstride};
  return 1;
}
bool aligned_rows(const void* p, uint64_t nrows, uint64_t stride, uint32_t a) {
  return (uintptr_t)p % a == 0 && (nrows <= 1 || stride % a == 0);
}
uint32_t log_lanes(uint32_t units) { uint32_t l = 0; while (l < 6 && (1u << l) < units) l++; return l; }
uint32_t grid_for(uint64_t nrows, uint32_t logL) {
  const uint64_t rpw = 64u >> logL, waves = (nrows + rpw - 1) / rpw;
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((waves + 3) / 4, 1), MAX_BLOCKS);
}

template <int PASS>
int launch_hist(const View& v, const SelectState* st, unsigned long long* hist, hipStream_t s) {
  if (aligned_rows(v.src, v.nrows, v.sstride, 16)) {
    const uint32_t logL = log_lanes((v.len + 3) / 4);
    hipLaunchKernelGGL((select_hist_kernel<4, PASS>), dim3(grid_for(v.nrows, logL)), dim3(256), 0, s, v.src, v.nrows, v.len, v.sstride, logL, st, hist);
  } else {
    const uint32_t logL = log_lanes(v.len);
    hipLaunchKernelGGL((select_hist_kernel<1, PASS>), dim3(grid_for(v.nrows, logL)), dim3(256), 0, s, v.src, v.nrows, v.len, v.sstride, logL, st, hist);
  }
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

}  // namespace

size_t quant_scratch_bytes() { return SCRATCH_HIST_OFF + 2 * QBINS * sizeof(unsigned long long); }

void quant_select_ranks(uint64_t len, int trim, uint64_t* a, uint64_t* b) {
  const long n = (long)len;
  if (trim) {
    const float cutoff = .0001f;                               // mips_point.h:448-451
    *a = (uint64_t)(long)(cutoff * n);                         // float arithmetic
    *b = (uint64_t)(long)((1.0 - cutoff) * (n - 1));           // double arithmetic
  } else { *a = 0; *b = len - 1; }
  if (*a >= len) *a = len - 1;
  if (*b >= len) *b = len - 1;
}

// The values at sorted positions rank_a and rank_b of the n * d floats (exact: three histogram passes, nothing is sorted).
// Synchronises st: the two keys come back to the host.
int quant_select_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, uint64_t rank_a, uint64_t rank_b, float* val_a,
                     float* val_b, void* scratch, hipStream_t st) {
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(sc + SCRATCH_HIST_OFF);
  View v[2];
  const int nv = make_views(d_rows, n, d, stride, nullptr, 0, v);
  hipLaunchKernelGGL(quant_init_kernel, dim3(1), dim3(256), 0, st, sc, (int)PANN_QUANT_MIPS_I8, (unsigned long long)rank_a, (unsigned long long)rank_b);
  PANN_HIP(hipGetLastError());
  SelectState* dst = reinterpret_cast<SelectState*>(sc);
  for (int pass = 1; pass <= 3; pass++) {
    for (int i = 0; i < nv; i++) {
      int rc = pass == 1 ? launch_hist<1>(v[i], dst, hist, st) : pass == 2 ? launch_hist<2>(v[i], dst, hist, st) : launch_hist<3>(v[i], dst, hist, st);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, st, dst, hist, pass);
    PANN_HIP(hipGetLastError());
  }
  SelectState h{};
  PANN_HIP(hipMemcpyAsync(&h, sc, sizeof(h), hipMemcpyDeviceToHost, st));
  PANN_HIP(hipStreamSynchronize(st));
  *val_a = key_to_float(h.prefix[0]);
  *val_b = key_to_float(h.prefix[1]);
  return PANN_OK;
}

int quant_params_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, int kind, int trim, pann_quant_params* out,
                     void* scratch, hipStream_t st) {
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  View v[2];
  const int nv = make_views(d_rows, n, d, stride, nullptr, 0, v);
  pann_quant_params p{};
  p.kind = kind; p.dims = (int32_t)d; p.slope = 1.0f; p.offset = 0; p.max_val = 0.0f;
  if (quant_kind_is_euclid(kind)) {
    hipLaunchKernelGGL(quant_init_kernel, dim3(1), dim3(256), 0, st, sc, kind, 0ull, 0ull);
    PANN_HIP(hipGetLastError());
    for (int i = 0; i < nv; i++) {
      if (aligned_rows(v[i].src, v[i].nrows, v[i].sstride, 16)) {
        const uint32_t logL = log_lanes((v[i].len + 3) / 4);
        hipLaunchKernelGGL(euclid_params_kernel<4>, dim3(grid_for(v[i].nrows, logL)), dim3(256), 0, st, v[i].src, v[i].nrows, v[i].len,
                           v[i].sstride, logL, reinterpret_cast<uint32_t*>(sc));
      } else {
        const uint32_t logL = log_lanes(v[i].len);
        hipLaunchKernelGGL(euclid_params_kernel<1>, dim3(grid_for(v[i].nrows, logL)), dim3(256), 0, st, v[i].src, v[i].nrows, v[i].len,
                           v[i].sstride, logL, reinterpret_cast<uint32_t*>(sc));
      }
      PANN_HIP(hipGetLastError());
    }
    uint32_t w[3] = {0, 0, 0};
    PANN_HIP(hipMemcpyAsync(w, sc, sizeof(w), hipMemcpyDeviceToHost, st));
    PANN_HIP(hipStreamSynchronize(st));
    float min_val = key_to_float(w[0]) + 0.0f, max_val = key_to_float(w[1]);     // (-0.0f + 0.0f == +0.0f: std::min(0.0f, -0.0f) keeps +0)
    const bool u4 = kind == PANN_QUANT_EUCLID_U4;
    if (!w[2] && !u4) { if (max_val < 256) max_val = 255; min_val = 0; }       // euclidian_point.h:228-231 (a cast cannot fit 4 bits)
    const long range = u4 ? 15 : 255;
    p.slope = range / (max_val - min_val);                                       // :106
    p.offset = (int32_t)std::round(min_val * p.slope);                           // :107
    p.min_seen = min_val; p.max_seen = max_val;
  } else {
    uint64_t ra, rb;
    quant_select_ranks(n * (uint64_t)d, trim, &ra, &rb);
    float min_val = 0.0f, max_val = 0.0f;
    if (int rc = quant_select_dev(d_rows, n, d, stride, ra, rb, &min_val, &max_val, scratch, st)) return rc;
    p.max_val = std::max(max_val, -min_val);                                     // mips_point.h:484
    p.min_seen = min_val; p.max_seen = max_val;
  }
  *out = p;
  return PANN_OK;
}

int quant_translate_dev(const pann_quant_params* p, const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, void* d_out,
                        uint64_t out_stride, hipStream_t st) {
  const QParams q = make_qparams(p);
  if (q.bits4) {
    const uint64_t total = n * (uint64_t)((d + 1) / 2);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((total + 255) / 256, 1), MAX_BLOCKS * 4);
    hipLaunchKernelGGL(translate4_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(d_rows), stride, n, d, q,
                       static_cast<uint8_t*>(d_out), out_stride);
    PANN_HIP(hipGetLastError());
    return PANN_OK;
  }
  View v[2];
  const int nv = make_views(d_rows, n, d, stride, static_cast<uint8_t*>(d_out), out_stride, v);
  for (int i = 0; i < nv; i++) {
    const View& w = v[i];
    const bool s16 = aligned_rows(w.src, w.nrows, w.sstride, 16);
    if (s16 && aligned_rows(w.dst, w.nrows, w.dstride, 16)) {
      const uint32_t logL = log_lanes((w.len + 15) / 16);
      hipLaunchKernelGGL(translate_kernel<16>, dim3(grid_for(w.nrows, logL)), dim3(256), 0, st, w.src, w.sstride, w.nrows, w.len, logL, q, w.dst, w.dstride);
    } else if (s16 && aligned_rows(w.dst, w.nrows, w.dstride, 4)) {
      const uint32_t logL = log_lanes((w.len + 3) / 4);
      hipLaunchKernelGGL(translate_kernel<4>, dim3(grid_for(w.nrows, logL)), dim3(256), 0, st, w.src, w.sstride, w.nrows, w.len, logL, q, w.dst, w.dstride);
    } else {
      const uint32_t logL = log_lanes(w.len);
      hipLaunchKernelGGL(translate_kernel<1>, dim3(grid_for(w.nrows, logL)), dim3(256), 0, st, w.src, w.sstride, w.nrows, w.len, logL, q, w.dst, w.dstride);
    }
    PANN_HIP(hipGetLastError());
  }
  return PANN_OK;
}

int quant_normalize_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, const pann_quant_params* p, void* d_out,
                        uint64_t out_stride, hipStream_t st) {
  const uint32_t ld = d | 1u;
  uint32_t R = 64;
  while (R > 1 && ((size_t)R * ld + R) * 4 > 64 * 1024) R >>= 1;
  const size_t lds = ((size_t)R * ld + R) * 4;
  if (lds > 64 * 1024) { set_error("normalize: rows of more than 16382 floats are not supported"); return PANN_ERR_UNSUPPORTED; }
  const int mode = p ? 1 : 0;
  QParams q{};
  if (p) q = make_qparams(p);
  const uint8_t* s = reinterpret_cast<const uint8_t*>(d_rows);
  uint8_t* o = static_cast<uint8_t*>(d_out);
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + R - 1) / R, 256 * 16);
  const int dst_al4 = aligned_rows(o, n, out_stride, 4) ? 1 : 0;
  const bool v4 = aligned_rows(s, n, stride, 16) && (mode == 1 || aligned_rows(o, n, out_stride, 16));
  if (v4) hipLaunchKernelGGL(normalize_rows_kernel<4>, dim3(grid), dim3(64), lds, st, s, stride, n, d, R, ld, mode, q, o, out_stride, dst_al4);
  else hipLaunchKernelGGL(normalize_rows_kernel<1>, dim3(grid), dim3(64), lds, st, s, stride, n, d, R, ld, mode, q, o, out_stride, dst_al4);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

}  // namespace pann
