// sketch.hip -- bit sketches of an f32 slab on the device: the reference's three low-precision point types that feed the
// second level of filtered_beam_search (beamSearch.h:117-123,139-146).
//
//   PANN_SKETCH_EUCLID_BIT  Euclidean_Bit_Point  euclidian_point.h:332-420  bit = x > (float) median          Hamming
//   PANN_SKETCH_MIPS_BIT    Mips_Bit_Point       mips_point.h:625-702       bit = x > 0                       Hamming
//   PANN_SKETCH_MIPS_2BIT   Mips_2Bit_Point      mips_point.h:495-623       per 64 dims: sign word, mask word  sum 2 pop(ne & nz) - pop(nz)
//
// Parameters (median, cut) are order statistics of all n * d coordinates: the radix select of quantize.hip finds them exactly,
// nothing is sorted.  Bits the reference never writes (positions >= d, sign bits under a clear mask bit, mask bits past the
// first position >= d) are 0 here, so no distance depends on them (DESIGN.md "Two-level search").
//
// Row layout: host-visible rows are the reference's num_bytes() -- 8 * ceil(d / 64) (one-bit kinds) or 16 * ceil(d / 64) bytes,
// word 2i = sign, word 2i + 1 = mask (2-bit).  The handle's slab pads a row with zero bytes to a multiple of 16, so a search
// lane reads a candidate's sketch as whole 16-byte chunks.
#include <algorithm>
#include <cmath>

#include "pann_internal.h"

namespace pann {
namespace {

// One wave per row: 64 coordinates are read coalesced (256 B), tested, and packed by ONE ballot per word; lane b keeps the
// word(s) of block b, and when the row is done lanes 0 .. words-1 write whole 64-bit words side by side.  No bit is ever
// read back or merged into memory.  words_out: 64-bit words written per row (the row's words, then zero padding).
__global__ __launch_bounds__(256) void sketch_translate_kernel(const uint8_t* __restrict__ src, uint64_t sstride, uint64_t nrows,
                                                               uint32_t d, int kind, float thr, uint8_t* __restrict__ dst,
                                                               uint64_t dstride, uint32_t words_out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t nblk = (d + 63) / 64;                         // <= 32 (d <= 2048)
  for (uint64_t r = wave; r < nrows; r += nwaves) {
    const float* __restrict__ row = reinterpret_cast<const float*>(src + r * sstride);
    unsigned long long w_sign = 0, w_mask = 0;
    for (uint32_t b = 0; b < nblk; b++) {
      const uint32_t j = b * 64 + lane;
      const bool in = j < d;
      const float x = in ? row[j] : 0.0f;
      bool s, m = false;
      if (kind == PANN_SKETCH_MIPS_2BIT) {                     // mips_point.h:591-595
        const bool neg = x < -thr, pos = !neg && x > thr;
        m = in && (neg || pos);
        s = in && pos;
      } else {
        s = in && x > thr;                                     // euclidian_point.h:398 (thr = (float) median), mips_point.h:690 (thr = 0)
      }
      const unsigned long long sw = __ballot(s), mw = __ballot(m);
      if (lane == b) { w_sign = sw; w_mask = mw; }
    }
    unsigned long long* o = reinterpret_cast<unsigned long long*>(dst + r * dstride);
    if (kind == PANN_SKETCH_MIPS_2BIT) {
      if (2 * lane < words_out) { o[2 * lane] = w_sign; o[2 * lane + 1] = w_mask; }     // lanes >= nblk hold zeros
    } else {
      if (lane < words_out) o[lane] = w_sign;
    }
  }
}

}  // namespace

bool sketch_kind_ok(int kind) { return kind == PANN_SKETCH_EUCLID_BIT || kind == PANN_SKETCH_MIPS_BIT || kind == PANN_SKETCH_MIPS_2BIT; }

uint32_t sketch_row_bytes(int kind, uint32_t d) {              // parameters::num_bytes()
  return ((d - 1) / 64 + 1) * 8 * (kind == PANN_SKETCH_MIPS_2BIT ? 2 : 1);
}
uint32_t sketch_dev_stride(int kind, uint32_t d) { return (sketch_row_bytes(kind, d) + 15) / 16 * 16; }

void sketch_select_ranks(uint64_t len, int kind, uint64_t* a, uint64_t* b) {
  const long n = (long)len;
  if (kind == PANN_SKETCH_EUCLID_BIT) {
    *a = *b = (uint64_t)(n / 2);                               // vals[n*dims/2], euclidian_point.h:412
  } else if (kind == PANN_SKETCH_MIPS_2BIT) {
    const float cutoff = .3f;                                  // mips_point.h:612-614
    *a = (uint64_t)(long)(cutoff * n);                         // float arithmetic
    *b = (uint64_t)(long)((1.0 - cutoff) * (n - 1));           // double arithmetic
  } else { *a = 0; *b = 0; }
  if (*a >= len) *a = len - 1;
  if (*b >= len) *b = len - 1;
}

int sketch_params_dev(const float* d_rows, uint64_t n, uint32_t d, uint64_t stride, int kind, pann_sketch_params* out, void* scratch,
                      hipStream_t st) {
  pann_sketch_params p{};
  p.kind = kind; p.dims = (int32_t)d; p.median = 0; p.cut = 0.0f; p.hamming_as_written = 0;
  if (kind == PANN_SKETCH_MIPS_BIT) {
    PANN_HIP(hipStreamSynchronize(st));
  } else {
    uint64_t ra, rb;
    sketch_select_ranks(n * (uint64_t)d, kind, &ra, &rb);
    float va = 0.0f, vb = 0.0f;
    if (int rc = quant_select_dev(d_rows, n, d, stride, ra, rb, &va, &vb, scratch, st)) return rc;
    if (kind == PANN_SKETCH_EUCLID_BIT) {
      // long median = vals[...]: the truncating conversion; values no long can hold (the conversion is undefined there) saturate
      if (va != va) p.median = 0;
      else if (va >= 9223372036854775807.0f) p.median = INT64_MAX;
      else if (va <= -9223372036854775808.0f) p.median = INT64_MIN;
      else p.median = (int64_t)va;
    } else {
      p.cut = std::max(vb, -va);                               // mips_point.h:615
    }
  }
  *out = p;
  return PANN_OK;
}

float sketch_threshold(const pann_sketch_params* p) {
  return p->kind == PANN_SKETCH_EUCLID_BIT ? (float)p->median : p->kind == PANN_SKETCH_MIPS_BIT ? 0.0f : p->cut;
}

int sketch_translate_dev(const pann_sketch_params* p, const float* d_rows, uint64_t n, uint64_t stride, void* d_out, uint64_t out_stride,
                         uint32_t out_row_bytes, hipStream_t st) {
  const uint32_t d = (uint32_t)p->dims;
  const float thr = sketch_threshold(p);
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 3) / 4, 1), 2048);
  hipLaunchKernelGGL(sketch_translate_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(d_rows), stride, n, d,
                     (int)p->kind, thr, static_cast<uint8_t*>(d_out), out_stride, out_row_bytes / 8);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

}  // namespace pann
