// quant_device.h -- translate_point of the two one-byte quantisers (euclidian_point.h:182-209, mips_point.h:416-430) and of their
// four-bit forms (range = 15, two values per byte) as device functions, shared by quantize.hip and the query preparation of
// search_rerank.hip: both must give the same bytes.
#pragma once
#include <math.h>

#include "pann_internal.h"

namespace pann {

struct QParams {
  int kind, identity;
  float slope; int32_t offset;      // Euclid u8 / u4
  float max_val, scale;             // MIPS i8 / i4: scale = 127 / max_val, 7 / max_val
  int bits4;                        // a four-bit kind: quantize_one returns a nibble, two of them make an output byte
};

__host__ __device__ inline bool quant_kind_is_4bit(int kind) { return kind == PANN_QUANT_EUCLID_U4 || kind == PANN_QUANT_MIPS_I4; }
__host__ __device__ inline bool quant_kind_is_euclid(int kind) { return kind == PANN_QUANT_EUCLID_U8 || kind == PANN_QUANT_EUCLID_U4; }
inline int quant_kind_dtype(int kind) {
  return kind == PANN_QUANT_EUCLID_U8 ? PANN_U8 : kind == PANN_QUANT_MIPS_I8 ? PANN_I8 : kind == PANN_QUANT_EUCLID_U4 ? PANN_U4 : PANN_I4;
}

// products are rounded before anything else happens to them; rounding is roundf (halves away from zero)
__device__ __forceinline__ uint32_t quantize_one(float x, const QParams& q) {
#pragma clang fp contract(off)
  if (q.kind == PANN_QUANT_EUCLID_U8) {
    if (q.identity) return (uint32_t)(int32_t)x & 0xFFu;                        // (uint8_t) x, euclidian_point.h:194
    long long r = (long long)roundf(x * q.slope) - (long long)q.offset;         // :197
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    return (uint32_t)r;
  }
  if (q.kind == PANN_QUANT_EUCLID_U4) {                                         // :193-207 with range = 15, never the cast
    long long r = (long long)roundf(x * q.slope) - (long long)q.offset;
    r = r < 0 ? 0 : (r > 15 ? 15 : r);
    return (uint32_t)r;
  }
  if (q.kind == PANN_QUANT_MIPS_I4) {                                           // mips_point.h:416-430 with range / 2 = 7
    if (x < -q.max_val) return (uint32_t)(-7) & 0xFu;
    if (x > q.max_val) return 7u;
    return (uint32_t)(int32_t)roundf(x * q.scale) & 0xFu;
  }
  if (x < -q.max_val) return (uint32_t)(-127) & 0xFFu;                          // mips_point.h:421-424
  if (x > q.max_val) return 127u;
  return (uint32_t)(int32_t)roundf(x * q.scale) & 0xFFu;                        // :426-427
}
__device__ __forceinline__ uint32_t quantize_four(float4 x, const QParams& q) {
  return quantize_one(x.x, q) | (quantize_one(x.y, q) << 8) | (quantize_one(x.z, q) << 16) | (quantize_one(x.w, q) << 24);
}

// one packed output byte: coordinate 2c in the low nibble, 2c + 1 in the high one (Quantized_Mips_Point<4>::assign,
// mips_point.h:399-406); `hi_valid` false (the last byte of an odd d): the high nibble is zero
__device__ __forceinline__ uint32_t quantize_pair4(float lo, float hi, bool hi_valid, const QParams& q) {
  return quantize_one(lo, q) | (hi_valid ? quantize_one(hi, q) << 4 : 0u);
}

inline QParams make_qparams(const pann_quant_params* p) {
  QParams q{};
  q.kind = p->kind;
  q.slope = p->slope; q.offset = p->offset;
  q.bits4 = quant_kind_is_4bit(p->kind) ? 1 : 0;
  q.identity = (p->kind == PANN_QUANT_EUCLID_U8 && p->slope == 1.0f && p->offset == 0) ? 1 : 0;
  q.max_val = p->max_val;
  q.scale = (q.bits4 ? 7 : 127) / p->max_val;   // float scale = (range / 2) / max_val, mips_point.h:419
  return q;
}

}  // namespace pann
