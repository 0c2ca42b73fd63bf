// quant_device.h -- translate_point of the two one-byte quantisers (euclidian_point.h:182-209, mips_point.h:416-430) as device
// functions, shared by quantize.hip and the query preparation of search_rerank.hip: both must give the same bytes.
#pragma once
#include <math.h>

#include "pann_internal.h"

namespace pann {

struct QParams {
  int kind, identity;
  float slope; int32_t offset;      // Euclid u8
  float max_val, scale;             // MIPS i8: scale = 127 / max_val
};

// products are rounded before anything else happens to them; rounding is roundf (halves away from zero)
__device__ __forceinline__ uint32_t quantize_one(float x, const QParams& q) {
#pragma clang fp contract(off)
  if (q.kind == PANN_QUANT_EUCLID_U8) {
    if (q.identity) return (uint32_t)(int32_t)x & 0xFFu;                        // (uint8_t) x, euclidian_point.h:194
    long long r = (long long)roundf(x * q.slope) - (long long)q.offset;         // :197
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    return (uint32_t)r;
  }
  if (x < -q.max_val) return (uint32_t)(-127) & 0xFFu;                          // mips_point.h:421-424
  if (x > q.max_val) return 127u;
  return (uint32_t)(int32_t)roundf(x * q.scale) & 0xFFu;                        // :426-427
}
__device__ __forceinline__ uint32_t quantize_four(float4 x, const QParams& q) {
  return quantize_one(x.x, q) | (quantize_one(x.y, q) << 8) | (quantize_one(x.z, q) << 16) | (quantize_one(x.w, q) << 24);
}

inline QParams make_qparams(const pann_quant_params* p) {
  QParams q{};
  q.kind = p->kind;
  q.slope = p->slope; q.offset = p->offset;
  q.identity = (p->slope == 1.0f && p->offset == 0) ? 1 : 0;
  q.max_val = p->max_val;
  q.scale = 127 / p->max_val;               // float scale = (range / 2) / max_val, mips_point.h:419
  return q;
}

}  // namespace pann
