"""Scalar quantisation of float points, as the reference's translating PointRange constructor does
(point_range.h:54-72) -- host-side preprocessing, numpy float32 arithmetic in the reference's order.

  Euclidian_Point<uint8_t>  generate_parameters  euclidian_point.h:211-235
                            translate_point      euclidian_point.h:182-209
  Quantized_Mips_Point<8>   generate_parameters  mips_point.h:433-486  (trim: 1e-4 quantiles)
                            translate_point      mips_point.h:416-430
  Mips_Point<T>::normalize                       mips_point.h:113-122

and the four-bit forms (range 15, two coordinates per byte; include/pann.h, PANN_QUANT_EUCLID_U4 / PANN_QUANT_MIPS_I4):
  Quantized_Mips_Point<4>   assign / operator[]  mips_point.h:306-311, 399-406  -> pack_nibbles / unpack_nibbles
                            translate_point      mips_point.h:416-430           -> mips_i4_translate
  the 4-bit analogue of Euclidian_Point<uint8_t>                               -> euclid_u4_params / euclid_u4_translate
"""
import numpy as np

F = np.float32


class EuclidParams:
    """Euclidian_Point<uint8_t>::parameters (euclidian_point.h:100-110): slope = range/(max-min),
    offset = (int32) round(min*slope)."""

    def __init__(self, min_val, max_val, dims, rng=255):
        self.range = rng
        self.slope = F(rng) / (F(max_val) - F(min_val))
        self.offset = np.int32(_round_half_away(F(min_val) * self.slope))
        self.dims = dims

    @property
    def identity(self):
        return self.slope == F(1.0) and self.offset == 0


def euclid_u8_params(x):
    x = np.asarray(x, dtype=F)
    min_val = F(min(0.0, float(x.min())))          # mins/maxs start at 0 (:217-218)
    max_val = F(max(0.0, float(x.max())))
    all_ints = bool(np.all(x >= 0) and np.all(x == np.trunc(x)))
    if all_ints:
        if max_val < 256:
            max_val = F(255)
        min_val = F(0)
    return EuclidParams(min_val, max_val, x.shape[1])


def _round_half_away(v):
    """std::round: halves away from zero (numpy's round is half-to-even)."""
    v = np.asarray(v, dtype=F)
    return np.where(v >= 0, np.floor(v + F(0.5)), np.ceil(v - F(0.5))).astype(F)


def euclid_u8_translate(x, p):
    x = np.asarray(x, dtype=F)
    if p.identity:
        return x.astype(np.uint8)
    r = _round_half_away(x * p.slope).astype(np.int64) - np.int64(p.offset)
    return np.clip(r, 0, p.range).astype(np.uint8)


def normalize_rows(x):
    """Mips_Point::normalize: norm accumulated in double over float products, inv_norm in float."""
    x = np.asarray(x, dtype=F)
    norm = np.sqrt(np.sum((x * x).astype(np.float64), axis=1))
    norm[norm == 0] = 1.0
    inv = (1.0 / norm).astype(F)
    return (x * inv[:, None]).astype(F)


def mips_i8_max_val(x, trim=True):
    x = np.asarray(x, dtype=F).ravel()
    n = x.size
    if trim:
        lo_i = int(F(0.0001) * F(n))                        # (long)(cutoff * len), float arithmetic
        hi_i = int((1.0 - float(F(0.0001))) * (n - 1))      # (long)((1.0 - cutoff) * (len-1)), double
        part = np.partition(x, [lo_i, hi_i])
        min_val, max_val = part[lo_i], part[hi_i]
    else:
        min_val, max_val = x.min(), x.max()
    return F(max(float(max_val), -float(min_val)))


def mips_i8_translate(x, max_val, rng=255):
    x = np.asarray(x, dtype=F)
    half = rng // 2                                         # integer 127
    scale = F(half) / F(max_val)
    v = _round_half_away(x * scale)
    v = np.where(x < -F(max_val), -half, np.where(x > F(max_val), half, v))
    return v.astype(np.int8)


# ---- four-bit rows ----

def pack_nibbles(values):
    """n x d nibble values (0..15, or -8..7 in two's complement) -> n x ceil(d / 2) uint8 rows packed as
    Quantized_Mips_Point<4>::assign packs them (mips_point.h:399-406): coordinate j in byte j // 2, an even j in the low nibble;
    for odd d the high nibble of the last byte is 0."""
    v = np.asarray(values)
    if v.ndim != 2:
        raise ValueError("values must be n x d")
    if v.size and (v.min() < -8 or v.max() > 15):
        raise ValueError("values do not fit four bits")
    n, d = v.shape
    nib = np.zeros((n, 2 * ((d + 1) // 2)), np.uint8)
    nib[:, :d] = v.astype(np.int16) & 15
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def unpack_nibbles(rows, d, signed):
    """packed rows -> n x d values, one per byte: uint8 0..15, or with signed int8 -8..7 (operator[], mips_point.h:306-311:
    0x8..0xF are -8..-1)"""
    r = np.asarray(rows, dtype=np.uint8)
    if r.ndim != 2 or r.shape[1] != (d + 1) // 2:
        raise ValueError(f"rows must be n x {(d + 1) // 2} uint8")
    nib = np.empty((r.shape[0], 2 * r.shape[1]), np.uint8)
    nib[:, 0::2] = r & 15
    nib[:, 1::2] = r >> 4
    nib = nib[:, :d]
    if not signed:
        return np.ascontiguousarray(nib)
    return np.ascontiguousarray(((nib.astype(np.int16) ^ 8) - 8).astype(np.int8))


def euclid_u4_params(x):
    """min / max as euclid_u8_params finds them (they start at 0), WITHOUT the all-integers substitution; range 15"""
    x = np.asarray(x, dtype=F)
    min_val = F(min(0.0, float(x.min())))
    max_val = F(max(0.0, float(x.max())))
    return EuclidParams(min_val, max_val, x.shape[1], rng=15)


def euclid_u4_translate(x, p):
    """euclidian_point.h:193-207 with range 15 (never the plain cast) -> nibble values, one per byte"""
    x = np.asarray(x, dtype=F)
    r = _round_half_away(x * p.slope).astype(np.int64) - np.int64(p.offset)
    return np.clip(r, 0, 15).astype(np.uint8)


def mips_i4_translate(x, max_val):
    """mips_point.h:416-430 with range 15: scale = 7 / max_val, clamped to +-7 -> nibble values, one per int8"""
    return mips_i8_translate(x, max_val, rng=15)


def quant_row_bytes(kind, dims):
    """bytes of one translated row: dims, or ceil(dims / 2) for the four-bit kinds"""
    from . import _capi
    return (dims + 1) // 2 if kind in (_capi.PANN_QUANT_EUCLID_U4, _capi.PANN_QUANT_MIPS_I4) else dims


# ---- device counterparts (csrc/quantize.hip through the C-ABI): bit-identical to the reference's loops, std::round included ----

def device_quantize_rows(x, params, normalize_first=False, device=0):
    """Q_Query_Points(Query_Points, Q_Points.params): float rows -> uint8 (Euclid) / int8 (MIPS) rows, translated on the device
    with the QuantParams of DeviceIndex.quantized(); normalize_first: every row goes through Point::normalize first.
    Four-bit kinds: packed uint8 rows of ceil(dims / 2) bytes (unpack_nibbles gives the values)."""
    import ctypes as C

    from . import _capi
    x = np.ascontiguousarray(x, dtype=F)
    if x.ndim != 2 or x.shape[1] != params.dims:
        raise ValueError(f"rows must be n x {params.dims} float32")
    rb = quant_row_bytes(params.kind, params.dims)
    out = np.empty((len(x), rb), np.int8 if params.kind == _capi.PANN_QUANT_MIPS_I8 else np.uint8)
    if len(x):
        _capi.check(_capi.load().pann_quantize_rows(C.byref(params), x.ctypes.data_as(C.c_void_p), len(x), x.shape[1] * 4,
                                                    1 if normalize_first else 0, out.ctypes.data_as(C.c_void_p), rb, device))
    return out


def device_params(kind, dims, slope=1.0, offset=0, max_val=0.0):
    """QuantParams from known values (parameters read from elsewhere, tests)"""
    from . import _capi
    from .index import quant_kind
    return _capi.QuantParams(kind=quant_kind(kind), dims=dims, slope=float(F(slope)), offset=int(offset), max_val=float(F(max_val)))
