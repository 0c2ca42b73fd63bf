"""FP8 (OCP E4M3FN) for numpy, which has no such type: a one-field structured dtype over uint8.  An array of `float8_e4m3` is one
byte per element like the device rows, is told apart from a plain uint8 array by its dtype (so the C-ABI gets PANN_F8), and converts
with `to_f8` / `from_f8`.  A byte is 1 sign bit, 4 exponent bits (bias 7), 3 mantissa bits; there are subnormals and no infinities,
the largest magnitude is 448, and the codes 0x7F / 0xFF are NaN.  (PANN_F8 is this build's extension.)"""
import numpy as np

float8_e4m3 = np.dtype([("f8", np.uint8)])
F8_MAX = np.float32(448.0)


def _table():
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (8.0 + m) * 2.0 ** (e.astype(np.float64) - 10))      # subnormals: m / 8 * 2^-6
    v = np.where(c & 128, -v, v)
    v[[0x7F, 0xFF]] = np.nan
    return v.astype(np.float32)                                                               # every value is exact in f32


TABLE = _table()
_POS = TABLE[:0x7F].astype(np.float64)                                                        # the 127 codes 0 .. 448, ascending


def from_f8(a):
    """float8_e4m3 (or plain uint8 codes) -> float32, exact, from the 256-entry table"""
    return TABLE[np.ascontiguousarray(a).view(np.uint8)].reshape(np.shape(a))


def to_f8(x):
    """float array -> float8_e4m3 array: round to nearest on the E4M3 grid, ties to the even code; magnitudes above 448 saturate to
    +-448, so a finite input never gives a NaN code; -0.0 keeps its sign (code 0x80).  NaN -> 0x7F."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    mag = np.minimum(np.abs(f.astype(np.float64)), 448.0)
    hi = np.clip(np.searchsorted(_POS, mag, side="left"), 1, 0x7E)                            # _POS[hi - 1] <= mag <= _POS[hi]
    lo = hi - 1
    dl, dh = mag - _POS[lo], _POS[hi] - mag                                                   # exact in f64
    code = np.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi).astype(np.uint8)        # neighbouring codes: one is even
    code[np.isnan(f)] = 0x7F
    code |= (np.signbit(f) & ~np.isnan(f)).astype(np.uint8) << 7
    return code.view(float8_e4m3).reshape(f.shape)
