"""Bit sketches for the two-level search: the reference's low-precision point types that feed
filtered_beam_search(..., use_filtering = true) (beamSearch.h:98-100,117-123,139-146).

  Euclidean_Bit_Point  euclidian_point.h:332-420  median = (long) sorted[n*d/2]; bit = x > (float) median; Hamming
  Mips_Bit_Point       mips_point.h:625-702       bit = x > 0; Hamming
  Mips_2Bit_Point      mips_point.h:495-623       cut = max(sorted[b], -sorted[a]); per 64 dims a sign word and a
                                                  non-zero-mask word; distance sum 2 pop(ne & nz) - pop(nz)

The device path (csrc/sketch.hip through the C-ABI) is what the product runs; the *_numpy functions restate the same
rules on the host and are what the tests check it against.  Rows are uint8 arrays in the reference's layout
(num_bytes() per row, little-endian 64-bit words); bits the reference never writes are 0.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import PANN_SKETCH_EUCLID_BIT, PANN_SKETCH_MIPS_2BIT, PANN_SKETCH_MIPS_BIT, SketchParams, check

F = np.float32
_KINDS = {"euclid_bit": PANN_SKETCH_EUCLID_BIT, "euclidean_bit": PANN_SKETCH_EUCLID_BIT, "mips_bit": PANN_SKETCH_MIPS_BIT,
          "mips_2bit": PANN_SKETCH_MIPS_2BIT, "2bit": PANN_SKETCH_MIPS_2BIT}


def sketch_kind(kind):
    if kind in (PANN_SKETCH_EUCLID_BIT, PANN_SKETCH_MIPS_BIT, PANN_SKETCH_MIPS_2BIT):
        return int(kind)
    try:
        return _KINDS[str(kind).lower()]
    except KeyError:
        raise ValueError(f"unknown sketch kind {kind!r}") from None


def row_bytes(kind, dims):
    """parameters::num_bytes()"""
    return ((dims - 1) // 64 + 1) * 8 * (2 if sketch_kind(kind) == PANN_SKETCH_MIPS_2BIT else 1)


def make_params(kind, dims, median=0, cut=0.0, hamming_as_written=False):
    return SketchParams(kind=sketch_kind(kind), dims=int(dims), median=int(median), cut=float(F(cut)),
                        hamming_as_written=1 if hamming_as_written else 0)


# ---- device path --------------------------------------------------------------------------------------------------------------

def select_ranks(length, kind):
    """pann_sketch_select_ranks: the sorted positions generate_parameters reads for `length` values"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _capi.load().pann_sketch_select_ranks(int(length), sketch_kind(kind), C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def sketch_params(index, kind):
    """generate_parameters over the rows of a float32 DeviceIndex, on the device (exact order statistics, no sort)"""
    p = SketchParams()
    check(_capi.load().pann_sketch_params_generate(index.handle, sketch_kind(kind), C.byref(p)))
    return p


def attach_sketch(index, src, params):
    """Sketch every row of the float32 DeviceIndex `src` with `params`; the slab belongs to `index` (the handle that is
    searched: any element type, same n, d and device; may be `src`) and replaces a sketch attached earlier."""
    check(_capi.load().pann_index_attach_sketch(index.handle, src.handle, C.byref(params)))


def drop_sketch(index):
    check(_capi.load().pann_index_drop_sketch(index.handle))


def attached_kind(index):
    """-1: no sketch attached"""
    return int(_capi.load().pann_index_sketch_kind(index.handle))


def download_sketch(index, first_row=0, nrows=None):
    kind = attached_kind(index)
    if kind < 0:
        raise ValueError("no sketch attached")
    nrows = index.n - first_row if nrows is None else nrows
    out = np.empty((nrows, row_bytes(kind, index.d)), np.uint8)
    check(_capi.load().pann_index_download_sketch(index.handle, first_row, nrows, out.ctypes.data_as(C.c_void_p), out.shape[1]))
    return out


def sketch_rows(x, params, device=0):
    """Sketches of float rows (the queries), translated on the device -> uint8[n, num_bytes()]"""
    x = np.ascontiguousarray(x, dtype=F)
    if x.ndim != 2 or x.shape[1] != params.dims:
        raise ValueError(f"rows must be n x {params.dims} float32")
    out = np.empty((len(x), row_bytes(params.kind, params.dims)), np.uint8)
    if len(x):
        check(_capi.load().pann_sketch_rows(C.byref(params), x.ctypes.data_as(C.c_void_p), len(x), x.shape[1] * 4,
                                            out.ctypes.data_as(C.c_void_p), out.shape[1], device))
    return out


# ---- numpy reference ----------------------------------------------------------------------------------------------------------

def select_ranks_numpy(length, kind):
    """the reference's index expressions, evaluated with numpy scalars of the same types"""
    kind = sketch_kind(kind)
    n = int(length)
    if kind == PANN_SKETCH_EUCLID_BIT:
        a = b = n // 2                                                   # vals[n*dims/2]
    elif kind == PANN_SKETCH_MIPS_2BIT:
        a = int(F(0.3) * F(n))                                           # (long)(cutoff * len): float arithmetic
        b = int((np.float64(1.0) - np.float64(F(0.3))) * np.float64(n - 1))   # (long)((1.0 - cutoff) * (len - 1)): double
    else:
        a = b = 0
    return min(a, n - 1), min(b, n - 1)


def sketch_params_numpy(x, kind, hamming_as_written=False):
    """generate_parameters by a full sort of every coordinate"""
    x = np.asarray(x, dtype=F)
    kind = sketch_kind(kind)
    p = make_params(kind, x.shape[1], hamming_as_written=hamming_as_written)
    if kind == PANN_SKETCH_MIPS_BIT:
        return p
    vals = np.sort(x.ravel())
    a, b = select_ranks_numpy(vals.size, kind)
    if kind == PANN_SKETCH_EUCLID_BIT:
        p.median = int(np.trunc(np.float64(vals[a])))                    # long median = vals[...]: truncating conversion
    else:
        p.cut = float(max(vals[b], -vals[a]))
    return p


def sketch_rows_numpy(x, params):
    x = np.asarray(x, dtype=F)
    n, d = x.shape
    assert d == params.dims
    nblk = (d - 1) // 64 + 1
    pad = np.zeros((n, nblk * 64), bool)

    def words(bits):
        pad[:] = False
        pad[:, :d] = bits
        return np.packbits(pad, axis=1, bitorder="little").reshape(n, nblk, 8)

    if params.kind == PANN_SKETCH_MIPS_2BIT:
        cv = F(params.cut)
        neg = x < -cv
        pos = ~neg & (x > cv)
        out = np.empty((n, nblk, 2, 8), np.uint8)
        out[:, :, 0] = words(pos)                                        # sign: 1 above the cut, 0 below -cut (and where mask = 0)
        out[:, :, 1] = words(neg | pos)                                  # mask: the coordinate is not "zero"
        return out.reshape(n, nblk * 16)
    thr = F(np.int64(params.median)) if params.kind == PANN_SKETCH_EUCLID_BIT else F(0)
    return words(x > thr).reshape(n, nblk * 8).copy()


def _popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1), axis=1).sum(axis=1, dtype=np.int64)


def sketch_distance_numpy(rows, q, params):
    """distance() of every sketch row to the sketch q, as the float32 the reference returns"""
    rows = np.asarray(rows, np.uint8)
    q = np.asarray(q, np.uint8).reshape(1, -1)
    n = rows.shape[0]
    if params.kind == PANN_SKETCH_MIPS_2BIT:
        r = rows.reshape(n, -1, 2, 8)
        qq = q.reshape(1, -1, 2, 8)
        ne = r[:, :, 0] ^ qq[:, :, 0]
        nz = r[:, :, 1] & qq[:, :, 1]
        return (2 * _popcount(ne & nz) - _popcount(nz)).astype(F)
    x = rows ^ q
    if params.hamming_as_written:                                        # the loop never advances: block 0, num_blocks times
        nblk = (params.dims - 1) // 64 + 1
        return (nblk * _popcount(x[:, :8])).astype(F)
    return _popcount(x).astype(F)
