"""Bit sketches on the device (csrc/sketch.hip) against the numpy restatement in parlayann_amd/sketch.py: parameters equal a
full-sort reference exactly, attached and query sketches are bit-identical to the numpy packer, undefined bits are zero."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import DeviceIndex, PannError, _capi
from parlayann_amd import sketch as sk

pytestmark = pytest.mark.gpu

KINDS = ("euclid_bit", "mips_bit", "mips_2bit")


def _param_data(name):
    rng = np.random.default_rng(5)
    if name == "signed":
        return (rng.standard_normal((301, 37)) * 900).astype(np.float32)                 # n * d odd
    if name == "duplicates":
        return rng.integers(-3, 4, size=(300, 38)).astype(np.float32)                    # n * d even, few distinct values
    if name == "constant":
        return np.full((64, 9), 2.5, np.float32)
    if name == "zeros":
        x = rng.integers(-1, 2, size=(257, 31)).astype(np.float32)
        x[x == 0] = np.where(rng.random(int((x == 0).sum())) < 0.5, 0.0, -0.0)            # +0 and -0 mixed
        return x
    if name == "fractional":
        return (rng.random((128, 64)) * 7.9 - 3.3).astype(np.float32)                     # truncation towards zero on both sides
    raise KeyError(name)


@pytest.mark.parametrize("name", ["signed", "duplicates", "constant", "zeros", "fractional"])
def test_parameters_equal_a_full_sort(name):
    X = _param_data(name)
    ix = DeviceIndex(X, max_degree=4, metric="mips")
    try:
        for kind in KINDS:
            p, e = sk.sketch_params(ix, kind), sk.sketch_params_numpy(X, kind)
            assert (p.kind, p.dims, p.hamming_as_written) == (e.kind, X.shape[1], 0)
            assert p.median == e.median, (kind, p.median, e.median)
            assert np.float32(p.cut) == np.float32(e.cut), (kind, p.cut, e.cut)
    finally:
        ix.close()


@pytest.mark.parametrize("d", [1, 63, 64, 65, 100, 128, 200, 768, 1024, 2048])
def test_attached_sketch_is_bit_identical(d):
    rng = np.random.default_rng(d)
    n = 257
    X = (rng.standard_normal((n, d)) * 2).astype(np.float32)
    X[rng.random((n, d)) < 0.1] = 0.0
    ix = DeviceIndex(X, max_degree=4, metric="mips")
    try:
        assert sk.attached_kind(ix) == -1
        for kind in KINDS:
            p = sk.sketch_params(ix, kind)
            sk.attach_sketch(ix, ix, p)
            assert sk.attached_kind(ix) == p.kind
            got, exp = sk.download_sketch(ix), sk.sketch_rows_numpy(X, p)
            assert got.shape == exp.shape == (n, sk.row_bytes(kind, d))
            np.testing.assert_array_equal(got, exp)
            # undefined bits: positions >= d (and, 2-bit, sign bits under a clear mask bit) are zero
            w = got.view("<u8").reshape(n, -1)
            tail = d % 64
            if tail:
                hi = np.uint64(~((1 << tail) - 1) & (2 ** 64 - 1))
                assert not (w[:, -1] & hi).any() and (kind != "mips_2bit" or not (w[:, -2] & hi).any())
            if kind == "mips_2bit":
                assert not (w[:, 0::2] & ~w[:, 1::2]).any()
            part = sk.download_sketch(ix, 5, 11)
            np.testing.assert_array_equal(part, exp[5:16])
        sk.drop_sketch(ix)
        assert sk.attached_kind(ix) == -1
    finally:
        ix.close()


def test_sketch_on_another_handle_and_replacement():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((500, 96)).astype(np.float32)
    X8 = np.clip(np.rint(X * 40), -127, 127).astype(np.int8)
    src, ix = DeviceIndex(X, max_degree=4, metric="mips"), DeviceIndex(X8, max_degree=4, metric="mips")
    try:
        p = sk.sketch_params(src, "mips_2bit")
        sk.attach_sketch(ix, src, p)
        np.testing.assert_array_equal(sk.download_sketch(ix), sk.sketch_rows_numpy(X, p))
        p1 = sk.make_params("mips_bit", 96)
        sk.attach_sketch(ix, src, p1)                  # replaces
        assert sk.attached_kind(ix) == _capi.PANN_SKETCH_MIPS_BIT
        np.testing.assert_array_equal(sk.download_sketch(ix), sk.sketch_rows_numpy(X, p1))
        assert sk.attached_kind(src) == -1
    finally:
        src.close(); ix.close()


def test_width_and_source_limits():
    X = np.zeros((8, 2049), np.float32)
    ix = DeviceIndex(X, max_degree=4, metric="mips")
    i8 = DeviceIndex(np.zeros((8, 16), np.int8), max_degree=4, metric="mips")
    try:
        with pytest.raises(PannError) as e:
            sk.sketch_params(ix, "mips_bit")
        assert e.value.code == 4                       # PANN_ERR_UNSUPPORTED
        with pytest.raises(PannError) as e:
            sk.attach_sketch(ix, ix, sk.make_params("mips_bit", 2049))
        assert e.value.code == 4
        with pytest.raises(PannError) as e:
            sk.sketch_params(i8, "mips_bit")           # not an f32 source
        assert e.value.code == 4
        with pytest.raises(PannError) as e:
            sk.sketch_rows(np.zeros((2, 2049), np.float32), sk.make_params("mips_bit", 2049))
        assert e.value.code == 4
    finally:
        ix.close(); i8.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [65, 128, 200])
def test_query_sketches_host_and_device_forms_agree(kind, d):
    import torch
    rng = np.random.default_rng(d + len(kind))
    n, pad = 70, 3
    buf = np.full((n, d + pad), 3.0e30, np.float32)    # strided host rows; the pad floats must never be read
    buf[:, :d] = rng.standard_normal((n, d)) * 3
    X = buf[:, :d]
    p = sk.make_params(kind, d, median=1, cut=0.7)
    exp = sk.sketch_rows_numpy(np.ascontiguousarray(X), p)
    rb = sk.row_bytes(kind, d)
    lib = _capi.load()
    # host form, strided input and strided output
    out = np.full((n, rb + 8), 0x5A, np.uint8)
    _capi.check(lib.pann_sketch_rows(C.byref(p), buf.ctypes.data_as(C.c_void_p), n, buf.strides[0], out.ctypes.data_as(C.c_void_p),
                                     out.strides[0], 0))
    np.testing.assert_array_equal(out[:, :rb], exp)
    assert (out[:, rb:] == 0x5A).all()
    np.testing.assert_array_equal(sk.sketch_rows(np.ascontiguousarray(X), p), exp)
    # device form
    t = torch.from_numpy(buf).cuda()
    o = torch.full((n, rb + 8), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _capi.check(lib.pann_sketch_rows_dev(C.byref(p), C.c_void_p(t.data_ptr()), n, buf.strides[0], C.c_void_p(o.data_ptr()), rb + 8, None))
    torch.cuda.synchronize()
    od = o.cpu().numpy()
    np.testing.assert_array_equal(od[:, :rb], exp)
    assert (od[:, rb:] == 0x5A).all()
