"""Scalar quantisation on the device (csrc/quantize.hip: Euclid parameters, exact order statistics, normalize, translate)
against the oracle's sequential C++ restatement of euclidian_point.h:182-235 and mips_point.h:115-124,416-486.
Everything is compared bit for bit: no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import DeviceIndex, PannError, _capi, datasets, io, quantize, wrapper

pytestmark = pytest.mark.gpu

EU, MI = _capi.PANN_QUANT_EUCLID_U8, _capi.PANN_QUANT_MIPS_I8
PAD_VALUE = 3.0e30          # sits between the rows of a strided source: a kernel that reads it shows in min / max / the ranks


def _dev_rows(X, pad=0):
    """X on the device as rows with a stride of (d + pad) floats; -> (tensor that owns the memory, address, stride in bytes)"""
    import torch
    X = np.ascontiguousarray(X, np.float32)
    buf = np.full((X.shape[0], X.shape[1] + pad), PAD_VALUE, np.float32)
    buf[:, :X.shape[1]] = X
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr(), buf.shape[1] * 4


def _params_dev(X, kind, trim=True, pad=0):
    t, ptr, stride = _dev_rows(X, pad)
    p = _capi.QuantParams()
    _capi.check(_capi.load().pann_quantize_params_dev(C.c_void_p(ptr), X.shape[0], X.shape[1], stride, kind, 1 if trim else 0,
                                                      C.byref(p), None))
    return p


def _rows_dev(X, p, pad=0, out_pad=0, normalize_first=False):
    """pann_quantize_rows_dev on a strided source into a strided destination; the destination's pad bytes must stay untouched"""
    import torch
    t, ptr, stride = _dev_rows(X, pad)
    n, d = X.shape
    out = torch.full((n, d + out_pad), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _capi.check(_capi.load().pann_quantize_rows_dev(C.byref(p), C.c_void_p(ptr), n, stride, 1 if normalize_first else 0,
                                                    C.c_void_p(out.data_ptr()), d + out_pad, None))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, d:] == 0x5A).all(), "bytes beyond a destination row were written"
    return o[:, :d].view(np.uint8 if p.kind == EU else np.int8)


# ---- 1. Euclid u8, real-valued --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [96, 100, 25, 3, 1])
@pytest.mark.parametrize("pad", [0, 4, 1])
def test_euclid_u8_real_valued(oracle, d, pad):
    X = np.ascontiguousarray((datasets.deep_like(3000, d, seed=1) * 3.0 - 0.7).astype(np.float32))
    slope, offset = oracle.euclid_u8_params(X)
    p = _params_dev(X, EU, pad=pad)
    assert np.float32(p.slope) == slope and p.offset == offset and p.dims == d and not p.identity
    exp = oracle.euclid_u8_translate(X, slope, offset)
    np.testing.assert_array_equal(_rows_dev(X, p, pad=pad, out_pad=0), exp)
    np.testing.assert_array_equal(_rows_dev(X, p, pad=pad, out_pad=16 - d % 16), exp)      # 16-byte aligned destination rows
    np.testing.assert_array_equal(_rows_dev(X, p, pad=pad, out_pad=3), exp)
    np.testing.assert_array_equal(quantize.device_quantize_rows(X, p), exp)                # host-pointer form
    if d == 96 and pad == 0:
        pn = quantize.euclid_u8_params(X)                                                  # second witness (numpy)
        assert pn.slope == np.float32(p.slope) and int(pn.offset) == p.offset


def test_euclid_u8_from_index_slab(oracle):
    for d in (96, 100, 25):
        X = np.ascontiguousarray((datasets.deep_like(3000, d, seed=1) * 3.0 - 0.7).astype(np.float32))
        slope, offset = oracle.euclid_u8_params(X)
        ix = DeviceIndex(X, max_degree=4)
        q, p = ix.quantized("euclid_u8")
        assert np.float32(p.slope) == slope and p.offset == offset
        np.testing.assert_array_equal(q.points(), oracle.euclid_u8_translate(X, slope, offset))
        np.testing.assert_array_equal(ix.points(), X)
        np.testing.assert_array_equal(ix.points(10, 5), X[10:15])
        q.close(); ix.close()


# ---- 2. Euclid u8, integer-valued ------------------------------------------------------------------------------------------

def test_euclid_u8_integer_valued_is_plain_cast(oracle):
    X = datasets.sift_like(2000, 64, seed=1, dtype=np.float32)
    slope, offset = oracle.euclid_u8_params(X)
    assert slope == 1.0 and offset == 0
    for pad in (0, 4):
        p = _params_dev(X, EU, pad=pad)
        assert p.identity and p.slope == 1.0 and p.offset == 0 and p.min_seen == 0.0 and p.max_seen == 255.0
        np.testing.assert_array_equal(_rows_dev(X, p, pad=pad), X.astype(np.uint8))
    np.testing.assert_array_equal(oracle.euclid_u8_translate(X, slope, offset), X.astype(np.uint8))
    # one non-integer value (min 0, max 255 as seen: still slope 1, now as real-valued data), one negative value (slope 255 / 256)
    for bad in (0.5, -1.0):
        Y = X.copy(); Y[1234, 17] = bad
        s2, o2 = oracle.euclid_u8_params(Y)
        p = _params_dev(Y, EU)
        assert np.float32(p.slope) == s2 and p.offset == o2 and p.identity == (s2 == 1.0 and o2 == 0)
        np.testing.assert_array_equal(_rows_dev(Y, p), oracle.euclid_u8_translate(Y, s2, o2))


# ---- 3. rounding -------------------------------------------------------------------------------------------------------------

def test_rounding_is_std_round(oracle):
    h = [np.float32(0.49999997) / 2, 0.5 / 2, 1.5 / 2, 2.5 / 2, 126.5 / 2, 254.5 / 2]
    x = np.array([h + [-v for v in h] + [200.0, 1e9, -200.0, -1e9, 127.75, 0.0]], np.float32)
    p = quantize.device_params("euclid_u8", x.shape[1], slope=2.0, offset=0)
    exp = oracle.euclid_u8_translate(x, np.float32(2.0), 0)
    assert exp[0, 0] == 0 and exp[0, 1] == 1                       # 0.49999997 -> 0, 0.5 -> 1: floor(v + 0.5f) gives 1, 1
    np.testing.assert_array_equal(_rows_dev(x, p), exp)
    np.testing.assert_array_equal(quantize.device_quantize_rows(x, p), exp)
    p = quantize.device_params("euclid_u8", x.shape[1], slope=2.0, offset=-3)
    np.testing.assert_array_equal(_rows_dev(x, p), oracle.euclid_u8_translate(x, np.float32(2.0), -3))

    x = np.array([[0.5 / 127, -0.5 / 127, 2.0, -2.0, 1.0, 2.5 / 127]], np.float32)       # the row of test_mips_int8
    p = quantize.device_params("mips_i8", 6, max_val=1.0)
    np.testing.assert_array_equal(_rows_dev(x, p), oracle.mips_i8_translate(x, np.float32(1.0)))
    x = np.array([[0.49999997, -0.49999997, 126.5, 127.0, 127.00001, -126.5, -127.0, -127.00001, 0.5, -0.5, 1.5, -1.5]], np.float32)
    p = quantize.device_params("mips_i8", x.shape[1], max_val=127.0)                       # scale == 1
    exp = oracle.mips_i8_translate(x, np.float32(127.0))
    assert exp[0, 0] == 0 and exp[0, 1] == 0 and exp[0, 2] == 127
    np.testing.assert_array_equal(_rows_dev(x, p), exp)
    np.testing.assert_array_equal(quantize.device_quantize_rows(x, p), exp)


# ---- 4. normalize ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4000, 20000])
def test_normalize_is_the_sequential_double_sum(oracle, n):
    X = datasets.t2i_like(n, 200, seed=1)
    X[7] = 0.0                                                       # norm == 0 -> 1: the row stays zero
    ix = DeviceIndex(X, max_degree=4, metric="mips")
    ix.normalize()
    got = ix.points()
    exp = oracle.normalize(X)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert not got[7].any()
    ix.close()


@pytest.mark.parametrize("d", [200, 100, 25, 3, 1, 300])
def test_normalize_then_translate_of_const_rows(oracle, d):
    X = datasets.t2i_like(1500, d, seed=3)
    X[11] = 0.0
    Xn = oracle.normalize(X)
    mv = oracle.mips_i8_maxval(Xn, trim=True)
    p = quantize.device_params("mips_i8", d, max_val=mv)
    exp = oracle.mips_i8_translate(Xn, mv)
    for pad, out_pad in ((0, 0), (4, 16 - d % 16), (1, 3)):
        np.testing.assert_array_equal(_rows_dev(X, p, pad=pad, out_pad=out_pad, normalize_first=True), exp)
    np.testing.assert_array_equal(quantize.device_quantize_rows(X, p, normalize_first=True), exp)
    ix = DeviceIndex(X, max_degree=4, metric="mips")
    ix.normalize()
    assert np.array_equal(ix.points().view(np.uint32), Xn.view(np.uint32))
    ix.close()


# ---- 5. order statistics -----------------------------------------------------------------------------------------------------

def _check_maxval(oracle, X, pads=(0,)):
    X = np.ascontiguousarray(X, np.float32)
    for trim in (True, False):
        exp = oracle.mips_i8_maxval(X, trim=trim)
        for pad in pads:
            p = _params_dev(X, MI, trim=trim, pad=pad)
            assert np.float32(p.max_val) == exp, (trim, pad, p.max_val, exp)
            assert np.float32(max(p.max_seen, -p.min_seen)) == exp


def test_select_normalised_t2i(oracle):
    Xn = oracle.normalize(datasets.t2i_like(4000, 200, seed=1))
    _check_maxval(oracle, Xn, pads=(0, 4, 1))
    assert quantize.mips_i8_max_val(Xn, trim=True) == np.float32(_params_dev(Xn, MI).max_val)      # second witness


def test_select_fewer_values_than_one_histogram(oracle):
    _check_maxval(oracle, np.array([[0.3, -0.9, 0.1, 0.0, 0.7, -0.2, 0.5]], np.float32), pads=(0, 1))
    _check_maxval(oracle, np.array([[0.25]], np.float32))
    _check_maxval(oracle, np.array([[-0.25], [0.125], [0.0]], np.float32), pads=(0, 3))


def test_select_all_values_equal(oracle):
    _check_maxval(oracle, np.full((500, 30), -0.375, np.float32), pads=(0, 2))
    _check_maxval(oracle, np.zeros((100, 9), np.float32))


@pytest.mark.parametrize("rep", [-10.0, 10.0, 0.25])
def test_select_repeated_value_straddles_a_rank(oracle, rep):
    rng = np.random.default_rng(5)
    X = rng.standard_normal(1000 * 50).astype(np.float32)
    X[rng.permutation(X.size)[:X.size * 6 // 10]] = rep            # 60 % one number: below every other value, above, in the middle
    _check_maxval(oracle, X.reshape(1000, 50), pads=(0, 2))


def test_select_mixed_signs_and_both_zeros(oracle):
    rng = np.random.default_rng(6)
    X = np.zeros(40000, np.float32)
    X[::2] = -0.0
    X[:3] = [-5.0, 7.0, -1e-40]                                      # a subnormal too
    _check_maxval(oracle, rng.permutation(X).reshape(400, 100))         # both ranks land on a zero: compared with ==
    Y = rng.standard_normal(30000).astype(np.float32)
    Y[::3] = 0.0; Y[1::3] = -0.0
    _check_maxval(oracle, Y.reshape(300, 100))
    _check_maxval(oracle, -np.abs(Y).reshape(300, 100))                 # nothing positive: max_val = -v[a]


def test_select_values_differ_in_lowest_mantissa_bits(oracle):
    rng = np.random.default_rng(7)
    k = rng.integers(0, 1024, size=60000).astype(np.float32)
    X = (np.float32(1.0) + k * np.float32(2.0 ** -23)).astype(np.float32)      # 22 leading key bits in common: the last pass decides
    _check_maxval(oracle, X.reshape(600, 100))
    _check_maxval(oracle, -X.reshape(600, 100))


def test_select_forty_million_values(oracle):
    rng = np.random.default_rng(8)
    X = rng.standard_normal((200_000, 200), dtype=np.float32)
    X *= np.float32(0.07)
    _check_maxval(oracle, X)


# ---- 6. create_quantized against the host path ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["euclid_u8", "mips_i8"])
def test_create_quantized_equals_uploading_host_quantised_bytes(oracle, kind):
    eu = kind == "euclid_u8"
    d = 100 if eu else 200                                           # 100 bytes: a device row with pad bytes
    X = (datasets.deep_like(5000, d, seed=1) * 2.0).astype(np.float32) if eu else datasets.t2i_like(5000, d, seed=1)
    Q = (datasets.deep_like(80, d, seed=2) * 2.0).astype(np.float32) if eu else datasets.t2i_like(80, d, seed=2)
    metric = "Euclidian" if eu else "mips"
    ix = DeviceIndex(X, max_degree=32, metric=metric)
    if not eu:
        ix.normalize()
        X = oracle.normalize(X); Q = oracle.normalize(Q)
        np.testing.assert_array_equal(ix.points(), X)
    ix.vamana_build(32, 64, 1.2 if eu else 1.0, seed=3)
    G = ix.get_graph()
    q, p = ix.quantized(kind, trim=True)
    if eu:
        slope, offset = oracle.euclid_u8_params(X)
        assert np.float32(p.slope) == slope and p.offset == offset
        Xq = oracle.euclid_u8_translate(X, slope, offset); Qq = oracle.euclid_u8_translate(Q, slope, offset)
    else:
        mv = oracle.mips_i8_maxval(X, trim=True)
        assert np.float32(p.max_val) == mv
        Xq = oracle.mips_i8_translate(X, mv); Qq = oracle.mips_i8_translate(Q, mv)
    ref = DeviceIndex(Xq, G, metric=metric)
    assert q.dtype == Xq.dtype and q.n == ix.n and q.d == d and q.max_degree == 32
    np.testing.assert_array_equal(q.points(), Xq)
    np.testing.assert_array_equal(q.get_graph(), G)                                       # copied device to device
    np.testing.assert_array_equal(quantize.device_quantize_rows(Q, p), Qq)
    rng = np.random.default_rng(1)
    a = rng.integers(0, q.n, 4000).astype(np.uint32); b = rng.integers(0, q.n, 4000).astype(np.uint32)
    np.testing.assert_array_equal(q.pair_distances(a, b), ref.pair_distances(a, b))       # pad bytes are zero on both
    r1 = q.batch_search(Qq, k=10, beam=64); r2 = ref.batch_search(Qq, k=10, beam=64)
    for f in ("ids", "dists", "dist_cmps", "visited_count"):
        np.testing.assert_array_equal(r1[f], r2[f], err_msg=f)
    q2, _ = ix.quantized(kind, params=p, copy_graph=False)
    assert not q2.get_graph()[:, 0].any()                                                   # empty graph when not asked
    np.testing.assert_array_equal(q2.points(), Xq)
    for h in (q, q2, ref, ix):
        h.close()


# ---- 7. GraphIndex on written files ----------------------------------------------------------------------------------------------

def test_graph_index_float_euclidian_real_valued(tmp_path, oracle):
    X = (datasets.deep_like(3000, 96, seed=1) * 2.0).astype(np.float32)
    io.write_bin(tmp_path / "b.bin", X)
    wrapper.build_vamana_index("Euclidian", "float", str(tmp_path / "b.bin"), str(tmp_path / "g"), 32, 64, 1.2, False)
    Index = wrapper.load_index("Euclidian", "float", str(tmp_path / "b.bin"), str(tmp_path / "g"))
    slope, offset = oracle.euclid_u8_params(X)
    assert Index.eparams.slope == slope and int(Index.eparams.offset) == offset and not Index.eparams.identity
    np.testing.assert_array_equal(Index.q_index.points(), oracle.euclid_u8_translate(X, slope, offset))
    np.testing.assert_array_equal(Index.points, X)
    np.testing.assert_array_equal(Index.q_index.get_graph(), io.read_graph(tmp_path / "g"))


def test_graph_index_float_euclidian_integer_valued(tmp_path, oracle):
    X = datasets.sift_like(3000, 128, seed=1234, dtype=np.float32)
    io.write_bin(tmp_path / "b.bin", X)
    wrapper.build_vamana_index("Euclidian", "float", str(tmp_path / "b.bin"), str(tmp_path / "g"), 32, 64, 1.2, True)
    Index = wrapper.load_index("Euclidian", "float", str(tmp_path / "b.bin"), str(tmp_path / "g"))
    assert Index.eparams.identity and Index.eparams.slope == 1.0 and Index.eparams.offset == 0
    np.testing.assert_array_equal(Index.q_index.points(), X.astype(np.uint8))


def test_graph_index_float_mips(tmp_path, oracle):
    X = datasets.t2i_like(3000, 200, seed=1)
    io.write_bin(tmp_path / "b.bin", X)
    wrapper.build_vamana_index("mips", "float", str(tmp_path / "b.bin"), str(tmp_path / "g"), 40, 80, 1.0, False)
    Index = wrapper.load_index("mips", "float", str(tmp_path / "b.bin"), str(tmp_path / "g"))
    Xn = oracle.normalize(X)
    assert np.array_equal(Index.points.view(np.uint32), Xn.view(np.uint32))
    mv = oracle.mips_i8_maxval(Xn, trim=True)
    assert Index.mmax == mv and isinstance(Index.mmax, np.float32)
    np.testing.assert_array_equal(Index.q_index.points(), oracle.mips_i8_translate(Xn, mv))
    np.testing.assert_array_equal(Index.index.points(), Xn)


# ---- 8. error paths ------------------------------------------------------------------------------------------------------------

def test_error_paths():
    lib = _capi.load()
    Xf = datasets.deep_like(64, 16, seed=1).astype(np.float32)
    u8 = DeviceIndex(np.zeros((64, 16), np.uint8), max_degree=4)
    for call in (u8.normalize, lambda: u8.quantize_params("euclid_u8"), lambda: u8.quantized("euclid_u8")):
        with pytest.raises(PannError) as e:
            call()
        assert e.value.code == 4 and lib.pann_last_error()                          # PANN_ERR_UNSUPPORTED: not an f32 handle
    l2 = DeviceIndex(Xf, max_degree=4, metric="Euclidian")
    mips = DeviceIndex(Xf, max_degree=4, metric="mips")
    for ix, kind in ((l2, "mips_i8"), (mips, "euclid_u8")):
        with pytest.raises(PannError) as e:
            ix.quantize_params(kind)
        assert e.value.code == 1 and b"metric" in lib.pann_last_error()             # PANN_ERR_BAD_ARG: kind does not fit the metric
    p = l2.quantize_params("euclid_u8")
    with pytest.raises(PannError) as e:
        mips.quantized("euclid_u8", params=p)
    assert e.value.code == 1
    assert lib.pann_quantize_params(l2.handle, EU, 1, None) == 1 and lib.pann_last_error()
    assert lib.pann_quantize_params(l2.handle, 7, 1, C.byref(p)) == 1 and lib.pann_last_error()
    assert lib.pann_index_create_quantized(None, l2.handle, C.byref(p), 0) == 1 and lib.pann_last_error()
    assert lib.pann_index_download_points(l2.handle, 0, 1, None, 64) == 1 and lib.pann_last_error()
    out = np.empty((64, 16), np.uint8)
    assert lib.pann_index_download_points(l2.handle, 60, 5, out.ctypes.data_as(C.c_void_p), 64) == 1      # beyond the index
    xp = Xf.ctypes.data_as(C.c_void_p)
    assert lib.pann_quantize_rows(C.byref(p), xp, 64, 64, 0, None, 16, 0) == 1 and lib.pann_last_error()
    assert lib.pann_quantize_rows(C.byref(p), xp, 0, 64, 0, out.ctypes.data_as(C.c_void_p), 16, 0) == 1       # n * d == 0
    assert lib.pann_quantize_rows(C.byref(p), xp, 64, 60, 0, out.ctypes.data_as(C.c_void_p), 16, 0) == 1      # stride < row
    t, ptr, stride = _dev_rows(Xf)
    assert lib.pann_quantize_params_dev(C.c_void_p(ptr), 0, 16, stride, EU, 1, C.byref(p), None) == 1
    assert lib.pann_quantize_params_dev(C.c_void_p(ptr), 64, 16, stride, EU, 1, None, None) == 1 and lib.pann_last_error()
    assert lib.pann_quantize_rows_dev(C.byref(p), C.c_void_p(ptr), 64, stride, 0, None, 16, None) == 1 and lib.pann_last_error()
    for h in (u8, l2, mips):
        h.close()
