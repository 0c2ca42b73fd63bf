"""Four-bit rows, host side: the numpy restatements that the GPU tests compare the device against (parlayann_amd/quantize.py)
-- nibble packing as Quantized_Mips_Point<4>::assign / operator[] (mips_point.h:306-311, 399-406), translate_point with
range 15 (mips_point.h:416-430, euclidian_point.h:193-207) -- on hand-computed cases, and the argument checks of
GraphIndex(quant_bits=...), which come before any device call.  All values are dyadic, so every product below is exact in
float32 and the expected numbers can be worked out on paper."""
import numpy as np
import pytest

from parlayann_amd import quantize
from parlayann_amd.graph_index import FloatEuclidianIndex, FloatMipsIndex


@pytest.mark.parametrize("d", [1, 2, 7, 33])
@pytest.mark.parametrize("signed", [False, True])
def test_pack_unpack_round_trip(d, signed):
    rng = np.random.default_rng(d)
    v = rng.integers(-8, 8, (5, d)).astype(np.int8) if signed else rng.integers(0, 16, (5, d)).astype(np.uint8)
    v[0, :] = -8 if signed else 15                      # the extreme value in every position
    p = quantize.pack_nibbles(v)
    assert p.dtype == np.uint8 and p.shape == (5, (d + 1) // 2)
    back = quantize.unpack_nibbles(p, d, signed)
    assert back.dtype == (np.int8 if signed else np.uint8) and np.array_equal(back, v)
    if d % 2:
        assert (p[:, -1] >> 4 == 0).all()               # odd d: the last high nibble is zero


def test_even_coordinate_sits_in_the_low_nibble():
    p = quantize.pack_nibbles(np.array([[1, 2, 3, 4, 5]], np.uint8))
    assert p.tolist() == [[0x21, 0x43, 0x05]]
    p = quantize.pack_nibbles(np.array([[-1, 7, -8]], np.int8))
    assert p.tolist() == [[0x7F, 0x08]]


def test_signed_unpack_of_8_to_f_is_minus_8_to_minus_1():
    rows = np.array([[0x98, 0xBA, 0xDC, 0xFE]], np.uint8)          # nibbles 8, 9, ..., 15 in coordinate order
    assert quantize.unpack_nibbles(rows, 8, True).tolist() == [[-8, -7, -6, -5, -4, -3, -2, -1]]
    assert quantize.unpack_nibbles(rows, 8, False).tolist() == [[8, 9, 10, 11, 12, 13, 14, 15]]
    assert quantize.unpack_nibbles(rows, 7, True).tolist() == [[-8, -7, -6, -5, -4, -3, -2]]


def test_pack_refuses_what_does_not_fit():
    with pytest.raises(ValueError):
        quantize.pack_nibbles(np.array([[16]], np.int16))
    with pytest.raises(ValueError):
        quantize.pack_nibbles(np.array([[-9]], np.int16))
    with pytest.raises(ValueError):
        quantize.unpack_nibbles(np.zeros((2, 3), np.uint8), 8, False)


def test_mips_i4_translate():
    # max_val 7: scale = 7 / 7 = 1, so the rounding is on the values themselves
    x = np.array([[7.0, -7.0, 8.0, -100.0, 0.0, 0.5, -0.5, 2.5, -2.5, 1.25, -0.25, 6.5]], np.float32)
    got = quantize.mips_i4_translate(x, np.float32(7.0))
    assert got.dtype == np.int8
    #                        +-max     beyond    0   halves go away from zero      plain
    assert got.tolist() == [[7, -7,    7, -7,    0,  1, -1, 3, -3,                 1, 0, 7]]
    # max_val 3.5: scale 2
    got = quantize.mips_i4_translate(np.array([[0.25, 1.25, -1.75, 3.5, 3.75, -3.5]], np.float32), np.float32(3.5))
    assert got.tolist() == [[1, 3, -4, 7, 7, -7]]
    assert quantize.pack_nibbles(quantize.mips_i4_translate(np.zeros((1, 3), np.float32), np.float32(1.0))).tolist() == [[0, 0]]


def test_euclid_u4_params_and_translate_by_hand():
    # min -1, max 2: slope = 15 / 3 = 5, offset = round(-5) = -5, r = round(5 x) + 5
    X = np.array([[-1.0, 0.0, 0.5, 2.0],            # 5x = -5, 0, 2.5 (-> 3), 10            -> 0, 5, 8, 15
                  [0.25, -0.5, 1.0, 1.75],          # 1.25 (-> 1), -2.5 (-> -3), 5, 8.75 (-> 9) -> 6, 2, 10, 14
                  [-0.75, 1.5, 0.125, -0.125]],     # -3.75 (-> -4), 7.5 (-> 8), .625, -.625  -> 1, 13, 6, 4
                 np.float32)
    p = quantize.euclid_u4_params(X)
    assert (p.slope, int(p.offset), p.range, p.dims) == (np.float32(5.0), -5, 15, 4)
    got = quantize.euclid_u4_translate(X, p)
    assert got.dtype == np.uint8
    assert got.tolist() == [[0, 5, 8, 15], [6, 2, 10, 14], [1, 13, 6, 4]]
    # query rows beyond min / max clamp to 0 and 15
    assert quantize.euclid_u4_translate(np.array([[-2.0, 3.0, -1.25, 2.125]], np.float32), p).tolist() == [[0, 15, 0, 15]]


def test_euclid_u4_params_start_at_zero_and_never_become_a_cast():
    # all values positive: the running minimum starts at 0 (euclidian_point.h:216-217)
    p = quantize.euclid_u4_params(np.array([[1.0, 3.0]], np.float32))
    assert (p.slope, int(p.offset)) == (np.float32(5.0), 0)
    # non-negative integers below 256: the one-byte quantiser substitutes max = 255 and casts; four bits cannot
    Xi = np.array([[0, 1, 2, 3]], np.float32)
    assert quantize.euclid_u8_params(Xi).identity
    p = quantize.euclid_u4_params(Xi)
    assert (p.slope, int(p.offset)) == (np.float32(5.0), 0)
    assert quantize.euclid_u4_translate(Xi, p).tolist() == [[0, 5, 10, 15]]
    # slope 1, offset 0 (max - min = 15) still rounds and clamps
    p = quantize.euclid_u4_params(np.array([[0.0, 15.0]], np.float32))
    assert p.slope == np.float32(1.0) and int(p.offset) == 0
    assert quantize.euclid_u4_translate(np.array([[2.5, 200.0, -3.0]], np.float32), p).tolist() == [[3, 15, 0]]


@pytest.mark.parametrize("cls", [FloatEuclidianIndex, FloatMipsIndex])
def test_graph_index_checks_quant_bits_before_anything_else(cls, tmp_path):
    missing = str(tmp_path / "no-such-file")              # the checks come before the files are opened or a device is used
    with pytest.raises(ValueError, match="quant_bits"):
        cls(missing, missing, quant_bits=5)
    with pytest.raises(ValueError, match="quant_bits"):
        cls(missing, missing, quant_bits=0)
    with pytest.raises(ValueError, match="quant_bits=4"):
        cls(missing, missing, quant_bits=4, second_level="bit")
