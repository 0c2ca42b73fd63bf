"""CPU-only: the sorted positions the device radix select looks for (pann_quantize_select_ranks) are the ones
Quantized_Mips_Point<8, trim>::generate_parameters reads (mips_point.h:448-451).  Witness: the oracle, which sorts -- on
x = 0, 1, 2, ... its max_val is the value at position b, on the negated array it is len - 1 - a."""
import ctypes as C

import numpy as np
import pytest


def _ranks(n, trim):
    from parlayann_amd import _capi
    a, b = C.c_uint64(), C.c_uint64()
    _capi.load().pann_quantize_select_ranks(n, 1 if trim else 0, C.byref(a), C.byref(b))
    return a.value, b.value


@pytest.mark.parametrize("n", [1, 2, 7, 9999, 10000, 10001, 123457, 1 << 20, 4_000_003])
def test_ranks_are_the_positions_the_oracle_reads(oracle, n):
    x = np.arange(n, dtype=np.float32)[:, None]              # exact in f32 (n < 2^24)
    for trim in (True, False):
        a, b = _ranks(n, trim)
        assert b == int(oracle.mips_i8_maxval(x, trim=trim))
        assert n - 1 - a == int(oracle.mips_i8_maxval(-x, trim=trim))


def test_ranks_at_two_billion_values():
    n = 2_000_000_000                                            # 10M x 200
    a, b = _ranks(n, True)
    assert a == int(np.float32(0.0001) * np.float32(n))          # (long)(cutoff * len): float arithmetic
    assert b == int((1.0 - float(np.float32(0.0001))) * (n - 1)) # (long)((1.0 - cutoff) * (len - 1)): double
    assert _ranks(n, False) == (0, n - 1)
