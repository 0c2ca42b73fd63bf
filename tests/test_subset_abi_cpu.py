"""CPU-only: libpann.so exports the two subset entry points, and each refuses a NULL source handle before it touches a device."""
import ctypes as C

import pytest

from parlayann_amd import _capi

NAMES = ("pann_index_create_subset", "pann_index_create_subset_dev")


@pytest.mark.parametrize("name", NAMES)
def test_subset_entry_points_are_exported_and_refuse_a_null_source(name):
    assert name in _capi.SIGNATURES
    lib = _capi.load()
    fn = getattr(lib, name)
    out, kept = C.c_void_p(), C.c_uint64(12345)
    rc = fn(C.byref(out), None, None, 0, 1, None, 0, None, C.byref(kept))
    assert rc == _capi.PANN_ERR_BAD_ARG and out.value is None and kept.value == 12345
    assert name in lib.pann_last_error().decode()
    assert fn(None, None, None, 0, 1, None, 0, None, None) == _capi.PANN_ERR_BAD_ARG          # and a NULL `out`
