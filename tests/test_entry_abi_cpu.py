"""CPU-only: libpann.so exports the six entry-point symbols (DESIGN.md "Entry points"), each refuses a NULL handle before it
touches a device and leaves its outputs alone, and without a GPU no handle can be made for them to run on."""
import ctypes as C

import numpy as np
import pytest

from parlayann_amd import _capi

MEDOIDS = ("pann_filter_medoids_labeled", "pann_filter_medoids_labeled_dev", "pann_filter_medoids_masked", "pann_filter_medoids_masked_dev")
SEARCHES = ("pann_batch_search_grouped_labeled", "pann_batch_search_grouped_labeled_dev")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("name", MEDOIDS)
def test_medoid_entry_points_refuse_a_null_handle(name):
    assert name in _capi.SIGNATURES
    lib = _capi.load()
    ids, dists, counts = np.full(4, 7, np.uint32), np.full(4, 7, np.float32), np.full(1, 7, np.uint32)
    table = np.zeros((1, 2), np.uint32)
    head = (_capi.PANN_PRED_RANGE, _p(table), 1) if "labeled" in name else (None, 1, 0)
    tail = (None,) if name.endswith("_dev") else ()
    rc = getattr(lib, name)(None, *head, 4, 0, 0, _p(ids), _p(dists), _p(counts), None, *tail)
    assert rc == _capi.PANN_ERR_BAD_ARG and name in lib.pann_last_error().decode()
    assert (ids == 7).all() and (dists == 7).all() and (counts == 7).all()


@pytest.mark.parametrize("name", SEARCHES)
def test_grouped_search_entry_points_refuse_a_null_handle(name):
    assert name in _capi.SIGNATURES
    lib = _capi.load()
    ids = np.full((2, 10), 7, np.uint32)
    out = _capi.SearchOut(ids=_p(ids), out_k=10)
    qp = _capi.QueryParams(k=10, beam=64, cut=1.35, limit=100, degree_limit=32, rerank_factor=100, pad=1.0)
    q, starts, table, group = np.zeros((2, 8), np.uint8), np.zeros(1, np.uint32), np.zeros((1, 2), np.uint32), np.zeros(2, np.uint32)
    tail = (None,) if name.endswith("_dev") else ()
    rc = getattr(lib, name)(None, _p(q), None, 2, 8, _p(starts), 1, 1, C.byref(qp), _capi.PANN_PRED_RANGE, _p(table), 1, _p(group),
                            C.byref(out), None, None, 0, 0, None, *tail)
    assert rc == _capi.PANN_ERR_BAD_ARG and name in lib.pann_last_error().decode()
    assert (ids == 7).all()


def test_the_status_bit_is_bound():
    assert _capi.PANN_STATUS_BAD_GROUP == 8
    assert _capi.PANN_STATUS_BAD_GROUP not in (_capi.PANN_STATUS_VISITED_OVERFLOW, _capi.PANN_STATUS_DROPPED_OVERFLOW,
                                               _capi.PANN_STATUS_SHORT_FRONTIER)


def test_no_gpu_no_handle_for_them():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from parlayann_amd import DeviceIndex, PannError
    with pytest.raises(PannError) as e:
        DeviceIndex(np.zeros((16, 8), np.uint8), max_degree=4)
    assert e.value.code == 3                           # PANN_ERR_NO_DEVICE
