"""CPU-only: the ctypes side of pann_batch_search_rerank* (include/pann.h): the struct layout, the two signatures and the
status bit.  The calls themselves need two device handles, so they are exercised in tests/test_search_rerank_gpu.py."""
import ctypes as C


def test_rerank_out_has_the_seven_pointers_of_the_header_in_order():
    from parlayann_amd import _capi
    names = [f[0] for f in _capi.RerankOut._fields_]
    assert names == ["ids", "dists", "frontier_size", "visited_count", "dist_cmps", "pruned_cmps", "status"]
    assert all(f[1] is C.c_void_p for f in _capi.RerankOut._fields_)
    assert C.sizeof(_capi.RerankOut) == 56
    assert [getattr(_capi.RerankOut, n).offset for n in names] == list(range(0, 56, 8))


def test_signatures_load_and_the_status_bit_is_exported():
    import parlayann_amd
    from parlayann_amd import _capi
    lib = _capi.load()
    host, dev = lib.pann_batch_search_rerank, lib.pann_batch_search_rerank_dev
    assert host.restype is C.c_int and dev.restype is C.c_int
    assert len(host.argtypes) == 12 and len(dev.argtypes) == 13          # the _dev form adds the stream
    assert list(dev.argtypes[:12]) == list(host.argtypes)
    assert host.argtypes[2] == C.POINTER(_capi.QuantParams) and host.argtypes[10] == C.POINTER(_capi.QueryParams)
    assert host.argtypes[11] == C.POINTER(_capi.RerankOut)
    assert parlayann_amd.PANN_STATUS_SHORT_FRONTIER == 4 == _capi.PANN_STATUS_SHORT_FRONTIER
    # no handle, no search: refused loudly before any device is touched
    qp = _capi.QueryParams(k=10, beam=64, cut=1.35, limit=100, degree_limit=32, rerank_factor=100, pad=1.0)
    out = _capi.RerankOut()
    assert host(None, None, None, None, 0, 0, 0, 0, None, 0, C.byref(qp), C.byref(out)) == 1
    assert lib.pann_last_error()
