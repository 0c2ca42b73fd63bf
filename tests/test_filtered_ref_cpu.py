"""CPU-only checks of the two-level search's test infrastructure and host-only surface:

* tests/filtered_ref.py with use_filtering=False equals the C++ oracle field for field (the checker is pinned before the
  device is compared against it);
* pann_sketch_select_ranks equals the reference's float / double index expressions evaluated with numpy scalars;
* the new C-ABI symbols exist in libpann.so and in the ctypes table, and the ABI version is still 3;
* every case of tests/test_filtered_search_gpu.py is non-vacuous: the sketch drops at least one neighbour in at least half of
  the queries, and in at least one query the final ids differ from the unfiltered search.
"""
import ctypes as C

import numpy as np
import pytest

import filtered_cases as fc
from filtered_cases import random_rows as _data
import filtered_ref
import oracle_api
from parlayann_amd import sketch as sk

FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum")


PIN_CASES = [
    # dtype, metric, beam, k, extra
    (np.uint8, "l2", 4, 0, {}),
    (np.uint8, "l2", 16, 10, {"cut": 1.35}),
    (np.uint8, "mips", 64, 10, {"cut": 1.35, "limit": 30}),
    (np.uint8, "l2", 100, 10, {"cut": 1.35, "degree_limit": 9}),
    (np.float32, "l2", 16, 10, {"cut": 1.35, "starts": (0, 5, 901)}),
    (np.float32, "mips", 4, 0, {"query_ids": True}),
    (np.float32, "l2", 64, 10, {"cut": 1.35, "query_ids": True}),
    (np.float32, "mips", 100, 0, {"limit": 50, "degree_limit": 9}),
    (np.uint8, "l2", 64, 0, {"query_ids": True, "starts": (3, 4)}),
    (np.float32, "l2", 100, 10, {"cut": 1.35}),
]


@pytest.mark.parametrize("dtype,metric,beam,k,extra", PIN_CASES, ids=[f"{np.dtype(c[0]).name}-{c[1]}-b{c[2]}-k{c[3]}-{i}"
                                                                      for i, c in enumerate(PIN_CASES)])
def test_checker_without_filtering_equals_the_oracle(dtype, metric, beam, k, extra):
    o = oracle_api.load()
    n, d, nq = 1200, 24, 10
    X = _data(dtype, n, d, 11 + beam)
    Q = _data(dtype, nq, d, 12 + beam)
    G = fc.random_graph(n, 16, 13 + beam)
    extra = dict(extra)
    kw = dict(k=k, beam=beam, metric=metric, out_k=beam, visited_cap=n)
    if extra.pop("query_ids", False):
        kw["query_ids"] = np.arange(3, 3 + 7 * nq, 7, dtype=np.uint32)
    else:
        kw["queries"] = Q
    kw.update(extra)
    r = o.batch_search(X, G, **kw)
    assert r["rc"] == 0
    g = filtered_ref.filtered_batch_search(X, G, use_filtering=False, **kw)
    for f in FIELDS:
        assert np.array_equal(g[f], r[f]), f
    assert np.array_equal(g["pruned_cmps"], r["dist_cmps"])          # without filtering both counters are the same
    assert not g["sketch_dropped"].any()
    for i in range(nq):
        v = int(r["visited_count"][i])
        assert np.array_equal(g["visited_ids"][i, :v], r["visit_order_ids"][i, :v])
        assert np.array_equal(g["visited_sorted_ids"][i, :v], r["visited_ids"][i, :v])
        srt = np.lexsort((g["visited_ids"][i, :v], g["visited_dists"][i, :v]))
        assert np.array_equal(g["visited_dists"][i, :v][srt], r["visited_dists"][i, :v])


@pytest.mark.parametrize("length", [1, 2, 3, 9999, 10000, 10001, 2 ** 24 + 1, 3 * 10 ** 9])
def test_sketch_select_ranks_follow_the_reference_expressions(length):
    F = np.float32
    for kind in ("euclid_bit", "mips_bit", "mips_2bit"):
        a, b = sk.select_ranks(length, kind)
        if kind == "euclid_bit":
            ea = eb = length // 2
        elif kind == "mips_bit":
            ea = eb = 0
        else:
            ea = int(F(0.3) * F(length))                                       # (long)(cutoff * len): float
            eb = int((np.float64(1.0) - np.float64(F(0.3))) * np.float64(length - 1))   # (long)((1.0 - cutoff) * (len - 1)): double
        ea, eb = min(ea, length - 1), min(eb, length - 1)
        assert (a, b) == (ea, eb), (kind, length)
        assert (a, b) == sk.select_ranks_numpy(length, kind)


NEW_SYMBOLS = ["pann_sketch_params_generate", "pann_sketch_select_ranks", "pann_index_attach_sketch", "pann_index_drop_sketch", "pann_index_upload_sketch",
               "pann_index_sketch_kind", "pann_index_download_sketch", "pann_sketch_rows", "pann_sketch_rows_dev",
               "pann_batch_search_filtered", "pann_batch_search_filtered_dev"]


def test_new_symbols_exported_and_bound():
    from parlayann_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _capi.SIGNATURES, s
    assert _capi.load().pann_abi_version() == 3
    assert C.sizeof(_capi.SketchParams) == 24 and _capi.SketchParams.median.offset == 8 and _capi.SketchParams.cut.offset == 16


def test_numpy_sketch_layout():
    """bit j of 64-bit word i is dimension 64 i + j; 2-bit rows interleave sign and mask words; undefined bits are 0"""
    x = np.zeros((1, 70), np.float32)
    x[0, [0, 9, 63, 64, 69]] = 1.0
    x[0, 5] = -1.0
    p = sk.make_params("mips_bit", 70)
    w = sk.sketch_rows_numpy(x, p).view("<u8")[0]
    assert w.tolist() == [(1 << 0) | (1 << 9) | (1 << 63), (1 << 0) | (1 << 5)]
    p2 = sk.make_params("mips_2bit", 70, cut=0.5)
    w2 = sk.sketch_rows_numpy(x, p2).view("<u8")[0]
    assert w2.tolist() == [(1 << 0) | (1 << 9) | (1 << 63), (1 << 0) | (1 << 5) | (1 << 9) | (1 << 63),
                           (1 << 0) | (1 << 5), (1 << 0) | (1 << 5)]
    q = np.zeros((1, 70), np.float32)
    q[0, [0, 5, 64]] = [1.0, 1.0, -1.0]
    sq = sk.sketch_rows_numpy(q, p2)
    # common non-zero dims: 0 (equal), 5 (differ), 64 (differ) -> 2 * 2 - 3
    assert sk.sketch_distance_numpy(sk.sketch_rows_numpy(x, p2), sq[0], p2).tolist() == [1.0]
    pw = sk.make_params("mips_bit", 70, hamming_as_written=True)
    s1, s2 = sk.sketch_rows_numpy(x, p), sk.sketch_rows_numpy(q, p)
    assert sk.sketch_distance_numpy(s1, s2[0], p).tolist() == [float(3 + 2)]            # x > 0: dims {0, 9, 63, 64, 69}; q > 0: dims {0, 5}
    assert sk.sketch_distance_numpy(s1, s2[0], pw).tolist() == [2.0 * 3]                # block 0 (xor = {9, 63, 5}) counted twice


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_gpu_cases_are_not_vacuous(case):
    c = fc.build_case(case)
    filt = filtered_ref.filtered_batch_search(**fc.checker_args(c, True))
    plain = filtered_ref.filtered_batch_search(**fc.checker_args(c, False))
    dropped = filt["sketch_dropped"]
    assert (dropped > 0).sum() * 2 >= len(dropped), dropped
    assert (filt["ids"] != plain["ids"]).any(axis=1).any()
    assert (filt["dist_cmps"] <= filt["pruned_cmps"]).all() and (filt["dist_cmps"] < filt["pruned_cmps"]).any()
