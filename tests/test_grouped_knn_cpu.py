"""CPU-only checks of the exact kNN by predicate group (DESIGN.md "Exact kNN by predicate group"):

* the library exports the four new entry points, parlayann_amd._capi declares them, include/pann.h too, the ABI version is 3;
* each refuses a NULL handle with PANN_ERR_BAD_ARG before it touches a device;
* the table of tests/grouped_knn_cases.py reaches the regimes tests/test_grouped_knn_gpu.py relies on -- group sizes 65, 64 and
  1, an entry nobody names in the middle, a repeated filter, an interleaved index array, allowed counts 0, k - 1, k, n // 2, n
  and the last five ids, dead bits set, ties on distance leading a list -- asserted from the oracle alone, so that no device
  test passes vacuously.
"""
import ctypes as C
import os

import numpy as np
import pytest

import grouped_knn_cases as gc
import masked_knn_cases as kc
from parlayann_amd import _capi, allow_count

NEW = ("pann_bruteforce_knn_labeled_grouped", "pann_bruteforce_knn_labeled_grouped_dev", "pann_bruteforce_knn_masked_grouped",
       "pann_bruteforce_knn_masked_grouped_dev")


def test_new_symbols_are_exported_and_declared():
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    assert _capi.load().pann_abi_version() == _capi.PANN_ABI_VERSION == 3
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pann.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name


def test_a_null_handle_is_refused_before_any_device_work():
    lib = _capi.load()
    buf = (C.c_uint32 * 64)()
    p = C.cast(buf, C.c_void_p)
    BAD = _capi.PANN_ERR_BAD_ARG
    assert lib.pann_bruteforce_knn_labeled_grouped(None, p, 1, 16, 1, _capi.PANN_PRED_RANGE, p, 1, p, 0, p, p, p) == BAD
    assert lib.pann_bruteforce_knn_labeled_grouped_dev(None, p, 1, 16, 1, _capi.PANN_PRED_RANGE, p, 1, p, 0, p, p, p, None) == BAD
    assert lib.pann_bruteforce_knn_masked_grouped(None, p, 1, 16, 1, p, 1, 1, p, 0, p, p, p) == BAD
    assert lib.pann_bruteforce_knn_masked_grouped_dev(None, p, 1, 16, 1, p, 1, 1, p, 0, p, p, p, None) == BAD
    assert b"null index handle" in lib.pann_last_error()


def test_the_index_array_reaches_its_regimes():
    g = gc.group_of_query()
    assert g.shape == (gc.NQ,) and g.dtype == np.uint32 and g.max() < len(gc.ENTRIES)
    sizes = np.bincount(g, minlength=len(gc.ENTRIES)).tolist()
    assert sizes == [gc.GROUP_SIZES[e] for e in gc.ENTRIES]
    assert 65 in sizes and 64 in sizes and 1 in sizes                            # a second A tile of one row, a full tile, one row
    unused = gc.ENTRIES.index("unused")
    assert sizes[unused] == 0 and 0 < unused < len(gc.ENTRIES) - 1 and sizes[unused - 1] and sizes[unused + 1]
    assert (np.diff(g.astype(np.int64)) < 0).sum() > 30                          # interleaved, not sorted
    assert [gc.ENTRIES[i] for i in g[:4]] == ["all", "all", "half", "half"]      # the queries that equal copied rows


@pytest.mark.parametrize("k", gc.KS)
def test_the_table_reaches_its_regimes(k):
    n = gc.N
    assert n % 32 == 11 and (n + 31) // 32 > 2 * 256 and (n + 4095) // 4096 == 5
    lab = gc.labels()
    A = gc.allow_rows(lab, k)
    want = gc.wanted_counts(k)
    assert A.sum(axis=1).tolist() == [want[e] for e in gc.ENTRIES]
    assert set(want.values()) >= {0, k - 1, k, n // 2, n, 5}
    assert np.flatnonzero(A[gc.ENTRIES.index("tail")]).tolist() == list(range(n - 5, n))
    h, h2 = gc.ENTRIES.index("half"), gc.ENTRIES.index("half_again")
    assert np.array_equal(A[h], A[h2]) and np.array_equal(gc.table(k)[h], gc.table(k)[h2])      # two entries, one filter
    dups = kc.dup_groups(n).ravel()
    assert A[h][dups[dups < n - 5]].all()                                         # the copied rows meet under `half`
    rows = gc.bitmap_rows(lab, k)
    assert rows.shape == (len(gc.ENTRIES), (n + 31) // 32)
    assert (rows[:, -1] >> np.uint32(n & 31) == (1 << (32 - (n & 31))) - 1).all()                # dead bits set ...
    assert allow_count(rows, n).tolist() == A.sum(axis=1).tolist()                               # ... and they do not count
    # the chunking test's budget: chunks end between groups, and the two large groups exceed it alone
    assert want["half"] > gc.CHUNK_IDS and want["all"] > gc.CHUNK_IDS
    small = [want[e] for e in gc.ENTRIES if gc.GROUP_SIZES[e] and want[e] <= gc.CHUNK_IDS]
    assert len(small) >= 4 and sum(small) <= gc.CHUNK_IDS


def test_reference_rows_follow_the_index_array(oracle):
    """rows of one group share their filter's counts; the queries that equal copied rows have the copies tied at the head"""
    tname, metric, d, k = "u8", "l2", 200, 10
    ids, dists, counts = gc.reference(oracle, tname, metric, d, k)
    assert gc.reference(oracle, tname, metric, d, k)[0] is ids                   # computed once
    g = gc.group_of_query()
    want = gc.wanted_counts(k)
    for e, name in enumerate(gc.ENTRIES):
        sel = g == e
        assert (counts[sel] == min(k, want[name])).all()
        assert (ids[sel][:, min(k, want[name]):] == kc.PAD_ID).all() and np.isinf(dists[sel][:, min(k, want[name]):]).all()
    assert (np.sort(ids[g == gc.ENTRIES.index("tail")][:, :5], axis=1) == np.arange(gc.N - 5, gc.N)).all()
    groups = kc.dup_groups(gc.N)
    tied = 0
    for q in range(4):                                                          # query q equals the rows of copied group q
        grp = sorted(groups[q].tolist())
        allowed = [i for i in grp if gc.allow_rows(gc.labels(), k)[g[q]][i]]
        head = ids[q, :len(allowed)].tolist()
        if len(allowed) >= 2:
            assert head == allowed and len({dists[q, j].tobytes() for j in range(len(allowed))}) == 1
            tied += 1
    assert tied >= 2, "no copied group led a list"
