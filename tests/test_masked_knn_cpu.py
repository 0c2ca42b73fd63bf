"""CPU-only checks of the exact masked kNN's interface and of its test tables (DESIGN.md "Exact masked kNN"):

* the library exports the three new entry points, parlayann_amd._capi declares them, and the ABI version is still 3;
* allow_count counts as a bit loop does, dead bits (positions >= n, words past ceil(n / 32)) left out;
* the tables of tests/masked_knn_cases.py reach the regimes tests/test_masked_knn_gpu.py relies on -- short row, empty row,
  exact-k row, a first allowed id in the last step, whole tiles and carried ids, ties on distance among the first k --
  asserted from the oracle alone, so that no device test passes vacuously.
"""
import ctypes as C
import os

import numpy as np
import pytest

import masked_knn_cases as kc
from parlayann_amd import _capi, allow_count
from parlayann_amd.index import pack_allow

NEW = ("pann_allow_count_dev", "pann_bruteforce_knn_masked", "pann_bruteforce_knn_masked_dev")


def test_new_symbols_are_exported_and_declared():
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    assert _capi.load().pann_abi_version() == _capi.PANN_ABI_VERSION == 3
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pann.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name


def _bit_loop(words, n):
    return sum(1 for i in range(n) if (int(words[i >> 5]) >> (i & 31)) & 1)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 70, 1000])
def test_allow_count_is_the_bit_loop(n):
    rng = np.random.default_rng(n)
    w = (n + 31) // 32
    rows = rng.integers(0, 2 ** 32, size=(5, w + 2), dtype=np.uint64).astype(np.uint32)      # dead bits and two dead words set
    rows[0] = 0
    rows[1] = 0xFFFFFFFF
    got = allow_count(rows, n)
    assert got.tolist() == [_bit_loop(r, n) for r in rows]
    assert got[0] == 0 and got[1] == n
    assert allow_count(rows[2], n) == got[2] and isinstance(allow_count(rows[2], n), int)
    b = rng.random((3, n)) < 0.5
    assert allow_count(b, n).tolist() == b.sum(axis=1).tolist() and allow_count(b[0], n) == int(b[0].sum())
    assert allow_count(pack_allow(b, n), n).tolist() == b.sum(axis=1).tolist()


def test_shared_tables_reach_their_regimes():
    n = kc.N_SHARED
    assert n % 32 and (n + 31) // 32 > 2 * 256                                   # a partial last word, three compaction blocks
    for k in kc.KS_SHARED:
        m = kc.shared_masks(n, k)
        c = {name: int(a.sum()) for name, a in m.items()}
        assert c["exactly_k"] == k and c["k_minus_1"] == k - 1 and c["one"] == 1 and c["none"] == 0 and c["all"] == n
        assert np.flatnonzero(m["tail"]).tolist() == list(range(n - 5, n))
        assert 100 < c["1pct"] < 400 and 9000 < c["50pct"] < 11000
        for a in m.values():                                                     # the dead bits are set, and do not count
            w = kc.pack_shared(a, n)
            assert int(w[-1]) >> (n & 31) == (1 << (32 - (n & 31))) - 1
            assert allow_count(w, n) == int(a.sum())


def test_row_table_reaches_its_regimes():
    n = kc.N_ROWS
    A, names = kc.row_masks(n)
    assert (n + 31) // 32 == 157 and A.shape == (kc.NQ, n)
    assert len({a.tobytes() for a in A}) == kc.NQ                                # every row is another mask
    cnt = A.sum(axis=1)
    assert cnt.min() == 0 and cnt.max() == n
    for k in kc.KS_ROWS:                                                         # an exact-k row and a short row for every k
        assert (cnt == k).any() and (cnt == k - 1).any()
    first = lambda r: int(np.flatnonzero(A[r])[0])
    step = lambda r: set((np.flatnonzero(A[r]) // kc.CHUNK).tolist())
    assert step(names["one_step"]) == {1} and cnt[names["one_step"]] > 64
    assert first(names["last_step_only"]) >= 2 * kc.CHUNK
    assert step(names["last_word"]) == {2} and cnt[names["last_word"]] == n & 31
    per_step = lambda r: np.bincount(np.flatnonzero(A[r]) // kc.CHUNK, minlength=3).tolist()
    assert per_step(names["tiles_64_64"]) == [64, 64, 0]
    assert per_step(names["carry_63_1"]) == [63, 0, 1] and per_step(names["carry_100_100"]) == [100, 0, 100]
    assert (cnt > 64).sum() > 20 and ((cnt > 0) & (cnt < 64)).sum() > 10


@pytest.mark.parametrize("tname,metric,d", kc.GRID, ids=kc.GRID_IDS)
def test_ties_on_distance_lead_the_lists(oracle, tname, metric, d):
    """the queries that equal a dup group get that group's rows at one distance among their first k: the id decides"""
    for n, allow in ((kc.N_SHARED, kc.shared_masks(kc.N_SHARED, 10)["1pct"]), (kc.N_ROWS, kc.row_masks(kc.N_ROWS)[0])):
        X, Q = kc.data(tname, d, n)
        groups = kc.dup_groups(n)
        ids, dists, _ = kc.reference(oracle, X, Q[:len(groups)], allow if allow.ndim == 1 else allow[:len(groups)], 10, metric)
        tied = 0
        for g, grp in enumerate(groups):
            pos = [int(np.flatnonzero(ids[g] == i)[0]) for i in grp if (ids[g] == i).any()]
            if len(pos) == len(grp):
                assert len({dists[g, p].tobytes() for p in pos}) == 1            # one distance ...
                assert [int(ids[g, p]) for p in sorted(pos)] == sorted(grp.tolist())   # ... in id order
                tied += 1
        assert tied >= 1, "no dup group made it into a list"
