"""Cases shared by the tests of the exact kNN by predicate group (DESIGN.md "Exact kNN by predicate group"):
tests/test_grouped_knn_cpu.py asserts from the oracle alone that the table reaches every regime it is there for,
tests/test_grouped_knn_gpu.py runs it on the device and compares ids, distances and counts bit for bit.  Plain Python.

The reference is masked_knn_cases.reference (the oracle's brute force over the allowed rows) once per distinct filter, its rows
placed by the index array.

Shapes are the smallest at which a piece can go wrong:
    n = 20 011       626 bitmap words: three compaction blocks of 256 words, five tiles of 4 096 labels, 11 live bits in the last
                     word; the bitmap rows have their 21 dead bits SET.
    data             masked_knn_cases.data (integer-valued, copied rows so that equal distances are decided by the id), NQ = 200
                     queries: its 65, of which the first four equal a copied group, and 135 more.
    labels           bits 8..31: a rank, so that a RANGE window allows an exact number of points; the last five ids hold the top
                     five ranks, the copied rows hold ranks inside the `half` window.
    table            G = 8 entries, sizes of their groups in GROUP_SIZES: 65 queries (a second A tile of one row), exactly 64,
                     one, an entry in the middle that no query names, two entries holding the same filter.  The allowed counts
                     are n // 2, k - 1, 0, 7, k, n, the last five ids, and n // 2 again.
    index array      interleaved (a fixed shuffle), not sorted; queries 0 and 1 (copied rows) name `all`, 2 and 3 name `half`.
"""
import numpy as np

import masked_knn_cases as kc
from parlayann_amd.index import label_allow

N, NQ = kc.N_SHARED, 200
KS = (1, 10, 128)
ENTRIES = ("half", "k_minus_1", "none", "unused", "exactly_k", "all", "tail", "half_again")
GROUP_SIZES = {"half": 65, "k_minus_1": 64, "none": 1, "unused": 0, "exactly_k": 20, "all": 20, "tail": 15, "half_again": 15}
HALF_LO, DUP_RANK = 100, 200                         # the half window is ranks [100, 100 + n // 2); the copied rows sit at 200 ..
CHUNK_IDS = 3000                                     # the max_list_ids of the chunking test

# (type, metric, d, exact float order): what the device tests run
GRID = [("f16", "l2", 128, False), ("bf16", "mips", 100, False), ("u8", "l2", 200, False), ("i8", "mips", 100, False),
        ("f32", "l2", 128, False), ("f32", "l2", 128, True)]
GRID_IDS = [f"{t}-{m}-d{d}{'-exact' if e else ''}" for t, m, d, e in GRID]


def data(tname, d):
    """(X, Q): masked_knn_cases.data with 135 more queries behind its 65"""
    X, Q = kc.data(tname, d, N)
    more = kc._mk(NQ - kc.NQ, d, kc._NAMES[tname], 977 + d)
    return X, np.ascontiguousarray(np.concatenate([Q, more]))


def labels():
    """uint32 (N,): rank << 8 | a random byte.  ids N - 5 .. N - 1 hold ranks N - 5 .. N - 1, the copied rows ranks DUP_RANK ..."""
    rng = np.random.default_rng(31)
    dups = kc.dup_groups(N).ravel()
    tail = np.arange(N - 5, N)
    fixed_ids = np.concatenate([dups[~np.isin(dups, tail)], tail])
    fixed_ranks = np.concatenate([DUP_RANK + np.arange(len(fixed_ids) - 5), tail])
    rank = np.empty(N, np.int64)
    rank[fixed_ids] = fixed_ranks
    rest_ids = np.setdiff1d(np.arange(N), fixed_ids)
    rest_ranks = np.setdiff1d(np.arange(N), fixed_ranks)
    rank[rest_ids] = rng.permutation(rest_ranks)
    assert sorted(rank.tolist()) == list(range(N))
    return ((rank.astype(np.uint32) << np.uint32(8)) | rng.integers(0, 256, N).astype(np.uint32)).astype(np.uint32)


def window(lo, count):
    """the RANGE predicate of the `count` points of ranks lo .. lo + count - 1 (count 0: a > b)"""
    if count == 0:
        return ((lo + 1) << 8, lo << 8)
    return (lo << 8, ((lo + count - 1) << 8) | 0xFF)


def table(k):
    """uint32 (G, 2): the RANGE predicates of ENTRIES for this k"""
    w = {"half": window(HALF_LO, N // 2), "k_minus_1": window(11000, k - 1), "none": window(5, 0), "unused": window(13000, 7),
         "exactly_k": window(12000, k), "all": window(0, N), "tail": window(N - 5, 5), "half_again": window(HALF_LO, N // 2)}
    return np.array([w[e] for e in ENTRIES], np.uint32)


def wanted_counts(k):
    return {"half": N // 2, "k_minus_1": k - 1, "none": 0, "unused": 7, "exactly_k": k, "all": N, "tail": 5, "half_again": N // 2}


def group_of_query():
    """uint32 (NQ,): the table index of every query, shuffled; queries 0, 1 -> `all`, 2, 3 -> `half`"""
    rng = np.random.default_rng(5)
    g = np.concatenate([np.full(c, ENTRIES.index(e), np.uint32) for e, c in GROUP_SIZES.items()])
    assert len(g) == NQ
    g = g[rng.permutation(NQ)]
    for q, e in ((0, "all"), (1, "all"), (2, "half"), (3, "half")):          # swap, so that the group sizes stay
        want = ENTRIES.index(e)
        if g[q] != want:
            other = next(int(j) for j in np.flatnonzero(g == want) if j > 3)
            g[q], g[other] = g[other], g[q]
    return g


def allow_rows(lab, k):
    """boolean (G, N): what every table entry allows"""
    return label_allow(lab, "range", table(k))


def bitmap_rows(lab, k):
    """the table as packed bitmap rows with their dead bits set"""
    return np.stack([kc.pack_shared(a, N) for a in allow_rows(lab, k)])


_REF = {}


def reference(oracle, tname, metric, d, k):
    """(ids, dists, counts) of the rule, computed once per (type, metric, d, k) and shared: read only"""
    key = (tname, metric, d, k)
    if key not in _REF:
        X, Q = data(tname, d)
        A, g = allow_rows(labels(), k), group_of_query()
        ids = np.full((NQ, k), kc.PAD_ID, np.uint32)
        dists = np.full((NQ, k), np.inf, np.float32)
        counts = np.zeros(NQ, np.uint32)
        for e in np.unique(g):
            sel = np.flatnonzero(g == e)
            ids[sel], dists[sel], counts[sel] = kc.reference(oracle, X, np.ascontiguousarray(Q[sel]), A[e], k, metric)
        for a in (ids, dists, counts):
            a.setflags(write=False)
        _REF[key] = (ids, dists, counts)
    return _REF[key]
