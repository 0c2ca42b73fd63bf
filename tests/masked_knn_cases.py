"""Cases shared by the tests of the exact masked kNN (DESIGN.md "Exact masked kNN"): tests/test_masked_knn_cpu.py asserts from the
oracle alone that every case meets the regime it is there for, tests/test_masked_knn_gpu.py runs the same cases on the device
and compares ids, distances and counts with the oracle bit for bit.  Plain Python: nothing here needs a GPU.

The reference is oracle.bruteforce_knn over the ALLOWED rows in ascending id order, local ids mapped back through that array and
rows padded to k with 0xFFFFFFFF / +inf: order under (dist, local id) is order under (dist, global id).

Shapes are the smallest at which each piece can go wrong:
    shared route     n = 20 011: 626 bitmap words, so three compaction blocks of 256 words, the last one partial, and a last
                     word with 11 live bits; every shared bitmap has its 21 dead bits SET.  nq = 65: one query past a tile of 64.
    per-query route  n = 5 003: 157 words, so three steps of 64 words (2 048 positions), the last one partial; nq = 65 rows that
                     all differ.
    data             integer-valued (tests/test_dense_gpu.py::_mk), with DUP rows copied so that equal distances are decided by
                     the id, and the first queries equal to copied rows so that the ties lead their lists.
"""
import numpy as np

from parlayann_amd import bfloat16, datasets
from parlayann_amd.index import pack_allow

PAD_ID = 0xFFFFFFFF
N_SHARED, N_ROWS, NQ = 20011, 5003, 65
KS_SHARED, KS_ROWS = (1, 10, 100, 128), (1, 10, 64)
CHUNK = 2048                                         # positions one step of the per-query scan covers

_NAMES = {"u8": np.uint8, "i8": np.int8, "f32": np.float32, "f16": np.float16, "bf16": bfloat16}
# (type, metric, d): every element type the brute force accepts on both metrics at d = 100 and 128 (rows of one chunk per lane
# and padded rows), f32 and u8 also at d = 200 (rows wider than 256 bytes)
GRID = [(t, m, d) for t in _NAMES for m in ("l2", "mips") for d in (100, 128)] + \
       [(t, m, 200) for t in ("f32", "u8") for m in ("l2", "mips")]
GRID_IDS = [f"{t}-{m}-d{d}" for t, m, d in GRID]


def _mk(n, d, dtype, seed):
    X = datasets.sift_like(n, d, seed=seed, dtype=np.float32)
    if dtype == np.int8:
        return (X - 128).clip(-127, 127).astype(np.int8)
    return datasets.sift_like(n, d, seed=seed, dtype=bfloat16) if dtype == bfloat16 else X.astype(dtype)


def dup_groups(n):
    """four groups of four ids whose rows are equal: one in the first step, one across steps, one in the last words"""
    return np.array([[7, 8, 1500, n - 2], [4100, 2048, 63, n - 1], [31, 32, 33, 64], [n // 2, n // 2 + 1, 2047, 4096]])


def data(tname, d, n):
    """(X, Q): n base rows with the rows of every dup group equal, NQ queries of which query g equals the rows of group g"""
    dtype = _NAMES[tname]
    X, Q = _mk(n, d, dtype, 1234 + d), _mk(NQ, d, dtype, 4321 + d)
    for g, ids in enumerate(dup_groups(n)):
        X[ids[1:]] = X[ids[0]]
        Q[g] = X[ids[0]]
    return np.ascontiguousarray(X), np.ascontiguousarray(Q)


def shared_masks(n, k):
    """name -> boolean (n,).  Every random mask allows the dup groups, so that tied distances meet in a result."""
    rng = np.random.default_rng(99)
    dups = dup_groups(n).ravel()
    order = rng.permutation(n)
    m = {}
    for name, p in (("1pct", 0.01), ("50pct", 0.5)):
        a = rng.random(n) < p
        a[dups] = True
        m[name] = a
    for name, c in (("exactly_k", k), ("k_minus_1", k - 1), ("one", 1), ("none", 0)):
        a = np.zeros(n, bool)
        a[order[:c]] = True
        m[name] = a
    m["all"] = np.ones(n, bool)
    m["tail"] = np.arange(n) >= n - 5
    return m


def pack_shared(allow, n):
    """the packed bitmap with its dead bits (positions >= n in the last word) set"""
    w = pack_allow(allow, n).copy()
    if n & 31:
        w[-1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
    return w


def row_masks(n):
    """boolean (NQ, n): every row another mask.  -> (A, name -> row): four rows for the dup groups, the named rows, then
    random densities from 0.05 % to 95 %."""
    rng = np.random.default_rng(7)
    dups = dup_groups(n)
    A = np.zeros((NQ, n), bool)
    for g in range(len(dups)):                       # rows 0..3 answer the queries that equal a dup group: ties lead the list
        A[g] = rng.random(n) < (0.02, 0.3, 0.004, 0.6)[g]
        A[g, dups[g]] = True
    r = len(dups)

    def pick(lo, hi, c):
        a = np.zeros(n, bool)
        a[lo + rng.choice(hi - lo, c, replace=False)] = True
        return a
    named = {
        "none": np.zeros(n, bool), "all": np.ones(n, bool), "first_id": np.arange(n) == 0, "last_id": np.arange(n) == n - 1,
        "one_step": (np.arange(n) // CHUNK == 1) & (rng.random(n) < 0.3),          # every allowed id in the second step
        "last_step_only": (np.arange(n) >= 2 * CHUNK) & (rng.random(n) < 0.2),     # the first allowed id is in the last step
        "last_word": np.arange(n) >= n - (n & 31),
        "count_9": pick(0, n, 9), "count_10": pick(0, n, 10), "count_63": pick(0, n, 63), "count_64": pick(0, n, 64),
        "count_65": pick(0, n, 65),
        "tiles_64_64": pick(0, CHUNK, 64) | pick(CHUNK, 2 * CHUNK, 64),             # whole tiles: nothing is carried over
        "carry_63_1": pick(0, CHUNK, 63) | pick(2 * CHUNK, n, 1),                   # 63 ids wait two steps for the 64th
        "carry_100_100": pick(0, CHUNK, 100) | pick(2 * CHUNK, n, 100),
    }
    names = {}
    for name, a in named.items():
        A[r] = a
        names[name] = r
        r += 1
    dens = np.geomspace(0.0005, 0.95, NQ - r)
    for i, p in enumerate(dens):
        A[r + i] = rng.random(n) < p
    return A, names


def reference(oracle, X, Q, allow, k, metric):
    """(ids, dists, counts) of the rule for a shared boolean mask (n,) or per-query rows (nq, n)"""
    nq = len(Q)
    ids = np.full((nq, k), PAD_ID, np.uint32)
    dists = np.full((nq, k), np.inf, np.float32)
    counts = np.zeros(nq, np.uint32)
    if allow.ndim == 1:
        live = np.flatnonzero(allow).astype(np.uint32)
        c = min(k, len(live))
        if c:
            li, ld = oracle.bruteforce_knn(np.ascontiguousarray(X[live]), Q, c, metric=metric)
            ids[:, :c], dists[:, :c] = live[li], ld
        counts[:] = c
        return ids, dists, counts
    for q in range(nq):
        live = np.flatnonzero(allow[q]).astype(np.uint32)
        c = min(k, len(live))
        if c:
            li, ld = oracle.bruteforce_knn(np.ascontiguousarray(X[live]), Q[q:q + 1], c, metric=metric)
            ids[q, :c], dists[q, :c] = live[li[0]], ld[0]
        counts[q] = c
    return ids, dists, counts


def head(ref, k):
    """the reference at a smaller k: the first k columns of a reference computed at kmax >= k"""
    ids, dists, counts = ref
    return ids[:, :k], dists[:, :k], np.minimum(counts, k).astype(np.uint32)
