"""Inputs of the HCNNG leaf tests: builds whose trees end in leaves the other suites never produce.

    leaves above 4096 members    leaf_mst_kernel keeps its union-find state in HBM scratch and reads ids and degrees live;
                                 the leaf kNN kernels stream a leaf of thousands of members
    leaves on both sides of it   one launch, LDS-mode and HBM-mode blocks side by side
    halved clusters              bit-identical pivots (duplicated rows), an empty first or second side (MIPS on a ray: every
                                 split is halved, so the leaves depend on positions alone; MIPS in a narrow cone: a builder
                                 without the empty-first-side guard ends in other leaves)
    leaves of identical points   every distance equal: the result rests on the tie rules alone
    leaves of 1 .. 11 members    the N < 2 return, kNN rows with empty slots, KEY_INF padding inside a key segment
    no split level at all        n <= cluster_size

One table, built once per process: case(name) gives the rows, trees(name) the restated trees (tests/hcnng_ref.py),
oracle_graph(name) the oracle's build.  CONDITIONS holds what every case is there for as a predicate over its restated trees;
tests/test_hcnng_cases_cpu.py asserts them on the CPU, so that no device test (tests/test_hcnng_leaves_gpu.py) passes vacuously.
All rows are integer valued: every comparison with the device is bit for bit.  Plain Python: nothing here needs a GPU.

Out of scope: a leaf at the 16-bit local-index limit (cluster_size = 65535 with 65535 members).  The oracle's all-pairs leaf
kNN needs about 20 s for it on a workstation CPU, far beyond what a test of this suite may take.
"""
import numpy as np

import hcnng_ref
import oracle_api
from parlayann_amd import datasets

LDS_CAP = 4096                 # leaf_mst_kernel: leaves above this many members run in HBM mode (hcnng_build.hip)
D = 16

# name -> (rows, metric, T, cluster_size, mst_deg, seed)
CASES = {
    "straddle": ("sift10k_u8", "l2", 3, 6000, 3, 5),            # leaves 5759/3446/795, 2405/5064/120/2411, 4440/4339/1221
    "straddle_f16": ("sift10k_f16", "l2", 3, 6000, 3, 5),
    # seeds scanned upward from 1 with hcnng_ref.tree; 19 is the first whose every tree has a leaf above the cap and one in
    # [2, 4096] (MIPS often splits 10000 rows into two leaves above it): leaves 2109/5534/2357, 3761/4929/1310, 3648/984/5368
    "straddle_mips": ("sift10k_i8", "mips", 3, 6000, 3, 19),
    "one_big_leaf": ("sift5k_u8", "l2", 2, 5000, 3, 5),
    "dup5": ("dup5", "l2", 3, 50, 3, 3),
    "all_same": ("all_same", "l2", 2, 64, 2, 3),
    "ray_mips": ("ray_i8", "mips", 3, 100, 3, 3),
    "cone_mips": ("cone_i8", "mips", 3, 100, 3, 3),
    "tiny2": ("sift777", "l2", 3, 2, 1, 3),
    "tiny11": ("sift777", "l2", 3, 11, 12, 3),                  # mst_deg 12: no member of an 11-member leaf reaches it
    "one_leaf": ("sift300", "l2", 2, 300, 3, 3),
    "n1": ("sift1", "l2", 2, 2, 3, 3),
    "n2": ("sift2", "l2", 2, 2, 3, 3),
    "n3": ("sift3", "l2", 2, 2, 3, 3),
}
NAMES = tuple(CASES)
STRADDLES = ("straddle", "straddle_f16", "straddle_mips")

_rows, _trees, _oracle = {}, {}, {}


def _make_rows(kind):
    if kind == "sift10k_u8":
        return datasets.sift_like(10000, D, seed=1234)
    if kind == "sift10k_f16":
        return rows("sift10k_u8").astype(np.float16)
    if kind == "sift10k_i8":
        return (rows("sift10k_u8").astype(np.int16) - 128).astype(np.int8)
    if kind == "sift5k_u8":
        return np.ascontiguousarray(rows("sift10k_u8")[:5000])
    if kind == "dup5":                                            # 5 vectors, every row one of them
        rng = np.random.default_rng(0)
        V = rng.integers(0, 256, (5, D), dtype=np.uint8)
        return np.ascontiguousarray(V[rng.integers(0, 5, 3000)])
    if kind == "all_same":
        return np.tile(np.arange(7, 7 + D, dtype=np.uint8), (1000, 1))
    if kind == "ray_i8":                                          # points on one ray: under MIPS every split is one-sided
        X = np.zeros((3000, 8), np.int8)
        X[:, 0] = np.random.default_rng(0).integers(1, 128, 3000)
        return X
    if kind == "cone_i8":       # a narrow cone of positive rows: a much longer pivot takes every member, two alike split them
        rng = np.random.default_rng(1)
        c = rng.integers(1, 13, 3000)
        return (c[:, None] * np.array([9, 7, 5, 3, 2, 1, 1, 1]) + rng.integers(0, 4, (3000, 8))).astype(np.int8)
    if kind == "sift777":
        return datasets.sift_like(777, D, seed=1)
    if kind == "sift300":
        return datasets.sift_like(300, D, seed=1)
    if kind in ("sift1", "sift2", "sift3"):
        return np.ascontiguousarray(rows("sift300")[:int(kind[4:])])
    raise KeyError(kind)


def rows(kind):
    """the rows of a data set of the table, made once and never changed"""
    if kind not in _rows:
        _rows[kind] = _make_rows(kind)
        _rows[kind].setflags(write=False)
    return _rows[kind]


def case(name):
    """(X, metric, T, cluster_size, mst_deg, seed) of a CASES entry"""
    kind, metric, T, cs, mst_deg, seed = CASES[name]
    return rows(kind), metric, T, cs, mst_deg, seed


def trees(name):
    """[(leaves, why)] for trees 0 .. T - 1: hcnng_ref.tree, made once"""
    if name not in _trees:
        X, metric, T, cs, _, seed = case(name)
        _trees[name] = [hcnng_ref.tree(X, cs, seed, t, metric) for t in range(T)]
    return _trees[name]


def leaf_sizes(name):
    return [[len(l) for l in leaves] for leaves, _ in trees(name)]


def oracle_graph(name, oracle=None):
    """oracle.hcnng_build of a case (max_deg = T * mst_deg), made once"""
    if name not in _oracle:
        X, metric, T, cs, mst_deg, seed = case(name)
        o = oracle if oracle is not None else oracle_api.load()
        _oracle[name] = o.hcnng_build(X, T, cs, mst_deg, seed=seed, metric=metric)
        _oracle[name].setflags(write=False)
    return _oracle[name]


def norm(G):
    """slots past a row's degree zeroed (their content is unspecified)"""
    G = G.copy()
    cols = np.arange(G.shape[1] - 1)[None, :]
    G[:, 1:][cols >= G[:, :1]] = 0
    return G


# ---- what every case is there for, as a predicate over its restated trees ----

def _straddles(name):
    return all(max(s) > LDS_CAP and any(2 <= x <= LDS_CAP for x in s) for s in leaf_sizes(name))


def _same_leaves_as_straddle(name):
    mine, theirs = trees(name), trees("straddle")
    return _straddles(name) and len(mine) == len(theirs) and all(
        len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)) for (a, _), (b, _) in zip(mine, theirs))


def _sizes_occur(name, *ranges):
    sizes = [x for s in leaf_sizes(name) for x in s]
    return all(any(lo <= x <= hi for x in sizes) for lo, hi in ranges)


def _unguarded_differs(name):
    """every tree has both kinds of empty side, and without the empty-first-side guard its leaves come out different"""
    X, metric, T, cs, _, seed = case(name)
    for t, (leaves, why) in enumerate(trees(name)):
        other = hcnng_ref.tree(X, cs, seed, t, metric, first_empty_guard=False)[0]
        if len(other) == len(leaves) and all(np.array_equal(a, b) for a, b in zip(leaves, other)):
            return False
        if why["first_empty"] < 1 or why["second_empty"] < 1:
            return False
    return True


def _all_same(name):
    X = case(name)[0]
    return bool((X == X[0]).all()) and all(w["splits"] >= 1 and w["same"] == w["splits"] for _, w in trees(name))


CONDITIONS = {
    "straddle": _straddles,
    "straddle_f16": _same_leaves_as_straddle,
    "straddle_mips": _straddles,
    "one_big_leaf": lambda name: leaf_sizes(name) == [[5000], [5000]] and all(w["splits"] == 0 for _, w in trees(name)),
    "dup5": lambda name: all(w["same"] >= 1 for _, w in trees(name)),
    "all_same": _all_same,
    "ray_mips": lambda name: all(w["first_empty"] >= 1 and w["second_empty"] >= 1 for _, w in trees(name)),
    "cone_mips": _unguarded_differs,
    "tiny2": lambda name: _sizes_occur(name, (1, 1), (2, 2)),
    "tiny11": lambda name: _sizes_occur(name, (1, 1), (2, 10), (11, 11)),
    "one_leaf": lambda name: leaf_sizes(name) == [[300], [300]] and all(w["splits"] == 0 for _, w in trees(name)),
    "n1": None, "n2": None, "n3": None,
}
