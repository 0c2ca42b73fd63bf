"""Cases and oracle-side drivers of the two-phase (multi-GPU) build seams: pann_vamana_search_prune_dev / pann_vamana_apply_rows_dev
and pann_hcnng_build_trees_dev / pann_hcnng_assemble_dev (include/pann.h).

A single process can play any number of ranks W: phase A of a batch is called on the W slices of the batch (the slicing rule of
distributed.vamana_build_sharded), phase B on the whole batch; rank r of a tree-parallel HCNNG build owns trees r, r + W, ...
tests/test_two_phase_cases_cpu.py asserts on the oracle alone that these drivers reproduce the oracle's single-process builds and
that every case really contains the splits, paddings and idle ranks it is there for; tests/test_two_phase_build_gpu.py runs the
same loops on the device and compares phase by phase.  Plain Python: nothing here needs a GPU.

All data is integer valued (datasets.sift_like; two-byte floats hold the same values), so every distance is exact in any
summation order and every comparison of the device with the oracle is bit for bit.
"""
import numpy as np

import wide_cases
from parlayann_amd import bfloat16, distributed

N = 3000
WAVE = 64
SENTINEL = 0xFFFFFFFF
SEED = 7

# name -> (dtype, metric, d, R, max_deg, L, passes, Ws)
VAMANA_CASES = {
    "u8_L48": (np.uint8, "l2", 32, 16, 16, 48, 2, (1, 2, 3, 7)),         # beam-64 kernel; 64-byte rows
    "f16_L100": (np.float16, "l2", 64, 32, 32, 100, 1, (1, 2, 3, 7)),    # beam-128 kernel with the filter-code table
    "f16_L128": (np.float16, "l2", 64, 32, 32, 128, 1, (3,)),            # the same with a full frontier
    "i8_L70": (np.int8, "mips", 100, 24, 24, 70, 1, (3,)),               # beam-128 kernel without codes; multi-chunk rows
    "bf16_L64": (bfloat16, "l2", 128, 32, 32, 64, 1, (3,)),              # two-byte query in registers
    "f32_L200": (np.float32, "l2", 24, 16, 16, 200, 1, (3,)),            # generic kernel, filter table in HBM
    "u8_R96": (np.uint8, "l2", 32, 96, 129, 100, 1, (3,)),               # rows wider than a wave in scatter / reverse / re-prune
}
CODE_CASES = ("f16_L100", "f16_L128")          # the builds whose searches go through the 12-bit filter codes
VAMANA_PAIRS = [(name, W) for name, c in VAMANA_CASES.items() for W in c[7]]

HCNNG_D, MST_DEG, HCNNG_SEED = 64, 3, 11
HCNNG_FORESTS = ((5, 150), (6, 60))            # (trees, cluster_size)
# name -> (dtype, metric, Ws)
HCNNG_CASES = {
    "u8": (np.uint8, "l2", (1, 2, 3, 4, 7)),   # W = 7 > T: ranks without a tree
    "f16": (np.float16, "l2", (3,)),
    "i8": (np.int8, "mips", (3,)),
}
HCNNG_TRIPLES = [(name, W, f) for name, c in HCNNG_CASES.items() for W in c[2] for f in HCNNG_FORESTS]

_points, _builds, _trees = {}, {}, {}


def alpha_of(metric):
    return 1.2 if metric == "l2" else 1.0


def points(dtype, d, n=N):
    """the rows of a case, made once and never changed"""
    key = (np.dtype(dtype).str if np.dtype(dtype) != bfloat16 else "bf16", d, n)
    if key not in _points:
        _points[key] = wide_cases.rows_of(n, d, dtype, 1234)
    return _points[key]


def vamana_case(name):
    """(X, metric, R, max_deg, L, alpha, passes, Ws) of a VAMANA_CASES entry"""
    dtype, metric, d, R, max_deg, L, passes, Ws = VAMANA_CASES[name]
    return points(dtype, d), metric, R, max_deg, L, alpha_of(metric), passes, Ws


def vamana_oracle_build(oracle, name, sort_neighbors=True):
    """(graph, stats, (per-point visited, per-point comparisons)) of the oracle's single-process build of a case, made once"""
    key = (name, sort_neighbors)
    if key not in _builds:
        X, metric, R, max_deg, L, alpha, passes, _ = vamana_case(name)
        ps = (np.zeros(len(X), np.uint32), np.zeros(len(X), np.uint32))
        G, st = oracle.vamana_build(X, R, L, alpha, num_passes=passes, seed=SEED, metric=metric, max_degree=max_deg,
                                    sort_neighbors=sort_neighbors, point_stats=ps)
        _builds[key] = (G, st, ps)
    return _builds[key]


def slices(m, W):
    """[(s0, s1)] per rank: per = ceil(m / W) ids each, the last ranks short or empty (distributed.vamana_build_sharded)"""
    per = (m + W - 1) // W
    return [(min(m, r * per), min(m, (r + 1) * per)) for r in range(W)]


def schedule(n, seed, passes, alpha):
    """[(ids, alpha of the pass)] for every batch of every pass: distributed.build_schedule walked as build_index does
    (alpha = 1.0 on all but the last pass)"""
    perm, bounds = distributed.build_schedule(n, seed)
    return [(perm[lo:hi], alpha if p == passes - 1 else 1.0) for p in range(passes) for lo, hi in bounds]


def oracle_two_phase_build(oracle, X, R, L, alpha, passes, seed, W, metric, max_degree=None, start=0):
    """The build as W ranks run it, on the oracle: per batch phase A on each of the W slices, the rows concatenated in batch
    order, phase B on the whole batch.  Yields (batch ids, rows [m, R], a copy of the graph after the batch) for every batch of
    every pass, then (None, None, graph after the final neighbour sort)."""
    G = np.zeros((len(X), (R if max_degree is None else max_degree) + 1), np.uint32)
    for ids, a in schedule(len(X), seed, passes, alpha):
        parts = [oracle.vamana_phase_a(X, G, ids[s0:s1], R, L, a, start=start, metric=metric) for s0, s1 in slices(len(ids), W) if s1 > s0]
        rows = np.concatenate(parts)
        oracle.vamana_phase_b(X, G, ids, rows, R, a, metric=metric)
        yield ids, rows, G.copy()
    oracle.sort_neighbors(X, G, metric=metric)
    yield None, None, G


# No phase-A row of the one-pass u8_R96 build is longer than 76 (the candidate lists of a first pass at L = 100 are too short
# to leave 96 picks), so that case has padded rows wider than a wave but no FULL one.  One more batch covers it: ids of a
# seeded permutation inserted again into the finished (unsorted) u8_R96 graph at L = 200.
FULL_WIDE_M, FULL_WIDE_L, FULL_WIDE_SEED = 500, 200, 21


def full_wide_batch(oracle):
    """(X, metric, graph before, ids, rows, R, L, alpha) of that batch; the graph is a copy"""
    X, metric, R, _, _, alpha, _, _ = vamana_case("u8_R96")
    G = vamana_oracle_build(oracle, "u8_R96", sort_neighbors=False)[0].copy()
    ids = oracle.permutation(len(X), FULL_WIDE_SEED)[:FULL_WIDE_M]
    if "full_wide" not in _builds:
        _builds["full_wide"] = oracle.vamana_phase_a(X, G, ids, R, FULL_WIDE_L, alpha, metric=metric)
    return X, metric, G, ids, _builds["full_wide"], R, FULL_WIDE_L, alpha


def norm(G):
    """slots past a row's degree zeroed (a row that shrank keeps its old tail, in the oracle and on the device)"""
    G = G.copy()
    cols = np.arange(G.shape[1] - 1)[None, :]
    G[:, 1:][cols >= G[:, :1]] = 0
    return G


# ---- HCNNG ----

def hcnng_points(name):
    dtype, metric, _ = HCNNG_CASES[name]
    return points(dtype, HCNNG_D), metric


def oracle_tree(oracle, X, t, cluster_size, mst_deg, seed, metric="l2"):
    """tree t of the forest seeded by `seed` as an [n, mst_deg + 1] graph (count, then the edges in the tree's row order): the
    oracle seeds tree t with seed + t, so a one-tree build with that seed is the tree.  Made once per (points, tree)."""
    key = (id(X), t, cluster_size, mst_deg, seed, metric)
    if key not in _trees:
        _trees[key] = (X, oracle.hcnng_build(X, 1, cluster_size, mst_deg, seed=seed + t, metric=metric))      # X kept: id() stays unique
    return _trees[key][1]


def slab_stride(T, W, mst_deg):
    return (T + W - 1) // W * mst_deg


def oracle_tree_slabs(oracle, X, T, cluster_size, mst_deg, seed, W, metric="l2", stride=None):
    """[W, n, stride] uint32: the slab every rank is expected to hand to the all-gather.  Rank r owns trees r, r + W, ...; slots
    [j * mst_deg, (j + 1) * mst_deg) of row v hold the edges of the rank's j-th tree in that tree's row order, 0xFFFFFFFF elsewhere
    (the columns of trees the rank does not own, any columns beyond ceil(T / W) * mst_deg, the whole slab of a rank without trees)"""
    stride = slab_stride(T, W, mst_deg) if stride is None else stride
    slabs = np.full((W, len(X), stride), SENTINEL, np.uint32)
    cols = np.arange(mst_deg)[None, :]
    for r in range(W):
        for j, t in enumerate(range(r, T, W)):
            g = oracle_tree(oracle, X, t, cluster_size, mst_deg, seed, metric)
            slabs[r, :, j * mst_deg:(j + 1) * mst_deg] = np.where(cols < g[:, :1], g[:, 1:], SENTINEL)
    return slabs


def interleave(slabs, T, mst_deg, max_deg, order="tree", initial=None):
    """the graph the slabs assemble to: after a row's current neighbours the edges of trees 0 .. T - 1 in tree order, never beyond
    max_deg.  order = "slab" is the WRONG order (all trees of slab 0, then slab 1, ...), for the CPU test that shows the
    comparison tells the two apart."""
    W, n, _ = slabs.shape
    G = np.zeros((n, max_deg + 1), np.uint32) if initial is None else initial.copy()
    trees = range(T) if order == "tree" else [t for r in range(W) for t in range(r, T, W)]
    for t in trees:
        src = slabs[t % W][:, (t // W) * mst_deg:(t // W + 1) * mst_deg]
        for v in range(n):
            for a in src[v][src[v] != SENTINEL]:
                if G[v, 0] < max_deg:
                    G[v, 1 + G[v, 0]] = a
                    G[v, 0] += 1
    return G
