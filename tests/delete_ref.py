"""The delete consolidation restated on the CPU (DESIGN.md "Deleting points"), and the cases its CPU and GPU tests share.

One call deletes the set D from the graph G (reference layout, slot 0 = degree): every p outside D with an out-neighbour in D
gets robustPrune(p, candidates, alpha, R) in the id-only form without its own out-neighbours, where candidates are the survivors
of N(p) in row order followed, per deleted v of N(p) in row order, by the survivors of N(v) other than p in row order --
duplicates kept, every row read from G.  Then those rows are replaced and the rows of D emptied.  The prune is the oracle's.
Plain Python: nothing here needs a GPU.
"""
import numpy as np

import oracle_api
import wide_cases
from parlayann_amd import bfloat16, datasets

LONG = 3072         # keys the greedy prune keeps in LDS; longer lists are walked in HBM


def candidates(G, del_ids):
    """(inD[n], owners A in increasing id, candidate ids, CSR offsets) of one call"""
    n = len(G)
    inD = np.zeros(n, bool)
    inD[np.asarray(del_ids, np.int64)] = True
    owners, cand, off = [], [], [0]
    for p in np.flatnonzero(~inD):
        row = G[p, 1:1 + G[p, 0]]
        dead = inD[row]
        if not dead.any():
            continue
        parts = [row[~dead]]
        for v in row[dead]:
            rv = G[v, 1:1 + G[v, 0]]
            parts.append(rv[~inD[rv] & (rv != p)])
        owners.append(p)
        cand.append(np.concatenate(parts))
        off.append(off[-1] + len(cand[-1]))
    flat = np.concatenate(cand).astype(np.uint32) if cand else np.zeros(0, np.uint32)
    return inD, np.array(owners, np.uint32), flat, np.array(off, np.uint64)


def delete_ref(oracle, X, G, del_ids, alpha, R, metric="l2"):
    """-> (new graph, reference layout, zero beyond the degree; info: owners, per-owner dist_cmps, offsets, candidates, inD)"""
    inD, owners, cand, off = candidates(G, del_ids)
    out = normalized(G)
    dc = np.zeros(0, np.uint32)
    if len(owners):
        rows, dc = oracle.robust_prune_batch(X, G, owners, cand, None, off, alpha, R, add=False, metric=metric)
        out[owners] = 0
        out[owners, :R + 1] = rows
    out[inD] = 0
    return normalized(out), dict(owners=owners, dist_cmps=dc, offsets=off, cand=cand, inD=inD)


def normalized(G):
    """a copy with every slot beyond the row's degree zeroed (what get_graph returns)"""
    G = np.array(G, np.uint32, copy=True)
    G[:, 1:][np.arange(G.shape[1] - 1)[None, :] >= G[:, :1]] = 0
    return G


def expected_stats(info):
    return dict(deleted=int(info["inD"].sum()), affected=len(info["owners"]), candidates=int(info["offsets"][-1]),
                prune_dist_cmps=int(info["dist_cmps"].sum(dtype=np.uint64)))


# ---- cases -------------------------------------------------------------------------------------------------------
# layouts x types: name -> (n, d, dtype, metric, R = max_deg, L).  The graph is a Vamana build (the device's on the GPU, the
# oracle's on the CPU: the two are bit-identical, tests/test_build_gpu.py).
LAYOUTS = {
    "u8_24": (600, 24, np.uint8, "l2", 16, 32),         # 64-byte granules
    "i8_100": (500, 100, np.int8, "mips", 24, 48),      # rows ending inside a chunk
    "f16_128": (500, 128, np.float16, "l2", 32, 64),    # 256-byte rows
    "f32_96": (400, 96, np.float32, "l2", 32, 64),      # 384-byte rows
    "bf16_128": (400, 128, bfloat16, "l2", 32, 64),     # 256-byte rows
}
LAYOUT_ALPHA, LAYOUT_BUILD_SEED = 1.2, 5
WIDE_WIDTHS = (65, 80, 129)
WIDE_N, WIDE_D = 600, 16
LONG_DEG = 128

_cache = {}


def seeded_ids(n, fraction, seed, keep=()):
    """a seeded random `fraction` of the ids, never one of `keep`"""
    pool = np.setdiff1d(np.arange(n, dtype=np.uint32), np.asarray(keep, np.uint32))
    return np.sort(np.random.default_rng(seed).choice(pool, int(round(fraction * n)), replace=False)).astype(np.uint32)


def layout_points(name):
    n, d, dtype, metric, R, L = LAYOUTS[name]
    if ("pts", name) not in _cache:
        _cache[("pts", name)] = wide_cases.rows_of(n, d, dtype, 77) if np.dtype(dtype) != bfloat16 else datasets.sift_like(n, d, seed=77, dtype=bfloat16)
    return _cache[("pts", name)]


def layout_case(name, oracle=None):
    """(X, G, del_ids, R, alpha, metric) with the oracle's build of the layout's graph, 30 % deleted"""
    n, d, dtype, metric, R, L = LAYOUTS[name]
    X = layout_points(name)
    if ("graph", name) not in _cache:
        o = oracle if oracle is not None else oracle_api.load()
        _cache[("graph", name)] = o.vamana_build(X, R, L, LAYOUT_ALPHA, num_passes=1, seed=LAYOUT_BUILD_SEED, metric=metric)[0]
    return X, _cache[("graph", name)], seeded_ids(n, 0.30, 900 + n + d), R, LAYOUT_ALPHA, metric


def random_graph(n, deg, seed):
    """every row: `deg` distinct random ids other than the row's own, in random order"""
    rng = np.random.default_rng(seed)
    G = np.zeros((n, deg + 1), np.uint32)
    G[:, 0] = deg
    for v in range(n):
        nb = rng.choice(n - 1, deg, replace=False)
        G[v, 1:] = nb + (nb >= v)
    return G


def wide_points():
    if "wide_pts" not in _cache:
        _cache["wide_pts"] = datasets.sift_like(WIDE_N, WIDE_D, seed=78, dtype=np.uint8)
    return _cache["wide_pts"]


def wide_case(max_deg):
    """random full-degree rows wider than a wavefront over 600 x 16 uint8, 30 % deleted"""
    if ("wide", max_deg) not in _cache:
        _cache[("wide", max_deg)] = random_graph(WIDE_N, max_deg, 300 + max_deg)
    return wide_points(), _cache[("wide", max_deg)], seeded_ids(WIDE_N, 0.30, 400 + max_deg), max_deg, 1.2, "l2"


def long_case():
    """random rows of degree 128 with half of the points deleted: a list is ~64 + 64 * 64 keys, beyond what the greedy prune keeps
    in LDS.  Twenty surviving vertices get rows with only two deleted neighbours, so that short lists run in the same call."""
    if "long" not in _cache:
        n, deg = WIDE_N, LONG_DEG
        G = random_graph(n, deg, 555)
        D = seeded_ids(n, 0.50, 556)
        rng = np.random.default_rng(557)
        live = np.setdiff1d(np.arange(n, dtype=np.uint32), D)
        for p in rng.choice(live, 20, replace=False):
            row = np.concatenate([rng.choice(live[live != p], deg - 2, replace=False), rng.choice(D, 2, replace=False)])
            rng.shuffle(row)
            G[p, 1:] = row
        _cache["long"] = (G, D)
    G, D = _cache["long"]
    return wide_points(), G, D, LONG_DEG, 1.2, "l2"


def regime(G, info):
    """what a case exercises: (a) owners with >= 2 deleted neighbours, (b) owners listed by one of their deleted neighbours,
    (c) owners with an empty candidate list, the longest and shortest list, and the degrees of affected and deleted rows"""
    inD, owners = info["inD"], info["owners"]
    two = back = 0
    for p in owners:
        dead = [v for v in G[p, 1:1 + G[p, 0]] if inD[v]]
        two += len(dead) >= 2
        back += any(p in G[v, 1:1 + G[v, 0]] for v in dead)
    lens = np.diff(info["offsets"].astype(np.int64))
    return dict(two_deleted=int(two), back_edge=int(back), empty_list=int((lens == 0).sum()), longest=int(lens.max(initial=0)),
                shortest=int(lens.min(initial=1 << 30)), widest_affected=int(G[owners, 0].max(initial=0)),
                widest_deleted=int(G[inD, 0].max(initial=0)))


def empty_row_case(G, p):
    """D = N(p) and every neighbour of N(p), but not p: p is affected and its candidate list is empty"""
    nb = G[p, 1:1 + G[p, 0]]
    second = np.concatenate([G[v, 1:1 + G[v, 0]] for v in nb])
    D = np.union1d(nb, second)
    return D[D != p].astype(np.uint32)


def in_neighbours(G, v):
    return np.array([u for u in range(len(G)) if u != v and v in G[u, 1:1 + G[u, 0]]], np.uint32)
