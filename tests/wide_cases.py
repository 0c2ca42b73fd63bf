"""Cases shared by the wide-row tests: adjacency rows longer than one 64-lane wavefront.

The device graph row is gstride = ceil(max_deg / 16) * 16 words and a block is one wave, so every kernel that walks a row has a
single-pass shape (gstride <= 64) and a multi-pass shape.  tests/test_wide_cases_cpu.py asserts on the oracle alone that every
case below really walks rows wider than a wave (so that no device test passes vacuously); tests/test_wide_rows_gpu.py runs the
cases on the device.  Plain Python: nothing here needs a GPU.

Four point layouts (integer-valued data: any summation order is exact) and four widths:

    uint8   d = 32   L2     64-byte rows, 4 lanes per chunk, query in LDS
    float16 d = 128  L2     16 lanes per chunk, query in registers
    float32 d = 96   L2     8 lanes per chunk, three chunks
    int8    d = 200  MIPS   16 lanes per chunk, query in registers

    max_deg 65   gstride 80: 16 live lanes in the second pass
            80   an exact multiple of 16
            129  three passes, the last with 16 lanes
            200  four passes
"""
import numpy as np

import oracle_api
from parlayann_amd import datasets

N, NQ = 3000, 100
WAVE = 64
# name -> (dtype, d, metric)
LAYOUTS = {
    "u8": (np.uint8, 32, "l2"),
    "f16": (np.float16, 128, "l2"),
    "f32": (np.float32, 96, "l2"),
    "i8": (np.int8, 200, "mips"),
}
WIDTHS = (65, 80, 129, 200)
N_PLANTED = 10

# three visits from vertex 0 (full degree): the search whose degree_sum exceeds 64 per visit even at width 65
SHORT_SEARCH = dict(k=10, beam=64, cut=1.35, limit=3, out_k=64, visited_cap=2048)

_data, _graphs = {}, {}


def rows_of(n, d, dtype, seed):
    """sift_like rows; int8: shifted to signed values (as the other suites do)"""
    if np.dtype(dtype) == np.int8:
        x = datasets.sift_like(n, d, seed=seed, dtype=np.float32)
        return (x - 128.0).clip(-127, 127).astype(np.int8)
    return datasets.sift_like(n, d, seed=seed, dtype=dtype)


def layout_data(layout, n=N, nq=NQ):
    """(X, Q, metric) of a layout, made once and never changed"""
    key = (layout, n, nq)
    if key not in _data:
        dtype, d, metric = LAYOUTS[layout]
        _data[key] = (rows_of(n, d, dtype, 1234), rows_of(nq, d, dtype, 4321), metric)
    return _data[key]


def degree_choices(max_deg):
    """the seven degrees a row draws from: {0, 1, 63, 64, 65, max_deg - 1, max_deg}, clipped to max_deg.  At max_deg = 65 the
    sixth slot would repeat 64 and leave only 2 of 7 slots above a wave; a slot that repeats a narrower one goes to max_deg, so
    that 3 of the 7 slots are wider than a wave at every width (and 64 keeps at least one)."""
    out = []
    for v in (0, 1, WAVE - 1, WAVE, WAVE + 1, max_deg - 1, max_deg):
        v = min(v, max_deg)
        out.append(max_deg if (v in out and v <= WAVE) else v)
    return out


def wide_graph(X, max_deg, seed, metric, oracle=None):
    """An n x (max_deg + 1) graph in the reference layout (slot 0 = degree):
    - per-vertex degree drawn uniformly from degree_choices(max_deg);
    - the neighbours are the vertex's nearest neighbours (oracle.bruteforce_knn) with two entries replaced by random ids, shuffled;
    - vertex 0, the default start, has max_deg neighbours: every query walks at least one wide row;
    - N_PLANTED rows of full degree (vertex 0 among them) carry one duplicated id and the row's own id in SLAB columns >= 64.
      Slab column c holds neighbour c - 1 (column 0 is the degree), so slab columns >= 65 are the later passes of a kernel.  From
      width 80 on both planted ids sit in slab columns >= 65: the duplicate repeats an id of the first pass in a later one.
      Width 65 has one neighbour beyond the first pass: the own id takes it (slab column 65), the duplicate sits in slab
      column 64, the last lane of the first pass -- a duplicate across passes is not exercised at that width.
    oracle: the Oracle of tests/oracle_api.py (the `oracle` fixture); loaded here when not given."""
    o = oracle if oracle is not None else oracle_api.load()
    n = len(X)
    assert n > max_deg + 1 and max_deg > WAVE
    rng = np.random.default_rng(seed)
    nn, _ = o.bruteforce_knn(X, X, max_deg + 1, metric)
    deg = rng.choice(degree_choices(max_deg), size=n)
    deg[0] = max_deg
    full = np.flatnonzero(deg == max_deg)
    planted = np.concatenate([[0], rng.choice(full[full != 0], N_PLANTED - 1, replace=False)])
    G = np.zeros((n, max_deg + 1), np.uint32)
    for v in range(n):
        dv = int(deg[v])
        nb = nn[v][nn[v] != v][:dv].copy()         # the row itself is its own nearest neighbour under L2, not always under MIPS
        assert len(nb) == dv
        if dv >= 2:
            nb[rng.choice(dv, 2, replace=False)] = rng.integers(0, n, 2)
        rng.shuffle(nb)
        G[v, 0] = dv
        G[v, 1:1 + dv] = nb
    for v in planted:
        # slab columns (slot 0 = degree): column 64 is the last neighbour of the first pass, 65.. belong to the later passes
        cols = rng.choice(np.arange(WAVE + 1, max_deg + 1), 2, replace=False) if max_deg - WAVE >= 2 else np.array([WAVE, WAVE + 1])
        G[v, cols[0]] = G[v, 3]                    # a duplicate of an id of the first pass
        G[v, cols[1]] = v                          # the row's own id
    return G


def planted_rows(G):
    """rows that hold their own id in a slab column >= 64 (neighbour index >= 63)"""
    return np.array([v for v in range(len(G)) if G[v, 0] > WAVE - 1 and v in G[v, WAVE:1 + G[v, 0]]], np.uint32)


def case(layout, max_deg, n=N, nq=NQ):
    """(X, Q, G, metric): a layout's points and queries with its wide graph of that width, made once and never changed"""
    key = (layout, max_deg, n, nq)
    if key not in _graphs:
        X, Q, metric = layout_data(layout, n, nq)
        _graphs[key] = wide_graph(X, max_deg, 100 + max_deg, metric)
    X, Q, metric = layout_data(layout, n, nq)
    return X, Q, _graphs[key], metric


# ---- build inputs: n = 3000, d = 32, the oracle's graph has at least 100 rows wider than a wave ----
BUILD_D = 32
VAMANA_BUILDS = {
    # name -> (dtype, R, L, alpha, passes, seed)
    "u8_R96": (np.uint8, 96, 128, 1.2, 2, 7),
    "f16_R130": (np.float16, 130, 200, 1.2, 2, 7),
}
HCNNG_BUILDS = {
    # name -> (clusters, cluster_size, mst_deg, seed)
    "30x100x3": (30, 100, 3, 9),
    "24x60x4": (24, 60, 4, 9),
}
_builds = {}


def build_points(dtype):
    return rows_of(N, BUILD_D, dtype, 1234)


def vamana_oracle_build(name, sort_neighbors=True):
    """(X, graph, stats) of the oracle's Vamana build of a VAMANA_BUILDS entry, made once"""
    key = ("vamana", name, sort_neighbors)
    if key not in _builds:
        dtype, R, L, alpha, passes, seed = VAMANA_BUILDS[name]
        X = build_points(dtype)
        G, st = oracle_api.load().vamana_build(X, R, L, alpha, num_passes=passes, seed=seed, sort_neighbors=sort_neighbors)
        _builds[key] = (X, G, st)
    return _builds[key]


def hcnng_oracle_build(name, dtype):
    key = ("hcnng", name, np.dtype(dtype).name)
    if key not in _builds:
        c, s, m, seed = HCNNG_BUILDS[name]
        X = build_points(dtype)
        _builds[key] = (X, oracle_api.load().hcnng_build(X, c, s, m, seed=seed))
    return _builds[key]


def hcnng_oracle_append(X, graph, clusters, cluster_size, mst_deg, seed, metric="l2", oracle=None):
    """pann_oracle_hcnng_build appends its edges to the rows it is given while they have room; the wrapper of oracle_api always
    starts from an empty slab, so a build onto an initial graph calls the entry point itself.  In place."""
    import ctypes as C
    o = oracle if oracle is not None else oracle_api.load()
    X = np.ascontiguousarray(X)
    assert graph.dtype == np.uint32 and graph.flags.c_contiguous
    rc = o.lib.pann_oracle_hcnng_build(
        X.ctypes.data_as(C.c_void_p), C.c_uint64(len(X)), C.c_uint32(X.shape[1]), C.c_int(oracle_api.DT[X.dtype]),
        C.c_uint64(X.strides[0]), C.c_int(oracle_api.METRIC[metric]), graph.ctypes.data_as(C.c_void_p),
        C.c_uint32(graph.shape[1] - 1), C.c_long(clusters), C.c_long(cluster_size), C.c_long(mst_deg), C.c_uint64(seed),
        C.c_int(o.threads))
    assert rc == 0
    return graph


# ---- one insert batch into the oracle-built R = 96 graph ----
INSERT_BUILD, INSERT_SEED, INSERT_M = "u8_R96", 21, 500


def insert_case(oracle=None):
    """(X, G, batch, R, L, alpha): INSERT_M ids of a seeded permutation to insert into the oracle's u8_R96 graph"""
    o = oracle if oracle is not None else oracle_api.load()
    X, G, _ = vamana_oracle_build(INSERT_BUILD)
    _, R, L, alpha, _, _ = VAMANA_BUILDS[INSERT_BUILD]
    return X, G, o.permutation(len(X), INSERT_SEED)[:INSERT_M], R, L, alpha


def range_radius(oracle, X, Q, rank, metric):
    """the median distance of the rank-th nearest neighbour: the radius of the range-search cases"""
    return float(np.median(oracle.bruteforce_knn(X, Q, rank, metric)[1][:, -1]))


def wide_count(G):
    return int((G[:, 0] > WAVE).sum())
