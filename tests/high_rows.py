"""Cases shared by the tests of rows past the 4 GiB / 2^32-element line (DESIGN.md "Rows past 4 GiB"):
tests/test_high_rows_cpu.py asserts on the CPU that the geometries sit on the line and that the data meets the conditions the
comparisons rest on, tests/test_high_rows_gpu.py runs every id-addressed operation on them.  Plain Python: nothing here needs a GPU.

The method: an index with n just above the line, created empty on the device, and ONE populated block of M = 4096 rows
[B0 - M/2, B0 + M/2), where B0 is the first row whose byte offset (points) or element offset (graph) is >= 2^32.  Everything
outside the block is a zero vector with an empty graph row, so an offset that wraps at 32 bits reads zeros or an empty row: a
wrong answer, never a fault.  Ids are the real ids, never shifted: hashes, (dist, id) tie-breaks and counters are those of
rows >= 2^24 (2^26).

Geometries (name: element types, d, row bytes, max_deg, n, B0):
    A   float16 + bfloat16 (l2)      128  256  64  2^24 + 4096  2^24   point bytes cross 2^32
    B   uint8 (l2) + int8 (mips)      64   64  64  2^26 + 4096  2^26   point bytes AND graph elements (n * gstride) cross 2^32
    C   float32 (l2)                  64  256  32  2^24 + 4096  2^24   point bytes of the full-precision table

Block data: integers, every coordinate in [128, 255] (int8 mips: [1, 127]), clustered, a few duplicated rows -- one pair on rows
B0 - 1 / B0.  Two CONDITIONS follow from the range and are asserted by the CPU test, not assumed:
    exactness   |a|^2, |b|^2, 2|ab| and sum (a - b)^2 stay below 2^24, so every float sum is exact in any order
    dominance   l2: every block point is nearer to every query than a zero row is; mips: every block distance is negative, a
                zero row's is 0 -- so brute force over the whole table has a block-local reference
The host side of every comparison is a SPARSE array of the full shape (np.zeros pages are untouched until written).
"""
import numpy as np

from parlayann_amd import bfloat16
from parlayann_amd.bf16 import from_bf16, to_bf16

LINE = 1 << 32
M = 4096                                   # rows of the populated block
ALPHA = {"l2": 1.2, "mips": 1.0}
BUILD_SEED = 9
BATCH_CAP = 512                            # prefix-doubling batches 1, 2, 4, ... capped here

# name -> element types with their metric, d, max_deg, n
GEOMS = {
    "A": dict(types=((np.dtype(np.float16), "l2"), (bfloat16, "l2")), d=128, max_deg=64, n=(1 << 24) + M),
    "B": dict(types=((np.dtype(np.uint8), "l2"), (np.dtype(np.int8), "mips")), d=64, max_deg=64, n=(1 << 26) + M),
    "C": dict(types=((np.dtype(np.float32), "l2"),), d=64, max_deg=32, n=(1 << 24) + M),
}

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def type_name(dtype):
    return "bf16" if np.dtype(dtype) == bfloat16 else np.dtype(dtype).name


def row_stride(geom, dtype):
    """bytes between two device rows: the row rounded up to 64 bytes (choose_point_layout: lanes x chunks x 16 = r64)"""
    return (GEOMS[geom]["d"] * np.dtype(dtype).itemsize + 63) // 64 * 64


def gstride(geom):
    """uint32 elements between two device graph rows"""
    return (GEOMS[geom]["max_deg"] + 15) // 16 * 16


def b0(geom):
    """the first row whose byte offset in the point slab is >= 2^32 (the same row for every type of a geometry)"""
    strides = {row_stride(geom, dt) for dt, _ in GEOMS[geom]["types"]}
    assert len(strides) == 1
    return -(-LINE // strides.pop())


def lo(geom):
    return b0(geom) - M // 2


def block_ids(geom):
    return np.arange(lo(geom), lo(geom) + M, dtype=np.uint32)


# (row, row it repeats), block-local: the first pair lies across B0
DUPLICATES = ((M // 2, M // 2 - 1), (M // 2 + 700, 3), (17, M - 5), (M - 1, M // 2 - 300))


def _typed(v, dtype):
    return to_bf16(v.astype(np.float32)) if np.dtype(dtype) == bfloat16 else v.astype(dtype)


def as_int(x):
    """rows of any element type as int64 (the data is integer-valued)"""
    x = np.asarray(x)
    f = from_bf16(x) if x.dtype == bfloat16 else x
    v = f.astype(np.int64)
    assert (v == f).all()
    return v


def _clustered(rng, rows, d, vlo, vhi, centres):
    c = centres[rng.integers(0, len(centres), rows)]
    return np.clip(c + rng.integers(-14, 15, (rows, d)), vlo, vhi)


def _value_range(dtype, metric):
    return (1, 127) if np.dtype(dtype) == np.int8 else (128, 255)


def _centres(geom, dtype, metric):
    vlo, vhi = _value_range(dtype, metric)
    return np.random.default_rng(50).integers(vlo + 10, vhi - 9, (24, GEOMS[geom]["d"]))


def block(geom, dtype, metric):
    """the M rows of the block, (M, d) of dtype, made once.  float16 and bfloat16 hold the same numbers."""
    def make():
        vlo, vhi = _value_range(dtype, metric)
        v = _clustered(np.random.default_rng(51), M, GEOMS[geom]["d"], vlo, vhi, _centres(geom, dtype, metric))
        for a, b in DUPLICATES:
            v[a] = v[b]
        out = _typed(v, dtype)
        out.setflags(write=False)
        return out
    return _once(("block", geom, type_name(dtype), metric), make)


def queries(geom, dtype, metric, nq=64):
    """external query rows from the same clusters, (nq, d) of dtype"""
    vlo, vhi = _value_range(dtype, metric)
    v = _clustered(np.random.default_rng(52), nq, GEOMS[geom]["d"], vlo, vhi, _centres(geom, dtype, metric))
    return _typed(v, dtype)


def sparse_points(geom, dtype, metric):
    """np.zeros((n, d), dtype) with the block written: only the block's pages are ever touched"""
    def make():
        g = GEOMS[geom]
        try:
            X = np.zeros((g["n"], g["d"]), dtype)
        except MemoryError as e:
            raise AssertionError(f"the host refused a lazily zeroed {g['n'] * g['d'] * np.dtype(dtype).itemsize} byte array") from e
        X[lo(geom):lo(geom) + M] = block(geom, dtype, metric)
        return X
    return _once(("sparse", geom, type_name(dtype), metric), make)


def sparse_graph(geom, max_deg=None):
    """a fresh np.zeros((n, max_deg + 1), uint32): the empty graph in the reference layout, no page touched"""
    g = GEOMS[geom]
    w = (g["max_deg"] if max_deg is None else max_deg) + 1
    try:
        return np.zeros((g["n"], w), np.uint32)
    except MemoryError as e:
        raise AssertionError(f"the host refused a lazily zeroed {g['n'] * w * 4} byte array") from e


def batches(oracle, geom):
    """(start, [batch ids]): oracle.permutation(M, seed) + lo in prefix-doubling batches capped at BATCH_CAP; start = its first id"""
    perm = (oracle.permutation(M, BUILD_SEED).astype(np.int64) + lo(geom)).astype(np.uint32)
    out, a, sz = [], 0, 1
    while a < M:
        out.append(perm[a:a + sz])
        a += sz
        sz = min(2 * sz, BATCH_CAP)
    return int(perm[0]), out


def block_graph(oracle, geom, dtype, metric, L=64):
    """(sparse graph, start): the oracle's Vamana graph of the block (R = max_deg), every row outside the block empty.  Cached:
    do not write to it."""
    def make():
        X = sparse_points(geom, dtype, metric)
        G = sparse_graph(geom)
        start, bs = batches(oracle, geom)
        for b in bs:
            oracle.vamana_insert_batch(X, G, b, GEOMS[geom]["max_deg"], L, ALPHA[metric], start=start, metric=metric)
        return G, start
    return _once(("graph", geom, type_name(dtype), metric, L), make)


def block_rows(G, geom):
    """rows [lo, lo + M) of a sparse graph as block-local rows: ids minus lo, zero beyond the degree (what
    subset(allow=block bitmap).get_graph() returns)"""
    rows = np.array(G[lo(geom):lo(geom) + M], np.int64)
    live = np.arange(rows.shape[1] - 1)[None, :] < rows[:, :1]
    assert (rows[:, 1:][live] >= lo(geom)).all() and (rows[:, 1:][live] < lo(geom) + M).all()
    rows[:, 1:] = np.where(live, rows[:, 1:] - lo(geom), 0)
    return rows.astype(np.uint32)


def block_allow(n, ids):
    """one packed allow row (ceil(n / 32) uint32 words) with exactly the bits of `ids`, without an n-byte boolean array"""
    w = np.zeros((int(n) + 31) // 32, np.uint32)
    ids = np.asarray(ids, np.int64)
    np.bitwise_or.at(w, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return w


# ---- block-local references: int64 numpy, (dist, id) order ----

def dist_matrix(Q, X, metric):
    """int64 (nq, rows): sum (q - x)^2, or -sum q x"""
    q, x = as_int(Q), as_int(X)
    dots = (q.astype(np.float64) @ x.astype(np.float64).T).astype(np.int64)       # exact: integers far below 2^53
    if metric == "mips":
        return -dots
    return (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2 * dots


def zero_row_dist(Q, metric):
    """int64 (nq,): the distance of every query to a zero row"""
    q = as_int(Q)
    return np.zeros(len(q), np.int64) if metric == "mips" else (q * q).sum(1)


def knn_ref(Q, X, first_id, k, metric, allowed=None):
    """the k nearest of rows X (ids first_id ...) per query, ties by id -> (ids uint32 (nq, k), dists float32 (nq, k), counts);
    allowed: boolean (rows,) -- short rows are padded with 0xFFFFFFFF / +inf"""
    D = dist_matrix(Q, X, metric)
    cols = np.arange(D.shape[1]) if allowed is None else np.flatnonzero(allowed)
    D = D[:, cols]
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    cnt = order.shape[1]
    ids = np.full((len(D), k), 0xFFFFFFFF, np.uint32)
    dists = np.full((len(D), k), np.inf, np.float32)
    ids[:, :cnt] = cols[order] + first_id
    dists[:, :cnt] = np.take_along_axis(D, order, 1).astype(np.float32)
    return ids, dists, np.full(len(D), cnt, np.uint32)


def range_ref(Q, X, first_id, radius, metric):
    """every row within `radius` (dist <= radius) per query as CSR -> (offsets uint64 (nq + 1,), ids uint32 ascending)"""
    hit = dist_matrix(Q, X, metric) <= radius
    off = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.uint64)
    return off, (np.nonzero(hit)[1] + first_id).astype(np.uint32)


RADIUS_QUANTILES = (0.002, 0.05)             # the radii of the range tests: these quantiles of all query-to-block distances


def radius(geom, dtype, metric, quantile):
    """a radius of the range tests, as the float32 the device compares with"""
    D = dist_matrix(queries(geom, dtype, metric), block(geom, dtype, metric), metric)
    return float(np.float32(np.quantile(D, quantile)))


def exactness_terms(Q, X, metric):
    """over every pair of rows of X + Q: the largest |a|^2, 2 |ab| and sum (a - b)^2 -- what has to stay below 2^24 for the float
    sums to be exact in either algebraic form (float64 products of these integers are exact)"""
    a = np.concatenate([as_int(X), as_int(Q)]).astype(np.float64)
    sq = (a * a).sum(1)
    dots = a @ a.T
    return dict(norm2=int(sq.max()), twice_dot=int(2 * np.abs(dots).max()), l2=int((sq[:, None] + sq[None, :] - 2 * dots).max()))
