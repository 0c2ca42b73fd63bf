"""On-disk formats of the reference:
  vectors  .bin  : [n:u32][d:u32][n*d*sizeof(T)]                 (point_range.h:74-117, python/_files.py:42-95)
  graph          : [n:u32][maxDeg:u32][deg[n]:u32][edges...:u32]  (graph.h:147-232)
  truth    .ibin : [n:i32][k:i32][ids n*k:u32][dists n*k:f32]     (types.h:48-73, compute_groundtruth.cpp:63-102)
  range truth    : [n:i32][num_matches:i32][sizes n:i32][ids num_matches:i32]
                                                                  (types.h:119-140, compute_range_groundtruth.cpp:64-88)
"""
import numpy as np


def write_bin(path, x):
    x = np.ascontiguousarray(x)
    with open(path, "wb") as f:
        np.array(x.shape, dtype=np.uint32).tofile(f)
        x.tofile(f)


def read_bin(path, dtype):
    with open(path, "rb") as f:
        n, d = np.fromfile(f, dtype=np.uint32, count=2)
        return np.fromfile(f, dtype=dtype, count=int(n) * int(d)).reshape(int(n), int(d))


def write_graph(path, graph):
    """graph: n x (maxDeg+1) uint32 in the in-memory reference layout (slot 0 = degree)."""
    g = np.ascontiguousarray(graph, dtype=np.uint32)
    n, w = g.shape
    deg = g[:, 0]
    with open(path, "wb") as f:
        np.array([n, w - 1], dtype=np.uint32).tofile(f)
        deg.tofile(f)
        mask = np.arange(w - 1)[None, :] < deg[:, None]
        g[:, 1:][mask].tofile(f)


def read_graph(path):
    with open(path, "rb") as f:
        n, maxdeg = (int(v) for v in np.fromfile(f, dtype=np.uint32, count=2))
        deg = np.fromfile(f, dtype=np.uint32, count=n)
        edges = np.fromfile(f, dtype=np.uint32, count=int(deg.sum()))
    g = np.zeros((n, maxdeg + 1), dtype=np.uint32)
    g[:, 0] = deg
    mask = np.arange(maxdeg)[None, :] < deg[:, None]
    g[:, 1:][mask] = edges
    return g


def write_ibin(path, ids, dists):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    with open(path, "wb") as f:
        np.array(ids.shape, dtype=np.int32).tofile(f)
        ids.tofile(f)
        dists.tofile(f)


def read_ibin(path):
    with open(path, "rb") as f:
        n, k = (int(v) for v in np.fromfile(f, dtype=np.int32, count=2))
        ids = np.fromfile(f, dtype=np.uint32, count=n * k).reshape(n, k)
        dists = np.fromfile(f, dtype=np.float32, count=n * k).reshape(n, k)
    return ids, dists


def write_range_gt(path, offsets, ids):
    """RangeGroundTruth file from CSR: offsets (n + 1 entries), ids (offsets[n] entries).  The header is 32-bit: a result with
    2^31 or more matches (or queries) cannot be written in this format and is refused."""
    offsets = np.asarray(offsets).astype(np.int64)
    if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must be n + 1 non-decreasing entries starting at 0")
    n, total = len(offsets) - 1, int(offsets[-1])
    if total >= 2 ** 31 or n >= 2 ** 31:
        raise ValueError(f"{n} queries / {total} matches do not fit the range ground-truth format (32-bit header)")
    if total != len(ids):
        raise ValueError(f"offsets end at {total}, {len(ids)} ids given")
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    if len(ids) and int(ids.max()) >= 2 ** 31:
        raise ValueError("ids of 2^31 and more do not fit the range ground-truth format (32-bit signed ids)")
    with open(path, "wb") as f:
        np.array([n, total], dtype=np.int32).tofile(f)
        np.diff(offsets).astype(np.int32).tofile(f)
        ids.astype(np.int32).tofile(f)


def read_range_gt(path):
    """-> (offsets uint64[n + 1], ids uint32[num_matches])"""
    with open(path, "rb") as f:
        n, total = (int(v) for v in np.fromfile(f, dtype=np.int32, count=2))
        sizes = np.fromfile(f, dtype=np.int32, count=n)
        ids = np.fromfile(f, dtype=np.int32, count=total)
    if n < 0 or total < 0 or len(sizes) != n or len(ids) != total or (sizes < 0).any() or int(sizes.sum(dtype=np.int64)) != total:
        raise ValueError(f"{path}: not a range ground-truth file (n = {n}, num_matches = {total})")
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(sizes, dtype=np.uint64, out=offsets[1:])
    return offsets, ids.astype(np.uint32)
