"""The rule of pann_index_create_subset* (include/pann.h, DESIGN.md "Subset index") restated in numpy: what the new handle holds,
from what the source handle holds.  Plain Python: nothing here needs a GPU.

Inputs, all in the layouts the downloads of a DeviceIndex return:
    points   uint8 (n, row_bytes): the host-layout rows as bytes (any element type; four-bit rows are bytes already)
    graph    uint32 (n, max_deg + 1), the reference layout: slot 0 = degree, slots past the degree 0
    labels   uint32 (n,) or None
    sketch   uint8 (n, sketch_row_bytes) or None
    allow    packed uint32 bitmap of at least ceil(n / 32) words, or None = keep every point; bits at positions >= n are ignored
    n_out    rows of the new handle, 0 = the number of kept points
Output: a dict with the same four things for the new handle (labels / sketch None where the source has none) plus
new_to_old (m,) and old_to_new (n,), 0xFFFFFFFF for a dropped id.
"""
import numpy as np

DROPPED = 0xFFFFFFFF


def kept_ids(allow, n):
    """the ids a packed bitmap keeps, ascending"""
    if allow is None:
        return np.arange(n, dtype=np.uint32)
    w = (n + 31) // 32
    bits = np.unpackbits(np.ascontiguousarray(np.asarray(allow, np.uint32)[:w]).view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(bits).astype(np.uint32)


def _maps(allow, n, n_out):
    K = kept_ids(allow, n)
    m = len(K)
    rows = n_out if n_out else m
    assert rows >= m and rows > 0, "the entry point refuses these sizes"
    o2n = np.full(n, DROPPED, np.uint32)
    o2n[K] = np.arange(m, dtype=np.uint32)
    return K, m, rows, o2n


def _rows(src, K, rows):
    if src is None:
        return None
    out = np.zeros((rows,) + src.shape[1:], src.dtype)
    out[:len(K)] = src[K]
    return out


def subset_ref(points, graph, labels, sketch, allow, n_out=0, copy_graph=True):
    n, width = graph.shape
    K, m, rows, o2n = _maps(allow, n, n_out)
    G = np.zeros((rows, width), np.uint32)
    if copy_graph and m:
        old = graph[K]
        live = np.arange(width - 1)[None, :] < old[:, :1]
        mapped = np.where(live, o2n[np.where(live, old[:, 1:], 0)], DROPPED)
        kept = mapped != DROPPED
        order = np.argsort(~kept, axis=1, kind="stable")            # the kept ones first, in row order
        deg = kept.sum(axis=1)
        packed = np.take_along_axis(mapped, order, axis=1)
        G[:m, 0] = deg
        G[:m, 1:] = np.where(np.arange(width - 1)[None, :] < deg[:, None], packed, 0)
    return dict(points=_rows(points, K, rows), graph=G, labels=_rows(labels, K, rows), sketch=_rows(sketch, K, rows),
                new_to_old=K, old_to_new=o2n)


def subset_ref_loop(points, graph, labels, sketch, allow, n_out=0, copy_graph=True):
    """the same, one row and one neighbour at a time"""
    n, width = graph.shape
    w = (n + 31) // 32
    K = [i for i in range(n) if allow is None or (int(allow[i >> 5]) >> (i & 31)) & 1]
    assert allow is None or len(allow) >= w
    m = len(K)
    rows = n_out if n_out else m
    o2n = [DROPPED] * n
    for r, i in enumerate(K):
        o2n[i] = r
    out = dict(points=np.zeros((rows, points.shape[1]), points.dtype), graph=np.zeros((rows, width), np.uint32),
               labels=None if labels is None else np.zeros(rows, np.uint32),
               sketch=None if sketch is None else np.zeros((rows, sketch.shape[1]), np.uint8),
               new_to_old=np.array(K, np.uint32), old_to_new=np.array(o2n, np.uint32))
    for r, i in enumerate(K):
        out["points"][r] = points[i]
        if labels is not None:
            out["labels"][r] = labels[i]
        if sketch is not None:
            out["sketch"][r] = sketch[i]
        if copy_graph:
            nb = [o2n[int(v)] for v in graph[i, 1:1 + int(graph[i, 0])] if o2n[int(v)] != DROPPED]
            out["graph"][r, 0] = len(nb)
            out["graph"][r, 1:1 + len(nb)] = nb
    return out


FIELDS = ("points", "graph", "labels", "sketch", "new_to_old", "old_to_new")


def same(a, b):
    """the first field in which two results differ, or None"""
    for f in FIELDS:
        if (a[f] is None) != (b[f] is None) or (a[f] is not None and not np.array_equal(a[f], b[f])):
            return f
    return None
