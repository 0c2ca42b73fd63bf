"""The rules of DESIGN.md "Entry points" restated in plain numpy: the centroid of what a filter allows, its conversion to the
handle's element type, the medoid rows (pann_filter_medoids_*), and the grouped labeled search (pann_batch_search_grouped_labeled).
Nothing here needs a GPU.

    centroid    centroid[j] = (float32)(S / (double)c), S = the sum over the allowed rows of coordinate j, c their number.  S is
                summed in Python integers: the one-byte types as they are, the float types as the integers their values are
                multiples of (exact_sums), so S is exact and double(S) is what math.fsum gives.  One double division, one
                rounding to float32.  c == 0: zeros.
    conversion  f32 as it is; f16 round to nearest even; bf16 as parlayann_amd.bf16.to_bf16; u8 / i8 rint (ties to even), clamped
    medoid rows the oracle's brute force over the allowed rows (masked_knn_cases.reference) for the converted centroid, k =
                per_filter, padding ids replaced by fill_id
    grouped     per distinct table entry: masked_ref / steered_ref with that entry's predicate (label_allow) and start row, the
                rows placed by the index array
"""
from fractions import Fraction

import numpy as np

import masked_knn_cases as kc
from parlayann_amd import bfloat16, from_bf16, to_bf16
from parlayann_amd.index import label_allow

SEARCH_FIELDS = ("ids", "dists", "frontier_size", "visited_count", "dist_cmps", "degree_sum", "result_count", "allowed_cmps")
STEER_FIELDS = ("bridge_rows", "hop2_cmps")


def widen(X):
    """rows as float64 (exact for every element type)"""
    return from_bf16(X).astype(np.float64) if X.dtype == bfloat16 else np.asarray(X).astype(np.float64)


def exact_sums(rows):
    """rows: (c, d) of any element type -> (sums, e): d Python integers and an exponent, column j sums EXACTLY to sums[j] * 2 ** e.
    A float is mantissa * 2 ** exponent with a 53-bit integer mantissa: the mantissas of one exponent are added in int64 (24
    significant bits each for f32 / f16 / bf16 data, so 2 ** 39 of them fit), the exponents are combined in Python integers."""
    if rows.dtype != bfloat16 and np.issubdtype(rows.dtype, np.integer):
        return [int(v) for v in rows.astype(np.int64).sum(axis=0)], 0
    W = widen(rows)
    d = W.shape[1]
    if len(W) == 0:
        return [0] * d, 0
    m, e = np.frexp(W)
    M = np.ldexp(m, 24)
    assert (M == np.rint(M)).all()                     # 24-bit mantissas: the data came from f32 or narrower
    M, e = M.astype(np.int64), e.astype(np.int64) - 24
    e[M == 0] = 0
    lo = int(e.min())
    sums = [0] * d
    for ex in np.unique(e):
        part = np.where(e == ex, M, 0).sum(axis=0)
        for j in range(d):
            sums[j] += int(part[j]) << (int(ex) - lo)
    return sums, lo


def exact_mean(rows):
    """d Fractions: the exact mean of every column (c >= 1)"""
    sums, e = exact_sums(rows)
    scale = Fraction(2) ** e
    return [Fraction(s) * scale / len(rows) for s in sums]


def centroid(X, allow):
    """float32 (d,): THE RULE for the rows of X that boolean `allow` selects"""
    rows = X[np.asarray(allow, bool)]
    c, d = len(rows), X.shape[1]
    if c == 0:
        return np.zeros(d, np.float32)
    sums, e = exact_sums(rows)
    scale = Fraction(2) ** e
    S = [float(Fraction(s) * scale) for s in sums]     # the double nearest to the exact sum (math.fsum's answer)
    return np.array([s / float(c) for s in S], np.float64).astype(np.float32)


def convert(cen, dtype):
    """the centroid as a query row of the handle's element type"""
    cen = np.asarray(cen, np.float32)
    if dtype == bfloat16:
        return to_bf16(cen)
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return cen.copy()
    if dtype == np.float16:
        return cen.astype(np.float16)
    info = np.iinfo(dtype)
    return np.clip(np.rint(cen), info.min, info.max).astype(dtype)


def filter_medoids(oracle, X, allow_rows, per_filter, metric, fill_id=kc.PAD_ID):
    """allow_rows boolean (G, n) -> {"ids" (G, E), "dists" (G, E), "counts" (G,), "centroids" (G, d)}"""
    A = np.asarray(allow_rows, bool).reshape(-1, len(X))
    G, E = len(A), per_filter
    out = {"ids": np.empty((G, E), np.uint32), "dists": np.empty((G, E), np.float32), "counts": np.empty(G, np.uint32),
           "centroids": np.empty((G, X.shape[1]), np.float32)}
    for g in range(G):
        out["centroids"][g] = centroid(X, A[g])
        q = np.ascontiguousarray(convert(out["centroids"][g], X.dtype)[None, :])
        ids, dists, counts = kc.reference(oracle, X, q, A[g], E, metric)
        ids[ids == kc.PAD_ID] = fill_id
        out["ids"][g], out["dists"][g], out["counts"][g] = ids[0], dists[0], counts[0]
    return out


def grouped_search_ref(points, graph, labels, kind, table, group, starts, steer=None, queries=None, query_ids=None, **kw):
    """pann_batch_search_grouped_labeled restated: table (G, 2) predicates of `kind` over `labels`, group (nq,) table indices,
    starts (nstarts,) or (G, nstarts); steer None (the masked walk) or the fill of the steered walk.  -> the dict of the walk's
    fields, rows placed by the index array.  kw: k, beam, cut, limit, degree_limit, metric, out_k, visited_cap."""
    import masked_ref
    import steered_ref
    table = np.asarray(table, np.uint32).reshape(-1, 2)
    group = np.asarray(group)
    starts = np.asarray(starts, np.uint32)
    out = None
    for g in np.unique(group):
        sel = np.flatnonzero(group == g)
        q = dict(queries=np.ascontiguousarray(queries[sel])) if queries is not None else dict(query_ids=np.ascontiguousarray(np.asarray(query_ids)[sel]))
        allow = label_allow(labels, kind, tuple(int(v) for v in table[g]))
        st = tuple(int(s) for s in (starts if starts.ndim == 1 else starts[g]))
        if steer is None:
            r = masked_ref.masked_batch_search(points, graph, allow, starts=st, **q, **kw)
        else:
            r = steered_ref.steered_batch_search(points, graph, allow, fill=steer, starts=st, **q, **kw)
        if out is None:
            out = {f: np.zeros((len(group),) + np.shape(v)[1:], np.asarray(v).dtype) for f, v in r.items()
                   if isinstance(v, np.ndarray) and len(v) == len(sel)}
        for f in out:
            out[f][sel] = r[f]
    return out
