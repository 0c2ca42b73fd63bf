#!/usr/bin/env python3
"""Recorder of tests/golden/binding_trace_v1.txt: what parlayann_amd/index.py and parlayann_amd/graph_index.py ASKED OF THE
C-ABI, and what they returned, at commit d0c7f13 -- the last one in which every method spelled out its own filter arms.  Run
by hand; tests/test_binding_trace_cpu.py recomputes the same rows and compares.

parlayann_amd._capi.load is replaced by a stand-in whose every pann_* attribute is a Python callable that returns 0: no
libpann.so, no device.  Per call the stand-in records the symbol, every scalar argument, null / non-null for every pointer (a
handle by its ordinal), the fields of every by-reference struct, and the BYTES of every input array (their sizes come from
SPECS below).  It fills every output array with a pattern that depends on the symbol, the argument position or struct field and
the element index, writes `kept` and the handle of the create calls and answers pann_index_size, so the post-processing (the
steer-counter split, range padding, n2o[:kept], GraphIndex._need) has something to get wrong.  One line per case: a SHA-256
over the recorded calls and the returned object (keys, shapes, dtypes, bytes) or the exception's type and text.

The recorder uses the public API only, so the same text runs at d0c7f13 and at any later commit.
usage: tests/golden/make_binding_trace.py [--out FILE] [--dump CASE]"""
import argparse
import ctypes as C
import hashlib
import operator
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))) if p not in sys.path]

from parlayann_amd import _capi, graph_index, io  # noqa: E402
from parlayann_amd import index as ixm  # noqa: E402
from parlayann_amd.index import DeviceIndex  # noqa: E402

N, D, DEG, NQ, K, BEAM = 70, 8, 4, 3, 2, 8
W = (N + 31) // 32
HANDLE0 = 0xDEAD00000000          # above every user-space address: a handle is never mistaken for an array


def _sha(b):
    return hashlib.sha256(b).hexdigest()[:16]


def _struct_fields(s):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        out.append((name, ("ptr" if v else "null") if typ is C.c_void_p else repr(v)))
    return tuple(out)


# ---- per-symbol tables: ("in", position, bytes) | ("out", position, bytes[, lo, count]) | ("fields", position, {field: bytes | (bytes, lo, count)})
def _search_out(L, s, nq):
    k = s.out_k
    return {"ids": nq * k * 4, "dists": nq * k * 4, "frontier_size": (nq * 4, 0 if L.short_frontier else k, 4), "visited_count": nq * 4,
            "dist_cmps": nq * 4, "degree_sum": nq * 4, "visited_ids": nq * s.visited_cap * 4, "visited_dists": nq * s.visited_cap * 4,
            "status": 4}


def _prefix(L, A, per_query=False):
    """h, queries, query_ids, nq, stride, starts, nstarts, query params"""
    nq = A[3]
    return [("in", 1, nq * A[4]), ("in", 2, nq * 4), ("in", 5, (nq if per_query else 1) * A[6] * 4)]


def _allow_at(L, A, pos, nq):
    """bitmap rows at `pos`, their stride in words behind them: 0 = one shared row of ceil(n / 32) words"""
    return ("in", pos, (nq * A[pos + 1] if A[pos + 1] else L.words(A[0])) * 4)


def _spec_search(L, A):
    return _prefix(L, A) + [("fields", 8, _search_out(L, A[8], A[3]))]


def _spec_search_pq(L, A):
    return _prefix(L, A, True) + [("fields", 8, _search_out(L, A[8], A[3]))]


def _spec_filtered(L, A):
    nq = A[3]
    return [("in", 1, nq * A[4]), ("in", 2, nq * 4), ("in", 5, nq * A[6]), ("in", 7, A[8] * 4), ("fields", 10, _search_out(L, A[10], nq)),
            ("out", 11, nq * 4)]


def _spec_masked(L, A, steer=False):
    nq = A[3]
    return _prefix(L, A) + [_allow_at(L, A, 8, nq), ("fields", 10, _search_out(L, A[10], nq)), ("out", 11, nq * 4), ("out", 12, nq * 4)] + \
        ([("out", 14, nq * 8)] if steer else [])


def _spec_labeled(L, A, steer=False):
    nq = A[3]
    return _prefix(L, A) + [("in", 9, A[10] * 8), ("fields", 11, _search_out(L, A[11], nq)), ("out", 12, nq * 4), ("out", 13, nq * 4)] + \
        ([("out", 15, nq * 8)] if steer else [])


def _rerank_out(L, nq, k):
    return {"ids": nq * k * 4, "dists": nq * k * 4, "frontier_size": (nq * 4, 0 if L.short_frontier else k, 4), "visited_count": nq * 4, "dist_cmps": nq * 4,
            "pruned_cmps": nq * 4, "status": 4}


def _spec_rerank(L, A, mode=None):
    """h, quant, quant params, queries, nq, stride, normalize, filter, starts, nstarts, query params, [filter], out, [two counters]"""
    nq, k = A[4], A[10].k
    s = [("in", 3, nq * A[5]), ("in", 8, A[9] * 4)]
    if mode == "masked":
        return s + [_allow_at(L, A, 11, nq), ("fields", 13, _rerank_out(L, nq, k)), ("out", 14, nq * 4), ("out", 15, nq * 4)]
    if mode == "labeled":
        return s + [("in", 12, A[13] * 8), ("fields", 14, _rerank_out(L, nq, k)), ("out", 15, nq * 4), ("out", 16, nq * 4)]
    return s + [("fields", 11, _rerank_out(L, nq, k))]


def _knn_outs(pos, nq, k):
    return [("out", pos, nq * k * 4), ("out", pos + 1, nq * k * 4), ("out", pos + 2, nq * 4, 0, k + 1)]


SPECS = {
    "pann_index_create": lambda L, A: [("in", 1, A[2] * A[5]), ("in", 7, A[2] * (A[8] + 1) * 4)],
    "pann_index_set_labels": lambda L, A: [("in", 2, A[3] * 4)],
    "pann_index_download_points": lambda L, A: [("out", 3, A[2] * A[4])],
    "pann_quantize_rows": lambda L, A: [("in", 1, A[2] * A[3]), ("out", 5, A[2] * A[6])],
    "pann_index_create_subset": lambda L, A: [("in", 2, L.words(A[1]) * 4), ("out", 5, A[6] * 4), ("out", 7, A[6] * 4)],
    "pann_batch_search": _spec_search,
    "pann_batch_search_per_query_starts": _spec_search_pq,
    "pann_batch_search_filtered": _spec_filtered,
    "pann_batch_search_masked": _spec_masked,
    "pann_batch_search_steered": lambda L, A: _spec_masked(L, A, True),
    "pann_batch_search_labeled": _spec_labeled,
    "pann_batch_search_steered_labeled": lambda L, A: _spec_labeled(L, A, True),
    "pann_batch_search_rerank": _spec_rerank,
    "pann_batch_search_masked_rerank": lambda L, A: _spec_rerank(L, A, "masked"),
    "pann_batch_search_labeled_rerank": lambda L, A: _spec_rerank(L, A, "labeled"),
    "pann_bruteforce_knn_masked": lambda L, A: [("in", 1, A[2] * A[3]), _allow_at(L, A, 5, A[2])] + _knn_outs(7, A[2], A[4]),
    "pann_bruteforce_knn_labeled": lambda L, A: [("in", 1, A[2] * A[3]), ("in", 6, A[7] * 8)] + _knn_outs(8, A[2], A[4]),
    "pann_bruteforce_knn_labeled_grouped": lambda L, A: [("in", 1, A[2] * A[3]), ("in", 6, A[7] * 8), ("in", 8, A[2] * 4)] + _knn_outs(10, A[2], A[4]),
    "pann_bruteforce_knn_masked_grouped": lambda L, A: [("in", 1, A[2] * A[3]), ("in", 5, A[6] * A[7] * 4), ("in", 8, A[2] * 4)] + _knn_outs(10, A[2], A[4]),
    "pann_range_search": lambda L, A: [("in", 1, A[3] * A[4]), ("in", 2, A[3] * 4), ("in", 5, (A[3] if A[7] else 1) * A[6] * 4),
                                       ("out", 10, A[3] * A[9] * 4), ("out", 11, A[3] * 4, 0, A[9] + 1), ("out", 12, A[3] * 4),
                                       ("out", 13, A[3] * 4, 0, 2)],
    "pann_range_query": lambda L, A: [("in", 1, A[3] * A[4]), ("in", 2, A[3] * 4), ("in", 5, A[6] * 4), ("out", 10, A[3] * A[9] * 4),
                                      ("out", 11, A[3] * 4, 0, A[9] + 1), ("out", 12, A[3] * 4), ("out", 13, A[3] * 4), ("out", 14, A[3] * 4),
                                      ("out", 15, A[3] * 4, 0, 2)],
    "pann_graph_reach": lambda L, A: [("in", 1, A[2] * 4), ("in", 3, L.words(A[0]) * 4), ("out", 5, A[8] * 4), ("out", 6, L.words(A[0]) * 4),
                                      ("out", 7, A[8] * 4)],
    "pann_vamana_insert_batch": lambda L, A: [("in", 1, A[2] * 4)],
}
UNTRACED = ("pann_index_destroy",)          # when a handle is dropped is the garbage collector's business


class StandIn:
    """what _capi.load() returns while a case runs"""

    def __init__(self):
        self.calls, self.size, self.dims = [], {}, {}
        self.identity = False           # pann_quantize_params: slope 1, offset 0 (the one-byte copy is a cast)
        self.short_frontier = False     # frontier sizes below k: GraphIndex._need has to raise
        self.kept = 37                  # what pann_index_create_subset reports for a bitmap
        self.reaches = 0

    def __getattr__(self, name):
        if not name.startswith("pann_"):
            raise AttributeError(name)
        return lambda *a: self._call(name, a)

    def words(self, h):
        return (self.size[h] + 31) // 32

    def _new_handle(self, ref, n, d):
        ref.value = HANDLE0 + 16 * len(self.size)
        self.size[ref.value], self.dims[ref.value] = n, d

    def _addr(self, a):
        return (a.value or 0) if isinstance(a, C.c_void_p) else a

    def _fill(self, name, tag, addr, spec):
        nbytes, lo, cnt = spec if isinstance(spec, tuple) else (spec, None, None)
        if not addr or not nbytes:
            return
        v = (np.uint32(zlib.crc32(f"{name}/{tag}".encode())) + np.arange((nbytes + 3) // 4, dtype=np.uint64) * 2654435761).astype(np.uint32)
        if lo is not None:
            v = (lo + v % np.uint32(cnt)).astype(np.uint32)
        C.memmove(addr, v.ctypes.data, nbytes)

    def _call(self, name, args):
        A, rec = [], [name]
        for a in args:
            if hasattr(a, "_obj"):                       # byref(x)
                A.append(a._obj)
            elif a is None or isinstance(a, C.c_void_p):
                A.append(self._addr(a))
            else:
                A.append(a)
        ptr = {}            # positions that hold an address
        for i, (a, v) in enumerate(zip(args, A)):
            if a is None or isinstance(a, C.c_void_p):
                ptr[i] = v
                rec.append(f"h{(v - HANDLE0) // 16}" if v in self.size else ("ptr" if v else "null"))
            elif isinstance(v, C.Structure):
                rec.append(_struct_fields(v))
            elif isinstance(v, (C.c_void_p, C.c_uint64)):    # an output cell: the handle or `kept`
                rec.append("cell")
            elif isinstance(v, (bytes, float)):
                rec.append(repr(v))
            else:
                rec.append(repr(operator.index(v)))         # what a C integer parameter makes of it
        for s in SPECS.get(name, lambda L, A: [])(self, A):
            kind, pos = s[0], s[1]
            if kind == "in":
                rec.append((pos, s[2], _sha(C.string_at(A[pos], s[2])) if A[pos] and s[2] else None))
            elif kind == "out":
                self._fill(name, pos, A[pos], s[2] if len(s) == 3 else s[2:])
            else:
                for f, spec in s[2].items():
                    self._fill(name, f"{pos}.{f}", getattr(A[pos], f), spec)
        if name not in UNTRACED:
            self.calls.append(tuple(rec))
        return getattr(self, "_" + name, lambda A: 0)(A)

    # ---- the calls that answer something
    def _pann_index_create(self, A):
        self._new_handle(A[0], A[2], A[3])
        return 0

    def _pann_index_create_empty(self, A):
        self._new_handle(A[0], A[1], A[2])
        return 0

    def _pann_index_create_quantized(self, A):
        self._new_handle(A[0], self.size[A[1]], self.dims[A[1]])
        return 0

    def _pann_index_create_subset(self, A):
        A[8].value = self.kept if A[2] else self.size[A[1]]
        self._new_handle(A[0], A[3] or A[8].value, self.dims[A[1]])
        return 0

    def _pann_index_size(self, A):
        return self.size[A[0]]

    def _pann_quantize_params(self, A):
        p = A[3]
        p.kind, p.dims = A[1], self.dims[A[0]]
        p.slope, p.offset = (1.0, 0) if self.identity else (0.5, 3)
        p.max_val, p.min_seen, p.max_seen = 2.5, -1.25, 7.75
        return 0

    def _pann_sketch_params_generate(self, A):
        A[2].kind, A[2].dims, A[2].median, A[2].cut = A[1], self.dims[A[0]], 5, 0.25
        return 0

    def _pann_graph_reach(self, A):
        st = A[9]
        st.unreached = max(0, 5 - 2 * self.reaches)
        st.reached, st.max_frontier, st.levels, st.truncated, st.t_s = A[8] - st.unreached, 9, 4, self.reaches & 1, 0.125
        self.reaches += 1
        return 0


# ---- canonical text of what a case returned
def canon(v):
    if v is None or isinstance(v, (bool, int, float, str, np.generic)):
        return f"{type(v).__name__}:{v!r}"
    if isinstance(v, np.ndarray):
        return f"nd:{v.dtype.str}:{v.shape}:{_sha(np.ascontiguousarray(v).tobytes())}"
    if isinstance(v, dict):
        return "{" + ",".join(f"{k}={canon(x)}" for k, x in v.items()) + "}"
    if isinstance(v, (tuple, list)):
        return type(v).__name__ + "(" + ",".join(canon(x) for x in v) + ")"
    if isinstance(v, C.Structure):
        return f"{type(v).__name__}{_struct_fields(v)}"
    if isinstance(v, DeviceIndex):
        h = v.handle.value
        return (f"DeviceIndex(n={v.n!r},d={v.d!r},max_degree={v.max_degree!r},dtype={np.dtype(v.dtype).str},metric={v.metric!r},"
                f"dtype4={v.dtype4!r},row_bytes={v.row_bytes!r},h{(h - HANDLE0) // 16})")
    raise TypeError(type(v))


# ---- fixtures
def rng(seed):
    return np.random.default_rng(seed)


X8 = rng(1).integers(0, 256, (N, D), dtype=np.uint8)
XF = rng(2).random((N, D), dtype=np.float32)
G = np.zeros((N, DEG + 1), np.uint32)
G[:, 0] = rng(3).integers(0, DEG + 1, N)
G[:, 1:] = rng(4).integers(0, N, (N, DEG))
G[:, 1:][np.arange(DEG)[None, :] >= G[:, :1]] = 0
Q8 = rng(5).integers(0, 256, (NQ, D), dtype=np.uint8)
QF = rng(6).random((NQ, D), dtype=np.float32)
QID = np.array([4, 69, 17], np.uint32)
B1 = rng(7).random(N) < 0.4                     # shared boolean row
B2 = rng(8).random((NQ, N)) < 0.3               # per-query boolean rows
B2[2, :] = B2[0, :]                             # two equal rows: np.unique has something to merge
P1 = ixm.pack_allow(B1, N)
P2 = np.concatenate([ixm.pack_allow(B2, N), np.full((NQ, 1), 0xABCD, np.uint32)], axis=1)      # packed rows wider than W
PR1 = (0x0F, 0x03)
PR2 = np.array([[1, 9], [4, 4], [1, 9]], np.int64)
LABELS = rng(9).integers(0, 64, N).astype(np.uint32)
QP = dict(k=K, beam=BEAM)


def u8(L):
    return DeviceIndex(X8, G)


def fq(L):
    f = DeviceIndex(XF, G)
    q, p = f.quantized("euclid_u8")
    return f, q, p


def graph(L, tmp, T=np.float32, identity=False, mips=False, **kw):
    L.identity = identity
    X = X8 if T == np.uint8 else XF
    io.write_bin(os.path.join(tmp, "x.bin"), X)
    io.write_graph(os.path.join(tmp, "g.bin"), G)
    cls = graph_index.UInt8EuclidianIndex if T == np.uint8 else graph_index.FloatMipsIndex if mips else graph_index.FloatEuclidianIndex
    return cls(os.path.join(tmp, "x.bin"), os.path.join(tmp, "g.bin"), **kw)


DEV = dict(d_queries_ptr=0x1000, nq=NQ, q_stride_bytes=32, d_starts_ptr=0x2000, nstarts=2, d_ids_ptr=0x3000, d_dists_ptr=0x4000, **QP)

CASES = {
    # construction
    "ctor-graph": lambda L, t: u8(L),
    "ctor-nograph-mips-exact": lambda L, t: DeviceIndex(XF, max_degree=DEG, metric="mips", device=1, exact_float_order=True),
    "ctor-refuse-no-degree": lambda L, t: DeviceIndex(X8),
    "ctor-refuse-graph-rows": lambda L, t: DeviceIndex(X8, G[:-1]),
    "ctor-refuse-points": lambda L, t: DeviceIndex(X8.astype(np.int32), G),
    "from_packed-u4-graph": lambda L, t: DeviceIndex.from_packed(X8[:, :4], D, "u4", graph=G),
    "from_packed-i4-degree": lambda L, t: DeviceIndex.from_packed(X8[:, :4], D - 1, "I4", max_degree=DEG, device=2),
    "from_packed-u4-mips": lambda L, t: DeviceIndex.from_packed(X8[:, :4], D, "u4", max_degree=DEG, metric="mips"),
    "from_packed-refuse-dtype": lambda L, t: DeviceIndex.from_packed(X8[:, :4], D, "u8", graph=G),
    "from_packed-refuse-rows": lambda L, t: DeviceIndex.from_packed(X8, D, "u4", graph=G),
    "from_packed-refuse-graph-rows": lambda L, t: DeviceIndex.from_packed(X8[:, :4], D, "u4", graph=G[:-1]),
    "from_packed-refuse-no-degree": lambda L, t: DeviceIndex.from_packed(X8[:, :4], D, "u4"),
    "empty": lambda L, t: DeviceIndex.empty(N, D, np.float16, DEG, metric="ip", device=1),
    "empty-refuse-dtype": lambda L, t: DeviceIndex.empty(N, D, np.int32, DEG),
    "quantized-euclid_u8": lambda L, t: DeviceIndex(XF, G).quantized("euclid_u8"),
    "quantized-mips_i8": lambda L, t: DeviceIndex(XF, G, metric="mips").quantized("mips_i8", trim=False),
    "quantized-euclid_u4": lambda L, t: DeviceIndex(XF, G).quantized("euclid_u4", copy_graph=False),
    "quantized-mips_i4": lambda L, t: DeviceIndex(XF, G, metric="mips").quantized("mips_i4"),
    "quantized-params-given": lambda L, t: DeviceIndex(XF, G).quantized("u8", params=_capi.QuantParams(kind=2, dims=D, slope=2.0, offset=1)),
    "subset-bool-maps": lambda L, t: u8(L).subset(B1),
    "subset-packed-nomaps": lambda L, t: u8(L).subset(P1, maps=False),
    "subset-capacity": lambda L, t: u8(L).subset(B1, capacity=80, copy_graph=False),
    "subset-clone": lambda L, t: u8(L).subset(),
    "subset-grow-nomaps": lambda L, t: u8(L).subset(capacity=100, maps=False),
    "subset-of-u4": lambda L, t: DeviceIndex.from_packed(X8[:, :4], D, "u4", graph=G).subset(B1),
    "subset-refuse-both": lambda L, t: u8(L).subset(B1, where=("any", PR1)),
    "subset-refuse-2d": lambda L, t: u8(L).subset(B2),
    "subset-refuse-capacity": lambda L, t: u8(L).subset(B1, capacity=-1),
    # batch_search
    "search-queries": lambda L, t: u8(L).batch_search(Q8, **QP),
    "search-query_ids": lambda L, t: u8(L).batch_search(query_ids=QID, starts=(0, 5), out_k=5, **QP),
    "search-2d-starts": lambda L, t: u8(L).batch_search(Q8, starts=[[0, 5], [1, 6], [2, 7]], **QP),
    "search-visited4-nodists": lambda L, t: u8(L).batch_search(Q8, visited_cap=4, want_dists=False, limit=30, degree_limit=3, cut=1.1, **QP),
    "search-refuse-starts-rows": lambda L, t: u8(L).batch_search(Q8, starts=[[0, 5], [1, 6]], **QP),
    "search-refuse-queries": lambda L, t: u8(L).batch_search(QF, **QP),
    "filtered-sketch_queries": lambda L, t: u8(L).batch_search_filtered(Q8, rng(10).integers(0, 256, (NQ, 4)), visited_cap=4, **QP),
    "filtered-query_ids": lambda L, t: u8(L).batch_search_filtered(query_ids=QID, starts=(3,), **QP),
    "filtered-refuse-sketch-alone": lambda L, t: u8(L).batch_search_filtered(query_ids=QID, sketch_queries=np.zeros((NQ, 4), np.uint8), **QP),
    "filtered-refuse-queries-alone": lambda L, t: u8(L).batch_search_filtered(Q8, **QP),
    "filtered-refuse-2d-starts": lambda L, t: u8(L).batch_search_filtered(query_ids=QID, starts=[[0], [1], [2]], **QP),
    "filtered-refuse-sketch-rows": lambda L, t: u8(L).batch_search_filtered(Q8, np.zeros((2, 4), np.uint8), **QP),
    # batch_search_masked
    "masked-bool-shared": lambda L, t: u8(L).batch_search_masked(Q8, B1, **QP),
    "masked-bool-rows": lambda L, t: u8(L).batch_search_masked(Q8, B2, starts=(0, 5), visited_cap=4, **QP),
    "masked-packed-shared": lambda L, t: u8(L).batch_search_masked(query_ids=QID, allow=P1, out_k=5, **QP),
    "masked-packed-rows": lambda L, t: u8(L).batch_search_masked(Q8, P2, want_dists=False, **QP),
    "masked-none": lambda L, t: u8(L).batch_search_masked(Q8, **QP),
    "masked-steer0": lambda L, t: u8(L).batch_search_masked(Q8, B1, steer=0, **QP),
    "masked-steer4-rows": lambda L, t: u8(L).batch_search_masked(Q8, P2, steer=4, degree_limit=3, **QP),
    "masked-steer4-query_ids": lambda L, t: u8(L).batch_search_masked(query_ids=QID, allow=B2, steer=np.int64(4), **QP),
    "masked-refuse-rows": lambda L, t: u8(L).batch_search_masked(Q8, B2[:2], **QP),
    "masked-refuse-steer-neg": lambda L, t: u8(L).batch_search_masked(Q8, B1, steer=-1, **QP),
    "masked-refuse-steer-big": lambda L, t: u8(L).batch_search_masked(Q8, B1, steer=2 ** 32, **QP),
    "masked-refuse-2d-starts": lambda L, t: u8(L).batch_search_masked(Q8, B1, starts=[[0], [1], [2]], **QP),
    "masked-refuse-bool-shape": lambda L, t: u8(L).batch_search_masked(Q8, B1[:-1], **QP),
    "masked-refuse-packed-short": lambda L, t: u8(L).batch_search_masked(Q8, P1[:2], **QP),
    "masked-order-starts-rows-first": lambda L, t: u8(L).batch_search_masked(Q8, B2[:2], starts=[[0], [1]], steer=-1, **QP),
    "masked-order-queries-before-starts": lambda L, t: u8(L).batch_search_masked(QF, B2[:2], starts=[[0], [1], [2]], steer=-1, **QP),
    "masked-order-starts-before-steer": lambda L, t: u8(L).batch_search_masked(Q8, B2[:2], starts=[[0], [1], [2]], steer=-1, **QP),
    "masked-order-steer-before-rows": lambda L, t: u8(L).batch_search_masked(Q8, B2[:2], steer=-1, **QP),
    # batch_search_labeled
    "labeled-any-shared": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", PR1), **QP),
    "labeled-match-rows": lambda L, t: u8(L).batch_search_labeled(Q8, ("Match", PR2), starts=(0, 5), visited_cap=4, **QP),
    "labeled-range-code-query_ids": lambda L, t: u8(L).batch_search_labeled(query_ids=QID, where=(2, [3, 40]), out_k=5, **QP),
    "labeled-steer4-shared": lambda L, t: u8(L).batch_search_labeled(Q8, ("range", PR1), steer=4, **QP),
    "labeled-steer0-rows": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", PR2.astype(np.uint32)), steer=0, want_dists=False, **QP),
    "labeled-refuse-none": lambda L, t: u8(L).batch_search_labeled(Q8, None, **QP),
    "labeled-refuse-triple": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", 1, 2), **QP),
    "labeled-refuse-shape": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", np.zeros((NQ, 3), np.uint32)), **QP),
    "labeled-refuse-3d": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", np.zeros((1, NQ, 2), np.uint32)), **QP),
    "labeled-refuse-word-big": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", (1, 2 ** 32)), **QP),
    "labeled-refuse-word-neg": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", (-1, 2)), **QP),
    "labeled-refuse-kind": lambda L, t: u8(L).batch_search_labeled(Q8, ("some", PR1), **QP),
    "labeled-refuse-rows": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", PR2[:2]), **QP),
    "labeled-refuse-steer": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", PR1), steer=-3, **QP),
    "labeled-refuse-2d-starts": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", PR1), starts=[[0], [1], [2]], **QP),
    "labeled-order-where-first": lambda L, t: u8(L).batch_search_labeled(Q8, ("any", PR2[:2]), starts=[[0], [1], [2]], steer=-1, **QP),
    "labeled-order-kind-before-preds": lambda L, t: u8(L).batch_search_labeled(Q8, ("some", (1, 2 ** 32)), **QP),
    # search_rerank
    "rerank-plain": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, **QP))(*fq(L)),
    "rerank-filter-normalize": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, use_filter=True, normalize_first=True, starts=[[0, 5]],
                                                                             rerank_factor=3, limit=20, degree_limit=2, **QP))(*fq(L)),
    "rerank-allow-shared": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, allow=B1, **QP))(*fq(L)),
    "rerank-allow-rows-filter": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, allow=P2, use_filter=True, **QP))(*fq(L)),
    "rerank-where-shared": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, where=("match", PR1), starts=(0, 5), **QP))(*fq(L)),
    "rerank-where-rows": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, where=("range", PR2), normalize_first=True, **QP))(*fq(L)),
    "rerank-refuse-both": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, allow=B1, where=("any", PR1), **QP))(*fq(L)),
    "rerank-refuse-allow-rows": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, allow=B2[:2], **QP))(*fq(L)),
    "rerank-refuse-where-rows": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, where=("any", PR2[:2]), **QP))(*fq(L)),
    "rerank-refuse-where-len": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, where=("any",), **QP))(*fq(L)),
    "rerank-order-both-before-where": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, QF, allow=B1[:-1], where=("some", PR1), **QP))(*fq(L)),
    "rerank-order-queries-first": lambda L, t: (lambda f, q, p: f.search_rerank(q, p, Q8, allow=B1, where=("any", PR1), **QP))(*fq(L)),
    "rerank_dev-plain": lambda L, t: (lambda f, q, p: f.search_rerank_dev(q, p, stream_ptr=0x9000, d_status_ptr=0x5000, **DEV))(*fq(L)),
    "rerank_dev-allow": lambda L, t: (lambda f, q, p: f.search_rerank_dev(q, p, d_allow_ptr=0x6000, allow_stride_words=W, d_result_count_ptr=0x7000,
                                                                        use_filter=True, d_pruned_cmps_ptr=0x8000, rerank_factor=5, **DEV))(*fq(L)),
    "rerank_dev-preds": lambda L, t: (lambda f, q, p: f.search_rerank_dev(q, p, d_preds_ptr=0x6000, pred_kind="range", npreds=NQ, d_allowed_cmps_ptr=0x7000,
                                                                        normalize_first=True, d_frontier_size_ptr=0x8000, limit=9, **DEV))(*fq(L)),
    "rerank_dev-preds-code": lambda L, t: (lambda f, q, p: f.search_rerank_dev(q, p, d_preds_ptr=0x6000, pred_kind=1, d_allow_ptr=0x7000, **DEV))(*fq(L)),
    "rerank_dev-refuse-kind": lambda L, t: (lambda f, q, p: f.search_rerank_dev(q, p, d_preds_ptr=0x6000, pred_kind="some", **DEV))(*fq(L)),
    # exact kNN under a filter
    "knn-masked-shared": lambda L, t: u8(L).bruteforce_knn_masked(Q8, K, B1),
    "knn-masked-rows": lambda L, t: u8(L).bruteforce_knn_masked(Q8, 5, P2),
    "knn-masked-refuse-rows": lambda L, t: u8(L).bruteforce_knn_masked(Q8, K, B2[:2]),
    "knn-labeled-shared": lambda L, t: u8(L).bruteforce_knn_labeled(Q8, K, ("any", PR1)),
    "knn-labeled-rows": lambda L, t: u8(L).bruteforce_knn_labeled(Q8, 5, ("range", PR2)),
    "knn-labeled-refuse-rows": lambda L, t: u8(L).bruteforce_knn_labeled(Q8, K, ("range", PR2[:2])),
    "knn-labeled-refuse-kind": lambda L, t: u8(L).bruteforce_knn_labeled(Q8, K, ("some", PR2)),
    "grouped-where-group": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, where=("match", PR2[:2]), group_of_query=[1, 0, 1], max_list_ids=16),
    "grouped-where-unique": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, where=("any", PR2)),
    "grouped-where-single": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, where=("any", PR1), group_of_query=np.zeros(NQ, np.int64)),
    "grouped-allow-group": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, 5, allow=B2[:2], group_of_query=np.array([1, 1, 0], np.uint8)),
    "grouped-allow-unique": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, allow=B2),
    "grouped-allow-unique-packed": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, allow=P2, max_list_ids=7),
    "grouped-allow-1d": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, allow=B1, group_of_query=[0, 0, 0]),
    "grouped-refuse-both": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, where=("any", PR1), allow=B1),
    "grouped-refuse-neither": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K),
    "grouped-refuse-group-range": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, allow=B2[:2], group_of_query=[0, 2, 1]),
    "grouped-refuse-group-neg": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, where=("any", PR2), group_of_query=[0, -1, 1]),
    "grouped-refuse-group-shape": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, allow=B2, group_of_query=[0, 1]),
    "grouped-refuse-table-len": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, allow=B1),
    "grouped-refuse-where-len": lambda L, t: u8(L).bruteforce_knn_grouped(Q8, K, where=("any", PR2[:2])),
    # range searches
    "range_search-shared": lambda L, t: u8(L).range_search((0, 5), 40.0, 6, queries=Q8),
    "range_search-rows-query_ids": lambda L, t: u8(L).range_search([[0, 5], [1, 0xFFFFFFFF], [2, 7]], 40.0, 6, query_ids=QID),
    "range_search-refuse-both": lambda L, t: u8(L).range_search((0,), 40.0, 6, queries=Q8, query_ids=QID),
    "range_search-refuse-neither": lambda L, t: u8(L).range_search((0,), 40.0, 6),
    "range_search-refuse-rows": lambda L, t: u8(L).range_search([[0], [1]], 40.0, 6, queries=Q8),
    "range_query-queries": lambda L, t: u8(L).range_query(Q8, radius=30.0, beam=BEAM, max_results=6),
    "range_query-query_ids": lambda L, t: u8(L).range_query(query_ids=QID, radius=30.0, beam=BEAM, max_results=5, starts=[[0, 5]], k=K, cut=1.2,
                                                            limit=40, degree_limit=3),
    "range_query-refuse-radius": lambda L, t: u8(L).range_query(Q8),
    "range_query-refuse-both": lambda L, t: u8(L).range_query(Q8, radius=1.0, query_ids=QID),
    # reachability
    "reach-consider-bool": lambda L, t: u8(L).reachability((0, 5), consider=B1, max_rounds=2),
    "reach-plain-nolevels-noids": lambda L, t: u8(L).reachability(levels=False, ids=False),
    "reach-refuse-consider": lambda L, t: u8(L).reachability(consider=B2),
    "reconnect-consider": lambda L, t: u8(L).reconnect(DEG, 8, 1.2, start=int(np.flatnonzero(B1)[0]), consider=P1),
    "reconnect-plain": lambda L, t: u8(L).reconnect(DEG, 8, 1.2, max_rounds=1),
    "reconnect-refuse-start": lambda L, t: u8(L).reconnect(DEG, 8, 1.2, start=int(np.flatnonzero(~B1)[0]), consider=B1),
    # GraphIndex
    "graph-u8-plain": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM),
    "graph-u8-plain-short": lambda L, t: (setattr(L, "short_frontier", True), graph(L, t, np.uint8).batch_search(Q8, K, BEAM, visit_limit=20))[1],
    "graph-f32-plain": lambda L, t: graph(L, t).batch_search(QF, K, BEAM),
    "graph-f32-quant-identity": lambda L, t: graph(L, t, identity=True).batch_search(QF, K, BEAM, quant=True),
    "graph-f32-quant-fused": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, quant=True, visit_limit=1),
    "graph-f32-quant-fused-bit": lambda L, t: graph(L, t, second_level="bit").batch_search(QF, K, BEAM, quant=True),
    "graph-mips-quant-fused": lambda L, t: graph(L, t, mips=True).batch_search(QF, K, BEAM, quant=True),
    "graph-mips-masked-fused-where": lambda L, t: graph(L, t, mips=True, labels=LABELS).batch_search_masked(QF, K, BEAM, quant=True, where=("any", PR1)),
    "graph-f32-quant4-identity": lambda L, t: graph(L, t, identity=True, quant_bits=4).batch_search(QF, K, BEAM, quant=True),
    "graph-f32-quant-short": lambda L, t: (setattr(L, "short_frontier", True), graph(L, t).batch_search(QF, K, BEAM, quant=True))[1],
    "graph-single_search": lambda L, t: graph(L, t, np.uint8).single_search(Q8[0], K, BEAM, False, -1),
    "graph-u8-allow": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, allow=B1),
    "graph-f32-allow-rows": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, allow=B2),
    "graph-u8-allow-quant": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, quant=True, allow=P1),
    "graph-f32-where": lambda L, t: graph(L, t, labels=LABELS).batch_search(QF, K, BEAM, where=("any", PR1)),
    "graph-u8-where-rows": lambda L, t: graph(L, t, np.uint8, labels=LABELS).batch_search(Q8, K, BEAM, where=("range", PR2)),
    "graph-f32-steer-allow": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, allow=B1, steer=3),
    "graph-u8-steer-where": lambda L, t: graph(L, t, np.uint8, labels=LABELS).batch_search(Q8, K, BEAM, where=("match", PR2), steer=0, quant=True),
    "graph-exact_below-shared-walk": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, allow=B1, exact_below=5),
    "graph-exact_below-shared-exact": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, allow=B1, exact_below=N),
    "graph-exact_below-split": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, allow=B2, exact_below=int(B2.sum(1)[1])),
    "graph-exact_below-split-steer": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, allow=B2, exact_below=int(B2.sum(1)[1]), steer=2),
    "graph-exact_below-all-exact": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, allow=P2, exact_below=N),
    "graph-exact_grouped": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, allow=B2, exact_below=int(B2.sum(1).min()), exact_grouped=True),
    "graph-masked-noquant": lambda L, t: graph(L, t).batch_search_masked(QF, K, BEAM, B1),
    "graph-masked-u8-quant": lambda L, t: graph(L, t, np.uint8).batch_search_masked(Q8, K, BEAM, B2, quant=True),
    "graph-masked-quant-identity": lambda L, t: graph(L, t, identity=True).batch_search_masked(QF, K, BEAM, B1, quant=True),
    "graph-masked-quant-identity-rows": lambda L, t: graph(L, t, identity=True).batch_search_masked(QF, K, BEAM, P2, quant=True, visit_limit=9),
    "graph-masked-quant-fused": lambda L, t: graph(L, t).batch_search_masked(QF, K, BEAM, B1, quant=True),
    "graph-masked-quant4-fused-rows": lambda L, t: graph(L, t, identity=True, quant_bits=4).batch_search_masked(QF, K, BEAM, B2, quant=True),
    "graph-masked-quant-split-grouped": lambda L, t: graph(L, t).batch_search_masked(QF, K, BEAM, B2, quant=True, exact_below=int(B2.sum(1)[1]),
                                                                                    exact_grouped=True),
    "graph-masked-where-noquant": lambda L, t: graph(L, t, labels=LABELS).batch_search_masked(QF, K, BEAM, where=("any", PR1)),
    "graph-masked-where-identity": lambda L, t: graph(L, t, identity=True, labels=LABELS).batch_search_masked(QF, K, BEAM, quant=True, where=("range", PR2)),
    "graph-masked-where-fused": lambda L, t: graph(L, t, labels=LABELS).batch_search_masked(QF, K, BEAM, quant=True, where=("match", PR2)),
    "graph-masked_from_string": lambda L, t: (lambda g: (io.write_bin(os.path.join(t, "q.bin"), QF),
                                                         g.batch_search_masked_from_string(os.path.join(t, "q.bin"), K, BEAM, B1, quant=True))[1])(graph(L, t)),
    "graph-from_string-allow": lambda L, t: (lambda g: (io.write_bin(os.path.join(t, "q.bin"), Q8),
                                                        g.batch_search_from_string(os.path.join(t, "q.bin"), K, BEAM, allow=B1))[1])(graph(L, t, np.uint8)),
    "graph-reachability": lambda L, t: graph(L, t, np.uint8).reachability(consider=B1),
    "graph-reconnect-u8": lambda L, t: graph(L, t, np.uint8).reconnect(DEG, 8, 1.2, consider=np.ones(N, bool)),
    "graph-refuse-reconnect-f32": lambda L, t: graph(L, t).reconnect(DEG, 8, 1.2),
    "graph-refuse-both": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, allow=B1, where=("any", PR1)),
    "graph-refuse-masked-both": lambda L, t: graph(L, t, np.uint8).batch_search_masked(Q8, K, BEAM, B1, where=("any", PR1)),
    "graph-refuse-masked-neither": lambda L, t: graph(L, t, np.uint8).batch_search_masked(Q8, K, BEAM),
    "graph-refuse-masked_from_string-none": lambda L, t: (lambda g: (io.write_bin(os.path.join(t, "q.bin"), Q8),
                                                                     g.batch_search_masked_from_string(os.path.join(t, "q.bin"), K, BEAM, None))[1])(graph(L, t, np.uint8)),
    "graph-refuse-steer-alone": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, steer=2),
    "graph-refuse-steer-quant": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, quant=True, allow=B1, steer=2),
    "graph-refuse-steer-quant-where": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, quant=True, where=("any", PR1), steer=2),
    "graph-refuse-allow-quant": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, quant=True, allow=B1),
    "graph-refuse-where-quant": lambda L, t: graph(L, t).batch_search(QF, K, BEAM, quant=True, where=("any", PR1)),
    "graph-refuse-second_level-masked": lambda L, t: graph(L, t, second_level="bit").batch_search_masked(QF, K, BEAM, B1, quant=True),
    "graph-refuse-second_level-where": lambda L, t: graph(L, t, second_level="bit").batch_search_masked(QF, K, BEAM, quant=True, where=("any", PR1)),
    "graph-refuse-second_level-identity": lambda L, t: graph(L, t, identity=True, second_level="bit"),
    "graph-refuse-exact-rows": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, allow=B2[:2], exact_below=N),
    "graph-refuse-walk-rows": lambda L, t: graph(L, t, np.uint8).batch_search(Q8, K, BEAM, allow=B2[:2]),
}


def run(name, tmp=None):
    """-> (the text the digest is taken over).  tmp: a directory for the files of the GraphIndex cases"""
    real, L = _capi.load, StandIn()
    _capi.load = lambda: L
    try:
        with tempfile.TemporaryDirectory(dir=tmp) as t:
            try:
                got = "return " + canon(CASES[name](L, t))
            except Exception as e:      # a refusal: its type and text are the contract
                got = f"raise {type(e).__name__}: {e}"
    finally:
        _capi.load = real
    return "\n".join(repr(c) for c in L.calls) + "\n" + got


def lines(tmp=None):
    return [f"{name} {hashlib.sha256(run(name, tmp).encode()).hexdigest()}" for name in CASES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "binding_trace_v1.txt"))
    ap.add_argument("--dump", help="print what one case recorded (or `all`) instead of writing the table")
    args = ap.parse_args()
    if args.dump:
        for name in (CASES if args.dump == "all" else [args.dump]):
            print(f"== {name}\n{run(name)}")
        return 0
    with open(args.out, "w") as f:
        f.write("\n".join(["# case sha256-of-recorded-calls-and-result"] + lines()) + "\n")
    print(f"{len(CASES)} cases -> {args.out}")


if __name__ == "__main__":
    sys.exit(main())
