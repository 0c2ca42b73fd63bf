"""DeviceIndex: thin Python owner of a pann_index handle (device mirror of PointRange + Graph).

Mirrors what python/graph_index.cpp:82-118 holds (points + graph) and the batched seam of
:192-216; numpy arrays in, numpy arrays out.  Every method goes through the C-ABI.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (PANN_BF16, PANN_F16, PANN_F32, PANN_I4, PANN_I8, PANN_L2, PANN_MIPS, PANN_PRED_ANY, PANN_PRED_MATCH, PANN_PRED_RANGE,
                    PANN_QUANT_EUCLID_U4, PANN_QUANT_EUCLID_U8, PANN_QUANT_MIPS_I4, PANN_QUANT_MIPS_I8, PANN_U4, PANN_U8, BuildStats,
                    DeleteStats, QuantParams, QueryParams, ReachStats, RerankOut, SearchOut, check)
from .bf16 import bfloat16

_DT = {np.dtype(np.uint8): PANN_U8, np.dtype(np.int8): PANN_I8, np.dtype(np.float32): PANN_F32,
       np.dtype(np.float16): PANN_F16, bfloat16: PANN_BF16}


# four-bit element types have no numpy dtype: they go by name, their rows are packed uint8 (quantize.pack_nibbles)
_DT4 = {"u4": PANN_U4, "uint4": PANN_U4, "i4": PANN_I4, "int4": PANN_I4}
_QUANT_DT = {PANN_QUANT_EUCLID_U8: (np.dtype(np.uint8), PANN_L2, None), PANN_QUANT_MIPS_I8: (np.dtype(np.int8), PANN_MIPS, None),
             PANN_QUANT_EUCLID_U4: (np.dtype(np.uint8), PANN_L2, PANN_U4), PANN_QUANT_MIPS_I4: (np.dtype(np.uint8), PANN_MIPS, PANN_I4)}


def dtype_code(dt):
    if isinstance(dt, str) and dt.lower() in _DT4:
        return _DT4[dt.lower()]
    return _DT[np.dtype(dt)]


def _metric_code(metric):
    if metric in (PANN_L2, PANN_MIPS):
        return metric
    m = str(metric).lower()
    if m in ("euclidian", "euclidean", "l2"):
        return PANN_L2
    if m in ("mips", "ip"):
        return PANN_MIPS
    raise ValueError(f"unknown metric {metric!r}")


def quant_kind(kind):
    if kind in (PANN_QUANT_EUCLID_U8, PANN_QUANT_MIPS_I8, PANN_QUANT_EUCLID_U4, PANN_QUANT_MIPS_I4):
        return kind
    k = str(kind).lower()
    if k in ("euclid_u8", "euclidian_u8", "u8"):
        return PANN_QUANT_EUCLID_U8
    if k in ("mips_i8", "i8"):
        return PANN_QUANT_MIPS_I8
    if k in ("euclid_u4", "euclidian_u4", "u4"):
        return PANN_QUANT_EUCLID_U4
    if k in ("mips_i4", "i4"):
        return PANN_QUANT_MIPS_I4
    raise ValueError(f"unknown quantisation kind {kind!r}")


def _row_stride(a):
    """row stride of a C-contiguous 2-D array (numpy may report anything for a length-1 axis)"""
    return a.shape[1] * a.itemsize


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def allow_bitmap(n, allowed_ids=None, deleted_ids=None):
    """The allow bitmap of batch_search_masked: ceil(n / 32) uint32 words, point i allowed iff bit i & 31 of word i >> 5.
    allowed_ids: only these are allowed (default: all n points); deleted_ids: these are then disallowed (lazy tombstones)."""
    n = int(n)
    bits = np.zeros(n, dtype=bool) if allowed_ids is not None else np.ones(n, dtype=bool)
    if allowed_ids is not None:
        bits[np.asarray(allowed_ids, dtype=np.int64)] = True
    if deleted_ids is not None:
        bits[np.asarray(deleted_ids, dtype=np.int64)] = False
    return pack_allow(bits, n)


def pack_allow(allow, n):
    """boolean (n,) / (nq, n) -> packed uint32 (W,) / (nq, W), W = ceil(n / 32); packed uint32 arrays pass through"""
    a = np.asarray(allow)
    w = (int(n) + 31) // 32
    if a.dtype == np.bool_:
        if a.ndim not in (1, 2) or a.shape[-1] != n:
            raise ValueError(f"a boolean allow mask must be ({n},) or (nq, {n}), got {a.shape}")
        by = np.packbits(a, axis=-1, bitorder="little")
        pad = w * 4 - by.shape[-1]
        if pad:
            by = np.concatenate([by, np.zeros(by.shape[:-1] + (pad,), np.uint8)], axis=-1)
        return np.ascontiguousarray(by).view("<u4").astype(np.uint32, copy=False)
    if a.dtype != np.uint32 or a.ndim not in (1, 2) or a.shape[-1] < w:
        raise ValueError(f"allow must be boolean or packed uint32 with at least {w} words per row, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def allow_count(allow, n):
    """number of allowed points below n per bitmap row: packed uint32 (W,) / (nq, W) or boolean (n,) / (nq, n) -> int /
    int64 (nq,).  Bits at positions >= n (the tail of the last word, words past ceil(n / 32)) do not count, as on the device."""
    a = pack_allow(allow, n)
    n = int(n)
    w = (n + 31) // 32
    a = a[..., :w].copy()
    if n & 31 and w:
        a[..., w - 1] &= np.uint32((1 << (n & 31)) - 1)
    c = np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=-1).sum(axis=-1, dtype=np.int64)
    return int(c) if a.ndim == 1 else c


_PRED = {"any": PANN_PRED_ANY, "match": PANN_PRED_MATCH, "range": PANN_PRED_RANGE}


def pred_kind(kind):
    """"any" | "match" | "range" (or the PANN_PRED_* code) -> PANN_PRED_* code"""
    if isinstance(kind, str):
        if kind.lower() not in _PRED:
            raise ValueError(f'unknown predicate kind {kind!r}: "any", "match" or "range"')
        return _PRED[kind.lower()]
    return int(kind)


_pred_kind = pred_kind      # (methods that take an argument called pred_kind)


def label_preds(preds):
    """(a, b) or an (m, 2) array -> C-contiguous uint32 (m, 2) (pann_label_pred[m]) and whether it was the single (a, b) form"""
    p = np.asarray(preds)
    if p.ndim not in (1, 2) or p.shape[-1] != 2:
        raise ValueError(f"preds must be (a, b) or an (nq, 2) array, got shape {p.shape}")
    if p.size and (p.min() < 0 or p.max() > 0xFFFFFFFF):
        raise ValueError("predicate words must fit 32 unsigned bits")
    return np.ascontiguousarray(p.reshape(-1, 2).astype(np.uint32)), p.ndim == 1


def label_allow(labels, kind, preds):
    """What a label predicate allows, on the host (DESIGN.md "Label predicates"): labels uint32 (n,); kind "any" | "match" |
    "range"; preds (a, b) -> boolean (n,), or an (nq, 2) array -> boolean (nq, n).
    any: (label & a) != 0; match: (label & a) == b; range: a <= label <= b, unsigned, both ends inclusive."""
    lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    k = pred_kind(kind)
    p, single = label_preds(preds)
    a, b = p[:, :1], p[:, 1:]
    if k == PANN_PRED_ANY:
        out = (lab[None, :] & a) != 0
    elif k == PANN_PRED_MATCH:
        out = (lab[None, :] & a) == b
    elif k == PANN_PRED_RANGE:
        out = (lab[None, :] >= a) & (lab[None, :] <= b)
    else:
        raise ValueError(f"unknown predicate kind {kind!r}")
    return out[0] if single else out


class PointFilter:
    """Which points a query may return, in one place (the C side: PointFilter, pann_internal.h; DESIGN.md "The point filter on
    the host"): bitmap rows (allow=) or label predicates (where=).  rows: packed uint32 (W,) / (m, W), W >= ceil(n / 32), with
    kind None; or uint32 (m, 2) predicates with their PANN_PRED_* kind.  shared: one row serves every query."""

    def __init__(self, rows, kind=None, shared=True):
        self.rows, self.kind, self.shared = rows, kind, shared

    @classmethod
    def masked(cls, allow, n):
        """allow: boolean or packed, (n,) / (W,) shared or one row per query"""
        rows = pack_allow(allow, n)
        return cls(rows, None, rows.ndim == 1)

    @classmethod
    def labeled(cls, where):
        """where = (kind, preds): preds (a, b) shared, or an (m, 2) array"""
        if where is None or len(where) != 2:
            raise ValueError('where must be (kind, preds): kind "any" | "match" | "range", preds (a, b) or an (nq, 2) array')
        kind = pred_kind(where[0])
        preds, single = label_preds(where[1])
        return cls(preds, kind, single)

    @classmethod
    def of(cls, n, allow=None, where=None):
        """the filter of an allow= / where= pair of keywords; None for neither"""
        if where is not None:
            if allow is not None:
                raise ValueError("where and allow exclude each other")
            return cls.labeled(where)
        return None if allow is None else cls.masked(allow, n)

    infix = property(lambda self: "masked" if self.kind is None else "labeled", doc="what names the C symbols of this mode")

    def check(self, nq):
        """per-query rows have to be nq; -> self"""
        if not self.shared and len(self.rows) != nq:
            raise ValueError("per-query allow rows must be nq x W" if self.kind is None else "per-query predicates must be an (nq, 2) array")
        return self

    def select(self, rows):
        """the filter of the queries a boolean mask selects: a shared one serves any of them"""
        return self if self.shared else PointFilter(self.rows[rows], self.kind, False)

    def count(self, index):
        """allowed points per row -> int (shared) or int64 (m,): bitmaps on the host, predicates on the device (index.label_count)"""
        return allow_count(self.rows, index.n) if self.kind is None else index.label_count(self.kw["where"])

    @property
    def kw(self):
        """the allow= / where= keyword that gives this filter again"""
        return {"allow": self.rows} if self.kind is None else {"where": (self.kind, self.rows[0] if self.shared else self.rows)}

    def table(self):
        """the rows as the filter table of the grouped calls: (G, W) or (G, 2)"""
        return self.rows[None, :] if self.rows.ndim == 1 else self.rows

    def args(self, table=False):
        """the C arguments: (kind, preds, count) for predicates; (rows, stride in words, 0 = one shared row) for a bitmap, or
        (rows, count, words per row) as a table.  A None bitmap goes through as a null pointer: the library refuses it."""
        if self.kind is not None:
            return self.kind, _ptr(self.rows), len(self.rows)
        if table:
            return _ptr(self.rows), len(self.rows), self.rows.shape[1]
        return _ptr(self.rows), 0 if self.shared else self.rows.shape[1]


def _knn_out(nq, k):
    return np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32), np.empty(nq, np.uint32)


def _pad_past_counts(ids, cnt):
    """entries past a row's count are unspecified after a range call: pad them"""
    w = int(cnt.max()) if len(cnt) else 0
    ids[:, w:] = 0xFFFFFFFF
    if w:
        sub = ids[:, :w]
        sub[np.arange(w, dtype=np.uint32)[None, :] >= cnt[:, None]] = 0xFFFFFFFF


def host_graph(n, max_deg):
    """An empty graph slab in the reference layout (graph.h:134-141): n x (max_deg+1), slot 0 = degree."""
    return np.zeros((n, max_deg + 1), dtype=np.uint32)


class DeviceIndex:
    def __init__(self, points, graph=None, max_degree=None, metric="Euclidian", device=0, exact_float_order=False):
        lib = _capi.load()
        points = np.ascontiguousarray(points)
        if points.ndim != 2 or points.dtype not in _DT:
            raise ValueError("points must be a 2-D uint8/int8/float32/float16/bfloat16 (parlayann_amd.bfloat16) array")
        self._create(lib, points, points.shape[1], points.dtype, None, graph, max_degree, metric, device)
        if exact_float_order:      # validation mode: bit-identical float results on real-valued data
            check(self._lib.pann_index_set_exact_float_order(self._h, 1))

    @classmethod
    def from_packed(cls, rows, dims, dtype, graph=None, max_degree=None, metric=None, device=0):
        """A four-bit index from rows that are already packed (quantize.pack_nibbles): rows is n x ceil(dims / 2) uint8, dtype
        "u4" (unsigned nibbles, Euclidian) or "i4" (two's-complement nibbles, mips).  metric defaults to the one the type goes
        with; the other one is refused by the library."""
        lib = _capi.load()
        code = _DT4.get(str(dtype).lower())
        if code is None:
            raise ValueError('dtype must be "u4" or "i4"')
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        dims = int(dims)
        if rows.ndim != 2 or rows.shape[1] != (dims + 1) // 2:
            raise ValueError(f"rows must be n x {(dims + 1) // 2} uint8 (two coordinates per byte)")
        if metric is None:
            metric = PANN_L2 if code == PANN_U4 else PANN_MIPS
        return cls.__new__(cls)._create(lib, rows, dims, rows.dtype, code, graph, max_degree, metric, device)

    def _create(self, lib, rows, dims, dtype, dtype4, graph, max_degree, metric, device):
        """pann_index_create over host rows, with the one check of the graph argument -> self"""
        if graph is not None:
            graph = np.ascontiguousarray(graph, dtype=np.uint32)
            if graph.ndim != 2 or graph.shape[0] != len(rows):
                raise ValueError("graph must be n x (max_deg+1) uint32 (reference layout)")
            max_degree = graph.shape[1] - 1
        if max_degree is None:
            raise ValueError("give a graph or max_degree")
        max_degree, metric, h = int(max_degree), _metric_code(metric), C.c_void_p()
        check(lib.pann_index_create(C.byref(h), _ptr(rows), len(rows), dims, _DT[dtype] if dtype4 is None else dtype4, _row_stride(rows),
                                    metric, _ptr(graph), max_degree, device))
        return self._adopt(lib, h, len(rows), dims, max_degree, dtype, metric, dtype4)

    def _adopt(self, lib, h, n, d, max_degree, dtype, metric, dtype4=None):
        """the one place that makes an object the owner of a handle -> self"""
        self._lib, self._h = lib, h
        self.n, self.d, self.max_degree = n, d, max_degree
        self.dtype, self.metric, self.dtype4 = dtype, metric, dtype4
        return self

    dtype4 = None          # PANN_U4 / PANN_I4 for a four-bit index: rows are packed uint8, row_bytes of them per row

    @property
    def row_bytes(self):
        """bytes of one host-layout row"""
        return (self.d + 1) // 2 if self.dtype4 is not None else self.d * np.dtype(self.dtype).itemsize

    @classmethod
    def empty(cls, n, d, dtype, max_degree, metric="Euclidian", device=0):
        """pann_index_create_empty: n zero vectors of d coordinates and an empty graph, both filled on the device -- nothing
        crosses the bus.  Rows come later (upload_points, update_rows, vamana_insert_batch)."""
        lib = _capi.load()
        dt = np.dtype(dtype)
        if dt not in _DT:
            raise ValueError("dtype must be uint8/int8/float32/float16/bfloat16 (parlayann_amd.bfloat16)")
        n, d, max_degree, metric, h = int(n), int(d), int(max_degree), _metric_code(metric), C.c_void_p()
        check(lib.pann_index_create_empty(C.byref(h), n, d, _DT[dt], metric, max_degree, device))
        return cls.__new__(cls)._adopt(lib, h, n, d, max_degree, dt, metric)

    @classmethod
    def from_files(cls, points_path, dtype, graph_path=None, max_degree=None, metric="Euclidian", device=0, rows=None,
                   chunk_bytes=256 << 20, exact_float_order=False):
        """Stream a reference-format vector file (point_range.h:74-117: [n:u32][d:u32][rows]) -- and, optionally, a graph file
        (graph.h:147-232: [n:u32][maxDeg:u32][deg[n]][edges]) -- onto the device in chunks of about chunk_bytes, without
        holding either whole on the host.  rows = (lo, hi): only that range of the vector file becomes the index (row lo is
        vertex 0: one shard of a sharded index; the graph file, if given, must describe exactly these hi - lo vertices)."""
        lib = _capi.load()
        dt = np.dtype(dtype)
        if dt not in _DT:
            raise ValueError("dtype must be uint8/int8/float32/float16/bfloat16 (parlayann_amd.bfloat16)")
        with open(points_path, "rb") as f:
            n_file, d = (int(v) for v in np.fromfile(f, dtype=np.uint32, count=2))
        lo, hi = (0, n_file) if rows is None else (int(rows[0]), int(rows[1]))
        if not (0 <= lo < hi <= n_file):
            raise ValueError(f"rows {rows} outside the {n_file} rows of {points_path}")
        n = hi - lo
        gf = None
        if graph_path is not None:
            gf = open(graph_path, "rb")
            gn, gmax = (int(v) for v in np.fromfile(gf, dtype=np.uint32, count=2))
            if gn != n:
                gf.close()
                raise ValueError(f"graph file has {gn} vertices, the index {n}")
            max_degree = gmax
        if max_degree is None:
            raise ValueError("give a graph file or max_degree")
        self = cls.empty(n, d, dt, max_degree, metric=metric, device=device)
        h = self._h
        try:
            row_bytes = d * dt.itemsize
            step = max(1, int(chunk_bytes) // row_bytes)
            mm = np.memmap(points_path, dtype=np.uint8, mode="r", offset=8 + lo * row_bytes, shape=(n, row_bytes))
            for a in range(0, n, step):
                chunk = np.ascontiguousarray(mm[a:min(a + step, n)])
                check(lib.pann_index_upload_points(h, a, _ptr(chunk), len(chunk), row_bytes))
            del mm
            if gf is not None:
                deg = np.fromfile(gf, dtype=np.uint32, count=n)
                if deg.size != n or (deg > self.max_degree).any():
                    raise ValueError("graph file: bad degree array")
                gstep = max(1, int(chunk_bytes) // (4 * (self.max_degree + 1)))
                cols = np.arange(self.max_degree)[None, :]
                for a in range(0, n, gstep):
                    b = min(a + gstep, n)
                    dg = deg[a:b]
                    edges = np.fromfile(gf, dtype=np.uint32, count=int(dg.sum(dtype=np.int64)))
                    blk = np.zeros((b - a, self.max_degree + 1), dtype=np.uint32)
                    blk[:, 0] = dg
                    blk[:, 1:][cols < dg[:, None]] = edges
                    self.update_rows(np.arange(a, b, dtype=np.uint32), blk)
            if exact_float_order:
                check(lib.pann_index_set_exact_float_order(h, 1))
        except Exception:
            self.close()
            raise
        finally:
            if gf is not None:
                gf.close()
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pann_index_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def _queries(self, queries):
        """external query rows: C-contiguous nq x d of the INDEX dtype (a float32 array handed to an f16 index would be
        reinterpreted byte-wise by the C-ABI, which only sees a pointer and a stride)"""
        q = np.ascontiguousarray(queries)
        cols = self.row_bytes if self.dtype4 is not None else self.d        # four-bit: packed rows (quantize.pack_nibbles)
        if q.dtype != self.dtype or q.ndim != 2 or q.shape[1] != cols:
            raise ValueError(f"queries must be nq x {cols} of dtype {self.dtype}, got {q.shape} {q.dtype}")
        return q

    def reserve_dropped(self, cap):
        """pann_index_reserve_dropped: per-query scratch of the cut-prune bookkeeping (include/pann.h)"""
        check(self._lib.pann_index_reserve_dropped(self._h, int(cap)))

    @property
    def dropped_capacity(self):
        return int(self._lib.pann_index_dropped_capacity(self._h))

    # ---- graph ----
    def set_graph(self, graph):
        graph = np.ascontiguousarray(graph, dtype=np.uint32)
        assert graph.shape == (self.n, self.max_degree + 1)
        check(self._lib.pann_index_set_graph(self._h, _ptr(graph)))

    def update_rows(self, row_ids, rows):
        row_ids = np.ascontiguousarray(row_ids, dtype=np.uint32)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert rows.shape == (len(row_ids), self.max_degree + 1)
        check(self._lib.pann_index_update_rows(self._h, _ptr(row_ids), _ptr(rows), len(row_ids)))

    def clear_graph(self):
        """empty graph again (Graph(maxDeg, n), graph.h:145-147), on the device"""
        check(self._lib.pann_index_clear_graph(self._h))

    def upload_points(self, first_row, rows):
        """pann_index_upload_points: replace the vectors of rows first_row .. first_row + len(rows) (the graph is not touched):
        new vectors for slots freed by vamana_delete_batch, to be inserted with vamana_insert_batch"""
        rows = np.ascontiguousarray(rows)
        if rows.ndim != 2 or rows.dtype != self.dtype or rows.shape[1] * rows.itemsize != self.row_bytes:
            raise ValueError("rows must be a 2-D array of the index's dtype and width")
        check(self._lib.pann_index_upload_points(self._h, int(first_row), _ptr(rows), len(rows), _row_stride(rows)))

    # ---- labels: one uint32 per point, what the label predicates are evaluated on (DESIGN.md "Label predicates") ----
    def set_labels(self, labels, first_row=0):
        """pann_index_set_labels: rows first_row .. first_row + len(labels) get these labels (uint32).  The first call gives the
        handle its label array, zero filled."""
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        check(self._lib.pann_index_set_labels(self._h, int(first_row), _ptr(lab), len(lab)))

    def labels(self, first_row=0, nrows=None):
        """pann_index_get_labels: the labels of rows [first_row, first_row + nrows) as uint32"""
        nrows = self.n - first_row if nrows is None else nrows
        out = np.empty(nrows, np.uint32)
        check(self._lib.pann_index_get_labels(self._h, int(first_row), int(nrows), _ptr(out)))
        return out

    def drop_labels(self):
        check(self._lib.pann_index_drop_labels(self._h))

    @property
    def has_labels(self):
        return bool(self._lib.pann_index_has_labels(self._h))

    def _label_rows_dev(self, where, words=None):
        """The one device-side evaluation of the predicates of `where` -> (int32 tensor on the handle's device, complete; the
        filter).  words=None: pann_label_count_dev, one count per predicate; else pann_labels_to_allow_dev, `words` bitmap words
        per predicate.  Both take device pointers and run on torch's current stream, which is synchronised here."""
        import torch
        flt = PointFilter.labeled(where)
        m = len(flt.rows)
        dev = torch.device("cuda", int(self._lib.pann_index_device(self._h)))
        d_p = torch.from_numpy(flt.rows.view(np.int32)).to(dev)
        d_out = torch.empty(m if words is None else (m, words), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev)
        p, out, stream = C.c_void_p(d_p.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(st.cuda_stream or None)
        if words is None:
            check(self._lib.pann_label_count_dev(self._h, flt.kind, p, m, out, stream))
        else:
            check(self._lib.pann_labels_to_allow_dev(self._h, flt.kind, p, m, out, words, stream))
        st.synchronize()
        return d_out, flt

    def label_count(self, where):
        """pann_label_count_dev: the number of points each predicate of `where` allows, nothing materialised -> int for the
        (a, b) form, int64 (m,) for an (m, 2) array"""
        d_c, flt = self._label_rows_dev(where)
        c = d_c.cpu().numpy().view(np.uint32).astype(np.int64)
        return int(c[0]) if flt.shared else c

    def labels_to_allow(self, where):
        """pann_labels_to_allow_dev: the bitmap rows of the predicates of `where`, in the format of batch_search_masked ->
        packed uint32 (W,) for the (a, b) form, (m, W) for an (m, 2) array, W = ceil(n / 32); bits at positions >= n are 0"""
        d_a, flt = self._label_rows_dev(where, (self.n + 31) // 32)
        a = d_a.cpu().numpy().view(np.uint32)
        return a[0] if flt.shared else a

    def set_stream(self, stream_ptr, private=False):
        """pann_index_set_stream: run the handle's calls on the caller's stream (a hipStream_t as an integer; 0 = the device's
        default stream, torch's usual current stream); private=True: back to the handle's own stream"""
        check(self._lib.pann_index_set_stream(self._h, C.c_void_p(stream_ptr or None), 1 if private else 0))

    def get_option(self, name):
        return int(self._lib.pann_index_get_option(self._h, name.encode()))

    def set_option(self, name, value):
        """pann_index_set_option: per-handle tuning knobs ("forest_group", "gt_pieces"); results never depend on them"""
        check(self._lib.pann_index_set_option(self._h, name.encode(), int(value)))

    def get_graph(self):
        g = np.empty((self.n, self.max_degree + 1), dtype=np.uint32)
        check(self._lib.pann_index_get_graph(self._h, _ptr(g)))
        return g

    # ---- points: download, normalize, scalar quantisation on the device (csrc/quantize.hip) ----
    def points(self, first_row=0, nrows=None):
        """pann_index_download_points: rows [first_row, first_row + nrows) of the device slab as an nrows x d array (a four-bit
        index: nrows x ceil(d / 2) packed uint8 rows)"""
        nrows = self.n - first_row if nrows is None else nrows
        out = np.empty((nrows, self.row_bytes if self.dtype4 is not None else self.d), dtype=self.dtype)
        check(self._lib.pann_index_download_points(self._h, first_row, nrows, _ptr(out), _row_stride(out)))
        return out

    def normalize(self):
        """Point::normalize (mips_point.h:115-124) for every row, in place on the device; float32 handles only"""
        check(self._lib.pann_index_normalize(self._h))

    def quantize_params(self, kind, trim=True):
        """generate_parameters (euclidian_point.h:211-235 / mips_point.h:433-486) over the device slab -> QuantParams"""
        p = QuantParams()
        check(self._lib.pann_quantize_params(self._h, quant_kind(kind), 1 if trim else 0, C.byref(p)))
        return p

    def quantized(self, kind, trim=True, params=None, copy_graph=True):
        """QPR Q_Points(Points): -> (DeviceIndex of uint8 / int8 rows translated on the device, QuantParams).  kind:
        "euclid_u8" | "mips_i8" | "euclid_u4" | "mips_i4" (packed four-bit rows); params: translate with these instead of
        generating them from this index's rows."""
        p = self.quantize_params(kind, trim) if params is None else params
        h = C.c_void_p()
        check(self._lib.pann_index_create_quantized(C.byref(h), self._h, C.byref(p), 1 if copy_graph else 0))
        return DeviceIndex.__new__(DeviceIndex)._adopt(self._lib, h, self.n, self.d, self.max_degree, *_QUANT_DT[p.kind]), p

    # ---- subset index: carve out, compact or grow a handle on the device (DESIGN.md "Subset index") ----
    def subset(self, allow=None, *, where=None, capacity=None, copy_graph=True, maps=True):
        """pann_index_create_subset*: a new DeviceIndex over the points a bitmap keeps, in ascending id order, renumbered graph,
        labels and sketch carried over; nothing but the bitmap and the maps crosses the bus.
        allow: boolean (n,) or one packed row (allow_bitmap); None keeps every point (a clone; with capacity > n a grown copy).
        where=(kind, (a, b)): a single label predicate instead, expanded on the device (pann_labels_to_allow_dev) -- no bitmap
        crosses the bus; the index needs labels.  capacity: rows of the new index (default: the kept points; the rows behind
        them are zero with empty graph rows).  copy_graph=False: an empty graph (a dedicated index to be built).
        maps=True -> (index, new_to_old uint32 (m,), old_to_new uint32 (n,), 0xFFFFFFFF for a dropped id); else the index alone.
        Compaction after deletions: ix.subset(allow_bitmap(ix.n, deleted_ids=D))."""
        if allow is not None and where is not None:
            raise ValueError("give allow or where, not both")
        n, cap = self.n, 0 if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError("capacity must not be negative")
        h, kept = C.c_void_p(), C.c_uint64(0)
        if where is not None:
            import torch
            if np.asarray(where[1]).ndim != 1:
                raise ValueError("subset takes a single predicate (a, b)")
            d_a, _ = self._label_rows_dev(where, (n + 31) // 32)     # complete on return: the subset runs on the handle's stream
            d_n2o = torch.empty(n, dtype=torch.int32, device=d_a.device) if maps else None
            d_o2n = torch.empty(n, dtype=torch.int32, device=d_a.device) if maps else None
            check(self._lib.pann_index_create_subset_dev(C.byref(h), self._h, C.c_void_p(d_a.data_ptr()), cap, 1 if copy_graph else 0,
                                                         C.c_void_p(d_n2o.data_ptr()) if maps else None, n,
                                                         C.c_void_p(d_o2n.data_ptr()) if maps else None, C.byref(kept)))
            if maps:
                n2o = d_n2o[:kept.value].cpu().numpy().view(np.uint32)
                o2n = d_o2n.cpu().numpy().view(np.uint32)
        else:
            a = None
            if allow is not None:
                a = pack_allow(allow, n)
                if a.ndim != 1:
                    raise ValueError("subset takes one bitmap: boolean (n,) or one packed row")
            n2o = np.empty(n, np.uint32) if maps else None
            o2n = np.empty(n, np.uint32) if maps else None
            check(self._lib.pann_index_create_subset(C.byref(h), self._h, _ptr(a), cap, 1 if copy_graph else 0, _ptr(n2o), n, _ptr(o2n),
                                                     C.byref(kept)))
            if maps:
                n2o = n2o[:kept.value].copy()
        s = DeviceIndex.__new__(DeviceIndex)._adopt(self._lib, h, int(self._lib.pann_index_size(h)), self.d, self.max_degree, self.dtype,
                                                    self.metric, self.dtype4)
        return (s, n2o, o2n) if maps else s

    # ---- batched beam search: the searchAll / qsearchAll seam (beamSearch.h:374,556) ----
    def batch_search(self, queries=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None, starts=(0,),
                     query_ids=None, out_k=None, visited_cap=0, want_dists=True):
        return self._batch_search(queries, k, beam, cut, limit, degree_limit, starts, query_ids, out_k, visited_cap, want_dists)

    def batch_search_filtered(self, queries=None, sketch_queries=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None,
                              starts=(0,), query_ids=None, out_k=None, visited_cap=0, want_dists=True):
        """filtered_beam_search(..., use_filtering = true) (beamSearch.h:117-123,139-146) with the sketch attached to this
        index (parlayann_amd.sketch.attach_sketch).  queries go with sketch_queries (uint8[nq, num_bytes()], sketch.sketch_rows);
        query_ids use the index's own sketch rows.  Returns what batch_search returns -- dist_cmps being the reference's
        full_dist_cmps -- plus "pruned_cmps": starts + neighbours that passed the hash filter."""
        if (queries is None) != (sketch_queries is None):
            raise ValueError("sketch_queries go with queries, and only with them")
        return self._batch_search(queries, k, beam, cut, limit, degree_limit, starts, query_ids, out_k, visited_cap, want_dists,
                                  filtered=True, sketch_queries=sketch_queries)

    def batch_search_masked(self, queries=None, allow=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None, starts=(0,),
                            query_ids=None, out_k=None, visited_cap=0, want_dists=True, steer=None):
        """pann_batch_search_masked: the traversal of batch_search, results restricted to the points `allow` allows
        (DESIGN.md "Masked search").  allow: packed uint32 (W,) or (nq, W), W = ceil(n / 32) (allow_bitmap), or boolean (n,)
        or (nq, n); one row serves the whole batch.  ids/dists: per query the best allowed points among ALL points the search
        computed a full distance for, padded with 0xFFFFFFFF / +inf; the other fields are batch_search's.  Adds
        "result_count" (entries per row) and "allowed_cmps" (full distances of allowed points).
        steer (None: the call above, untouched): an integer makes it pann_batch_search_steered, the walk that spends its
        distances on allowed points only -- disallowed neighbours are bridges to their own allowed neighbours (DESIGN.md
        "Steered masked search").  The integer is `fill`, the number of waiting points at which a visit stops expanding
        bridges: 1 .. min(degree_limit, max_degree), 0 means that bound.  Adds "bridge_rows" and "hop2_cmps" per query."""
        flt = PointFilter(None) if allow is None else PointFilter.masked(allow, self.n)      # no bitmap: the library's refusal
        return self._batch_search(queries, k, beam, cut, limit, degree_limit, starts, query_ids, out_k, visited_cap, want_dists,
                                  flt=flt, steer=steer)

    def batch_search_labeled(self, queries=None, where=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None, starts=(0,),
                             query_ids=None, out_k=None, visited_cap=0, want_dists=True, steer=None):
        """pann_batch_search_labeled: batch_search_masked with a label predicate in place of the bitmap (DESIGN.md "Label
        predicates").  where = (kind, preds): kind "any" | "match" | "range"; preds (a, b) for the whole batch or an (nq, 2)
        uint32 array, one predicate per query.  Returns, field for field, what batch_search_masked returns for
        allow = label_allow(self.labels(), kind, preds).  steer: as batch_search_masked (pann_batch_search_steered_labeled)."""
        nq = len(queries) if queries is not None else len(query_ids)
        return self._batch_search(queries, k, beam, cut, limit, degree_limit, starts, query_ids, out_k, visited_cap, want_dists,
                                  flt=PointFilter.labeled(where).check(nq), steer=steer)

    def batch_search_grouped(self, queries=None, where=None, group_of_query=None, k=10, beam=64, cut=1.35, limit=None,
                             degree_limit=None, starts=(0,), query_ids=None, out_k=None, visited_cap=0, want_dists=True, steer=None):
        """pann_batch_search_grouped_labeled: batch_search_labeled for many queries that share few predicates, with a row of
        starts per predicate (DESIGN.md "Entry points").  where = (kind, preds[G, 2]) is a table, group_of_query (nq, each < G)
        names every query's entry; starts: one row (nstarts,) for the batch or an array (G, nstarts), one row per table entry --
        filter_medoids(where=..., fill_id=...)["ids"] as it stands.  Row q of every field is what batch_search_labeled returns
        for query q alone under the ONE predicate preds[group_of_query[q]] from its entry's start row; steer as there."""
        nq = len(queries) if queries is not None else len(query_ids)
        flt = PointFilter.labeled(where)
        table = PointFilter(np.ascontiguousarray(flt.table(), dtype=np.uint32), flt.kind, False)
        if group_of_query is None:
            raise ValueError("batch_search_grouped needs group_of_query, one table index per query")
        group = np.asarray(group_of_query)
        if group.shape != (nq,):
            raise ValueError("group_of_query must hold one table index per query")
        if nq and (group.min() < 0 or group.max() >= len(table.rows)):
            raise ValueError("group_of_query: a table index is out of range")
        return self._batch_search(queries, k, beam, cut, limit, degree_limit, starts, query_ids, out_k, visited_cap, want_dists,
                                  flt=table, steer=steer, group=np.ascontiguousarray(group.reshape(-1), dtype=np.uint32))

    def _query_rows(self, queries, query_ids):
        """queries or query_ids -> (query rows or None, uint32 ids or None, nq, row stride in bytes)"""
        if queries is not None:
            q = self._queries(queries)
            return q, None, len(q), _row_stride(q)
        qid = np.ascontiguousarray(query_ids, dtype=np.uint32)
        return None, qid, len(qid), 0

    def _qp(self, k, beam, cut, limit, degree_limit, rerank_factor=100):
        return QueryParams(k=k, beam=beam, cut=cut, limit=self.n if limit is None else limit,
                           degree_limit=self.max_degree if degree_limit is None else degree_limit,
                           rerank_factor=rerank_factor, pad=1.0)

    @staticmethod
    def _filter_counters(res, nq):
        """the two per-query outputs every filtered search adds -> their pointers, the tail of the C call"""
        res["result_count"], res["allowed_cmps"] = np.empty(nq, np.uint32), np.empty(nq, np.uint32)
        return _ptr(res["result_count"]), _ptr(res["allowed_cmps"])

    def _batch_search(self, queries, k, beam, cut, limit, degree_limit, starts, query_ids, out_k, visited_cap, want_dists,
                      filtered=False, sketch_queries=None, flt=None, steer=None, group=None):
        """One body for pann_batch_search{, _per_query_starts, _filtered, _masked, _labeled, _steered, _steered_labeled,
        _grouped_labeled}: they share (handle, queries, ids, nq, stride, [sketch rows, bytes,] starts, nstarts, [start rows,]
        params, [filter, [table indices,]] out, [extra outputs]).  group: the table indices of a grouped call, whose flt is the
        table and whose starts are one row or one row per table entry."""
        nq = len(queries) if queries is not None else len(query_ids)
        qp = self._qp(k, beam, cut, limit, degree_limit)
        out_k = k if out_k is None else out_k
        res = {
            "ids": np.empty((nq, out_k), dtype=np.uint32),
            "dists": np.empty((nq, out_k), dtype=np.float32) if want_dists else None,
            "frontier_size": np.empty(nq, dtype=np.uint32),
            "visited_count": np.empty(nq, dtype=np.uint32),
            "dist_cmps": np.empty(nq, dtype=np.uint32),
            "degree_sum": np.empty(nq, dtype=np.uint32),
            "visited_ids": np.empty((nq, visited_cap), dtype=np.uint32) if visited_cap else None,
            "visited_dists": np.empty((nq, visited_cap), dtype=np.float32) if visited_cap else None,
            "status": np.zeros(1, dtype=np.uint32),
        }
        out = SearchOut(ids=_ptr(res["ids"]), dists=_ptr(res["dists"]), out_k=out_k,
                        frontier_size=_ptr(res["frontier_size"]), visited_count=_ptr(res["visited_count"]),
                        dist_cmps=_ptr(res["dist_cmps"]), degree_sum=_ptr(res["degree_sum"]),
                        visited_ids=_ptr(res["visited_ids"]), visited_dists=_ptr(res["visited_dists"]),
                        visited_cap=visited_cap, status=_ptr(res["status"]))
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        per_query = starts.ndim == 2 and group is None          # nq x nstarts: beamSearchRandom-style, one start set per query
        if per_query and starts.shape[0] != nq:
            raise ValueError("per-query starts must be nq x nstarts")
        q, qid, _, stride = self._query_rows(queries, query_ids)
        if per_query and (filtered or flt is not None):
            raise ValueError(f"{'filtered' if filtered else 'masked'} searches take shared starts")
        name, sketch, mid, tail, counters, start_rows = "pann_batch_search", (), (), (), None, ()
        if filtered:
            sq = None
            if sketch_queries is not None:
                sq = np.ascontiguousarray(sketch_queries, dtype=np.uint8)
                if sq.ndim != 2 or sq.shape[0] != nq:
                    raise ValueError("sketch_queries must be nq rows of uint8")
            res["pruned_cmps"] = np.empty(nq, dtype=np.uint32)
            name, sketch, tail = name + "_filtered", (_ptr(sq), 0 if sq is None else sq.shape[1]), (_ptr(res["pruned_cmps"]),)
        elif flt is not None:
            if steer is not None:
                fill = int(steer)
                if fill < 0 or fill > 0xFFFFFFFF:
                    raise ValueError("steer is the fill count: 0 (the degree bound) or a positive integer")
            if steer is not None:
                counters = np.empty((nq, 2), dtype=np.uint32)
            if group is not None:      # flt is the table: steer is a flag of the one symbol
                if starts.ndim == 2 and starts.shape[0] != len(flt.rows):
                    raise ValueError("starts must be one row, or one row per table entry")
                start_rows, mid = (1 if starts.ndim == 1 else len(starts),), flt.args() + (_ptr(group),)
                tail = self._filter_counters(res, nq) + ((0, 0, None) if steer is None else (1, fill, _ptr(counters)))
                name += "_grouped_labeled"
            else:
                mid, tail = flt.check(nq).args(), self._filter_counters(res, nq)
                if steer is None:
                    name += "_" + flt.infix
                else:
                    name, tail = name + "_steered" + ("" if flt.kind is None else "_labeled"), tail + (fill, _ptr(counters))
        elif per_query:
            name += "_per_query_starts"
        check(getattr(self._lib, name)(self._h, _ptr(q), _ptr(qid), nq, stride, *sketch, _ptr(starts), starts.shape[-1], *start_rows,
                                       C.byref(qp), *mid, C.byref(out), *tail))
        if counters is not None:
            res["bridge_rows"], res["hop2_cmps"] = counters[:, 0].copy(), counters[:, 1].copy()
        return res

    # ---- quantised search + exact rerank in one call: beam_search_rerank (beamSearch.h:390-454) ----
    def search_rerank(self, quant, qparams, queries, k=10, beam=64, cut=1.35, limit=None, degree_limit=None, starts=(0,),
                      normalize_first=False, use_filter=False, rerank_factor=100, allow=None, where=None):
        """pann_batch_search_rerank on this (float32) index: `queries` (float32 rows) are quantised with `qparams` on the
        device, searched on `quant` (the one-byte DeviceIndex of quantized(); use_filter: through the sketch attached to it),
        and the first min(k * rerank_factor, frontier size) frontier ids are re-scored here and sorted.  normalize_first:
        every query goes through Point::normalize first, and the rerank scores against the normalised row.  Returns a dict
        of numpy arrays: ids, dists (nq x k), frontier_size, visited_count, dist_cmps, status (PANN_STATUS_* bits; a query
        with fewer than k frontier entries sets PANN_STATUS_SHORT_FRONTIER and pads its row), pruned_cmps with use_filter.
        allow (an allow bitmap or boolean mask, as batch_search_masked): pann_batch_search_masked_rerank -- the masked search
        of quant with a result list of min(k * rerank_factor, beam, 64) allowed points, all of them re-scored here, k kept
        (DESIGN.md "Masked search on the fused path").  The dict gains result_count (length of the quantised list) and
        allowed_cmps; a short row is padded and raises no status bit.
        where = (kind, preds), as batch_search_labeled: pann_batch_search_labeled_rerank -- the same with label predicates in
        place of the bitmap, evaluated on THIS handle's labels (quant needs none).  Not together with allow."""
        q = self._queries(queries)
        nq = len(q)
        qp = self._qp(k, beam, cut, limit, degree_limit, rerank_factor)
        res = {"ids": np.empty((nq, k), np.uint32), "dists": np.empty((nq, k), np.float32),
               "frontier_size": np.empty(nq, np.uint32), "visited_count": np.empty(nq, np.uint32),
               "dist_cmps": np.empty(nq, np.uint32), "status": np.zeros(1, np.uint32)}
        if use_filter:
            res["pruned_cmps"] = np.empty(nq, np.uint32)
        out = RerankOut(ids=_ptr(res["ids"]), dists=_ptr(res["dists"]), frontier_size=_ptr(res["frontier_size"]),
                        visited_count=_ptr(res["visited_count"]), dist_cmps=_ptr(res["dist_cmps"]),
                        pruned_cmps=_ptr(res.get("pruned_cmps")), status=_ptr(res["status"]))
        starts = np.ascontiguousarray(starts, dtype=np.uint32).reshape(-1)
        flt = PointFilter.of(self.n, allow, where)
        name, mid, tail = "pann_batch_search_rerank", (), ()
        if flt is not None:
            name, mid, tail = f"pann_batch_search_{flt.infix}_rerank", flt.check(nq).args(), self._filter_counters(res, nq)
        check(getattr(self._lib, name)(self._h, quant.handle, C.byref(qparams), _ptr(q), nq, _row_stride(q), 1 if normalize_first else 0,
                                       1 if use_filter else 0, _ptr(starts), len(starts), C.byref(qp), *mid, C.byref(out), *tail))
        return res

    def search_rerank_dev(self, quant, qparams, d_queries_ptr, nq, q_stride_bytes, d_starts_ptr, nstarts, d_ids_ptr, d_dists_ptr,
                          k=10, beam=64, cut=1.35, limit=None, degree_limit=None, normalize_first=False, use_filter=False,
                          rerank_factor=100, d_frontier_size_ptr=None, d_visited_count_ptr=None, d_dist_cmps_ptr=None,
                          d_pruned_cmps_ptr=None, d_status_ptr=None, stream_ptr=None, d_allow_ptr=None, allow_stride_words=0,
                          d_result_count_ptr=None, d_allowed_cmps_ptr=None, d_preds_ptr=None, pred_kind=None, npreds=1):
        """pann_batch_search_rerank_dev: the same on raw device addresses (integers), enqueued on `stream_ptr` (a hipStream_t as
        an integer; None / 0 = the device's default stream).  Nothing is synchronised: read the outputs after the stream has
        been.  The first call grows quant's scratch.  d_allow_ptr (packed bitmap rows on the device, allow_stride_words 0 =
        one shared row): pann_batch_search_masked_rerank_dev, with the two optional per-query outputs.  d_preds_ptr (npreds = 1 or nq
        predicates of kind pred_kind on the device, 8-byte aligned): pann_batch_search_labeled_rerank_dev, on this handle's labels."""
        qp = self._qp(k, beam, cut, limit, degree_limit, rerank_factor)
        vp = lambda a: C.c_void_p(a or None)
        out = RerankOut(ids=vp(d_ids_ptr), dists=vp(d_dists_ptr), frontier_size=vp(d_frontier_size_ptr),
                        visited_count=vp(d_visited_count_ptr), dist_cmps=vp(d_dist_cmps_ptr), pruned_cmps=vp(d_pruned_cmps_ptr),
                        status=vp(d_status_ptr))
        name, mid, tail = "pann_batch_search_rerank_dev", (), ()
        if d_preds_ptr is not None:
            name, mid = "pann_batch_search_labeled_rerank_dev", (_pred_kind(pred_kind), vp(d_preds_ptr), npreds)
        elif d_allow_ptr is not None:
            name, mid = "pann_batch_search_masked_rerank_dev", (vp(d_allow_ptr), allow_stride_words)
        if mid:
            tail = (vp(d_result_count_ptr), vp(d_allowed_cmps_ptr))
        check(getattr(self._lib, name)(self._h, quant.handle, C.byref(qparams), vp(d_queries_ptr), nq, q_stride_bytes,
                                       1 if normalize_first else 0, 1 if use_filter else 0, vp(d_starts_ptr), nstarts, C.byref(qp), *mid,
                                       C.byref(out), *tail, vp(stream_ptr)))

    # ---- robustPrune (vamana/index.h:63-137), batched ----
    def robust_prune_batch(self, owners, cand_ids, cand_offsets, alpha, R, cand_dists=None, add_out_nbrs=True):
        owners = np.ascontiguousarray(owners, dtype=np.uint32)
        cand_ids = np.ascontiguousarray(cand_ids, dtype=np.uint32)
        off = np.ascontiguousarray(cand_offsets, dtype=np.uint64)
        cd = None if cand_dists is None else np.ascontiguousarray(cand_dists, dtype=np.float32)
        m = len(owners)
        rows = np.zeros((m, R + 1), np.uint32)
        dc = np.zeros(m, np.uint32)
        check(self._lib.pann_robust_prune_batch(self._h, _ptr(owners), m, _ptr(cand_ids), _ptr(cd), _ptr(off),
                                                float(alpha), R, 1 if add_out_nbrs else 0, _ptr(rows), _ptr(dc)))
        return rows, dc

    # ---- Vamana (vamana/index.h:150-316) ----
    def vamana_insert_batch(self, batch_ids, R, L, alpha, start=0):
        b = np.ascontiguousarray(batch_ids, dtype=np.uint32)
        st = BuildStats()
        check(self._lib.pann_vamana_insert_batch(self._h, _ptr(b), len(b), start, R, L, float(alpha), C.byref(st)))
        return st

    def vamana_build(self, R, L, alpha, num_passes=1, seed=1, sort_neighbors=True, single_batch=0, point_stats=None):
        """build_index (vamana/index.h:150-186).  single_batch = degree != 0: BuildParams::single_batch -- `degree` random
        start edges per vertex, then every pass is one batch of all points (:156-170,236-240).
        point_stats = (visited[n], dist_cmps[n]) uint32 arrays: accumulated per point like the reference's BuildStats (stats.h:63-73)."""
        st = BuildStats()
        if point_stats is not None:
            vis, dc = point_stats
            if not all(a.dtype == np.uint32 and a.flags.c_contiguous and a.shape == (self.n,) for a in (vis, dc)):
                raise ValueError("point_stats must be two C-contiguous uint32 arrays of n entries")
            st.per_point_visited = vis.ctypes.data_as(C.c_void_p)
            st.per_point_dist_cmps = dc.ctypes.data_as(C.c_void_p)
        if single_batch:
            check(self._lib.pann_vamana_build_single_batch(self._h, R, L, float(alpha), num_passes, int(single_batch), seed,
                                                           1 if sort_neighbors else 0, C.byref(st)))
        else:
            check(self._lib.pann_vamana_build(self._h, R, L, float(alpha), num_passes, seed, 1 if sort_neighbors else 0,
                                              C.byref(st)))
        return st

    # ---- the two phases of a batch on device pointers (multi-GPU build, parlayann_amd/distributed.py) ----
    def vamana_search_prune_dev(self, d_batch_ptr, m, R, L, alpha, d_rows_ptr, start=0, stats=None):
        """phase A (vamana/index.h:247-266) for m batch ids at device address d_batch_ptr -> rows [m, R] at d_rows_ptr"""
        st = BuildStats() if stats is None else stats
        check(self._lib.pann_vamana_search_prune_dev(self._h, C.c_void_p(d_batch_ptr), m, start, R, L, float(alpha),
                                                     C.c_void_p(d_rows_ptr), C.byref(st)))
        return st

    def vamana_apply_rows_dev(self, d_batch_ptr, m, d_rows_ptr, R, alpha, stats=None):
        """phase B (vamana/index.h:268-300) for the whole batch: rows [m, R] at device address d_rows_ptr"""
        st = BuildStats() if stats is None else stats
        check(self._lib.pann_vamana_apply_rows_dev(self._h, C.c_void_p(d_batch_ptr), m, C.c_void_p(d_rows_ptr), R, float(alpha),
                                                   C.byref(st)))
        return st

    # ---- deleting points: batched consolidation (DESIGN.md "Deleting points") ----
    def _delete_stats(self, point_stats):
        st = DeleteStats()
        if point_stats is not None:
            if not (point_stats.dtype == np.uint32 and point_stats.flags.c_contiguous and point_stats.shape == (self.n,)):
                raise ValueError("point_stats must be a C-contiguous uint32 array of n entries")
            st.per_point_dist_cmps = point_stats.ctypes.data_as(C.c_void_p)
        return st

    @staticmethod
    def _delete_dict(st):
        return {f: getattr(st, f) for f in ("t_expand_s", "t_prune_s", "deleted", "affected", "candidates", "prune_dist_cmps")}

    def vamana_delete_batch(self, ids, R, alpha, point_stats=None):
        """pann_vamana_delete_batch: delete the ids given (any order, repeats allowed) in one call -- every vertex with a deleted
        out-neighbour is re-pruned over its surviving neighbours and those of its deleted neighbours, then the deleted rows are
        emptied.  Search from a vertex that is still live afterwards.  point_stats: uint32[n], the prune comparisons of every
        re-pruned vertex are added to it.  Returns the call's pann_delete_stats as a dict."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        st = self._delete_stats(point_stats)
        check(self._lib.pann_vamana_delete_batch(self._h, _ptr(ids), len(ids), R, float(alpha), C.byref(st)))
        return self._delete_dict(st)

    def vamana_delete_batch_dev(self, d_ids_ptr, m, R, alpha, point_stats=None):
        """the same for m ids at device address d_ids_ptr, on the handle's stream"""
        st = self._delete_stats(point_stats)
        check(self._lib.pann_vamana_delete_batch_dev(self._h, C.c_void_p(d_ids_ptr or None), m, R, float(alpha), C.byref(st)))
        return self._delete_dict(st)

    def vamana_sort_neighbors(self):
        check(self._lib.pann_vamana_sort_neighbors(self._h))

    # ---- graph reachability: BFS levels, degrees, reconnect (DESIGN.md "Graph reachability") ----
    def _consider(self, consider):
        if consider is None:
            return None
        a = pack_allow(consider, self.n)
        if a.ndim != 1:
            raise ValueError("consider is one bitmap: boolean (n,) or one packed row")
        return a

    def reachability(self, starts=(0,), consider=None, max_rounds=0, levels=True, ids=True):
        """pann_graph_reach: which vertices can a search from `starts` reach at all?  A breadth-first walk over the graph rows
        on the device; points are not read, so it works on every element type.
        consider: what allow= accepts elsewhere (boolean (n,) or one packed row, allow_bitmap): it does not steer the walk, it
        selects which vertices count and are listed as unreached -- typically the live set, allow_bitmap(n, deleted_ids=D).
        max_rounds: 0 = until the frontier is empty; r = at most r rounds (levels 0 .. r).
        Returns a dict: level uint32 (n,) with 0xFFFFFFFF for no path (None with levels=False); reached, the packed bitmap (it
        goes as it is into subset(allow=) and every masked search); unreached_ids uint32, ascending (None with ids=False);
        reached_count, unreached_count, levels, max_frontier, truncated, seconds (on the device).
        ids=True makes room for n ids and calls ONCE (the list that comes back is cut to unreached_count); only the ids found
        cross the bus."""
        n = self.n
        s = np.ascontiguousarray(starts, dtype=np.uint32).reshape(-1)
        c = self._consider(consider)
        level = np.empty(n, np.uint32) if levels else None
        reached = np.empty((n + 31) // 32, np.uint32)
        uid = np.empty(n, np.uint32) if ids else None
        st = ReachStats()
        check(self._lib.pann_graph_reach(self._h, _ptr(s), len(s), _ptr(c), int(max_rounds), _ptr(level), _ptr(reached), _ptr(uid), n,
                                         C.byref(st)))
        return {"level": level, "reached": reached, "unreached_ids": uid[:st.unreached].copy() if ids else None,
                "reached_count": int(st.reached), "unreached_count": int(st.unreached), "levels": int(st.levels),
                "max_frontier": int(st.max_frontier), "truncated": bool(st.truncated), "seconds": float(st.t_s)}

    def degrees(self):
        """pann_graph_degrees -> (out_deg, in_deg), uint32 (n,) each: the neighbour slots of a row that hold an id, and the
        (row, slot) pairs that name a vertex (a repeated neighbour counts every time, a self loop counts)"""
        out_deg, in_deg = np.empty(self.n, np.uint32), np.empty(self.n, np.uint32)
        check(self._lib.pann_graph_degrees(self._h, _ptr(out_deg), _ptr(in_deg)))
        return out_deg, in_deg

    def reconnect(self, R, L, alpha, start=0, consider=None, max_rounds=3):
        """Re-insert what a search from `start` cannot reach.  A composition, nothing more.  One round:
          U = reachability((start,), consider)["unreached_ids"]; stop if U is empty;
          vamana_insert_batch(U[i : i + b], R, L, alpha, start) over U in ascending order, b = max(1, n // 50) -- the batch bound
          of the reference's batch_insert (max_fraction .02).  A vertex that has a row is inserted as a second build pass inserts
          it: its row is overwritten.
        It stops after max_rounds rounds, or as soon as a round does not strictly reduce |U| (re-insertion stalls on some graphs).
        consider: as in reachability, typically the live set -- a deleted id must not be considered, it would be inserted again.
        Raises ValueError if `start` is not in consider.
        Returns {"unreached": [|U| before round 1, after round 1, ...], "remaining_ids": the last U}.  The filter-code state of
        the index is whatever vamana_insert_batch leaves."""
        n, start = self.n, int(start)
        c = self._consider(consider)
        if not 0 <= start < n or (c is not None and not (int(c[start >> 5]) >> (start & 31)) & 1):
            raise ValueError(f"start {start} is not a considered vertex")
        b = max(1, n // 50)
        U = self.reachability((start,), c, levels=False)["unreached_ids"]
        counts = [len(U)]
        for _ in range(int(max_rounds)):
            if len(U) == 0:
                break
            for i in range(0, len(U), b):
                self.vamana_insert_batch(U[i:i + b], R, L, alpha, start)
            U = self.reachability((start,), c, levels=False)["unreached_ids"]
            counts.append(len(U))
            if counts[-1] >= counts[-2]:
                break
        return {"unreached": counts, "remaining_ids": U}

    # ---- distances / dense all-pairs ----
    def hcnng_build(self, num_clusters, cluster_size, mst_deg, seed=1):
        """hcnng_index.h:273-281 on the device (trees, leaf kNN, Kruskal); returns {tree_s, leaf_knn_s, mst_s}."""
        times = np.zeros(3, np.float64)
        check(self._lib.pann_hcnng_build(self._h, num_clusters, cluster_size, mst_deg, seed, _ptr(times)))
        return {"tree_s": times[0], "leaf_knn_s": times[1], "mst_s": times[2]}

    def range_search(self, starts, radius_2, max_results, queries=None, query_ids=None):
        """beamSearch.h:245-306: BFS from the starts that lie within radius_2 over all vertices within radius_2.
        starts: (ns,) shared or (nq, ns) per query, 0xFFFFFFFF = padding.  Rows of `ids` are in BFS order."""
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        per_query = starts.ndim == 2
        if (queries is None) == (query_ids is None):
            raise ValueError("exactly one of queries / query_ids must be given")
        q, qid, nq, qs = self._query_rows(queries, query_ids)
        if per_query and len(starts) != nq:
            raise ValueError("per-query starts must have one row per query")
        ids = np.empty((nq, max_results), np.uint32)
        cnt = np.zeros(nq, np.uint32); cmps = np.zeros(nq, np.uint32); trunc = np.zeros(nq, np.uint32)
        check(self._lib.pann_range_search(self._h, _ptr(q), _ptr(qid), nq, qs, _ptr(starts), starts.shape[-1], 1 if per_query else 0,
                                          float(radius_2), max_results, _ptr(ids), _ptr(cnt), _ptr(cmps), _ptr(trunc)))
        _pad_past_counts(ids, cnt)
        return {"ids": ids, "counts": cnt, "dist_cmps": cmps, "truncated": trunc}

    def range_query(self, queries=None, radius=None, beam=10, max_results=1024, query_ids=None, starts=(0,), k=None, cut=0.0,
                    limit=None, degree_limit=None):
        """RangeSearch (beamSearch.h:567-614) in one call (pann_range_query): a beam search from `starts`, then the BFS of
        range_search seeded per query with its whole final frontier; the frontiers never leave the device.  Defaults are
        QueryParams(beam, beam, 0.0, n, max_degree) (:587).  Returns range_search's dict (`dist_cmps` = the BFS's comparisons)
        plus `search_cmps`, `visited` (the beam search's counters) and `range_cmps`."""
        if radius is None:
            raise ValueError("radius must be given")
        if (queries is None) == (query_ids is None):
            raise ValueError("exactly one of queries / query_ids must be given")
        q, qid, nq, qs = self._query_rows(queries, query_ids)
        starts = np.ascontiguousarray(starts, dtype=np.uint32).reshape(-1)
        qp = self._qp(beam if k is None else k, beam, cut, limit, degree_limit)
        ids = np.empty((nq, max_results), np.uint32)
        cnt = np.zeros(nq, np.uint32); trunc = np.zeros(nq, np.uint32)
        scmps = np.zeros(nq, np.uint32); vis = np.zeros(nq, np.uint32); rcmps = np.zeros(nq, np.uint32)
        check(self._lib.pann_range_query(self._h, _ptr(q), _ptr(qid), nq, qs, _ptr(starts), len(starts), C.byref(qp), float(radius),
                                         max_results, _ptr(ids), _ptr(cnt), _ptr(scmps), _ptr(vis), _ptr(rcmps), _ptr(trunc)))
        _pad_past_counts(ids, cnt)
        return {"ids": ids, "counts": cnt, "dist_cmps": rcmps, "truncated": trunc, "search_cmps": scmps, "visited": vis,
                "range_cmps": rcmps}

    def pair_distances(self, a_ids, b_ids):
        a = np.ascontiguousarray(a_ids, dtype=np.uint32); b = np.ascontiguousarray(b_ids, dtype=np.uint32)
        out = np.empty(len(a), np.float32)
        check(self._lib.pann_pair_distances(self._h, _ptr(a), _ptr(b), len(a), _ptr(out)))
        return out

    def query_distances(self, queries, ids):
        q = self._queries(queries); ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.empty((len(q), len(ids)), np.float32)
        check(self._lib.pann_query_distances(self._h, _ptr(q), len(q), _row_stride(q), _ptr(ids), len(ids), _ptr(out)))
        return out

    def leaf_knn_batch(self, ids, leaf_offsets, m):
        """hcnng_index.h:145-181 for many leaves: per member the m nearest other members."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.ascontiguousarray(leaf_offsets, dtype=np.uint64)
        oi = np.empty((len(ids), m), np.uint32); od = np.empty((len(ids), m), np.float32)
        check(self._lib.pann_leaf_knn_batch(self._h, _ptr(ids), _ptr(off), len(off) - 1, m, _ptr(oi), _ptr(od)))
        return oi, od

    def leaf_knn(self, ids, m):
        return self.leaf_knn_batch(ids, [0, len(ids)], m)

    def bruteforce_knn(self, queries, k):
        """data_tools/compute_groundtruth.cpp:22-59."""
        q = self._queries(queries)
        oi = np.empty((len(q), k), np.uint32); od = np.empty((len(q), k), np.float32)
        check(self._lib.pann_bruteforce_knn(self._h, _ptr(q), len(q), _row_stride(q), k, _ptr(oi), _ptr(od)))
        return oi, od

    def bruteforce_knn_masked(self, queries, k, allow):
        """pann_bruteforce_knn_masked: the exact k nearest ALLOWED points of every query (DESIGN.md "Exact masked kNN") ->
        (ids uint32[nq, k], dists float32[nq, k], counts uint32[nq]).  allow: as batch_search_masked -- packed uint32 (W,) or
        (nq, W), or boolean (n,) or (nq, n); one row serves the whole batch (k <= 128), rows are per query (k <= 64).  Row q
        holds counts[q] = min(k, allowed points) entries sorted by (dist, id), then 0xFFFFFFFF / +inf."""
        q = self._queries(queries)
        return self._knn_filtered(q, k, PointFilter.masked(allow, self.n))

    def bruteforce_knn_labeled(self, queries, k, where):
        """pann_bruteforce_knn_labeled: bruteforce_knn_masked with a label predicate in place of the bitmap.  where = (kind,
        preds), as batch_search_labeled: (a, b) is the shared route (k <= 128), an (nq, 2) array the per-query one (k <= 64).
        -> (ids uint32[nq, k], dists float32[nq, k], counts uint32[nq])"""
        q = self._queries(queries)
        return self._knn_filtered(q, k, PointFilter.labeled(where))

    def _knn_filtered(self, q, k, flt):
        """pann_bruteforce_knn_masked / _labeled: (handle, queries, nq, stride, k, filter, ids, dists, counts)"""
        fn, outs = getattr(self._lib, "pann_bruteforce_knn_" + flt.check(len(q)).infix), _knn_out(len(q), k)
        check(fn(self._h, _ptr(q), len(q), _row_stride(q), k, *flt.args(), *map(_ptr, outs)))
        return outs

    def bruteforce_knn_grouped(self, queries, k, *, where=None, allow=None, group_of_query=None, max_list_ids=0):
        """pann_bruteforce_knn_labeled_grouped / _masked_grouped: exact kNN for many queries that share few filters (DESIGN.md
        "Exact kNN by predicate group") -> (ids uint32[nq, k], dists float32[nq, k], counts uint32[nq]), k <= 128.
        The filters are a table: where = (kind, preds[G, 2]), or allow rows (G, W) packed / (G, n) boolean; group_of_query
        (nq, each < G) names the table entry of every query, and row q is what bruteforce_knn_labeled / bruteforce_knn_masked
        returns for query q under that ONE filter.  group_of_query=None: the table holds one filter per query (nq of them) and is
        deduplicated here (np.unique over the rows).  max_list_ids: the ids materialised at once (0: the library's default);
        results do not depend on it."""
        q = self._queries(queries)
        nq = len(q)
        if (where is None) == (allow is None):
            raise ValueError("bruteforce_knn_grouped needs where (label predicates) or allow (bitmap rows), not both")
        flt = PointFilter.of(self.n, allow, where)
        table = flt.table()
        if group_of_query is None:
            if len(table) != nq:
                raise ValueError("without group_of_query the table holds one filter per query")
            table, group = np.unique(table, axis=0, return_inverse=True)
        else:
            group = np.asarray(group_of_query)
            if group.shape != (nq,):
                raise ValueError("group_of_query must hold one table index per query")
            if nq and (group.min() < 0 or group.max() >= len(table)):
                raise ValueError("group_of_query: a table index is out of range")
        table = PointFilter(np.ascontiguousarray(table, dtype=np.uint32), flt.kind, False)
        group = np.ascontiguousarray(np.asarray(group).reshape(-1), dtype=np.uint32)
        fn, outs = getattr(self._lib, f"pann_bruteforce_knn_{flt.infix}_grouped"), _knn_out(nq, k)
        check(fn(self._h, _ptr(q), nq, _row_stride(q), k, *table.args(table=True), _ptr(group), int(max_list_ids), *map(_ptr, outs)))
        return outs

    # ---- entry points: where a filtered search starts (DESIGN.md "Entry points") ----
    def filter_medoids(self, where=None, allow=None, per_filter=1, fill_id=0xFFFFFFFF, max_list_ids=0, centroids=False):
        """pann_filter_medoids_labeled / _masked: for every filter of a table the per_filter (<= 128) allowed points nearest to
        the centroid of what it allows, on the device.  where = (kind, preds[G, 2]) or allow rows (G, W) packed / (G, n) boolean
        (one predicate or one row is a table of one); neither: every point, the medoid of the index.
        Returns {"ids" uint32 (G, per_filter), "dists" float32 (G, per_filter), "counts" uint32 (G,)} and, with centroids=True,
        "centroids" float32 (G, d).  Row g: min(per_filter, c_g) ids sorted by (dist, id), then fill_id / +inf -- with the
        ordinary start as fill_id every row is a row of starts as it stands (batch_search_grouped)."""
        flt = PointFilter.of(self.n, allow, where)
        if flt is None:
            infix, G, args = "masked", 1, (None, 1, 0)
        else:
            table = PointFilter(np.ascontiguousarray(flt.table(), dtype=np.uint32), flt.kind, False)
            infix, G, args = flt.infix, len(table.rows), table.args(table=True)
        E = int(per_filter)
        res = {"ids": np.empty((G, E), np.uint32), "dists": np.empty((G, E), np.float32), "counts": np.empty(G, np.uint32)}
        if centroids:
            res["centroids"] = np.empty((G, self.d), np.float32)
        check(getattr(self._lib, "pann_filter_medoids_" + infix)(self._h, *args, E, int(fill_id), int(max_list_ids), _ptr(res["ids"]),
                                                                 _ptr(res["dists"]), _ptr(res["counts"]), _ptr(res.get("centroids"))))
        return res

    def medoid(self, consider=None):
        """The point nearest to the centroid of the considered points -> int.  consider: what reachability takes (boolean (n,)
        or one packed row), typically the live set after vamana_delete_batch; None: every point.  ValueError if nothing is
        allowed."""
        r = self.filter_medoids(allow=self._consider(consider))
        if r["counts"][0] == 0:
            raise ValueError("medoid: no point is considered")
        return int(r["ids"][0, 0])

    def bruteforce_knn_masked_dev(self, d_queries_ptr, nq, q_stride_bytes, k, d_allow_ptr, allow_stride_words, d_ids_ptr,
                                  d_dists_ptr, d_counts_ptr=None, stream_ptr=None):
        """pann_bruteforce_knn_masked_dev: the same on raw device addresses (integers), enqueued on `stream_ptr`.  Per-query rows
        (allow_stride_words != 0): nothing is synchronised; a shared bitmap synchronises the stream once."""
        vp = lambda a: C.c_void_p(a or None)
        check(self._lib.pann_bruteforce_knn_masked_dev(self._h, vp(d_queries_ptr), nq, q_stride_bytes, k, vp(d_allow_ptr),
                                                       allow_stride_words, vp(d_ids_ptr), vp(d_dists_ptr), vp(d_counts_ptr),
                                                       vp(stream_ptr)))

    def bruteforce_range(self, queries, radius):
        """data_tools/compute_range_groundtruth.cpp:13-29: every base point within `radius` of every query, as CSR ->
        (offsets uint64[nq + 1], ids uint32[total]); the ids of a query are ascending.  A count call, then a fill call."""
        q = self._queries(queries)
        nq = len(q)
        off = np.zeros(nq + 1, np.uint64)
        check(self._lib.pann_bruteforce_range(self._h, _ptr(q), nq, _row_stride(q), float(radius), _ptr(off), None, 0))
        ids = np.empty(int(off[nq]), np.uint32)
        if len(ids):
            check(self._lib.pann_bruteforce_range(self._h, _ptr(q), nq, _row_stride(q), float(radius), _ptr(off), _ptr(ids), len(ids)))
        return off, ids

    def pivot_split(self, ids, seg_offsets, pivot_a, pivot_b):
        """clusterEdge.h:66-83: side 0 when d(id, pivot_a) <= d(id, pivot_b)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
        pa = np.ascontiguousarray(pivot_a, dtype=np.uint32); pb = np.ascontiguousarray(pivot_b, dtype=np.uint32)
        side = np.empty(len(ids), np.uint8)
        check(self._lib.pann_pivot_split(self._h, _ptr(ids), _ptr(off), len(off) - 1, _ptr(pa), _ptr(pb), _ptr(side)))
        return side

    def rerank(self, queries, cand_ids, cand_counts, k, resort=True):
        """beamSearch.h:426-452: exact distances of each query's candidates, (re)sorted, first k."""
        q = self._queries(queries)
        cand = np.ascontiguousarray(cand_ids, dtype=np.uint32)
        cnt = None if cand_counts is None else np.ascontiguousarray(cand_counts, dtype=np.uint32)
        oi = np.empty((len(q), k), np.uint32); od = np.empty((len(q), k), np.float32)
        check(self._lib.pann_rerank(self._h, _ptr(q), len(q), _row_stride(q), _ptr(cand), cand.shape[1], _ptr(cnt), k,
                                    1 if resort else 0, _ptr(oi), _ptr(od)))
        return oi, od
