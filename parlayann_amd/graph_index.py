"""Python mirror of python/graph_index.cpp (GraphIndex<T,Point>, :48-337) and of the six index
classes python/module.cpp registers (:50-57,150-155), over the C-ABI.

    Index(data_path, index_path)                       (positional order of graph_index.cpp:82)
    .batch_search(queries, knn, beam_width, quant=False, visit_limit=-1, allow=None, exact_below=None, where=None,
                  exact_grouped=False)
                                                                         -> (uint32[nq,knn], float32[nq,knn])
    .single_search(q, knn, beam_width, quant, visit_limit)               -> uint32[knn]
    .batch_search_from_string(queries_path, knn, beam_width, quant=False, visit_limit=-1)
    .batch_search_masked(queries, knn, beam_width, allow, quant=False, visit_limit=-1, exact_below=None, where=None,
                         exact_grouped=False)
                                                                         this project's own: masked results
    .set_labels(labels, first_row=0)                                     ... by label predicates: where=(kind, preds)
    .check_recall(queries_file, gt_file, neighbors, k)   prints "Recall: x"
"""
import numpy as np

from . import io, quantize, sketch
from .index import DeviceIndex, PointFilter
from .recall import recall_at_k


class GraphIndex:
    T = None
    metric = None

    def __init__(self, data_path, index_path, hnsw=False, device=0, second_level=None, quant_bits=8, labels=None):
        """labels: one uint32 per point (set_labels), what where= predicates are evaluated on (DESIGN.md "Label predicates").
        quant_bits: 8 | 4 -- bits per coordinate of the quantised copy that quant=True searches (float points only).  4: the
        four-bit quantisers ("euclid_u4" / "mips_i4", packed rows of ceil(d / 2) bytes) for the copy and for the fused rerank
        call; it has no second level, and its Euclidian translate is never a plain cast.  The default changes nothing.
        second_level: None | "bit" | "2bit" -- the three-range beam_search_rerank of graph_index.cpp:156-185: quantised
        searches (quant=True) of the one-byte copy run with a bit-sketch pre-filter (filtered_beam_search, use_filtering) before
        the exact rerank.  "bit": Euclidean_Bit_Point / Mips_Bit_Point by the metric; "2bit": Mips_2Bit_Point (mips only).
        Off by default, so results do not change unless asked for.  It needs float points whose one-byte quantisation is not
        the identity; anything else raises ValueError instead of searching unfiltered without notice.  The reference switches its second level on by itself for
        Euclidian data of more than 800 dimensions (a JL sketch, which this build does not provide) and for mips data of more
        than 200 dimensions (Mips_2Bit_Point: second_level="2bit" here)."""
        if hnsw:
            raise NotImplementedError("HNSW indices are out of scope (SURVEY.md section 2 #17)")
        if second_level not in (None, "bit", "2bit"):
            raise ValueError('second_level must be None, "bit" or "2bit"')
        if second_level == "2bit" and self.metric == "Euclidian":
            raise ValueError('second_level="2bit" (Mips_2Bit_Point) is a mips sketch')
        if quant_bits not in (8, 4):
            raise ValueError("quant_bits must be 8 or 4")
        if quant_bits == 4 and second_level is not None:
            raise ValueError("quant_bits=4 has no second level: sketches are not attached to four-bit indices")
        self.quant_bits = quant_bits
        if second_level is not None and np.dtype(self.T).itemsize == 1:
            raise ValueError("second_level needs float points: one-byte indices are searched directly (no quantised copy to filter)")
        self.second_level = second_level
        self.sparams = None
        self.points = io.read_bin(data_path, self.T)
        self.graph = io.read_graph(index_path)
        if len(self.graph) != len(self.points):        # graph_index.cpp:113-116
            raise RuntimeError("graph size and point size do not match")
        self.use_quantization = np.dtype(self.T).itemsize > 1     # :86
        self.q_index = None
        self.device = device
        # the float base goes to the device once; normalize, generate_parameters and translate_point run there (csrc/quantize.hip)
        self.index = DeviceIndex(self.points, self.graph, metric=self.metric, device=device)
        if self.use_quantization:
            if self.metric == "Euclidian":
                self.q_index, self.qparams = self.index.quantized("euclid_u8" if quant_bits == 8 else "euclid_u4")   # EQuantRange(Points) :90
                self.eparams = quantize.EuclidParams.__new__(quantize.EuclidParams)
                self.eparams.range, self.eparams.dims = (255 if quant_bits == 8 else 15), self.qparams.dims
                self.eparams.slope, self.eparams.offset = np.float32(self.qparams.slope), np.int32(self.qparams.offset)
            else:
                self.index.normalize()                                               # :94-95
                self.points = self.index.points()
                self.q_index, self.qparams = self.index.quantized("mips_i8" if quant_bits == 8 else "mips_i4", trim=True)   # Quantized_Mips_Point<8,true> :69
                self.mmax = np.float32(self.qparams.max_val)
            if second_level is not None and self.metric == "Euclidian" and self.eparams.identity:
                raise ValueError("second_level: these points quantise to themselves (slope 1), so quantised searches are plain "
                                 "searches of the one-byte copy (graph_index.cpp:145-149) and nothing would be filtered")
            if second_level is not None:                  # QQ range over the (normalised) float rows, owned by the one-byte handle
                kind = "mips_2bit" if second_level == "2bit" else ("euclid_bit" if self.metric == "Euclidian" else "mips_bit")
                self.sparams = sketch.sketch_params(self.index, kind)
                sketch.attach_sketch(self.q_index, self.index, self.sparams)
        if labels is not None:
            self.set_labels(labels)

    def set_labels(self, labels, first_row=0):
        """Labels of rows first_row .. first_row + len(labels) (DeviceIndex.set_labels).  The quantised copy gets them too: the
        fused call reads the float handle's, the plain search of a copy that is a cast (slope 1) its own."""
        self.index.set_labels(labels, first_row)
        if self.q_index is not None:
            self.q_index.set_labels(labels, first_row)

    # ---- graph reachability (DESIGN.md "Graph reachability"): from vertex 0, the start of every search of this class ----
    def reachability(self, consider=None, max_rounds=0, levels=True, ids=True):
        """DeviceIndex.reachability from vertex 0 on the searched graph (a quantised copy holds the same rows)."""
        return self.index.reachability((0,), consider, max_rounds, levels, ids)

    def reconnect(self, R, L, alpha, consider=None, max_rounds=3):
        """DeviceIndex.reconnect from vertex 0.  It rewrites graph rows, so an index with a quantised copy refuses: the copy's
        graph would go stale, and rebuilding the copy (quantized(copy_graph=True)) is the caller's decision."""
        if self.q_index is not None:
            raise ValueError("reconnect would leave the graph of the quantised copy stale: reconnect the DeviceIndex and make "
                             "the copy again with quantized(copy_graph=True)")
        return self.index.reconnect(R, L, alpha, 0, consider, max_rounds)

    # QueryParams(knn, beam, 1.35, visit_limit, min(maxDeg, 3*visit_limit))   (:198,:222,:242)
    def _qp(self, knn, beam_width, visit_limit):
        return dict(k=knn, beam=beam_width, cut=1.35, limit=visit_limit,
                    degree_limit=min(self.index.max_degree, 3 * visit_limit))

    def _search(self, queries, knn, beam_width, quant, visit_limit, allow=None, where=None, steer=None):   # search_dispatch :120-190
        queries = np.ascontiguousarray(queries, dtype=self.T)
        qp = self._qp(knn, beam_width, visit_limit)
        if steer is not None:      # the steered walk (DESIGN.md "Steered masked search"): plain masked / labeled searches only
            if allow is None and where is None:
                raise ValueError("steer= goes with allow= or where=")
            if quant and self.use_quantization:
                raise ValueError("steer= goes with quant=False: the quantised and rerank paths have no steered form")
            qp = dict(qp, steer=steer)
        if where is not None or allow is not None:
            # masked search (this project's own, DESIGN.md "Masked search"; where=: "Label predicates"): the plain search's walk
            # over the full-precision points, results = the best allowed points it compared.  Rows may be short (padding
            # 0xFFFFFFFF / +inf), so the k-results check of the plain path does not apply.  Not in the quantised or rerank paths.
            if quant and self.use_quantization:
                raise ValueError("where= goes with quant=False here (batch_search_masked(..., quant=True, where=) is the fused form)"
                                 if where is not None else
                                 "allow= goes with quant=False: the quantised and rerank paths have no masked form here "
                                 "(batch_search_masked(..., quant=True) is the fused masked search)")
            return self._masked_walk(self.index, queries, knn, qp, allow, where)
        if not (quant and self.use_quantization):
            r = self.index.batch_search(queries, out_k=knn, **qp)                # :188
            self._need(r["frontier_size"], knn)
            return r["ids"], r["dists"]
        if self.metric == "Euclidian" and self.quant_bits == 8 and self.eparams.identity:   # slope == 1: plain search on the u8 copy (:148-152)
            qq = quantize.device_quantize_rows(queries, self.qparams, device=self.device)
            r = self.q_index.batch_search(qq, out_k=knn, **qp)
            self._need(r["frontier_size"], knn)
            return r["ids"], r["dists"]
        # beam_search_rerank (beamSearch.h:390-454) in one call: the queries are quantised (mips: normalised first, :172, and
        # re-scored as normalised), sketched for the three-range form (use_filtering, :410), searched on the one-byte copy,
        # and the first min(k * rerank_factor, |beam|) frontier ids are re-scored with exact distances, sorted, k kept
        r = self.index.search_rerank(self.q_index, self.qparams, queries, normalize_first=self.metric != "Euclidian",
                                     use_filter=self.sparams is not None, rerank_factor=100, **qp)   # QP.rerank_factor (types.h:224)
        self._need(r["frontier_size"], knn)
        return r["ids"], r["dists"]

    @staticmethod
    def _need(frontier_size, knn):
        if len(frontier_size) and int(frontier_size.min()) < knn:               # beamSearch.h:416-419
            raise RuntimeError(f"Error: beam search returned {int(frontier_size.min())} elements, which is less than k = {knn}")

    @staticmethod
    def _masked_walk(index, queries, knn, qp, allow, where):
        """the masked walk of `index`: a label predicate, if given, stands for the bitmap"""
        r = (index.batch_search_labeled(queries, where=where, out_k=knn, **qp) if where is not None else
             index.batch_search_masked(queries, allow=allow, out_k=knn, **qp))
        return r["ids"], r["dists"]

    def _medoid_walk(self, queries, knn, beam_width, visit_limit, where, steer):
        """batch_search(where=, entry="medoid"): a composition, nothing more"""
        queries = np.ascontiguousarray(queries, dtype=self.T)
        flt = PointFilter.labeled(where)
        if flt.shared:
            table, group = flt.table(), np.zeros(len(queries), np.uint32)
        else:
            table, group = np.unique(flt.check(len(queries)).rows, axis=0, return_inverse=True)
        table = (flt.kind, table)
        starts = self.index.filter_medoids(where=table, per_filter=1, fill_id=0)["ids"]
        r = self.index.batch_search_grouped(queries, where=table, group_of_query=np.asarray(group).reshape(-1), starts=starts, out_k=knn,
                                            steer=steer, **self._qp(knn, beam_width, visit_limit))
        return r["ids"], r["dists"]

    def _exact_or_walk(self, queries, knn, allow, where, exact_below, walk, grouped=False):
        """The rule of DESIGN.md "Exact masked kNN": a filter (allow= or where=, not both) with at most exact_below allowed
        points is answered exactly on the full-precision handle (DeviceIndex.bruteforce_knn_masked / _labeled), any other by
        walk(queries, allow=) or walk(queries, where=) -> (ids, dists).  The counts come from PointFilter.count: bitmaps on the
        host, predicates by DeviceIndex.label_count (nothing is materialised).  Per-query rows are split by their own counts,
        each part takes its route, and the rows come back in the given order.
        grouped: the exact part of per-query rows goes through DeviceIndex.bruteforce_knn_grouped (equal rows share one list)."""
        if where is not None and allow is not None:
            raise ValueError("where and allow exclude each other")
        if exact_below is None:
            return walk(queries, allow=allow, where=where)
        queries = np.ascontiguousarray(queries, dtype=self.T)
        flt = PointFilter.of(self.index.n, allow, where)
        cnt = flt.count(self.index)
        if flt.shared:
            if cnt > exact_below:
                return walk(queries, **flt.kw)
            ids, dists, _ = getattr(self.index, "bruteforce_knn_" + flt.infix)(queries, knn, **flt.kw)
            return ids, dists
        flt.check(len(queries))
        exact = cnt <= exact_below
        ids = np.full((len(queries), knn), 0xFFFFFFFF, np.uint32)
        dists = np.full((len(queries), knn), np.inf, np.float32)
        if exact.any():
            knn_exact = getattr(self.index, "bruteforce_knn_" + ("grouped" if grouped else flt.infix))
            ids[exact], dists[exact], _ = knn_exact(queries[exact], knn, **flt.select(exact).kw)
        if not exact.all():
            ids[~exact], dists[~exact] = walk(queries[~exact], **flt.select(~exact).kw)
        return ids, dists

    def batch_search(self, queries, knn, beam_width, quant=False, visit_limit=-1, allow=None, exact_below=None, where=None,
                     exact_grouped=False, steer=None, entry=None):
        """allow: an allow bitmap or boolean mask (DeviceIndex.batch_search_masked): only allowed points are returned.
        where = (kind, preds): the same by a label predicate (DeviceIndex.batch_search_labeled); not together with allow.
        exact_below, exact_grouped (with allow or where): as batch_search_masked
        steer (with allow or where, quant=False): the steered walk, DeviceIndex.batch_search_masked(steer=); None changes nothing
        entry (with where, quant=False, no exact_below): "medoid" starts every query at the medoid of what its predicate allows
        (DESIGN.md "Entry points") -- the distinct predicates (np.unique), DeviceIndex.filter_medoids(per_filter=1, fill_id=0),
        DeviceIndex.batch_search_grouped with those start rows, steer forwarded; None changes nothing"""
        if entry is not None:
            if entry != "medoid":
                raise ValueError('entry is None or "medoid"')
            if where is None or allow is not None or exact_below is not None or (quant and self.use_quantization):
                raise ValueError('entry="medoid" goes with where=, quant=False and no exact_below')
            return self._medoid_walk(queries, knn, beam_width, visit_limit, where, steer)
        if where is None and allow is None:
            return self._search(queries, knn, beam_width, quant, visit_limit, steer=steer)
        return self._exact_or_walk(queries, knn, allow, where, exact_below,
                                   lambda q, allow=None, where=None: self._search(q, knn, beam_width, quant, visit_limit, allow, where, steer),
                                   exact_grouped)

    def _search_masked(self, queries, knn, beam_width, allow, quant, visit_limit, where=None):
        """Masked searches (this project's own, DESIGN.md "Masked search").  Rows may be short (padding 0xFFFFFFFF / +inf):
        a short row is an answer under a mask, so the k-results check of the plain paths does not apply.
        where: a label predicate in place of allow (DESIGN.md "Label predicates")."""
        if allow is None and where is None:
            raise ValueError("batch_search_masked needs allow (a bitmap or boolean mask) or where (a label predicate)")
        if not (quant and self.use_quantization):        # one-byte points, or the float table: the plain masked search
            return self._search(queries, knn, beam_width, False, visit_limit, allow, where)
        if self.second_level is not None:
            raise ValueError("quant=True masked searches have no second level: a mask together with the sketch filter is not "
                             "supported (build the index without second_level=)")
        queries = np.ascontiguousarray(queries, dtype=self.T)
        qp = self._qp(knn, beam_width, visit_limit)
        if self.metric == "Euclidian" and self.quant_bits == 8 and self.eparams.identity:   # slope == 1: the u8 copy, as _search
            qq = quantize.device_quantize_rows(queries, self.qparams, device=self.device)
            return self._masked_walk(self.q_index, qq, knn, qp, allow, where)
        # the fused masked call: masked search of the quantised copy, exact rerank of its result list on the float handle
        r = self.index.search_rerank(self.q_index, self.qparams, queries, normalize_first=self.metric != "Euclidian",
                                     rerank_factor=100, allow=allow, where=where, **qp)
        return r["ids"], r["dists"]

    def batch_search_masked(self, queries, knn, beam_width, allow=None, quant=False, visit_limit=-1, exact_below=None, where=None,
                            exact_grouped=False):
        """Only allowed points are returned (allow: an allow bitmap or boolean mask, DeviceIndex.batch_search_masked; or
        where = (kind, preds): a label predicate over the labels of set_labels, 8 bytes per query in place of a bitmap row --
        every route below has the same form under it, and exact_below is decided by DeviceIndex.label_count).
        quant=False, or one-byte points: batch_search(..., allow=).  quant=True on float points: the masked search of the
        quantised copy (quant_bits 8 or 4) with an exact rerank of its result list, in one call on the device
        (DeviceIndex.search_rerank(allow=)); not with second_level=.
        exact_below: None (the default) -- every mask is walked, as above.  An integer: a mask that allows at most that many
        points is answered EXACTLY instead, by scoring its allowed points on the full-precision table (DESIGN.md "Exact masked
        kNN"; quant makes no difference there); per-query rows are split by their own counts.  There is no built-in
        threshold: the count at which the two routes cost the same depends on the data (tools/masked_time.py --exact).
        exact_grouped: the exact part of per-query rows or predicates is answered by DeviceIndex.bruteforce_knn_grouped, which
        scores the queries of equal filters together (DESIGN.md "Exact kNN by predicate group"): the same rows, faster when many
        queries share few filters.  The default changes nothing."""
        if where is None and allow is None:
            raise ValueError("batch_search_masked needs allow (a bitmap or boolean mask)")
        return self._exact_or_walk(queries, knn, allow, where, exact_below,
                                   lambda q, allow=None, where=None: self._search_masked(q, knn, beam_width, allow, quant, visit_limit, where),
                                   exact_grouped)

    def batch_search_masked_from_string(self, queries, knn, beam_width, allow, quant=False, visit_limit=-1):
        return self._search_masked(io.read_bin(queries, self.T), knn, beam_width, allow, quant, visit_limit)

    def single_search(self, q, knn, beam_width, quant, visit_limit):
        ids, _ = self._search(np.asarray(q)[None, :], knn, beam_width, quant, visit_limit)
        return ids[0]

    def batch_search_from_string(self, queries, knn, beam_width, quant=False, visit_limit=-1, allow=None):
        return self._search(io.read_bin(queries, self.T), knn, beam_width, quant, visit_limit, allow)

    def check_recall(self, queries_file, graph_file, neighbors, k):             # :259-305
        gt_ids, _ = io.read_ibin(graph_file)
        neighbors = np.asarray(neighbors)
        if neighbors.size and (neighbors[:, :k].max() >= len(self.points)):
            raise RuntimeError("neighbor reported by query out of range")
        # resolve_eq_distances (:263,:275-283): the tie set comes from distances RECOMPUTED between the query file's points and
        # this index's (full-precision) points, not from the distance column of the ground-truth file -- one rerank launch,
        # resort off = the given order with exact distances
        queries = io.read_bin(queries_file, self.T)
        _, gt_d = self.index.rerank(np.ascontiguousarray(queries, dtype=self.T), gt_ids, None, gt_ids.shape[1], resort=False)
        rec = recall_at_k(neighbors, gt_ids, gt_d, k)
        print(f"Recall: {rec:.6g}")
        return rec


def _mk(name, T, metric):
    return type(name, (GraphIndex,), {"T": T, "metric": metric})


FloatEuclidianIndex = _mk("FloatEuclidianIndex", np.float32, "Euclidian")
FloatMipsIndex = _mk("FloatMipsIndex", np.float32, "mips")
UInt8EuclidianIndex = _mk("UInt8EuclidianIndex", np.uint8, "Euclidian")
UInt8MipsIndex = _mk("UInt8MipsIndex", np.uint8, "mips")
Int8EuclidianIndex = _mk("Int8EuclidianIndex", np.int8, "Euclidian")
Int8MipsIndex = _mk("Int8MipsIndex", np.int8, "mips")
