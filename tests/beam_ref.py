"""The walk of the CPU checkers: a Python restatement of filtered_beam_search (beamSearch.h:22-214, use_filtering == false),
written once.  The `:NNN` comments are lines of that file.  Distances and the hash are the oracle's own
(pann_oracle_distance, pann_oracle_hash64_2); the threshold arithmetic is np.float32.

batch_search with no variant is the plain search and equals oracle.batch_search field for field (tests/test_beam_ref_cpu.py).
A search mode is a Variant: it changes the walk at the named points below and nowhere else.  tests/masked_ref.py,
tests/steered_ref.py, tests/filtered_ref.py and tests/seen_ref.py each state one rule that way.

Returns every pann_search_out field: "ids" / "dists" (the head of the frontier; "frontier_ids" / "frontier_dists" are the same
arrays under the name a variant with a result of its own leaves them), "frontier_size", "visited_count", "degree_sum",
"visited_ids" / "visited_dists" in VISIT order, as the device writes them, "visited_sorted_ids" in the reference's (dist, id)
order, "final_frontier" (per query: the whole final frontier as (dist, id) tuples) and two counters that differ only when a
variant keeps a neighbour from its distance: "dist_cmps", the full distances computed (what the reference returns, :213), and
"pruned_cmps", the reference's local counter (:83-84, :137).  Whatever Variant.end returns is stacked into further fields.
"""
import bisect
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

import oracle_api

F = np.float32
BIG = F(2147483648.0)          # (distanceType) numeric_limits<int>::max()  (:152)
_slots = {}                    # bits -> FilterSlots


class FilterSlots(dict):
    """id -> its slot in the visited filter, hash64_2(id) & ((1 << bits) - 1) (:52,:150), worked out when first asked for: a
    search touches a few thousand ids, whatever the size of the table"""

    def __init__(self, oracle, bits):
        super().__init__()
        self.hash, self.mask = oracle.hash64_2, (1 << bits) - 1

    def __missing__(self, a):
        v = self[a] = self.hash(int(a)) & self.mask
        return v


class Variant:
    """One per query, made by variant(w) before the start points are compared.  w is that query's walk:

        w.qi, w.self_id (-1 for an external query), w.k, w.beam, w.out_k, w.cut_prunes (:190 applies: k > 0 and L2)
        w.frontier, w.cand       the frontier and the pending candidates, (dist, id) tuples; cand may be appended to
        w.seen(a)                has_been_seen (:54-59)
        w.row(u)                 the first min(size, degree_limit) neighbours of u (:130)

    Every default below is the reference."""

    def __init__(self, w):
        self.w = w

    def on_distance(self, a, dist, cutoff):
        """after every full distance; cutoff is None for a start point"""

    def on_evict(self, old):
        """has_been_seen overwrote the live slot of `old`"""

    def after_direct_pass(self, pruned):
        """after the pass over the visited vertex's row (:128-136) -> the list that is counted and compared"""
        return pruned

    def before_distances(self, pruned, full):
        """the place of the use_filtering branch (:117-123, :139-146; nothing between the two reads the threshold)
        -> the neighbours that get a full distance"""
        return pruned

    def settle(self, a, cutoff, full):
        """per neighbour, before its distance -> True: the neighbour is dealt with and gets none"""
        return False

    def after_row(self):
        """after a row's comparisons, and once after the start points"""

    def after_cut_prune(self, msize):
        """after :190-196 has set the frontier's new size"""

    def end(self):
        """at the end of the query -> {field: this query's value (numpy scalar or row)} or None"""


def batch_search(points, graph, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None, degree_limit=None,
                 starts=(0,), metric="l2", out_k=None, visited_cap=0, variant=Variant):
    o = oracle_api.load()
    points = np.ascontiguousarray(points)
    graph = np.ascontiguousarray(graph, dtype=np.uint32)
    n, d = points.shape
    maxdeg = graph.shape[1] - 1
    nq = len(queries) if queries is not None else len(query_ids)
    out_k = k if out_k is None else out_k
    limit = n if limit is None else limit
    degree_limit = maxdeg if degree_limit is None else degree_limit
    starts = [int(s) for s in starts]
    mcode = oracle_api.METRIC[metric.lower() if isinstance(metric, str) else metric]
    dt = oracle_api.DT[points.dtype]
    if queries is not None:
        queries = np.ascontiguousarray(queries)
        assert queries.dtype == points.dtype
    cut_prunes = k > 0 and mcode == 0                    # :190 (is_metric(): L2 only)

    bits = max(10, int(math.ceil(math.log2(float(beam) * float(beam)))) - 2)           # :52
    if bits not in _slots:
        _slots[bits] = FilterSlots(o, bits)
    slot_of = _slots[bits]
    pbase, pstride = points.ctypes.data, points.strides[0]
    dist_fn = o.lib.pann_oracle_distance
    c_dt, c_m, c_d = C.c_int(dt), C.c_int(mcode), C.c_uint32(d)

    res = {
        "ids": np.full((nq, out_k), 0xFFFFFFFF, np.uint32), "dists": np.full((nq, out_k), np.inf, np.float32),
        "frontier_size": np.zeros(nq, np.uint32), "visited_count": np.zeros(nq, np.uint32),
        "dist_cmps": np.zeros(nq, np.uint32), "pruned_cmps": np.zeros(nq, np.uint32), "degree_sum": np.zeros(nq, np.uint32),
        "visited_ids": np.zeros((nq, visited_cap), np.uint32) if visited_cap else None,
        "visited_dists": np.zeros((nq, visited_cap), np.float32) if visited_cap else None,
        "visited_sorted_ids": np.zeros((nq, visited_cap), np.uint32) if visited_cap else None,
        "final_frontier": [],
    }
    res["frontier_ids"], res["frontier_dists"] = res["ids"], res["dists"]
    own = {}

    for qi in range(nq):
        self_id = int(query_ids[qi]) if query_ids is not None else -1
        qrow = points[self_id] if query_ids is not None else queries[qi]
        qptr = C.c_void_p(qrow.ctypes.data)
        memo, table = {}, {}                             # id -> distance; slot -> id (hash_filter, :53)
        dist_cmps = 0

        def dist(a, cutoff=None):                        # Points[a].distance(p): every call counted and shown to the variant
            nonlocal dist_cmps
            dv = memo.get(a)
            if dv is None:
                dv = memo[a] = F(dist_fn(c_dt, c_m, C.c_void_p(pbase + a * pstride), qptr, c_d))
            dist_cmps += 1
            v.on_distance(a, dv, cutoff)
            return dv

        def seen(a):                                     # has_been_seen (:54-59)
            loc = slot_of[a]
            old = table.get(loc, -1)
            if old == a:
                return True
            table[loc] = a
            if old != -1:
                v.on_evict(old)
            return False

        def row(u):
            r = graph[u]
            return r[1:1 + max(min(int(r[0]), degree_limit), 0)].tolist()                  # :130

        frontier, cand = [], []                          # (dist, id) tuples: tuple order == less (:46-48)
        w = SimpleNamespace(qi=qi, self_id=self_id, k=k, beam=beam, out_k=out_k, cut_prunes=cut_prunes, seen=seen, row=row,
                            frontier=frontier, cand=cand)
        v = variant(w)

        for s in starts:                                 # :66-70
            frontier.append((dist(s), s))
            seen(s)
        v.after_row()
        frontier.sort()
        unvisited = list(frontier)
        visited, visit_order = [], []
        pruned_cmps = len(starts)                        # :83-84
        remain, num_visited, offset = len(frontier), 0, 0
        degree_sum = 0

        while remain > offset and num_visited < limit:   # :107
            cur = unvisited[offset]
            bisect.insort_right(visited, cur)            # :112-113
            visit_order.append(cur)
            num_visited += 1
            full = len(frontier) == beam                 # :115
            nbrs = row(cur[1])                           # :128-130
            degree_sum += len(nbrs)
            pruned = v.after_direct_pass([a for a in nbrs if not (seen(a) or a == self_id)])      # :133
            pruned_cmps += len(pruned)                   # :137
            filtered = v.before_distances(pruned, full)
            cutoff = frontier[-1][0] if full else BIG    # :150-152
            for a in filtered:
                if v.settle(a, cutoff, full):
                    continue
                dv = dist(a, cutoff)                     # :153-155
                if dv >= cutoff:                         # :157
                    continue
                cand.append((dv, a))
            v.after_row()
            if len(cand) == 0 or (limit >= 2 * beam and len(cand) < beam // 8 and offset + 1 < remain):   # :162-168
                offset += 1
                continue
            offset = 0
            cand.sort()                                  # :173
            uniq = []
            for c in cand:                               # std::unique by id (:174-175)
                if not uniq or uniq[-1][1] != c[1]:
                    uniq.append(c)
            merged = sorted(set(frontier) | set(uniq))   # set_union of two sorted, duplicate-free ranges (:178-181)
            cand.clear()
            msize = min(beam, len(merged))               # :185
            if cut_prunes and msize > k:                 # :190
                thr = (F(np.float64(cut) * np.float64(merged[k][0])), 0)
                ub = bisect.bisect_right(merged, thr, 0, msize)
                msize = max(ub, len(frontier))
                v.after_cut_prune(msize)
            w.frontier = frontier = merged[:msize]       # :198-200
            vset = set(visited)
            unvisited = [e for e in frontier[:beam] if e not in vset]      # :203-208
            remain = len(unvisited)

        m = min(out_k, len(frontier))
        res["ids"][qi, :m] = [e[1] for e in frontier[:m]]
        res["dists"][qi, :m] = [e[0] for e in frontier[:m]]
        res["frontier_size"][qi] = len(frontier)
        res["visited_count"][qi] = len(visited)
        res["dist_cmps"][qi] = dist_cmps                 # :213
        res["pruned_cmps"][qi] = pruned_cmps
        res["degree_sum"][qi] = degree_sum
        res["final_frontier"].append(list(frontier))
        if visited_cap:
            assert len(visited) <= visited_cap
            nv = len(visited)
            res["visited_ids"][qi, :nv] = [e[1] for e in visit_order]
            res["visited_dists"][qi, :nv] = [e[0] for e in visit_order]
            res["visited_sorted_ids"][qi, :nv] = [e[1] for e in visited]
        for key, val in (v.end() or {}).items():
            own.setdefault(key, []).append(val)
    res.update((key, np.stack(vals)) for key, vals in own.items())
    return res
