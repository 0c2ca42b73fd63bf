"""CPU checker of the masked search: a Python restatement of filtered_beam_search (beamSearch.h:22-214, use_filtering ==
false) that also keeps the project's own result rule beside the walk (DESIGN.md "Masked search"):

    result of a query = the min(out_k, count) smallest (dist, id) keys among all ALLOWED points whose full distance the
    search computed -- the start points (:66-69) and every `a` of `filtered` (:153-155) whether or not dist < cutoff,
    candidates still unmerged at loop exit included, a point that was compared twice listed once.

The allow mask never reaches the loop: the traversal fields must equal oracle.batch_search for any mask
(tests/test_masked_ref_cpu.py pins that before anything is compared against this file).  Distances and the hash are the
oracle's own (pann_oracle_distance, pann_oracle_hash64_2).

Returns every pann_search_out field of the plain search ("frontier_ids" / "frontier_dists" are its ids / dists: the head of the
frontier; visited lists in VISIT order, as the device writes them), the masked result in "ids" / "dists" (padding 0xFFFFFFFF /
+inf), "result_count", "allowed_cmps" and three diagnostics per query:

    from_beyond_cutoff    result entries whose first comparison had dist >= cutoff (the plain search throws those away)
    from_unmerged         result entries that were still unmerged candidates when the loop ended
    recompared_in_result  result entries that were compared more than once (the hash filter is lossy)

on_distance(qi, a, dist): called for every full distance the loop computes, in order -- the hook of the independent statement
of the result in the tests.
"""
import bisect
import ctypes as C
import math

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


def unpack_allow(allow, n, nq):
    """boolean (n,) / (nq, n) or packed uint32 (W,) / (nq, W) -> boolean (nq, n) view; bits at positions >= n are dropped"""
    a = np.asarray(allow)
    if a.dtype != np.bool_:
        a = np.unpackbits(np.ascontiguousarray(a.astype("<u4")).view(np.uint8), axis=-1, bitorder="little")[..., :n].astype(bool)
    assert a.shape[-1] == n
    return np.broadcast_to(a, (nq, n))


def masked_batch_search(points, graph, allow, queries=None, query_ids=None, k=10, beam=64, cut=1.35, limit=None,
                        degree_limit=None, starts=(0,), metric="l2", out_k=None, visited_cap=0, on_distance=None):
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
    allow = unpack_allow(allow, n, nq)

    bits = max(10, int(math.ceil(math.log2(float(beam) * float(beam)))) - 2)           # :52
    hmask = (1 << bits) - 1
    if bits not in _slots:
        _slots[bits] = FilterSlots(o, bits)
    slot_of = _slots[bits]
    pbase, pstride = points.ctypes.data, points.strides[0]
    dist_fn = o.lib.pann_oracle_distance
    c_dt, c_m, c_d = C.c_int(dt), C.c_int(mcode), C.c_uint32(d)

    res = {
        "ids": np.full((nq, out_k), 0xFFFFFFFF, np.uint32), "dists": np.full((nq, out_k), np.inf, np.float32),
        "frontier_ids": np.full((nq, out_k), 0xFFFFFFFF, np.uint32), "frontier_dists": np.full((nq, out_k), np.inf, np.float32),
        "frontier_size": np.zeros(nq, np.uint32), "visited_count": np.zeros(nq, np.uint32),
        "dist_cmps": np.zeros(nq, np.uint32), "degree_sum": np.zeros(nq, np.uint32),
        "visited_ids": np.zeros((nq, visited_cap), np.uint32) if visited_cap else None,
        "visited_dists": np.zeros((nq, visited_cap), np.float32) if visited_cap else None,
        "result_count": np.zeros(nq, np.uint32), "allowed_cmps": np.zeros(nq, np.uint32),
        "from_beyond_cutoff": np.zeros(nq, np.uint32), "from_unmerged": np.zeros(nq, np.uint32),
        "recompared_in_result": np.zeros(nq, np.uint32),
        "final_frontier": [],          # per query: the whole final frontier as (dist, id) tuples (the post-filter baseline reads it)
    }

    for qi in range(nq):
        self_id = int(query_ids[qi]) if query_ids is not None else -1
        qrow = points[self_id] if query_ids is not None else queries[qi]
        qptr = C.c_void_p(qrow.ctypes.data)
        ok = allow[qi]
        seen_cmp = {}                                    # id -> [dist, times compared, first comparison was beyond the cutoff]
        allowed_cmps = 0

        def dist(a, cutoff=None):                        # Points[a].distance(p): one full distance, every call counted
            nonlocal allowed_cmps
            v = F(dist_fn(c_dt, c_m, C.c_void_p(pbase + a * pstride), qptr, c_d))
            if on_distance is not None:
                on_distance(qi, a, v)
            if ok[a]:
                allowed_cmps += 1
                e = seen_cmp.get(a)
                if e is None:
                    seen_cmp[a] = [v, 1, cutoff is not None and bool(v >= cutoff)]
                else:
                    e[1] += 1
            return v

        table = np.full(1 << bits, -1, dtype=np.int64)

        def seen(a):                                     # has_been_seen (:54-59)
            loc = slot_of[a]
            if table[loc] == a:
                return True
            table[loc] = a
            return False

        frontier = []                                    # (dist, id) tuples: tuple order == less (:46-48)
        for s in starts:                                 # :66-70
            frontier.append((dist(s), s))
            seen(s)
        frontier.sort()
        unvisited = list(frontier)
        visited, visit_order = [], []
        dist_cmps = len(starts)                          # :83-84
        remain, num_visited, offset = len(frontier), 0, 0
        degree_sum = 0
        cand = []

        while remain > offset and num_visited < limit:   # :107
            cur = unvisited[offset]
            bisect.insort_right(visited, cur)            # :112-113
            visit_order.append(cur)
            num_visited += 1
            full = len(frontier) == beam                 # :115
            row = graph[cur[1]]
            ne = max(min(int(row[0]), degree_limit), 0)  # :130
            degree_sum += ne
            pruned = []
            for i in range(ne):
                a = int(row[1 + i])
                if seen(a) or a == self_id:              # :133
                    continue
                pruned.append(a)
            dist_cmps += len(pruned)                     # :137
            cutoff = frontier[-1][0] if full else BIG    # :150-152
            for a in pruned:
                dv = dist(a, cutoff)
                if dv >= cutoff:                         # :157
                    continue
                cand.append((dv, a))
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
            cand = []
            msize = min(beam, len(merged))               # :185
            if k > 0 and msize > k and mcode == 0:       # :190 (is_metric(): L2 only)
                thr = (F(np.float64(cut) * np.float64(merged[k][0])), 0)
                ub = bisect.bisect_right(merged, thr, 0, msize)
                msize = max(ub, len(frontier))
            frontier = merged[:msize]                    # :198-200
            vset = set(visited)
            unvisited = [e for e in frontier[:beam] if e not in vset]      # :203-208
            remain = len(unvisited)

        # ---- the plain search's outputs ----
        m = min(out_k, len(frontier))
        res["frontier_ids"][qi, :m] = [e[1] for e in frontier[:m]]
        res["frontier_dists"][qi, :m] = [e[0] for e in frontier[:m]]
        res["frontier_size"][qi] = len(frontier)
        res["visited_count"][qi] = len(visited)
        res["dist_cmps"][qi] = dist_cmps
        res["degree_sum"][qi] = degree_sum
        res["final_frontier"].append(list(frontier))
        if visited_cap:
            assert len(visited) <= visited_cap
            v = len(visited)
            res["visited_ids"][qi, :v] = [e[1] for e in visit_order]
            res["visited_dists"][qi, :v] = [e[0] for e in visit_order]
        # ---- the masked result ----
        keys = sorted((e[0], a) for a, e in seen_cmp.items())[:out_k]
        unmerged = {a for _, a in cand}
        res["ids"][qi, :len(keys)] = [a for _, a in keys]
        res["dists"][qi, :len(keys)] = [v for v, _ in keys]
        res["result_count"][qi] = len(keys)
        res["allowed_cmps"][qi] = allowed_cmps
        res["from_beyond_cutoff"][qi] = sum(1 for _, a in keys if seen_cmp[a][2])
        res["from_unmerged"][qi] = sum(1 for _, a in keys if a in unmerged)
        res["recompared_in_result"][qi] = sum(1 for _, a in keys if seen_cmp[a][1] > 1)
    return res


def post_filter(res, allow, out_k):
    """The baseline a caller has without the masked search: the allowed entries of the plain search's FINAL FRONTIER, first out_k.
    -> (ids, dists) padded like the masked result."""
    nq = len(res["final_frontier"])
    allow = np.asarray(allow)
    assert allow.dtype == np.bool_                    # (n,) or (nq, n)
    allow = np.broadcast_to(allow, (nq, allow.shape[-1]))
    ids = np.full((nq, out_k), 0xFFFFFFFF, np.uint32)
    dists = np.full((nq, out_k), np.inf, np.float32)
    for qi, fr in enumerate(res["final_frontier"]):
        kept = [e for e in fr if allow[qi][e[1]]][:out_k]
        ids[qi, :len(kept)] = [e[1] for e in kept]
        dists[qi, :len(kept)] = [e[0] for e in kept]
    return ids, dists
